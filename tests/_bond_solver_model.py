"""The numpy float32 restatement of the bonds' coloured solver (include/gpe.h "the bonds' solver", csrc/bond_colours.h,
csrc/k_bond.h): the greedy colouring in plain Python, a relaxation as a sweep of the colours in order, every colour
vectorised over its bonds -- no two of them share a particle -- through tests/_bonds_model.corrections, which looks the
uids up afresh.  TEST INFRASTRUCTURE ONLY.

colours() colours a set, relax() is one coloured relaxation, apply() a pass of `iterations` of them.  Mixin gives a twin
that holds bonds (tests/_bonds_model.Twin and everything above it) the solver's mode; Twin is the bonds' twin with it,
and tests/_everything_model.Everything, the composed twin, has it in front of its bases.  hostile_scene() is tests/test_gpu_bonds._pass_scene with the hub cut to degree 30
(a hub of 200 needs more than 64 colours) and the late break moved to where a coloured sweep puts it; table_text() the
table tests/cpp/bond_colours_tests.cpp replays."""
import numpy as np

from tests import _bonds_model as BM
from tests import _colliders_model as CM

F32 = np.float32
U32 = np.uint32
COLOURS_MAX = 64
JACOBI, COLOURED = 0, 1
NAN, INF = float("nan"), float("inf")
WORLD = (200.0, 200.0)


def colours(bonds):
    """colour[j] = the least c >= 0 no bond of lower index has taken at uid_a, nor at uid_b for a pair -> int64[k]"""
    taken = {}
    out = np.zeros(len(bonds), np.int64)
    for j, (a, b, flags) in enumerate(zip(bonds["uid_a"].tolist(), bonds["uid_b"].tolist(), bonds["flags"].tolist())):
        ends = (a,) if flags & BM.BOND_ANCHOR else (a, b)
        mask = 0
        for e in ends:
            mask |= taken.get(e, 0)
        c = 0
        while (mask >> c) & 1:
            c += 1
        for e in ends:
            taken[e] = taken.get(e, 0) | (1 << c)
        out[j] = c
    return out


def colour_info(bonds):
    """-> (colours, largest_colour) as gpe_get_bond_solver_info reports them"""
    col = colours(bonds)
    if len(col) == 0:
        return 0, 0
    return int(col.max()) + 1, int(np.bincount(col).max())


def relax(pos, rad, uids, bonds, broken, world, col):
    """One coloured relaxation -> (new pos f32[n, 2], broken bool[k])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    broken = np.asarray(broken, bool).copy()
    W, H = F32(world[0]), F32(world[1])
    for c in range(int(col.max()) + 1 if len(col) else 0):
        idx = np.nonzero(col == c)[0]                                  # ascending bond index
        acts, breaks, cx, cy, sa, sb, anchor = BM.corrections(p, uids, bonds[idx], broken[idx])
        broken[idx] |= breaks
        with np.errstate(all="ignore"):
            for slots, sx, sy in ((sa[acts], cx[acts], cy[acts]),
                                  (sb[acts & ~anchor], -cx[acts & ~anchor], -cy[acts & ~anchor])):
                assert len(np.unique(slots)) == len(slots)             # within a colour no position has two writers
                qx = p[slots, 0] + sx
                qy = p[slots, 1] + sy
                x = CM.clamp_f(qx, r[slots], W - r[slots])
                y = CM.clamp_f(qy, r[slots], H - r[slots])
                p[slots, 0], p[slots, 1] = x, y
    return p, broken


def apply(pos, rad, uids, bonds, broken, iterations, world, col=None):
    """A coloured pass: `iterations` relaxations -> (new pos, broken)."""
    col = colours(bonds) if col is None else col
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    broken = np.asarray(broken, bool).copy()
    for _ in range(iterations):
        p, broken = relax(p, rad, uids, bonds, broken, world, col)
    return p, broken


class Refused(Exception):
    """what a context answers with GPE_ERR_INVALID_ARG: the set needs more than COLOURS_MAX colours"""


class Mixin:
    """In front of a twin that holds bonds: the solver's mode, kept by set_bonds and everything else."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bond_solver = JACOBI
        self.bond_colour = np.zeros(0, np.int64)
        self.solver_passes = 0

    def _coloured(self, bonds):
        col = colours(bonds)
        if len(col) and int(col.max()) + 1 > COLOURS_MAX:
            raise Refused(int(col.max()) + 1)
        return col

    def set_bond_solver(self, solver):
        mode = {"jacobi": JACOBI, "coloured": COLOURED}[solver]
        col = self._coloured(self.bonds) if mode == COLOURED else np.zeros(0, np.int64)    # (refused: nothing changes)
        self.bond_solver, self.bond_colour, self.solver_passes = mode, col, 0

    def set_bonds(self, bonds, iterations=1):
        b = np.array(bonds, BM.BOND_DTYPE).reshape(-1)
        col = self._coloured(b) if self.bond_solver == COLOURED else np.zeros(0, np.int64)  # (refused: the old set stays)
        super().set_bonds(bonds, iterations)
        self.bond_colour = col

    def apply_bonds(self):
        if self.bond_solver != COLOURED:
            return super().apply_bonds()
        if len(self.bonds) == 0 or self.uids is None:
            return
        self._pull()
        self.pos, self.broken = apply(self.pos, self.radius, self.uids, self.bonds, self.broken, self.bond_iterations,
                                      self.world, self.bond_colour)
        self.bond_passes += 1
        self.solver_passes += 1

    def bond_solver_info(self):
        """gpe_get_bond_solver_info without form and lds_nodes_max, which are the device's"""
        c, largest = colour_info(self.bonds) if self.bond_solver == COLOURED else (0, 0)
        return dict(mode=self.bond_solver, colours=c, largest_colour=largest, passes=self.solver_passes)


class Twin(Mixin, BM.Twin):
    """tests/_bonds_model.Twin with the solver's mode"""


def everything_class():
    """tests/_everything_model.Everything, which has this file's Mixin in front of its bases (imported late: that module
    imports this one, and GPU test files)"""
    from tests import _everything_model as EV
    assert EV.Everything.__mro__[1] is Mixin
    return EV.Everything


# ---- the hostile scene ----------------------------------------------------------------------------------------------
HUB_DEGREE = 30


def hostile_scene(n):
    """tests/test_gpu_bonds._pass_scene, its hub cut to degree HUB_DEGREE: n particles on a jittered 64-wide lattice of
    spacing 3 with uids that are no storage indices, and about 2800 bonds: near pairs, a chain, the hub, a leaf, a
    duplicate, absent uids, anchors, coincident ends, NaN / inf / 1e30 positions, breaks in the first and in the third
    relaxation, a pull across the world's edge.  The last 60 storage slots hold the particles with a special role.
    -> (pos, rad, uids, bonds, the index of the bond that breaks in the third relaxation)"""
    M = BM
    rng = np.random.default_rng(n)
    full = 4000
    i = np.arange(full)
    pos = np.stack([4.0 + 3.0 * (i % 64), 4.0 + 3.0 * (i // 64)], axis=1) + rng.uniform(-0.4, 0.4, (full, 2))
    pos = pos.astype(F32)
    rad = np.full(full, 0.5, F32)
    uids = (rng.permutation(full).astype(np.uint64) * 7919 + 11).astype(U32)     # distinct, far above n, unordered
    s = full - 60                                                                  # the first special slot
    u = lambda slot: uids[slot]
    parts = []
    a = rng.integers(0, s - 65, 2700)
    a = a[(a % 64) != 63]
    b = np.where(rng.random(len(a)) < 0.5, a + 1, a + 64)
    near = M.pairs(u(a), u(b), rng.uniform(2.0, 4.0, len(a)).astype(F32), rng.uniform(0.0, 1.0, len(a)).astype(F32))
    near["max_length"] = np.where(rng.random(len(a)) < 0.3, rng.uniform(2.6, 4.5, len(a)), 0.0).astype(F32)
    near["stiffness"][:20] = (0.0, 1.0) * 10
    parts.append(near)
    parts.append(M.pairs(u(np.arange(100, 160)), u(np.arange(101, 161)), 2.5, 0.5))           # a chain along a row
    hub, spokes = s + 0, rng.choice(s, HUB_DEGREE, replace=False)
    hub_bonds = M.pairs(u(np.full(HUB_DEGREE, hub)), u(spokes), 30.0, 0.01)
    hub_bonds["uid_a"][::2], hub_bonds["uid_b"][::2] = hub_bonds["uid_b"][::2].copy(), hub_bonds["uid_a"][::2].copy()
    parts.append(hub_bonds)                                                        # the hub on either side
    parts.append(M.pairs([u(s + 1)], [u(5)], 1.0, 1.0))                             # a leaf: s + 1 has this bond only
    parts.append(np.repeat(M.pairs([u(s + 2)], [u(s + 3)], 1.0, 0.75), 2))          # the same bond twice
    parts.append(M.pairs([u(7), 0xFFFFFFF0, 3], [0xFFFFFFF0, u(8), 5], 1.0, 1.0, 0.001))   # uids no particle has
    anchored = rng.choice(s, 50, replace=False)
    parts.append(M.anchors(u(anchored), pos[anchored] + rng.uniform(-2, 2, (50, 2)).astype(F32), rng.uniform(0, 1, 50),
                           rng.uniform(0, 1, 50)))
    pos[s + 5] = pos[s + 4]                                                        # coincident centres
    parts.append(M.pairs([u(s + 4)], [u(s + 5)], 1.0, 1.0, 0.5))
    parts.append(M.anchors([u(s + 4)], [pos[s + 4]], 1.0, 1.0, 0.5))                # and an anchor on its particle
    odd = [(NAN, 100.0), (100.0, NAN), (INF, 100.0), (-INF, -INF), (1e30, 100.0), (-3e38, 3e38)]
    for j, p in enumerate(odd):
        pos[s + 6 + j] = p
    parts.append(M.pairs(u(np.arange(s + 6, s + 12)), u(np.arange(20, 26)), 1.0, 1.0, 2.0))  # left alone, not broken
    parts.append(M.anchors(u(np.arange(s + 6, s + 12)), np.full((6, 2), 50.0, F32), 1.0, 1.0, 2.0))
    # breaks in the first relaxation: 10 apart, max_length 4
    pos[s + 12], pos[s + 13] = (150.0, 190.0), (160.0, 190.0)
    parts.append(M.pairs([u(s + 12)], [u(s + 13)], 1.0, 1.0, 4.0))
    # breaks in the third: P is drawn towards an anchor 16 away by a quarter of the rest per relaxation (4, 7, 9.25); Q,
    # 2 behind it, holds it by a bond of stiffness 0 and max_length 10, judged behind the anchor (the next colour at P):
    # 6, 9, 11.25 > 10
    pos[s + 14], pos[s + 15] = (100.0, 195.0), (98.0, 195.0)
    parts.append(M.anchors([u(s + 14)], [(116.0, 195.0)], 0.0, 0.25))
    parts.append(M.pairs([u(s + 15)], [u(s + 14)], 2.0, 0.0, 10.0))
    # pulled across the world's edge: the clamp is seen
    pos[s + 16], pos[s + 17] = (2.0, 150.0), (198.0, 198.5)
    parts.append(M.anchors([u(s + 16), u(s + 17)], [(-20.0, 150.0), (230.0, 260.0)], 0.0, 1.0))
    parts.append(M.pairs([u(full - 1)], [u(9)], 3.0, 0.5))                          # (absent when n = 3999)
    bonds = np.concatenate(parts)
    third = len(bonds) - 4                                                         # the bond that breaks in the third
    return pos[:n], rad[:n], uids[:n], bonds, third


# ---- the table the C++ definition replays -----------------------------------------------------------------------------
TABLE_N, TABLE_ITERATIONS = 3999, 3


def table_text():
    """hostile_scene(TABLE_N) and what a coloured pass of TABLE_ITERATIONS relaxations makes of it, every float as the
    hex of its bits: a header line, n particle lines (uid, radius, x, y, x', y'), k bond lines (the eight fields of
    gpe_bond, colour, broken afterwards)."""
    pos, rad, uids, bonds, _ = hostile_scene(TABLE_N)
    col = colours(bonds)
    out, broken = apply(pos, rad, uids, bonds, np.zeros(len(bonds), bool), TABLE_ITERATIONS, WORLD, col)
    h = lambda a: np.ascontiguousarray(a, F32).view(U32)
    lines = ["%d %d %d %08x %08x" % (len(pos), len(bonds), TABLE_ITERATIONS, h([WORLD[0]])[0], h([WORLD[1]])[0])]
    P, O, R = h(pos), h(out), h(rad)
    for i in range(len(pos)):
        lines.append("%u %08x %08x %08x %08x %08x" % (uids[i], R[i], P[i, 0], P[i, 1], O[i, 0], O[i, 1]))
    for j, q in enumerate(bonds):
        f = h([q["rest_length"], q["stiffness"], q["max_length"], q["anchor_x"], q["anchor_y"]])
        lines.append("%u %u %08x %08x %08x %u %08x %08x %d %d" % (q["uid_a"], q["uid_b"], f[0], f[1], f[2], q["flags"],
                                                                 f[3], f[4], col[j], broken[j]))
    return "\n".join(lines) + "\n"
