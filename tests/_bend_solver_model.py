"""The numpy float32 restatement of the bends' coloured solver (include/gpe.h "the bends' solver", csrc/bend_colours.h,
csrc/k_bend.h): the greedy colouring in plain Python, a relaxation as a sweep of the colours in order, every colour
vectorised over its bends -- no two of them share a particle -- through tests/_bends_model.rule, every bend moving its
three particles itself (p + share, then the world clamp with the stored radius).  TEST INFRASTRUCTURE ONLY.

colours() colours a set, relax() is one coloured relaxation, apply() a pass of `iterations` of them.  Mixin gives a twin
that holds bends (tests/_bends_model.Twin and everything above it) the solver's mode; Twin is the bends' twin with it.
hostile_scene() is about 3000 bends over 4000 particles with everything a bend can meet; table_text() the table
tests/cpp/bend_colours_tests.cpp replays."""
import math

import numpy as np

from tests import _bends_model as M
from tests import _colliders_model as CM

F32 = np.float32
U32 = np.uint32
COLOURS_MAX = 64
JACOBI, COLOURED = 0, 1
NAN, INF, PI = float("nan"), float("inf"), math.pi
WORLD = (200.0, 200.0)


def colours(bends):
    """colour[j] = the least c >= 0 no bend of lower index has taken at uid_a, at the hinge uid_b or at uid_c -> int64[k]"""
    taken = {}
    out = np.zeros(len(bends), np.int64)
    for j, nodes in enumerate(zip(bends["uid_a"].tolist(), bends["uid_b"].tolist(), bends["uid_c"].tolist())):
        mask = 0
        for e in nodes:
            mask |= taken.get(e, 0)
        c = 0
        while (mask >> c) & 1:
            c += 1
        for e in nodes:
            taken[e] = taken.get(e, 0) | (1 << c)
        out[j] = c
    return out


def colour_info(bends):
    """-> (colours, largest_colour) as gpe_get_bend_solver_info reports them"""
    col = colours(bends)
    if len(col) == 0:
        return 0, 0
    return int(col.max()) + 1, int(np.bincount(col).max())


def slots(uids, bends):
    """-> i64[k, 3]: the storage slots of a, the hinge and c; -1 where no particle has the uid"""
    return np.stack([M.slots_of(uids, bends["uid_a"]), M.slots_of(uids, bends["uid_b"]),
                     M.slots_of(uids, bends["uid_c"])], axis=1).reshape(-1, 3)


def relax(pos, rad, uids, bends, world, col, at=None):
    """One coloured relaxation -> new pos f32[n, 2]."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    b = M.stored(bends)
    at = slots(uids, b) if at is None else at
    present = (at >= 0).all(axis=1)
    W, H = F32(world[0]), F32(world[1])
    for c in range(int(col.max()) + 1 if len(col) else 0):
        idx = np.nonzero((col == c) & present)[0]                      # ascending bend index
        i, q = at[idx], b[idx]
        acts, _, dax, day, dcx, dcy = M.rule(p[i[:, 0], 0], p[i[:, 0], 1], p[i[:, 1], 0], p[i[:, 1], 1], p[i[:, 2], 0],
                                             p[i[:, 2], 1], q["rest_cos"], q["rest_sin"], q["stiffness"])
        i, dax, day, dcx, dcy = i[acts], dax[acts], day[acts], dcx[acts], dcy[acts]
        assert len(np.unique(i)) == i.size                             # within a colour no position has two writers
        with np.errstate(all="ignore"):
            hx = -(dax + dcx)                                          # the hinge's share: k_bend.h bend_hinge_share
            hy = -(day + dcy)
            for s, sx, sy in ((i[:, 0], dax, day), (i[:, 2], dcx, dcy), (i[:, 1], hx, hy)):
                qx = p[s, 0] + sx
                qy = p[s, 1] + sy
                x = CM.clamp_f(qx, r[s], W - r[s])
                y = CM.clamp_f(qy, r[s], H - r[s])
                p[s, 0], p[s, 1] = x, y
    return p


def apply(pos, rad, uids, bends, iterations, world, col=None):
    """A coloured pass: `iterations` relaxations -> new pos."""
    col = colours(bends) if col is None else col
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    at = slots(uids, M.stored(bends))
    for _ in range(iterations):
        p = relax(p, rad, uids, bends, world, col, at)
    return p


class Refused(Exception):
    """what a context answers with GPE_ERR_INVALID_ARG: the set needs more than COLOURS_MAX colours"""


class Mixin:
    """In front of a twin that holds bends: the solver's mode, kept by set_bends and everything else."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bend_solver = JACOBI
        self.bend_colour = np.zeros(0, np.int64)
        self.bend_solver_passes = 0

    def _bends_coloured(self, bends):
        col = colours(bends)
        if len(col) and int(col.max()) + 1 > COLOURS_MAX:
            raise Refused(int(col.max()) + 1)
        return col

    def set_bend_solver(self, solver):
        mode = {"jacobi": JACOBI, "coloured": COLOURED}[solver]
        col = self._bends_coloured(self.bends) if mode == COLOURED else np.zeros(0, np.int64)   # (refused: nothing changes)
        self.bend_solver, self.bend_colour, self.bend_solver_passes = mode, col, 0

    def set_bends(self, bends, iterations=1):
        b = np.array(bends, M.BEND_DTYPE).reshape(-1)
        col = self._bends_coloured(b) if self.bend_solver == COLOURED else np.zeros(0, np.int64)  # (refused: the old set stays)
        super().set_bends(bends, iterations)
        self.bend_colour = col

    def apply_bends(self):
        if self.bend_solver != COLOURED:
            return super().apply_bends()
        if len(self.bends) == 0 or self.uids is None:
            return
        self._pull()
        self.pos = apply(self.pos, self.radius, self.uids, self.bends, self.bend_iterations, self.world, self.bend_colour)
        self.bend_passes += 1
        self.bend_solver_passes += 1

    def bend_solver_info(self):
        """gpe_get_bend_solver_info without form and lds_nodes_max, which are the device's"""
        c, largest = colour_info(self.bends) if self.bend_solver == COLOURED else (0, 0)
        return dict(mode=self.bend_solver, colours=c, largest_colour=largest, passes=self.bend_solver_passes)


class Twin(Mixin, M.Twin):
    """tests/_bends_model.Twin with the solver's mode"""


# ---- the hostile scene ----------------------------------------------------------------------------------------------
HUB_DEGREE = 20
RESTS = np.array([PI, -PI, PI / 2, -PI / 2, 0.3, -2.5, 0.0, 3.0])
SPECIAL = 60                                                           # the storage slots at the end with a special role


def hostile_scene(n):
    """n particles on a jittered 64-wide lattice of spacing 3 with uids that are no storage indices, and about 3000
    bends: triples along rows and columns and round corners with mixed rest angles (most are more than 90 degrees off
    theirs), a triple listed twice, uids no particle has, NaN, inf and 1e20 positions, a coincident pair, an arm whose
    squared length underflows, an exact fold-back, a corner and a chain at the world's edge whose particles are clamped
    bend after bend, a hinge shared by HUB_DEGREE bends.  The last SPECIAL storage slots hold the particles with a
    special role.  -> (pos, rad, uids, bends)"""
    rng = np.random.default_rng(n)
    full = 4000
    i = np.arange(full)
    pos = np.stack([4.0 + 3.0 * (i % 64), 4.0 + 3.0 * (i // 64)], axis=1) + rng.uniform(-0.4, 0.4, (full, 2))
    pos = pos.astype(F32)
    rad = np.full(full, 0.5, F32)
    uids = (rng.permutation(full).astype(np.uint64) * 7919 + 11).astype(U32)     # distinct, far above n, unordered
    s = full - SPECIAL
    u = lambda slot: uids[np.asarray(slot)]
    parts = []

    def triples(a, b, c, stiffness=None, rest=None):
        k = len(a)
        st = rng.choice([0.0, 0.1, 0.25, 0.5, 1.0], k) if stiffness is None else stiffness
        return M.bends(u(a), u(b), u(c), rng.choice(RESTS, k) if rest is None else rest, st)

    a = rng.integers(0, s - 130, 3000)
    a = a[(a % 64) < 62]
    kind = rng.integers(0, 3, len(a))
    b = np.where(kind == 0, a + 1, np.where(kind == 1, a + 64, a))
    c = np.where(kind == 0, a + 2, np.where(kind == 1, a + 128, a + 64))
    a2 = np.where(kind == 2, a + 1, a)
    parts.append(triples(a2, b, c))
    parts.append(np.repeat(triples([s + 0], [s + 1], [s + 2], 0.25), 2))            # the same bend twice
    parts.append(M.bends([u(7), 0xFFFFFFF0, u(3)], [0xFFFFFFF0, u(8), u(5)], [u(9), u(10), 0xFFFFFFF1], PI, 1.0))
    pos[s + 4] = (NAN, 100.0)
    pos[s + 6] = pos[s + 5]                                                        # coincident centres
    pos[s + 7], pos[s + 8] = (INF, 50.0), (1e20, 50.0)
    parts.append(triples([s + 4, 20, 21, s + 5, 22, s + 7, 23], [24, s + 4, 25, s + 6, s + 5, 26, s + 8],
                         [27, 28, s + 4, 29, s + 6, 30, 31], 1.0))
    # a right angle at the world's corner with a straight rest: a and c are pushed out across the edge, and clamped
    pos[s + 10], pos[s + 11], pos[s + 12] = (2.75, 199.25), (0.75, 199.25), (0.75, 197.25)
    flat = M.bends([u(s + 10)], [u(s + 11)], [u(s + 12)], PI, 1.0)
    flat["rest_sin"] = -0.0                                                        # (the exact (-1, 0); -0.0 is stored as +0)
    parts.append(flat)
    # an arm whose squared length underflows to 0: inert, all three keep every bit though they lie outside the clamp
    pos[s + 14], pos[s + 15], pos[s + 16] = (1e-30, 0.0), (0.0, 0.0), (0.0, 5.0)
    parts.append(triples([s + 14], [s + 15], [s + 16], 1.0, PI))
    # an exact fold-back: both arms along +x, a straight rest given as the exact (-1, 0): cr == 0, dt < 0, it turns +1
    pos[s + 17], pos[s + 18], pos[s + 19] = (52.0, 195.0), (50.0, 195.0), (54.0, 195.0)
    fold = M.bends([u(s + 17)], [u(s + 18)], [u(s + 19)], PI, 0.5)
    fold["rest_sin"] = 0.0
    parts.append(fold)
    # a hinge shared by HUB_DEGREE bends with otherwise distinct ends: HUB_DEGREE colours at least
    spokes = rng.choice(s - 130, 2 * HUB_DEGREE, replace=False)
    pos[s + 20] = (100.0, 196.0)
    parts.append(triples(spokes[::2], np.full(HUB_DEGREE, s + 20), spokes[1::2], 0.05))
    # a chain along the left edge, bent into the wall: its inner particles sit in two bends and are clamped after each
    pos[s + 22], pos[s + 23], pos[s + 24], pos[s + 25] = (0.75, 100.0), (0.75, 102.0), (1.5, 104.0), (0.75, 106.0)
    parts.append(triples([s + 22, s + 23], [s + 23, s + 24], [s + 24, s + 25], 1.0, PI))
    parts.append(triples([full - 1], [40], [41], 0.5))                              # (absent when n = 3999)
    bends = np.concatenate(parts)
    return pos[:n], rad[:n], uids[:n], bends


# ---- the table the C++ definition replays -----------------------------------------------------------------------------
TABLE_N, TABLE_ITERATIONS = 3999, 3


def table_text():
    """hostile_scene(TABLE_N) and what a coloured pass of TABLE_ITERATIONS relaxations makes of it, every float as the
    hex of its bits: a header line, n particle lines (uid, radius, x, y, x', y'), k bend lines (uid_a, uid_b, uid_c,
    rest_cos, rest_sin, stiffness, colour)."""
    pos, rad, uids, bends = hostile_scene(TABLE_N)
    col = colours(bends)
    out = apply(pos, rad, uids, bends, TABLE_ITERATIONS, WORLD, col)
    h = lambda a: np.ascontiguousarray(a, F32).view(U32)
    lines = ["%d %d %d %08x %08x" % (len(pos), len(bends), TABLE_ITERATIONS, h([WORLD[0]])[0], h([WORLD[1]])[0])]
    P, O, R = h(pos), h(out), h(rad)
    for i in range(len(pos)):
        lines.append("%u %08x %08x %08x %08x %08x" % (uids[i], R[i], P[i, 0], P[i, 1], O[i, 0], O[i, 1]))
    for j, q in enumerate(bends):
        f = h([q["rest_cos"], q["rest_sin"], q["stiffness"]])
        lines.append("%u %u %u %08x %08x %08x %d" % (q["uid_a"], q["uid_b"], q["uid_c"], f[0], f[1], f[2], col[j]))
    return "\n".join(lines) + "\n"
