"""The numpy float32 restatement of the distance bonds' pass (include/gpe.h "distance bonds", csrc/k_bond.h): every
bond judged from the positions a relaxation starts with, in the exact operation order of the header, one binary32
rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are correctly
rounded); a particle's corrections added in ascending bond index.  No graph, no node table: the uids are looked up
afresh in every relaxation.  TEST INFRASTRUCTURE ONLY.

relax() is one relaxation, apply() a pass of `iterations` of them; Twin is a colliders Twin (an OracleModel with a
collider set) that also holds a bond set the way a context does: step = oracle step -> bonds -> colliders."""
import numpy as np

from tests import _colliders_model as CM
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
UID_ABSENT = 0xFFFFFFFF
BOND_ANCHOR, BOND_BROKEN = 1, 2
BONDS_MAX, BOND_MAX_DEGREE, BOND_ITER_MAX = 4194304, 1024, 32
# gpe_bond, field for field (32 bytes)
BOND_DTYPE = np.dtype([("uid_a", U32), ("uid_b", U32), ("rest_length", F32), ("stiffness", F32), ("max_length", F32),
                       ("flags", U32), ("anchor_x", F32), ("anchor_y", F32)])
assert BOND_DTYPE.itemsize == 32


def pairs(uid_a, uid_b, rest_length, stiffness=1.0, max_length=0.0):
    ua = np.asarray(uid_a, U32).reshape(-1)
    rows = np.zeros(len(ua), BOND_DTYPE)
    rows["uid_a"], rows["uid_b"] = ua, uid_b
    rows["rest_length"], rows["stiffness"], rows["max_length"] = rest_length, stiffness, max_length
    return rows


def anchors(uids, points, rest_length=0.0, stiffness=1.0, max_length=0.0):
    ua = np.asarray(uids, U32).reshape(-1)
    pts = np.asarray(points, F32).reshape(-1, 2)
    rows = np.zeros(len(ua), BOND_DTYPE)
    rows["uid_a"], rows["uid_b"], rows["flags"] = ua, UID_ABSENT, BOND_ANCHOR
    rows["rest_length"], rows["stiffness"], rows["max_length"] = rest_length, stiffness, max_length
    rows["anchor_x"], rows["anchor_y"] = pts[:, 0], pts[:, 1]
    return rows


def slots_of(uids, query):
    """the storage index of every queried uid, -1 where no particle has it"""
    uids = np.asarray(uids, U32)
    query = np.asarray(query, U32)
    order = np.argsort(uids, kind="stable")
    su = uids[order]
    at = np.searchsorted(su, query)
    at[at == len(su)] = 0
    return np.where(su[at] == query, order[at], -1).astype(np.int64)


def corrections(pos, uids, bonds, broken):
    """One relaxation's bond phase -> (acts bool[k], breaks bool[k], cx, cy f32[k], slot_a, slot_b i64[k], anchor bool[k]);
    cx, cy are meaningless where acts is False."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    anchor = (bonds["flags"] & BOND_ANCHOR) != 0
    sa = slots_of(uids, bonds["uid_a"])
    sb = np.where(anchor, 0, slots_of(uids, bonds["uid_b"]))
    present = (sa >= 0) & (sb >= 0)
    ia, ib = np.where(present, sa, 0), np.where(present, sb, 0)
    ax, ay = p[ia, 0], p[ia, 1]
    bx = np.where(anchor, bonds["anchor_x"], p[ib, 0]).astype(F32)
    by = np.where(anchor, bonds["anchor_y"], p[ib, 1]).astype(F32)
    rest = np.where(bonds["rest_length"] == 0, F32(0), bonds["rest_length"]).astype(F32)      # -0.0 is stored as +0
    maxl = bonds["max_length"].astype(F32)
    w = np.where(anchor, bonds["stiffness"], F32(0.5) * bonds["stiffness"]).astype(F32)
    with np.errstate(all="ignore"):
        dx = bx - ax
        dy = by - ay
        dxx = dx * dx
        dyy = dy * dy
        h = dxx + dyy
        d = np.sqrt(h)
        ok = present & ~np.asarray(broken, bool) & (d > F32(0)) & (d < F32(np.inf))
        breaks = ok & (maxl > F32(0)) & (d > maxl)
        acts = ok & ~breaks
        safe = np.where(acts, d, F32(1))
        e = d - rest
        f = e / safe
        g = f * w
        cx = (g * dx).astype(F32)
        cy = (g * dy).astype(F32)
    return acts, breaks, cx, cy, sa, sb, anchor


def relax(pos, rad, uids, bonds, broken, world):
    """One relaxation -> (new pos f32[n, 2], broken bool[k], moved bool[n])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    n = len(r)
    acts, breaks, cx, cy, sa, sb, anchor = corrections(p, uids, bonds, broken)
    j = np.nonzero(acts)[0]
    jb = np.nonzero(acts & ~anchor)[0]
    part = np.concatenate([sa[j], sb[jb]])
    bond = np.concatenate([j, jb])
    vx = np.concatenate([cx[j], -cx[jb]]).astype(F32)
    vy = np.concatenate([cy[j], -cy[jb]]).astype(F32)
    order = np.lexsort((bond, part))                                   # by particle, then ascending bond index
    part, vx, vy = part[order], vx[order], vy[order]
    first = np.searchsorted(part, part, side="left")
    rank = np.arange(len(part)) - first
    acc = np.zeros((n, 2), F32)                                        # +0.0f
    moved = np.zeros(n, bool)
    moved[part] = True
    with np.errstate(all="ignore"):
        for level in range(int(rank.max()) + 1 if len(rank) else 0):   # one addition per particle and level, in order
            sel = rank == level
            acc[part[sel], 0] = acc[part[sel], 0] + vx[sel]
            acc[part[sel], 1] = acc[part[sel], 1] + vy[sel]
        W, H = F32(world[0]), F32(world[1])
        qx = p[:, 0] + acc[:, 0]
        qy = p[:, 1] + acc[:, 1]
        x = CM.clamp_f(qx, r, W - r)
        y = CM.clamp_f(qy, r, H - r)
    out = p.copy()
    out[moved, 0] = x[moved]
    out[moved, 1] = y[moved]
    return out, np.asarray(broken, bool) | breaks, moved


def apply(pos, rad, uids, bonds, broken, iterations, world):
    """A pass: `iterations` relaxations -> (new pos, broken)."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    broken = np.asarray(broken, bool).copy()
    for _ in range(iterations):
        p, broken, _ = relax(p, rad, uids, bonds, broken, world)
    return p, broken


def node_count(bonds):
    anchor = (bonds["flags"] & BOND_ANCHOR) != 0
    return len(np.unique(np.concatenate([bonds["uid_a"], bonds["uid_b"][~anchor]])))


class Twin(CM.Twin):
    """A colliders Twin with the bonds of a context: a bonds pass, then the colliders' pass, after every step of step()
    / run(), none after the module calls; the set and its broken flags survive everything but set_bonds."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bonds = np.zeros(0, BOND_DTYPE)
        self.bond_iterations = 1
        self.broken = np.zeros(0, bool)
        self.bond_passes = 0

    def set_bonds(self, bonds, iterations=1):
        b = np.array(bonds, BOND_DTYPE).reshape(-1)
        self.broken = (b["flags"] & BOND_BROKEN) != 0                  # a bond given broken starts broken
        b["flags"] &= ~U32(BOND_BROKEN)
        for name in ("rest_length", "max_length"):
            b[name] = np.where(b[name] == 0, F32(0), b[name])          # -0.0 is stored as +0
        self.bonds, self.bond_iterations, self.bond_passes = b, iterations, 0

    def apply_bonds(self):
        if len(self.bonds) == 0 or self.uids is None:
            return
        self._pull()
        self.pos, self.broken = apply(self.pos, self.radius, self.uids, self.bonds, self.broken, self.bond_iterations,
                                      self.world)
        self.bond_passes += 1

    def bonds_info(self):
        k = len(self.bonds)
        if k == 0:
            return dict(iterations=0, k=0, nodes=0, passes=0, live=0, broken=0)
        nb = int(self.broken.sum())
        return dict(iterations=self.bond_iterations, k=k, nodes=node_count(self.bonds), passes=self.bond_passes,
                    live=k - nb, broken=nb)

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_bonds()
        self.apply_colliders()
