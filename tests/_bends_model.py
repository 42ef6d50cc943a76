"""The numpy float32 restatement of the bend constraints' pass (include/gpe.h "bend constraints", csrc/k_bend.h): every
bend judged from the positions a relaxation starts with, in the exact operation order of the header, one binary32
rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are correctly
rounded); a particle's shares added in ascending bend index, the hinge's formed as -(da + dc) where it is added.  No
graph, no node table: the uids are looked up afresh in every relaxation.  TEST INFRASTRUCTURE ONLY.

relax() is one relaxation, apply() a pass of `iterations` of them; Twin is a bonds Twin (an OracleModel with colliders
and bonds) that also holds a bend set the way a context does: step = oracle step -> bends -> bonds -> colliders."""
import numpy as np

from tests import _bonds_model as BM
from tests import _colliders_model as CM
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
UID_ABSENT = 0xFFFFFFFF
BENDS_MAX, BEND_MAX_DEGREE, BEND_ITER_MAX = 4194304, 1024, 32
# gpe_bend, field for field (32 bytes)
BEND_DTYPE = np.dtype([("uid_a", U32), ("uid_b", U32), ("uid_c", U32), ("rest_cos", F32), ("rest_sin", F32),
                       ("stiffness", F32), ("flags", U32), ("reserved", U32)])
assert BEND_DTYPE.itemsize == 32
slots_of = BM.slots_of


def bends(uid_a, uid_b, uid_c, angle, stiffness=1.0):
    """rows that hold the angle from (a - b) to (c - b) at `angle` radians: cos and sin in float64, rounded once"""
    ua = np.asarray(uid_a, U32).reshape(-1)
    rows = np.zeros(len(ua), BEND_DTYPE)
    rows["uid_a"], rows["uid_b"], rows["uid_c"] = ua, uid_b, uid_c
    theta = np.broadcast_to(np.asarray(angle, np.float64), ua.shape)
    rows["rest_cos"], rows["rest_sin"], rows["stiffness"] = np.cos(theta), np.sin(theta), stiffness
    return rows


def captured(pos, uids, triples, stiffness=1.0):
    """State.bends_from_positions: the rest angles are the angles the particles hold, float64 rounded once"""
    t = np.asarray(triples, U32).reshape(-1, 3)
    s = slots_of(uids, t.reshape(-1)).reshape(-1, 3)
    assert (s >= 0).all()
    p = np.asarray(pos, F32).reshape(-1, 2).astype(np.float64)[s]
    u, v = p[:, 0] - p[:, 1], p[:, 2] - p[:, 1]
    den = np.sqrt((u * u).sum(axis=1) * (v * v).sum(axis=1))
    rows = np.zeros(len(t), BEND_DTYPE)
    rows["uid_a"], rows["uid_b"], rows["uid_c"] = t[:, 0], t[:, 1], t[:, 2]
    with np.errstate(all="ignore"):                                    # (an arm of length 0: NaN, which a context refuses)
        rows["rest_cos"] = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) / den
        rows["rest_sin"] = (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]) / den
    rows["stiffness"] = stiffness
    return rows


def stored(rows):
    """the set as a context keeps it: -0.0 in rest_cos / rest_sin / stiffness is stored as +0"""
    b = np.array(rows, BEND_DTYPE).reshape(-1)
    for name in ("rest_cos", "rest_sin", "stiffness"):
        b[name] = np.where(b[name] == 0, F32(0), b[name])
    return b


def rule(ax, ay, bx, by, cx, cy, rc, rs, stiffness):
    """k_bend.h bend_correction over arrays -> (acts bool, s, dax, day, dcx, dcy f32); the corrections are meaningless
    where acts is False.  Every line is one line of the header."""
    ax, ay, bx, by, cx, cy, rc, rs, stiffness = (np.asarray(v, F32) for v in (ax, ay, bx, by, cx, cy, rc, rs, stiffness))
    one = F32(1)
    with np.errstate(all="ignore"):
        ux = ax - bx; uy = ay - by; vx = cx - bx; vy = cy - by
        lu = ux * ux + uy * uy
        lv = vx * vx + vy * vy
        tx = rc * ux - rs * uy
        ty = rs * ux + rc * uy
        cr = tx * vy - ty * vx
        dt = tx * vx + ty * vy
        den = np.sqrt(lu * lv)
        ok = (lu > 0) & (lv > 0) & (den > 0) & (den < F32(np.inf))
        s = cr / np.where(ok, den, one)
        s = np.where(dt < 0, np.where(cr < 0, -one, one), s).astype(F32)
        ok = ok & ~(s != s)
        slu, slv = np.where(ok, lu, one), np.where(ok, lv, one)
        gax = uy / slu; gay = -ux / slu
        gcx = -vy / slv; gcy = vx / slv
        gbx = -(gax + gcx); gby = -(gay + gcy)
        q = ((gax * gax + gay * gay) + (gcx * gcx + gcy * gcy)) + (gbx * gbx + gby * gby)
        ok = ok & (q > 0) & (q < F32(np.inf))
        m = s * stiffness
        lam = -m / np.where(ok, q, one)
        dax = lam * gax; day = lam * gay
        dcx = lam * gcx; dcy = lam * gcy
    return ok, s, dax.astype(F32), day.astype(F32), dcx.astype(F32), dcy.astype(F32)


def corrections(pos, uids, bends):
    """One relaxation's bend phase -> (acts bool[k], s, dax, day, dcx, dcy f32[k], slots i64[k, 3])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    b = stored(bends)
    slots = np.stack([slots_of(uids, b["uid_a"]), slots_of(uids, b["uid_b"]), slots_of(uids, b["uid_c"])], axis=1)
    slots = slots.reshape(-1, 3)
    present = (slots >= 0).all(axis=1)
    i = np.where(present[:, None], slots, 0)
    acts, s, dax, day, dcx, dcy = rule(p[i[:, 0], 0], p[i[:, 0], 1], p[i[:, 1], 0], p[i[:, 1], 1], p[i[:, 2], 0],
                                       p[i[:, 2], 1], b["rest_cos"], b["rest_sin"], b["stiffness"])
    return acts & present, s, dax, day, dcx, dcy, slots


def shares(pos, uids, bends):
    """-> (part i64, bend i64, vx, vy f32): every share of an acting bend, ordered by particle, then ascending bend index"""
    acts, _, dax, day, dcx, dcy, slots = corrections(pos, uids, bends)
    j = np.nonzero(acts)[0]
    with np.errstate(all="ignore"):
        hx = -(dax[j] + dcx[j])                                        # the hinge's share, formed where it is added
        hy = -(day[j] + dcy[j])
    part = np.concatenate([slots[j, 0], slots[j, 1], slots[j, 2]])
    bend = np.concatenate([j, j, j])
    vx = np.concatenate([dax[j], hx, dcx[j]]).astype(F32)
    vy = np.concatenate([day[j], hy, dcy[j]]).astype(F32)
    order = np.lexsort((bend, part))
    return part[order], bend[order], vx[order], vy[order]


def relax(pos, rad, uids, bends, world):
    """One relaxation -> (new pos f32[n, 2], moved bool[n])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    n = len(r)
    part, _, vx, vy = shares(p, uids, bends)
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
    return out, moved


def apply(pos, rad, uids, bends, iterations, world):
    """A pass: `iterations` relaxations -> new pos."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    for _ in range(iterations):
        p, _ = relax(p, rad, uids, bends, world)
    return p


def node_count(bends):
    return len(np.unique(np.concatenate([bends["uid_a"], bends["uid_b"], bends["uid_c"]])))


def deviation(pos, uids, bends):
    """float64: the signed angle (radians) by which each bend is off its rest angle, NaN where a uid is absent"""
    b = np.asarray(bends, BEND_DTYPE).reshape(-1)
    p = np.asarray(pos, np.float64).reshape(-1, 2)
    s = np.stack([slots_of(uids, b["uid_a"]), slots_of(uids, b["uid_b"]), slots_of(uids, b["uid_c"])], axis=1)
    ok = (s >= 0).all(axis=1)
    s = np.where(ok[:, None], s, 0)
    u, v = p[s[:, 0]] - p[s[:, 1]], p[s[:, 2]] - p[s[:, 1]]
    rc, rs = b["rest_cos"].astype(np.float64), b["rest_sin"].astype(np.float64)
    tx, ty = rc * u[:, 0] - rs * u[:, 1], rs * u[:, 0] + rc * u[:, 1]
    return np.where(ok, np.arctan2(tx * v[:, 1] - ty * v[:, 0], tx * v[:, 0] + ty * v[:, 1]), np.nan)


class Twin(BM.Twin):
    """A bonds Twin with the bends of a context: a bends pass, then the bonds' pass, then the colliders' pass, after
    every step of step() / run(), none after the module calls; the set survives everything but set_bends."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bends = np.zeros(0, BEND_DTYPE)
        self.bend_iterations = 1
        self.bend_passes = 0

    def set_bends(self, bends, iterations=1):
        self.bends, self.bend_iterations, self.bend_passes = stored(bends), iterations, 0

    def apply_bends(self):
        if len(self.bends) == 0 or self.uids is None:
            return
        self._pull()
        self.pos = apply(self.pos, self.radius, self.uids, self.bends, self.bend_iterations, self.world)
        self.bend_passes += 1

    def bends_info(self):
        k = len(self.bends)
        if k == 0:
            return dict(iterations=0, k=0, nodes=0, passes=0)
        return dict(iterations=self.bend_iterations, k=k, nodes=node_count(self.bends), passes=self.bend_passes)

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_bends()
        self.apply_bonds()
        self.apply_colliders()
