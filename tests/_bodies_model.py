"""The numpy float32 restatement of the rigid and soft bodies' pass (include/gpe.h "rigid and soft bodies",
csrc/k_body.h): shape matching per body in the exact operation order of the header, one binary32 rounding per
operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are correctly rounded); every
sum over members is the canonical sum S, whose order depends on the body's count alone.  No tables, no width classes:
the uids are looked up afresh in every pass.  Bodies of the same count are computed together, one row each.  TEST
INFRASTRUCTURE ONLY.

apply() is one pass; Twin is a bonds Twin (an OracleModel with colliders and bonds) that also holds a body set the way
a context does: step = oracle step -> bonds -> bodies -> colliders."""
import numpy as np

from tests import _bonds_model as BM
from tests import _colliders_model as CM
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
UID_ABSENT = 0xFFFFFFFF
BODY_BROKEN = 1
BODIES_MAX, BODY_MAX_MEMBERS, BODY_MEMBERS_MAX = 1048576, 4096, 16777216
# gpe_body, field for field (24 bytes)
BODY_DTYPE = np.dtype([("first", U32), ("count", U32), ("stiffness", F32), ("break_distance", F32), ("flags", U32),
                       ("reserved", U32)])
assert BODY_DTYPE.itemsize == 24
ACTS, BROKEN, INERT = 0, 1, 2


def rows(counts, stiffness=1.0, break_distance=0.0):
    """bodies of counts[i] members each, one behind the other in the member arrays"""
    counts = np.asarray(counts, U32).reshape(-1)
    out = np.zeros(len(counts), BODY_DTYPE)
    out["count"] = counts
    out["first"] = np.cumsum(counts, dtype=np.uint64) - counts
    out["stiffness"], out["break_distance"] = stiffness, break_distance
    return out


def width(count):
    g = 2
    while g < count and g < 64:
        g *= 2
    return g


def canon_sum(v):
    """S over the last axis of v f32[b, count] -> f32[b] (an absent member's entry is +0.0 already)."""
    v = np.ascontiguousarray(v, F32)
    b, count = v.shape
    G = width(count)
    rounds = -(-count // G)
    padded = np.zeros((b, rounds * G), F32)
    padded[:, :count] = v
    lanes = padded.reshape(b, rounds, G)
    partial = np.zeros((b, G), F32)                                    # +0.0f
    with np.errstate(all="ignore"):
        for t in range(rounds):                                        # lane l adds v_l, v_(l+G), ... in that order
            partial = partial + lanes[:, t, :]
        off = G // 2
        while off >= 1:
            partial = partial[:, :off] + partial[:, off:2 * off]
            off //= 2
    return partial[:, 0]


def match(rest, p, live, stiffness, bd):
    """Bodies of one count: rest, p f32[b, count, 2], live bool[b, count], stiffness, bd f32[b] ->
    (verdict u8[b], target f32[b, count, 2] before the clamp, pose f32[b, 4])."""
    b, count, _ = p.shape
    zero = F32(0)
    with np.errstate(all="ignore"):
        L = live.sum(axis=1)
        fL = L.astype(F32)
        m = lambda v: np.where(live, v, zero).astype(F32)
        rbx, rby = canon_sum(m(rest[:, :, 0])) / fL, canon_sum(m(rest[:, :, 1])) / fL
        cx, cy = canon_sum(m(p[:, :, 0])) / fL, canon_sum(m(p[:, :, 1])) / fL
        qx = rest[:, :, 0] - rbx[:, None]
        qy = rest[:, :, 1] - rby[:, None]
        dx = p[:, :, 0] - cx[:, None]
        dy = p[:, :, 1] - cy[:, None]
        a = qx * dx + qy * dy
        bb = qx * dy - qy * dx
        A, B = canon_sum(m(a)), canon_sum(m(bb))
        h = np.sqrt(A * A + B * B)
        fits = (L >= 2) & (h > zero) & (h < F32(np.inf))
        safe = np.where(fits, h, F32(1))
        co, si = A / safe, B / safe
        gx = cx[:, None] + (co[:, None] * qx - si[:, None] * qy)
        gy = cy[:, None] + (si[:, None] * qx + co[:, None] * qy)
        ex = gx - p[:, :, 0]
        ey = gy - p[:, :, 1]
        e2 = ex * ex + ey * ey
        bd2 = bd * bd                                                  # rounded once, as on the host
        breaks = fits & (bd > zero) & (live & (e2 > bd2[:, None])).any(axis=1)
        tx = p[:, :, 0] + stiffness[:, None] * ex
        ty = p[:, :, 1] + stiffness[:, None] * ey
    verdict = np.where(~fits, INERT, np.where(breaks, BROKEN, ACTS)).astype(np.uint8)
    pose = np.stack([cx, cy, co, si], axis=1).astype(F32)
    pose[verdict != ACTS] = np.nan
    return verdict, np.stack([tx, ty], axis=2).astype(F32), pose


def apply(pos, rad, uids, bodies, member_uid, member_rest, broken, world):
    """One pass -> (new pos f32[n, 2], broken bool[k], pose f32[k, 4], verdict u8[k]: ACTS / BROKEN (now or before) /
    INERT)."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    rest = np.ascontiguousarray(member_rest, F32).reshape(-1, 2)
    broken = np.asarray(broken, bool).copy()
    k = len(bodies)
    slot = BM.slots_of(uids, member_uid) if len(p) else np.full(len(member_uid), -1, np.int64)
    out = p.copy()
    pose = np.full((k, 4), np.nan, F32)
    verdict = np.full(k, BROKEN, np.uint8)
    W, H = F32(world[0]), F32(world[1])
    for count in np.unique(bodies["count"]):
        ids = np.nonzero((bodies["count"] == count) & ~broken)[0]
        if len(ids) == 0:
            continue
        member = bodies["first"][ids].astype(np.int64)[:, None] + np.arange(int(count))[None, :]
        s = slot[member]
        live = s >= 0
        at = np.where(live, s, 0)
        v, target, ps = match(rest[member], np.where(live[:, :, None], p[at], F32(0)).astype(F32), live,
                              bodies["stiffness"][ids].astype(F32), bodies["break_distance"][ids].astype(F32))
        verdict[ids], pose[ids] = v, ps
        broken[ids[v == BROKEN]] = True
        move = live & (v == ACTS)[:, None]
        dst = s[move]
        with np.errstate(all="ignore"):
            out[dst, 0] = CM.clamp_f(target[:, :, 0][move], r[dst], W - r[dst])
            out[dst, 1] = CM.clamp_f(target[:, :, 1][move], r[dst], H - r[dst])
    return out, broken, pose, verdict


class Twin(BM.Twin):
    """A bonds Twin with the bodies of a context: a bonds pass, a bodies pass, then the colliders' pass, after every
    step of step() / run(), none after the module calls; the set and its broken flags survive everything but
    set_bodies."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bodies = np.zeros(0, BODY_DTYPE)
        self.member_uid = np.zeros(0, U32)
        self.member_rest = np.zeros((0, 2), F32)
        self.bodies_broken = np.zeros(0, bool)
        self.body_passes = 0
        self.poses = np.zeros((0, 4), F32)

    def set_bodies(self, bodies, member_uid, member_rest):
        b = np.array(bodies, BODY_DTYPE).reshape(-1)
        self.bodies_broken = (b["flags"] & BODY_BROKEN) != 0           # a body given broken starts broken
        b["flags"] &= ~U32(BODY_BROKEN)
        b["break_distance"] = np.where(b["break_distance"] == 0, F32(0), b["break_distance"])   # -0.0 is stored as +0
        self.bodies, self.body_passes = b, 0
        self.member_uid = np.array(member_uid, U32).reshape(-1)
        self.member_rest = np.array(member_rest, F32).reshape(-1, 2)
        self.poses = np.full((len(b), 4), np.nan, F32)

    def apply_bodies(self):
        if len(self.bodies) == 0 or self.uids is None:
            return
        self._pull()
        self.pos, self.bodies_broken, self.poses, _ = apply(self.pos, self.radius, self.uids, self.bodies,
                                                            self.member_uid, self.member_rest, self.bodies_broken,
                                                            self.world)
        self.body_passes += 1

    def bodies_info(self):
        k = len(self.bodies)
        if k == 0:
            return dict(k=0, members=0, passes=0, live=0, broken=0)
        nb = int(self.bodies_broken.sum())
        return dict(k=k, members=len(self.member_uid), passes=self.body_passes, live=k - nb, broken=nb)

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_bonds()
        self.apply_bodies()
        self.apply_colliders()
