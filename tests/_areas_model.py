"""The numpy float32 restatement of the area constraints' pass (include/gpe.h "area constraints", csrc/k_area.h): every
loop judged from the positions a relaxation starts with, in the exact operation order of the header, one binary32
rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide is correctly rounded); both
sums over a loop's members the canonical sum S of the bodies (lane l of G adds v_l, v_(l+G), ... from +0.0f, then the
halving tree); a particle's shares added in ascending member index.  No tables, no node list: the uids are looked up
afresh in every relaxation.  TEST INFRASTRUCTURE ONLY.

relax() is one relaxation, apply() a pass of `iterations` of them; Twin is a bends Twin (an OracleModel with colliders,
bonds and bends) that also holds an area set the way a context does: step = oracle step -> bends -> areas -> bonds ->
colliders."""
import numpy as np

from tests import _bends_model as NM
from tests import _bonds_model as BM
from tests import _colliders_model as CM
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
UID_ABSENT = 0xFFFFFFFF
AREAS_MAX, AREA_MAX_MEMBERS, AREA_MEMBERS_MAX, AREA_MAX_DEGREE, AREA_ITER_MAX = 4194304, 4096, 16777216, 64, 32
# gpe_area, field for field (24 bytes)
AREA_DTYPE = np.dtype([("first", U32), ("count", U32), ("rest_area", F32), ("stiffness", F32), ("flags", U32),
                       ("reserved", U32)])
assert AREA_DTYPE.itemsize == 24
slots_of = BM.slots_of


def rows_for(counts, rest_area=0.0, stiffness=1.0):
    """rows whose member ranges tile [0, sum(counts)) in the order given"""
    counts = np.asarray(counts, np.int64).reshape(-1)
    rows = np.zeros(len(counts), AREA_DTYPE)
    rows["first"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else []
    rows["count"], rows["rest_area"], rows["stiffness"] = counts, rest_area, stiffness
    return rows


def shoelace64(p):
    """float64: the signed area of the polygon p[count, 2], taken from member 0"""
    q = np.asarray(p, np.float64)
    q = q - q[:1]
    nx, ny = np.roll(q[:, 0], -1), np.roll(q[:, 1], -1)
    return 0.5 * float((q[:, 0] * ny - nx * q[:, 1]).sum())


def captured(pos, uids, loops, stiffness=1.0, pressure=1.0):
    """State.areas_from_loops: the rest areas are the areas the particles enclose, float64 rounded once"""
    groups = [np.asarray(g, U32).reshape(-1) for g in loops]
    member_uid = np.concatenate(groups) if groups else np.zeros(0, U32)
    s = slots_of(uids, member_uid) if len(member_uid) else np.zeros(0, np.int64)
    assert (s >= 0).all()
    p = np.asarray(pos, F32).reshape(-1, 2)
    rows = rows_for([len(g) for g in groups], 0.0, stiffness)
    area = np.array([shoelace64(p[s[r["first"]:r["first"] + r["count"]]]) for r in rows], np.float64)
    rows["rest_area"] = area * np.broadcast_to(np.asarray(pressure, np.float64), area.shape)
    return rows, member_uid


def stored(rows):
    """the set as a context keeps it: -0.0 in rest_area / stiffness is stored as +0"""
    a = np.array(rows, AREA_DTYPE).reshape(-1)
    for name in ("rest_area", "stiffness"):
        a[name] = np.where(a[name] == 0, F32(0), a[name])
    return a


def width(count):
    g = 2
    while g < count and g < 64:
        g <<= 1
    return g


def canon_sum(v):
    """S over axis 1 of v f32[L, count]: the canonical sum of k_body.h -> f32[L]"""
    v = np.ascontiguousarray(v, F32)
    L, count = v.shape
    G = width(count)
    rounds = -(-count // G)
    pad = np.zeros((L, rounds * G), F32)           # (x + +0.0f == x for every x a sum from +0.0f holds)
    pad[:, :count] = v
    pad = pad.reshape(L, rounds, G)
    partial = np.zeros((L, G), F32)
    with np.errstate(all="ignore"):
        for t in range(rounds):
            partial = partial + pad[:, t, :]
        off = G // 2
        while off >= 1:
            partial = partial[:, :off] + partial[:, off:2 * off]
            off //= 2
    return partial[:, 0]


def rule(px, py, rest_area, stiffness):
    """k_area.h over L loops of one count whose members all have a particle: px, py f32[L, count] -> (acts bool[L],
    area, lam f32[L], cx, cy f32[L, count]); the corrections are meaningless where acts is False.  Every line is one
    line of the header."""
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    rest_area, stiffness = np.asarray(rest_area, F32), np.asarray(stiffness, F32)
    half, one, inf = F32(0.5), F32(1), F32(np.inf)
    with np.errstate(all="ignore"):
        qx = px - px[:, :1]
        qy = py - py[:, :1]
        nx, ny = np.roll(qx, -1, axis=1), np.roll(qy, -1, axis=1)
        mx, my = np.roll(qx, 1, axis=1), np.roll(qy, 1, axis=1)
        t = qx * ny - nx * qy
        A2 = canon_sum(t)
        area = half * A2
        C = area - rest_area
        gx = half * (ny - my)
        gy = half * (mx - nx)
        D = canon_sum(gx * gx + gy * gy)
        acts = (D > 0) & (D < inf) & (C > -inf) & (C < inf)
        s = C * stiffness
        lam = -(s / np.where(acts, D, one))
        cx = lam[:, None] * gx
        cy = lam[:, None] * gy
    return acts, area.astype(F32), lam.astype(F32), cx.astype(F32), cy.astype(F32)


def loop_phase(pos, uids, areas, member_uid):
    """One relaxation's loop phase -> (acts bool[k], value f32[k, 2] = (area, lambda) or NaNs, corr f32[members, 2],
    slots i64[members])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    a = stored(areas)
    member_uid = np.asarray(member_uid, U32).reshape(-1)
    slots = slots_of(uids, member_uid) if len(uids) else np.full(len(member_uid), -1, np.int64)
    k = len(a)
    acts = np.zeros(k, bool)
    value = np.full((k, 2), np.nan, F32)
    corr = np.zeros((len(member_uid), 2), F32)
    for count in np.unique(a["count"]):
        which = np.nonzero(a["count"] == count)[0]
        idx = a["first"][which].astype(np.int64)[:, None] + np.arange(int(count))[None, :]      # [L, count]
        s = slots[idx]
        whole = (s >= 0).all(axis=1)
        s = np.where(s >= 0, s, 0)
        ok, area, lam, cx, cy = rule(p[s, 0], p[s, 1], a["rest_area"][which], a["stiffness"][which])
        ok = ok & whole
        acts[which] = ok
        value[which[ok], 0], value[which[ok], 1] = area[ok], lam[ok]
        corr[idx, 0], corr[idx, 1] = cx, cy
    return acts, value, corr, slots


def shares(pos, uids, areas, member_uid):
    """-> (part i64, member i64, vx, vy f32, value): every share of an acting loop, ordered by particle, then ascending
    member index"""
    a = stored(areas)
    acts, value, corr, slots = loop_phase(pos, uids, a, member_uid)
    member_loop = np.zeros(len(slots), np.int64)
    for j, r in enumerate(a):
        member_loop[r["first"]:r["first"] + r["count"]] = j
    member = np.nonzero(acts[member_loop])[0] if len(slots) else np.zeros(0, np.int64)
    part = slots[member]
    order = np.lexsort((member, part))
    member, part = member[order], part[order]
    return part, member, corr[member, 0], corr[member, 1], value


def relax(pos, rad, uids, areas, member_uid, world):
    """One relaxation -> (new pos f32[n, 2], moved bool[n], value f32[k, 2])."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    n = len(r)
    part, _, vx, vy, value = shares(p, uids, areas, member_uid)
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
    return out, moved, value


def apply(pos, rad, uids, areas, member_uid, iterations, world, values=False):
    """A pass: `iterations` relaxations -> new pos (values: and the last relaxation's (area, lambda) per loop)."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2).copy()
    value = np.full((len(areas), 2), np.nan, F32)
    for _ in range(iterations):
        p, _, value = relax(p, rad, uids, areas, member_uid, world)
    return (p, value) if values else p


def node_count(member_uid):
    return len(np.unique(member_uid))


class Twin(NM.Twin):
    """A bends Twin with the areas of a context: the bends' pass, the areas' pass, the bonds' pass, then the colliders'
    pass, after every step of step() / run(), none after the module calls; the set survives everything but set_areas."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.areas = np.zeros(0, AREA_DTYPE)
        self.area_member_uid = np.zeros(0, U32)
        self.area_iterations = 1
        self.area_passes = 0
        self.area_value = np.zeros((0, 2), F32)

    def set_areas(self, areas, member_uid, iterations=1):
        self.areas, self.area_iterations, self.area_passes = stored(areas), iterations, 0
        self.area_member_uid = np.array(member_uid, U32).reshape(-1) if len(self.areas) else np.zeros(0, U32)
        self.area_value = np.full((len(self.areas), 2), np.nan, F32)

    def set_area_targets(self, first, rest_area):
        t = np.asarray(rest_area, F32).reshape(-1)
        self.areas["rest_area"][first:first + len(t)] = np.where(t == 0, F32(0), t)

    def apply_areas(self):
        if len(self.areas) == 0 or self.uids is None:
            return
        self._pull()
        if len(self.radius) == 0:
            return
        self.pos, self.area_value = apply(self.pos, self.radius, self.uids, self.areas, self.area_member_uid,
                                          self.area_iterations, self.world, values=True)
        self.area_passes += 1

    def areas_info(self):
        k = len(self.areas)
        if k == 0:
            return dict(iterations=0, k=0, members=0, nodes=0, passes=0)
        return dict(iterations=self.area_iterations, k=k, members=len(self.area_member_uid),
                    nodes=node_count(self.area_member_uid), passes=self.area_passes)

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_bends()
        self.apply_areas()
        self.apply_bonds()
        self.apply_colliders()
