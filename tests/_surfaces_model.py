"""The numpy float32 restatement of the surface materials (include/gpe.h "surface materials", csrc/k_surface.h): bounce
and Coulomb friction of the obstacle a pass picks, in the exact operation order of the header, one binary32 rounding
per operation, no FMA.  The winner is found with tests/_colliders_model.touch (brute force, no grid), the movers move
by tests/_movers_model.advance / pose.  TEST INFRASTRUCTURE ONLY.

respond() is the rule for particles whose obstacle is known; apply() one pass of a set with surfaces; Movers a mover
set with surfaces; Twin an OracleModel that holds both sets and their surfaces the way a context does; table_text() the
cases tests/cpp/surface_tests.cpp replays (tests/golden/surface_cases.txt); run_reference() the run scene."""
import numpy as np

from tests import _colliders_model as CM
from tests import _movers_model as M
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
PLAIN = 1
SURFACE_DTYPE = np.dtype([("restitution", F32), ("friction", F32), ("flags", U32), ("reserved", U32)])
assert SURFACE_DTYPE.itemsize == 16
BRANCHES = ("touched", "approaching", "separating", "sliding", "sticking", "plain", "not_finite", "wall_moved")


def rows(*surfaces):
    """rows of SURFACE_DTYPE from (restitution, friction[, flags]) tuples"""
    out = np.zeros(len(surfaces), SURFACE_DTYPE)
    for o, s in zip(out, surfaces):
        o["restitution"], o["friction"] = s[0], s[1]
        o["flags"] = s[2] if len(s) > 2 else 0
    return out


def uniform(k, restitution, friction, flags=0):
    out = np.zeros(k, SURFACE_DTYPE)
    out["restitution"], out["friction"], out["flags"] = restitution, friction, flags
    return out


def stored(surfaces):
    """the rows as a context stores them: -0.0 becomes +0"""
    s = np.array(surfaces, SURFACE_DTYPE).reshape(-1)
    for f in ("restitution", "friction"):
        s[f] = np.where(s[f] == 0, F32(0), s[f])
    return s


def contact_u(pos, c):
    """the clamped parameter u of collider_touch for one capsule c = (ax, ay, bx, by[, R]) -> f32[n]"""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    ax, ay, bx, by = (F32(v) for v in c[:4])
    with np.errstate(all="ignore"):
        dx, dy = F32(bx - ax), F32(by - ay)
        fx, fy = p[:, 0] - ax, p[:, 1] - ay
        A = F32(F32(dx * dx) + F32(dy * dy))
        u = (fx * dx + fy * dy) / A if A > 0 else np.zeros_like(fx)
        u = np.where(u > F32(0), u, F32(0)).astype(F32)
        u = np.where(u < F32(1), u, F32(1)).astype(F32)
    return u


def wall_move(old, cap, u):
    """surface_wall_move: old, cap f32[n, 4] (the capsule before and after the advance), u f32[n] -> (wx, wy)"""
    old, cap = np.asarray(old, F32).reshape(-1, 4), np.asarray(cap, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        wax, way = cap[:, 0] - old[:, 0], cap[:, 1] - old[:, 1]
        wbx, wby = cap[:, 2] - old[:, 2], cap[:, 3] - old[:, 3]
        wx = wax + u * (wbx - wax)
        wy = way + u * (wby - way)
    return wx.astype(F32), wy.astype(F32)


def velocity_finite(pos, prev):
    with np.errstate(all="ignore"):
        v = np.asarray(pos, F32) - np.asarray(prev, F32)
    return np.isfinite(v).all(axis=1)


def respond(pos, prev, rad, nx, ny, depth, wx, wy, e, mu, world):
    """surface_apply for every row -> (pos', prev', branches): all arguments f32[n] (pos, prev f32[n, 2])"""
    p, q0 = np.asarray(pos, F32).reshape(-1, 2), np.asarray(prev, F32).reshape(-1, 2)
    r = np.asarray(rad, F32).reshape(-1)
    nx, ny, depth, wx, wy, e, mu = (np.asarray(a, F32).reshape(-1) for a in (nx, ny, depth, wx, wy, e, mu))
    W, H = F32(world[0]), F32(world[1])
    with np.errstate(all="ignore"):
        qx = p[:, 0] + nx * depth
        qy = p[:, 1] + ny * depth
        vx = p[:, 0] - q0[:, 0]
        vy = p[:, 1] - q0[:, 1]
        relx = vx - wx
        rely = vy - wy
        vn = relx * nx + rely * ny
        t0x = relx - vn * nx
        t0y = rely - vn * ny
        approaching = vn < F32(0)
        on = np.where(approaching, (-e) * vn, vn).astype(F32)
        jn = on - vn
        tl = np.sqrt(t0x * t0x + t0y * t0y)
        s = mu * jn
        sliding = s < tl
        safe = np.where(sliding, tl, F32(1))
        k = (tl - s) / safe
        tx = np.where(sliding, t0x * k, F32(0)).astype(F32)
        ty = np.where(sliding, t0y * k, F32(0)).astype(F32)
        outx = (wx + on * nx) + tx
        outy = (wy + on * ny) + ty
        x = CM.clamp_f(qx - (t0x - tx), r, W - r)
        y = CM.clamp_f(qy - (t0y - ty), r, H - r)
        new_prev = np.stack([x - outx, y - outy], axis=1).astype(F32)
    branches = dict(approaching=approaching, separating=~approaching, sliding=sliding, sticking=~sliding)
    return np.stack([x, y], axis=1).astype(F32), new_prev, branches


def apply(pos, prev, rad, capsules, surfaces, world, old=None):
    """One pass of a set with surfaces -> (pos', prev', moved, branches).  capsules f32[k, 5] (posed, for movers), surfaces
    SURFACE_DTYPE[k], old f32[k, 4] the capsules before the advance (None: static, w = 0).  The winner is
    _colliders_model.apply's: the largest key bits(depth) << 32 | (0xFFFFFFFF - j)."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    q = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    cs = np.ascontiguousarray(capsules, F32).reshape(-1, 5)
    sf = np.ascontiguousarray(surfaces, SURFACE_DTYPE).reshape(-1)
    assert len(sf) == len(cs)
    n = len(r)
    best = np.zeros(n, U64)
    who = np.zeros(n, np.int64)
    b_depth, b_nx, b_ny, b_u = (np.zeros(n, F32) for _ in range(4))
    for j, c in enumerate(cs):
        touched, depth, nx, ny = CM.touch(p, r, c)
        key = (np.ascontiguousarray(depth).view(U32).astype(U64) << U64(32)) | U64(0xFFFFFFFF - j)
        take = touched & (key > best)
        best = np.where(take, key, best)
        who = np.where(take, j, who)
        b_depth = np.where(take, depth, b_depth)
        b_nx = np.where(take, nx, b_nx)
        b_ny = np.where(take, ny, b_ny)
        b_u = np.where(take, contact_u(p, c), b_u)
    moved = best != 0
    plain_pos, plain_moved = CM.apply(p, r, cs, world)
    assert np.array_equal(plain_moved, moved)
    if len(cs) == 0:
        return p.copy(), q.copy(), moved, {b: np.zeros(n, bool) for b in BRANCHES}
    row = sf[who]
    if old is None:
        wx, wy = np.zeros(n, F32), np.zeros(n, F32)
    else:
        wx, wy = wall_move(np.asarray(old, F32).reshape(-1, 4)[who], cs[who, :4], b_u)
    is_plain = (row["flags"] & PLAIN) != 0
    finite = velocity_finite(p, q)
    acts = moved & ~is_plain & finite
    s_pos, s_prev, br = respond(p, q, r, b_nx, b_ny, b_depth, wx, wy, row["restitution"], row["friction"], world)
    out_pos = np.where(acts[:, None], s_pos, plain_pos).astype(F32)
    out_prev = np.where(acts[:, None], s_prev, q).astype(F32)
    branches = {name: mask & acts for name, mask in br.items()}
    branches.update(touched=moved, plain=moved & is_plain, not_finite=moved & ~is_plain & ~finite,
                    wall_moved=acts & ((wx != 0) | (wy != 0)))
    return out_pos, out_prev, moved, branches


class Movers(M.Movers):
    """A mover set with its states and its surfaces (None: none, the plain pass)."""

    def __init__(self, movers=None):
        super().__init__(movers)

    def set(self, movers):
        super().set(movers)
        self.surfaces = None                                           # a new set gets new surfaces

    def set_surfaces(self, surfaces):
        s = stored(surfaces)
        assert len(s) in (0, len(self.movers))
        self.surfaces = s if len(s) else None

    def apply_surface(self, pos, prev, rad, world, dt):
        """gpe_apply_movers -> (pos', prev', moved, branches)"""
        if self.surfaces is None:
            out, moved = self.apply(pos, rad, world, dt)
            return out, np.array(prev, F32).reshape(-1, 2), moved, None
        old = M.pose(self.movers, self.q0, self.q1)
        self.q0, self.q1 = M.advance(self.movers, self.q0, self.q1, dt)
        out, new_prev, moved, br = apply(pos, prev, rad, self.capsules(), self.surfaces, world, old=old)
        self.passes += 1
        self.pushed += int(moved.sum())
        return out, new_prev, moved, br


class Twin(M.Twin):
    """An OracleModel with movers, static colliders and the surfaces of both: step -> movers -> colliders behind every
    step; set_colliders / set_movers drop their target's surfaces."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.m = Movers()
        self.collider_surfaces = None

    def set_colliders(self, capsules):
        super().set_colliders(capsules)
        self.collider_surfaces = None

    def set_surfaces(self, target, surfaces):
        if target == "movers":
            self.m.set_surfaces(surfaces)
        else:
            s = stored(surfaces)
            assert target == "colliders" and len(s) in (0, len(self.colliders))
            self.collider_surfaces = s if len(s) else None

    def surfaces(self, target):
        s = self.m.surfaces if target == "movers" else self.collider_surfaces
        return np.zeros(0, SURFACE_DTYPE) if s is None else s

    def apply_movers(self, dt):
        if len(self.m) == 0:
            return
        self._pull()
        self.pos, self.prev, _, _ = self.m.apply_surface(self.pos, self.prev, self.radius, self.world, dt)

    def apply_colliders(self):
        if self.collider_surfaces is None:
            return super().apply_colliders()
        self._pull()
        self.pos, self.prev, moved, _ = apply(self.pos, self.prev, self.radius, self.colliders, self.collider_surfaces, self.world)
        self.passes += 1
        self.pushed += int(moved.sum())

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_movers(dt)
        self.apply_colliders()


# ---- a single particle on one obstacle: the physics tests ------------------------------------------------------------
def drop(capsule, surface, pos, gravity, dt, steps, prev=None, radius=0.5, world=(60.0, 60.0)):
    """One particle under gravity on one static capsule with one surface, no other particle: Verlet as K12 integrates a
    lone particle (pos + (pos - prev) + g*dt*dt, clamped), then the surface pass -> f32[steps, 2] positions."""
    p = np.array([pos], F32)
    q = p.copy() if prev is None else np.array([prev], F32)
    r = np.array([radius], F32)
    cs = np.array([capsule], F32)
    sf = rows(surface)
    g = np.array(gravity, F32) * F32(dt) * F32(dt)
    trail = np.zeros((steps, 2), F32)
    for s in range(steps):
        nxt = (p + (p - q) + g).astype(F32)
        nxt[:, 0] = CM.clamp_f(nxt[:, 0], r, F32(world[0]) - r)
        nxt[:, 1] = CM.clamp_f(nxt[:, 1], r, F32(world[1]) - r)
        q, p = p, nxt
        p, q, _, _ = apply(p, q, r, cs, sf, world)
        trail[s] = p[0]
    return trail


# ---- the one-pass scene of the CPU and GPU tests ---------------------------------------------------------------------
def scene_surfaces(k, seed=3):
    """k mixed rows: every fourth PLAIN, restitution over [0, 1] with both ends, friction 0, small, large"""
    rng = np.random.default_rng(seed)
    out = np.zeros(k, SURFACE_DTYPE)
    out["restitution"] = rng.choice(np.array([0.0, 0.25, 0.5, 0.9, 1.0], F32), k)
    out["friction"] = rng.choice(np.array([0.0, 0.05, 0.3, 0.8, 5.0], F32), k)
    out["flags"] = np.where(np.arange(k) % 4 == 3, PLAIN, 0)
    return out


def scene_prev(pos, seed):
    """previous positions for a one-pass scene: velocities of every direction up to 0.6 per step, a share of them tiny
    (they stick), every 23rd not finite (prev NaN or infinite)"""
    p = np.asarray(pos, F32).reshape(-1, 2)
    n = len(p)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.6, 0.6, (n, 2))
    v[rng.random(n) < 0.3] *= 1e-3
    prev = (p - v.astype(F32)).astype(F32)
    odd = np.arange(n) % 23 == 11
    prev[odd, 0] = np.where(np.arange(n)[odd] % 2 == 0, np.nan, np.inf)
    return prev


# ---- the table tests/cpp/surface_tests.cpp replays (tests/golden/surface_cases.txt) ---------------------------------
TABLE_WORLD = (200.0, 200.0)


def table_cases():
    """-> dict of f32[n] / u32[n] inputs and outputs of 400 single contacts: a particle, its prev, its radius, one posed
    capsule with its radius, the capsule before the advance, one surface row; out: moved, pos', prev'"""
    rng = np.random.default_rng(29)
    n = 400
    a = rng.uniform(20, 180, (n, 2))
    b = a + rng.uniform(-30, 30, (n, 2))
    b[::7] = a[::7]                                                    # discs
    R = rng.choice([0.0, 0.5, 2.0, 6.0], n)
    cap = np.concatenate([a, b], axis=1).astype(F32)
    t = rng.uniform(-0.2, 1.2, n)[:, None]
    pos = (a + t * (b - a) + rng.uniform(-1, 1, (n, 2)) * (R[:, None] + 0.7)).astype(F32)
    pos[::31] = cap[::31, 0:2]                                         # on an end point: the axis normal, or (1, 0)
    rad = rng.choice(np.array([0.5, 0.25, -0.5], F32), n)
    prev = scene_prev(pos, 31)
    old = cap.copy()
    shift = rng.uniform(-0.8, 0.8, (n, 4)).astype(F32)
    shift[::3] = 0                                                     # a third of the walls stand still
    old = (cap - shift).astype(F32)
    surf = scene_surfaces(n, seed=37)
    out_pos, out_prev, moved = np.zeros((n, 2), F32), np.zeros((n, 2), F32), np.zeros(n, bool)
    for i in range(n):
        c5 = np.concatenate([cap[i], [R[i]]]).astype(F32)[None, :]
        p1, q1, m1, _ = apply(pos[i:i + 1], prev[i:i + 1], rad[i:i + 1], c5, surf[i:i + 1], TABLE_WORLD, old=old[i:i + 1])
        out_pos[i], out_prev[i], moved[i] = p1[0], q1[0], m1[0]
    return dict(pos=pos, prev=prev, rad=rad, cap=cap, R=R.astype(F32), old=old, surf=surf, moved=moved, out_pos=out_pos,
                out_prev=out_prev)


def table_text():
    """`c` lines, one per case: px py prevx prevy r | ax ay bx by R | a0x a0y b0x b0y | e mu flags | moved | pos'x pos'y
    prev'x prev'y, every number the hex word of its binary32 (flags and moved: integers)"""
    t = table_cases()
    lines = ["# c <case> px py prevx prevy r  ax ay bx by R  a0x a0y b0x b0y  e mu flags  moved  posx posy prevx prevy",
             "# binary32 words in hex; the world is %g x %g" % TABLE_WORLD,
             "# written by tests/_surfaces_model.table_text()"]
    for i in range(len(t["rad"])):
        f = np.concatenate([t["pos"][i], t["prev"][i], [t["rad"][i]], t["cap"][i], [t["R"][i]], t["old"][i],
                            [t["surf"]["restitution"][i], t["surf"]["friction"][i]]]).astype(F32).view(U32)
        o = np.concatenate([t["out_pos"][i], t["out_prev"][i]]).astype(F32).view(U32)
        lines.append("c %d " % i + " ".join("%08x" % w for w in f) + " %d %d " % (t["surf"]["flags"][i], t["moved"][i])
                     + " ".join("%08x" % w for w in o))
    return "\n".join(lines) + "\n"


# ---- the run scene: the movers' floor scene with surfaces on the floor, the piston and the paddle -------------------
RUN_COLLIDER_SURFACES = rows((0.5, 0.3))
RUN_MOVER_SURFACES = rows((0.3, 0.6), (0.8, 0.2))


def run_reference(oracle, dts, resort_every=0, resort_first=False, n=1500, collider_surfaces=RUN_COLLIDER_SURFACES,
                  mover_surfaces=RUN_MOVER_SURFACES):
    """-> (frames of (pos, prev, poses) after every step, pushed by the movers, pushed by the floor): the oracle's step,
    then the movers' pass, then the static colliders', each with its surfaces (None: without), the re-sorts taken as
    gpe_run(steps, resort_every, resort_first) takes them."""
    pos, rad = CM.floor_scene(n)
    tw = Twin(oracle, pos, rad, world=M.RUN_WORLD, gravity=M.RUN_GRAVITY)
    tw.set_colliders(M.RUN_FLOOR)
    tw.set_movers(M.run_movers())
    if collider_surfaces is not None:
        tw.set_surfaces("colliders", collider_surfaces)
    if mover_surfaces is not None:
        tw.set_surfaces("movers", mover_surfaces)
    frames = []
    for s, dt in enumerate(dts):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(dt, resort=bool(resort))
        p, q, _ = tw.arrays()
        frames.append((p.copy(), q.copy(), tw.m.poses()))
    out = frames, tw.m.pushed, tw.pushed
    tw.close()
    return out


# ---- the one-pass scenes the CPU and GPU tests share -----------------------------------------------------------------
ONE_PASS_WORLD = (200.0, 200.0)


def crowd(pos, caps, seed, lo=2000, hi=3600):
    """pos with the rows [lo, hi) (those there are) moved close to the capsules' surfaces: most of them touch"""
    p = np.array(pos, F32).reshape(-1, 2)
    hi = min(hi, len(p))
    if hi <= lo:
        return p
    rng = np.random.default_rng(seed)
    cs = np.asarray(caps, F32).reshape(-1, 5)[:-2].astype(np.float64)  # (not the two far ones)
    j = rng.integers(0, len(cs), hi - lo)
    u = rng.random(hi - lo)[:, None]
    on = cs[j, 0:2] + u * (cs[j, 2:4] - cs[j, 0:2])
    p[lo:hi] = (on + rng.uniform(-0.8, 0.8, (hi - lo, 2)) * (cs[j, 4] + 0.5)[:, None]).astype(F32)
    return p


def collider_scene(n):
    """-> (capsules f32[40, 5], surfaces, pos, prev, rad): the static colliders' one-pass scene (its colliders and its
    particles, those outside the grid, on axes and with NaN coordinates included), crowded, with mixed surfaces"""
    from tests.test_gpu_colliders import _scene_colliders, _scene_particles
    cs = _scene_colliders()
    pos, rad = _scene_particles(n, cs, seed=n)
    pos = crowd(pos, cs, n + 7)
    return cs, scene_surfaces(len(cs)), pos, scene_prev(pos, n + 1), rad


def mover_scene_set():
    """-> (movers, surfaces): the movers' one-pass scene (40 movers of both kinds) with mixed surfaces"""
    from tests.test_gpu_movers import _scene_movers
    movers = _scene_movers()
    return movers, scene_surfaces(len(movers), seed=5)


def mover_scene_particles(n, mv, dt, seed):
    """-> (pos, prev, rad) placed around the capsules as the NEXT apply_surface(dt) of mv will pose them"""
    from tests.test_gpu_colliders import _scene_particles
    q0, q1 = M.advance(mv.movers, mv.q0, mv.q1, dt)
    caps = np.concatenate([M.pose(mv.movers, q0, q1), mv.movers["radius"][:, None]], axis=1).astype(F32)
    pos, rad = _scene_particles(n, caps, seed=seed)
    pos = crowd(pos, caps, seed + 7)
    return pos, scene_prev(pos, seed + 1), rad


def coverage(moved, branches, n, movers=False):
    """the condition that keeps the one-pass tests from passing vacuously -> the counts; asserts it"""
    counts = {name: int(np.count_nonzero(mask)) for name, mask in branches.items()}
    assert counts["touched"] == int(moved.sum()) and 4 * counts["touched"] >= n, counts
    for name in BRANCHES[1:] if movers else BRANCHES[1:-1]:
        assert counts[name] >= 16, (name, counts)
    return counts
