"""The numpy float32 restatement of the static colliders' pass (include/gpe.h "static colliders", csrc/k_collider.h):
brute force over all colliders, vectorised over the particles, no grid, in the exact operation order of the header, one
binary32 rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are
correctly rounded).  TEST INFRASTRUCTURE ONLY.

apply() is the pass; floor_scene() / floor_reference() are the scene the CPU and GPU tests share (the CPU oracle's step
followed by the pass); Twin is an OracleModel that holds a collider set the way a context does."""
import numpy as np

from tests._oracle_model import OracleModel, max_abs_radius

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
COLLIDERS_MAX = 4096


def clamp_f(x, lo, hi):
    """gpe_internal.h clamp_f: (x > lo ? x : lo), then (m < hi ? m : hi): a NaN x gives lo"""
    m = np.where(x > lo, x, lo)
    return np.where(m < hi, m, hi).astype(F32)


def touch(pos, rad, c):
    """One collider c = (ax, ay, bx, by, R) against every particle -> (touched bool[n], depth, nx, ny f32[n]); depth and
    the normal are meaningless where touched is False."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    ax, ay, bx, by, R = (F32(v) for v in c)
    px, py = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        a = np.abs(r)
        dx = F32(bx - ax)
        dy = F32(by - ay)
        fx = px - ax
        fy = py - ay
        A = F32(F32(dx * dx) + F32(dy * dy))
        if A > 0:
            u = (fx * dx + fy * dy) / A
        else:
            u = np.zeros_like(px)
        u = np.where(u > F32(0), u, F32(0)).astype(F32)                # NaN -> 0
        u = np.where(u < F32(1), u, F32(1)).astype(F32)
        qx = fx - u * dx
        qy = fy - u * dy
        h = qx * qx + qy * qy
        s = R + a
        touched = h < s * s
        d = np.sqrt(h)
        depth = (s - d).astype(F32)
        if A > 0:
            L = np.sqrt(A)
            ex, ey = F32(F32(-dy) / L), F32(dx / L)
        else:
            ex, ey = F32(1), F32(0)
        on = d > F32(0)
        safe = np.where(on, d, F32(1))
        nx = np.where(on, qx / safe, ex).astype(F32)
        ny = np.where(on, qy / safe, ey).astype(F32)
    return touched, depth, nx, ny


def apply(pos, rad, colliders, world):
    """The pass -> (new pos f32[n, 2], moved bool[n]): every collider judged from `pos`, the touched one with the largest
    key bits(depth) << 32 | (0xFFFFFFFF - j) acts, then K12's clamp; an untouched particle keeps every bit."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    cs = np.ascontiguousarray(colliders, F32).reshape(-1, 5)
    n = len(r)
    assert len(cs) <= COLLIDERS_MAX
    best = np.zeros(n, U64)
    b_depth, b_nx, b_ny = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    for j, c in enumerate(cs):
        touched, depth, nx, ny = touch(p, r, c)
        key = (np.ascontiguousarray(depth).view(U32).astype(U64) << U64(32)) | U64(0xFFFFFFFF - j)
        take = touched & (key > best)
        best = np.where(take, key, best)
        b_depth = np.where(take, depth, b_depth)
        b_nx = np.where(take, nx, b_nx)
        b_ny = np.where(take, ny, b_ny)
    moved = best != 0
    W, H = F32(world[0]), F32(world[1])
    with np.errstate(all="ignore"):
        x = p[:, 0] + b_nx * b_depth
        y = p[:, 1] + b_ny * b_depth
        x = clamp_f(x, r, W - r)
        y = clamp_f(y, r, H - r)
    out = p.copy()
    out[moved, 0] = x[moved]
    out[moved, 1] = y[moved]
    return out, moved


# ---- the floor scene of the CPU and GPU tests -----------------------------------------------------------------------
FLOOR_WORLD = (60.0, 60.0)
FLOOR_GRAVITY = (0.0, 100.0)
FLOOR_DT = 1.0 / 60.0
FLOOR_COLLIDERS = np.array([[-5, 50, 65, 50, 9.5], [30, 25, 30, 25, 4], [10, 15, 25, 22, 0]], F32)


def floor_scene(n=1500, gravity=FLOOR_GRAVITY):
    rng = np.random.default_rng(5)
    pos = np.stack([rng.uniform(1, 59, n), rng.uniform(1, 38, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    return pos, rad


def floor_reference(oracle, steps, colliders=FLOOR_COLLIDERS, gravity=FLOOR_GRAVITY, n=1500, resort_every=0,
                    resort_first=False):
    """-> (frames of (pos, prev) after every step, pushes): a fresh oracle.Sim per step, then the pass.  The re-sorts of
    gpe_run(steps, resort_every, resort_first) are taken the same way."""
    pos, rad = floor_scene(n)
    prev = pos.copy()
    params = oracle.default_params(FLOOR_WORLD[0], FLOOR_WORLD[1], 0.5, gravity=gravity)
    frames, pushes = [], 0
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        sim = oracle.Sim(pos, rad, params, prev=prev)
        sim.step(FLOOR_DT, resort=bool(resort))
        pos, prev, rad = sim.pos, sim.prev, sim.radius
        sim.close()
        if colliders is not None and len(colliders):
            pos, moved = apply(pos, rad, colliders, FLOOR_WORLD)
            pushes += int(moved.sum())
        frames.append((pos, prev))
    return frames, pushes


class Twin(OracleModel):
    """An OracleModel with the colliders of a context: a pass after every step of step() / run(), none after the module
    calls; the set survives everything but set_colliders."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.colliders = np.zeros((0, 5), F32)
        self.passes = self.pushed = 0

    def set_colliders(self, capsules):
        c = np.array(capsules, F32).reshape(-1, 5)
        c[:, 4] = np.where(c[:, 4] == 0, F32(0), c[:, 4])              # -0.0 is stored as +0
        self.colliders = c
        self.passes = self.pushed = 0

    def set_particles(self, pos, prev, radius):
        """gpe_set_particles on a live context: the colliders stay"""
        self._pull()
        self.pos = np.array(pos, F32).reshape(-1, 2)
        self.prev = self.pos.copy() if prev is None else np.array(prev, F32).reshape(-1, 2)
        self.radius = np.array(radius, F32).reshape(-1)
        self.max_radius = self.grid_max_radius = max_abs_radius(self.radius)
        if self.uids is not None:
            self.uids = np.arange(len(self), dtype=np.uint32)
            self.next_uid = len(self)

    def apply_colliders(self):
        if len(self.colliders) == 0:
            return
        self._pull()
        self.pos, moved = apply(self.pos, self.radius, self.colliders, self.world)
        self.passes += 1
        self.pushed += int(moved.sum())

    def step(self, dt, resort=False):
        super().step(dt, resort=resort)
        self.apply_colliders()
