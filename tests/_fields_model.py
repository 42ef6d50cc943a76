"""The numpy float32 restatement of the force fields' pass (include/gpe.h "force fields", csrc/k_field.h): brute force
over all fields in ascending index, vectorised over the particles, no grid, in the exact operation order of the header,
one binary32 rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are
correctly rounded).  TEST INFRASTRUCTURE ONLY.

apply() is the pass; rows() builds sets; pool_scene() / pool_reference() are the scene the GPU tests step (the CPU
oracle's step followed by the pass); Twin is an OracleModel that holds a field set the way a context does."""
import numpy as np

from tests._oracle_model import OracleModel, max_abs_radius

F32 = np.float32
U32 = np.uint32
FIELDS_MAX = 4096
EVERYWHERE, CIRCLE, BOX = 0, 1, 2
UNIFORM, RADIAL, VORTEX, DRAG = 0, 1, 2, 3
NONE, LINEAR = 0, 1
_U = ("shape", "kind", "falloff", "flags")
_F = ("x0", "y0", "x1", "y1", "px", "py", "fx", "fy", "strength", "reach")
DTYPE = np.dtype([(n, U32) for n in _U] + [(n, F32) for n in _F])     # gpe_field, 56 bytes
assert DTYPE.itemsize == 56


def field(shape=EVERYWHERE, kind=UNIFORM, falloff=NONE, region=(0, 0, 0, 0), pole=(0, 0), f=(0, 0), strength=0.0, reach=0.0):
    """One row of DTYPE.  region: (x0, y0, radius, 0) for a circle, (x0, y0, x1, y1) for a box."""
    r = np.zeros(1, DTYPE)
    r["shape"], r["kind"], r["falloff"] = shape, kind, falloff
    r["x0"], r["y0"], r["x1"], r["y1"] = region
    r["px"], r["py"] = pole
    r["fx"], r["fy"] = f
    r["strength"], r["reach"] = strength, reach
    return r


def rows(*fields):
    return np.concatenate(fields) if fields else np.zeros(0, DTYPE)


def matches(pos, f):
    """bool[n]: the field's region holds the centre (the predicates of the region queries and the kicks)."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    cx, cy = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        if f["shape"] == CIRCLE:
            dx = cx - f["x0"]
            dy = cy - f["y0"]
            rr = F32(f["x1"] * f["x1"])
            return (dx * dx + dy * dy) <= rr
        if f["shape"] == BOX:
            return (f["x0"] <= cx) & (cx <= f["x1"]) & (f["y0"] <= cy) & (cy <= f["y1"])
    return np.ones(len(p), bool)


def contribution(pos, f):
    """(gx, gy) f32[n] of a UNIFORM, RADIAL or VORTEX field at every particle."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    cx, cy = p[:, 0], p[:, 1]
    if f["kind"] == UNIFORM:
        return np.full(len(p), f["fx"], F32), np.full(len(p), f["fy"], F32)
    with np.errstate(all="ignore"):
        dx = f["px"] - cx
        dy = f["py"] - cy
        ln = np.sqrt(dx * dx + dy * dy)
        w = np.full(len(p), f["strength"], F32)
        if f["falloff"] == LINEAR:
            t = ln / f["reach"]
            w1 = F32(1) - t
            w1 = np.where(w1 > F32(0), w1, F32(0)).astype(F32)
            w = f["strength"] * w1
        if f["kind"] == RADIAL:
            gx = (dx / ln) * w
            gy = (dy / ln) * w
        else:
            gx = ((-dy) / ln) * w
            gy = (dx / ln) * w
        off = ~(ln > F32(0))
        gx = np.where(off, F32(0), gx).astype(F32)
        gy = np.where(off, F32(0), gy).astype(F32)
    return gx, gy


def apply(pos, prev, fields, dt):
    """The pass -> (new prev f32[n, 2], touched bool[n]).  dt2 = dt * dt in binary32.  A particle no field matches keeps
    every bit."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    q = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    fs = np.ascontiguousarray(fields, DTYPE).reshape(-1)
    assert len(fs) <= FIELDS_MAX
    n = len(p)
    dt2 = F32(F32(dt) * F32(dt))
    ax, ay, s = np.zeros(n, F32), np.zeros(n, F32), np.ones(n, F32)
    accel, drag = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for f in fs:
            m = matches(p, f)
            if not m.any():
                continue
            if f["kind"] == DRAG:
                s = np.where(m, s * f["strength"], s).astype(F32)
                drag |= m
            else:
                gx, gy = contribution(p, f)
                ax = np.where(m, ax + gx, ax).astype(F32)
                ay = np.where(m, ay + gy, ay).astype(F32)
                accel |= m
        out = q.copy()
        for c, a in ((0, ax), (1, ay)):
            x = q[:, c]
            v = p[:, c] - x
            v = v * s
            x = np.where(drag, p[:, c] - v, x).astype(F32)
            x = np.where(accel, x - a * dt2, x).astype(F32)
            touched = accel | drag
            out[touched, c] = x[touched]
    return out, accel | drag


def stored(fields):
    """The set as a context gives it back: -0.0 as a circle's radius is stored as +0."""
    fs = np.array(fields, DTYPE).reshape(-1)
    z = (fs["shape"] == CIRCLE) & (fs["x1"] == 0)
    fs["x1"] = np.where(z, F32(0), fs["x1"])
    return fs


# ---- the scene the GPU tests step: a vortex, a well and a drag pool -------------------------------------------------
POOL_WORLD = (120.0, 120.0)
POOL_GRAVITY = (0.0, 30.0)
POOL_DT = 1.0 / 60.0
POOL_FIELDS = rows(
    field(CIRCLE, VORTEX, NONE, (40, 40, 30, 0), pole=(40, 40), strength=100.0),
    field(CIRCLE, RADIAL, LINEAR, (85, 50, 28, 0), pole=(85, 50), strength=150.0, reach=28.0),
    field(BOX, DRAG, NONE, (10, 80, 110, 118), strength=0.9),
    field(BOX, UNIFORM, NONE, (0, 100, 120, 120), f=(30.0, -20.0)),
)


def pool_scene(n=3000):
    rng = np.random.default_rng(17)
    pos = np.stack([rng.uniform(1, 119, n), rng.uniform(1, 100, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    return pos, rad


def pool_reference(oracle, steps, fields=POOL_FIELDS, n=3000, resort_every=0, resort_first=False):
    """-> (frames of (pos, prev) after every step, touched): a fresh oracle.Sim per step, then the pass.  The re-sorts of
    gpe_run(steps, resort_every, resort_first) are taken the same way."""
    pos, rad = pool_scene(n)
    prev = pos.copy()
    params = oracle.default_params(POOL_WORLD[0], POOL_WORLD[1], 0.5, gravity=POOL_GRAVITY)
    frames, total = [], 0
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        sim = oracle.Sim(pos, rad, params, prev=prev)
        sim.step(POOL_DT, resort=bool(resort))
        pos, prev, rad = sim.pos, sim.prev, sim.radius
        sim.close()
        if fields is not None and len(fields):
            prev, touched = apply(pos, prev, fields, POOL_DT)
            total += int(touched.sum())
        frames.append((pos, prev))
    return frames, total


class Twin(OracleModel):
    """An OracleModel with the fields of a context: a pass after every step of step() / run(), none after the module
    calls; the set survives everything but set_fields."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fields = np.zeros(0, DTYPE)
        self.passes = self.touched = 0

    def set_fields(self, fields):
        self.fields = stored(fields)
        self.passes = self.touched = 0

    def set_particles(self, pos, prev, radius):
        """gpe_set_particles on a live context: the fields stay"""
        self._pull()
        self.pos = np.array(pos, F32).reshape(-1, 2)
        self.prev = self.pos.copy() if prev is None else np.array(prev, F32).reshape(-1, 2)
        self.radius = np.array(radius, F32).reshape(-1)
        self.max_radius = self.grid_max_radius = max_abs_radius(self.radius)
        if self.uids is not None:
            self.uids = np.arange(len(self), dtype=np.uint32)
            self.next_uid = len(self)

    def apply_fields(self, dt):
        if len(self.fields) == 0:
            return
        self._pull()
        self.prev, touched = apply(self.pos, self.prev, self.fields, dt)
        self.passes += 1
        self.touched += int(touched.sum())

    def step(self, dt, resort=False):
        super().step(dt, resort=resort)
        self.apply_fields(dt)
