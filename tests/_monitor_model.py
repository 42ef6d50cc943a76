"""The run monitor (gpe_measure / gpe_monitor_*, include/gpe.h) restated in numpy.  TEST INFRASTRUCTURE ONLY.

measure() is the definition with nothing of the implementation in it: binary32 differences and squares one rounding at a
time, the regular / irregular split tested on every coordinate and on v2 as the header words it, extents and the fastest
particle by the integer keys the header names, counts by masks, and the five sums by math.fsum over the binary32 terms
(each converted exactly to a Python float): the correctly rounded value of the exact sum, against which the header's
bound |D - S| <= m * 2^-52 * sum|t_i| is checked (sum_bounds).  MonitorModel is the ring and the schedule over
tests/_oracle_model.OracleModel.
"""
import collections
import math

import numpy as np

F32 = np.float32
UID_ABSENT = 0xFFFFFFFF
NO_INDEX = 0xFFFFFFFF
FIELDS = ("step", "n", "irregular", "moving", "outside", "sum_x", "sum_y", "sum_vx", "sum_vy", "sum_v2", "min_x", "min_y",
          "max_x", "max_y", "max_v2", "max_v2_index", "max_v2_uid", "first_irregular", "first_irregular_uid", "reserved")
SUMS = ("sum_x", "sum_y", "sum_vx", "sum_vy", "sum_v2")
EXACT = tuple(f for f in FIELDS if f not in SUMS)          # compared bit for bit
Measures = collections.namedtuple("Measures", FIELDS + ("abs_sums", "regular"))
DTYPE = np.dtype([(f, np.uint64) for f in FIELDS[:5]] + [(f, np.float64) for f in SUMS]
                 + [(f, np.float32) for f in FIELDS[10:15]] + [(f, np.uint32) for f in FIELDS[15:]])
assert DTYPE.itemsize == 120


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def order_key(x):
    """The sign-magnitude total order of binary32 as an unsigned integer order (-0 < +0)."""
    b = bits(x).astype(np.uint64)
    return np.where(b >> np.uint64(31), np.uint64(0xFFFFFFFF) - b, b + np.uint64(0x80000000))


def measure(pos, prev, uids, world, rest_speed, step=0):
    """-> Measures; abs_sums: sum|t_i| of each of the five sums (for the bound), regular: the number of regular
    particles.  uids None: off."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    q = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    n = p.shape[0]
    with np.errstate(all="ignore"):
        vx = p[:, 0] - q[:, 0]
        vy = p[:, 1] - q[:, 1]
        vxx = vx * vx
        vyy = vy * vy
        v2 = vxx + vyy
        rs2 = F32(rest_speed) * F32(rest_speed)
    assert vx.dtype == vy.dtype == v2.dtype == F32
    reg = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(v2)
    irr = np.nonzero(~reg)[0]
    r = np.nonzero(reg)[0]
    W, H = F32(world[0]), F32(world[1])
    px, py = p[r, 0], p[r, 1]
    inside = (px >= F32(0)) & (px <= W) & (py >= F32(0)) & (py <= H)
    terms = (px, py, vx[r], vy[r], v2[r])
    terms = [t.astype(np.float64) for t in terms]                  # exact
    sums = [math.fsum(t.tolist()) for t in terms]
    abs_sums = tuple(math.fsum(np.abs(t).tolist()) for t in terms)

    def extreme(x, hi):
        if x.size == 0:
            return F32(-np.inf) if hi else F32(np.inf)
        k = order_key(x)
        return x[np.argmax(k) if hi else np.argmin(k)]

    def uid_of(i):
        return UID_ABSENT if uids is None or i == NO_INDEX else int(uids[i])

    if r.size:
        key = (bits(v2[r]).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r.astype(np.uint64))
        fastest = int(r[np.argmax(key)])
        max_v2 = v2[fastest]
    else:
        fastest, max_v2 = NO_INDEX, F32(0.0)
    first = int(irr[0]) if irr.size else NO_INDEX
    return Measures(step, n, int(irr.size), int((v2[r] > rs2).sum()), int((~inside).sum()), *sums,
                    extreme(px, False), extreme(py, False), extreme(px, True), extreme(py, True), max_v2, fastest,
                    uid_of(fastest), first, uid_of(first), 0, abs_sums, int(r.size))


def sum_bounds(want):
    """The header's bound on each of the five sums: m * 2^-52 * sum|t_i|, plus half an ulp of the reference itself
    (math.fsum delivers the exact sum correctly rounded, so it may be that far from S)."""
    return tuple(want.regular * 2.0 ** -52 * a + 0.5 * math.ulp(getattr(want, f)) * (a != 0.0)
                 for f, a in zip(SUMS, want.abs_sums))


def same(got, want, exact_sums=False, skip=()):
    """None when the record `got` (anything with the fields as attributes / keys) meets `want`; else what differs."""
    def field(f):
        return got[f] if isinstance(got, (np.void, dict)) else getattr(got, f)

    for f in EXACT:
        if f in skip:
            continue
        g, w = field(f), getattr(want, f)
        if f in ("min_x", "min_y", "max_x", "max_y", "max_v2"):
            gb, wb = int(bits(F32(g)).reshape(-1)[0]), int(bits(F32(w)).reshape(-1)[0])
            if gb != wb:
                return "%s: got %r (0x%08x), want %r (0x%08x)" % (f, g, gb, w, wb)
        elif int(g) != int(w):
            return "%s: got %r, want %r" % (f, g, w)
    for f, bound in zip(SUMS, sum_bounds(want)):
        g, w = float(field(f)), getattr(want, f)
        if not (abs(g - w) <= (0.0 if exact_sums else bound)):
            return "%s: got %r, want %r, |difference| %r > bound %r" % (f, g, w, abs(g - w), 0.0 if exact_sums else bound)
    return None


class MonitorModel:
    """Wraps an OracleModel: drive the steps through step() / run() here -- or step the model itself and call after_step()
    after each step, as tests/_interactive_sequences.py does -- and everything else on the model itself."""

    def __init__(self, model, every=1, frames=1024, rest_speed=0.0):
        assert every >= 1 and frames >= 1 and rest_speed >= 0.0
        self.m = model
        self.every, self.frames, self.rest_speed = int(every), int(frames), rest_speed
        self.steps_seen = 0
        self.recorded = 0
        self.ring = collections.deque(maxlen=self.frames)      # Measures, oldest first

    def sample(self):
        m = self.m
        pos, prev = (m._sim.pos, m._sim.prev) if m._sim is not None else (m.pos, m.prev)
        self.ring.append(measure(pos, prev, m.uids, m.world, self.rest_speed, step=self.steps_seen))
        self.recorded += 1

    def after_step(self):
        """The model has made one step (whoever drove it): count it, and take a frame on every every-th."""
        self.steps_seen += 1
        if self.steps_seen % self.every == 0:
            self.sample()

    def step(self, dt, resort=False):
        self.m.step(dt, resort=resort)
        self.after_step()

    def run(self, dt, steps, resort_every=0, resort_first=True):
        for s in range(steps):
            resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
            self.step(dt, resort=bool(resort))

    def read(self, capacity=None, consume=False):
        """-> (records delivered, count, recorded)"""
        held = list(self.ring)
        count = len(held)
        give = held if capacity is None else held[count - min(count, capacity):]
        if consume:
            self.ring.clear()
        return give, count, self.recorded
