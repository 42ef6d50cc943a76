"""The numpy float32 restatement of the moving colliders (include/gpe.h "moving colliders", csrc/k_mover.h): the motion
in the exact operation order of the header, one binary32 rounding per operation, no FMA, no sin / cos; the push is
tests/_colliders_model.apply on the posed capsules (brute force, no grid).  TEST INFRASTRUCTURE ONLY.

prepare() is what the host derives at set time, advance() one step of every mover's state, pose() the posed capsules;
Movers holds a set with its states the way a context does; Twin is an OracleModel with the pass behind every step."""
import numpy as np

from tests import _colliders_model as CM
from tests._oracle_model import OracleModel

F32 = np.float32
U32 = np.uint32
LINEAR, ROTATE = 0, 1
MOVERS_MAX = 1024
MAX_TURN = F32(0.5)
FIELDS = ("ax", "ay", "bx", "by", "radius", "kind", "vx", "vy", "travel", "px", "py", "omega", "flags", "reserved")
MOVER_DTYPE = np.dtype([(f, U32 if f in ("kind", "flags", "reserved") else F32) for f in FIELDS])
POSE_DTYPE = np.dtype([(f, F32) for f in ("ax", "ay", "bx", "by", "q0", "q1")])
assert MOVER_DTYPE.itemsize == 56 and POSE_DTYPE.itemsize == 24

S = [F32(float.fromhex(h)) for h in ("-0x1.555556p-3", "0x1.111112p-7", "-0x1.a01a02p-13", "0x1.71de3ap-19")]
C = [F32(float.fromhex(h)) for h in ("-0x1p-1", "0x1.555556p-5", "-0x1.6c16c2p-10", "0x1.a01a02p-16", "-0x1.27e4fcp-22")]
assert S == [F32(-1 / 6), F32(1 / 120), F32(-1 / 5040), F32(1 / 362880)]
assert C == [F32(-1 / 2), F32(1 / 24), F32(-1 / 720), F32(1 / 40320), F32(-1 / 3628800)]


def linear(a, b, radius, v=(0.0, 0.0), travel=0.0):
    """one row: the capsule a -> b sliding with velocity v, back and forth over `travel` (0: for ever)"""
    row = np.zeros((), MOVER_DTYPE)
    row["ax"], row["ay"], row["bx"], row["by"], row["radius"] = a[0], a[1], b[0], b[1], radius
    row["kind"], row["vx"], row["vy"], row["travel"] = LINEAR, v[0], v[1], travel
    return row


def rotor(a, b, radius, pivot, omega):
    """one row: the capsule a -> b turning about `pivot` at omega rad / s"""
    row = np.zeros((), MOVER_DTYPE)
    row["ax"], row["ay"], row["bx"], row["by"], row["radius"] = a[0], a[1], b[0], b[1], radius
    row["kind"], row["px"], row["py"], row["omega"] = ROTATE, pivot[0], pivot[1], omega
    return row


def rows(*movers):
    return np.array(list(movers), MOVER_DTYPE).reshape(-1)


def prepare(movers):
    """set time -> (rate, ux, uy): LINEAR: speed = sqrt(vx*vx + vy*vy) and u = v / speed ((0, 0) when speed == 0);
    ROTATE: omega and the pivot"""
    m = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
    with np.errstate(all="ignore"):
        vx, vy = m["vx"], m["vy"]
        speed = np.sqrt(vx * vx + vy * vy)
        safe = np.where(speed > 0, speed, F32(1))
        ux = np.where(speed > 0, vx / safe, F32(0)).astype(F32)
        uy = np.where(speed > 0, vy / safe, F32(0)).astype(F32)
    lin = m["kind"] == LINEAR
    return (np.where(lin, speed, m["omega"]).astype(F32), np.where(lin, ux, m["px"]).astype(F32),
            np.where(lin, uy, m["py"]).astype(F32))


def fresh(movers):
    m = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
    lin = m["kind"] == LINEAR
    return np.where(lin, F32(0), F32(1)).astype(F32), np.where(lin, F32(1), F32(0)).astype(F32)


def advance(movers, q0, q1, dt):
    """mover_advance for every mover -> (q0, q1)"""
    m = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
    rate, _, _ = prepare(m)
    dt = F32(dt)
    q0, q1 = np.array(q0, F32), np.array(q1, F32)
    lin = m["kind"] == LINEAR
    with np.errstate(all="ignore"):
        # LINEAR
        travel = m["travel"]
        d = rate * dt
        g1 = q0 + q1 * d
        sgn = q1.copy()
        bounded = travel > 0
        over = bounded & (g1 > travel)
        under = bounded & ~over & (g1 < 0)
        g1 = np.where(over, travel - (g1 - travel), g1).astype(F32)
        g1 = np.where(under, -g1, g1).astype(F32)
        sgn = np.where(over | under, -sgn, sgn).astype(F32)
        g1 = np.where(bounded & (g1 < 0), F32(0), g1).astype(F32)
        g1 = np.where(bounded & (g1 > travel), travel, g1).astype(F32)
        # ROTATE
        x = rate * dt
        x2 = x * x
        sa = x + x * (x2 * (S[0] + x2 * (S[1] + x2 * (S[2] + x2 * S[3]))))
        ca = F32(1) + x2 * (C[0] + x2 * (C[1] + x2 * (C[2] + x2 * (C[3] + x2 * C[4]))))
        c2 = q0 * ca - q1 * sa
        s2 = q1 * ca + q0 * sa
        mag = np.sqrt(c2 * c2 + s2 * s2)
        still = x == 0
        rc = np.where(still, q0, c2 / mag).astype(F32)
        rs = np.where(still, q1, s2 / mag).astype(F32)
    return np.where(lin, g1, rc).astype(F32), np.where(lin, sgn, rs).astype(F32)


def pose(movers, q0, q1):
    """mover_pose for every mover -> f32[k, 4] posed (ax, ay, bx, by)"""
    m = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
    _, ux, uy = prepare(m)
    q0, q1 = np.asarray(q0, F32), np.asarray(q1, F32)
    lin = m["kind"] == LINEAR
    out = np.zeros((len(m), 4), F32)
    with np.errstate(all="ignore"):
        ox, oy = q0 * ux, q0 * uy
        for e, (fx, fy) in enumerate((("ax", "ay"), ("bx", "by"))):
            rx, ry = m[fx] - ux, m[fy] - uy
            tx = rx * q0 - ry * q1
            ty = rx * q1 + ry * q0
            out[:, 2 * e] = np.where(lin, m[fx] + ox, ux + tx)
            out[:, 2 * e + 1] = np.where(lin, m[fy] + oy, uy + ty)
    return out


def dt_allowed(movers, dt):
    """the host's dt contract: finite, |max|omega| * dt| <= 0.5, and max speed * |dt| <= min travel over the movers that
    go back and forth"""
    m = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
    if len(m) == 0:
        return True
    dt = F32(dt)
    if not np.isfinite(dt):
        return False
    rate, _, _ = prepare(m)
    rot = m["kind"] == ROTATE
    with np.errstate(all="ignore"):
        if rot.any() and not (abs(F32(np.abs(m["omega"][rot]).max()) * dt) <= MAX_TURN):
            return False
        b = ~rot & (m["travel"] > 0)
        if b.any() and not (abs(F32(rate[b].max()) * dt) <= F32(m["travel"][b].min())):
            return False
    return True


class Movers:
    """A set with its states, as a context holds it."""

    def __init__(self, movers=None):
        self.set(np.zeros(0, MOVER_DTYPE) if movers is None else movers)

    def set(self, movers):
        m = np.array(movers, MOVER_DTYPE).reshape(-1)
        assert len(m) <= MOVERS_MAX
        m["radius"] = np.where(m["radius"] == 0, F32(0), m["radius"])  # -0.0 is stored as +0
        self.movers = m
        self.q0, self.q1 = fresh(m)
        self.passes = self.pushed = 0

    def __len__(self):
        return len(self.movers)

    def poses(self):
        out = np.zeros(len(self.movers), POSE_DTYPE)
        caps = pose(self.movers, self.q0, self.q1)
        for i, f in enumerate(("ax", "ay", "bx", "by")):
            out[f] = caps[:, i]
        out["q0"], out["q1"] = self.q0, self.q1
        return out

    def set_poses(self, poses):
        p = np.ascontiguousarray(poses, POSE_DTYPE).reshape(-1)
        assert len(p) == len(self.movers)
        self.q0, self.q1 = p["q0"].copy(), p["q1"].copy()

    def capsules(self):
        """f32[k, 5]: the posed capsules with their radii, what _colliders_model.apply takes"""
        return np.concatenate([pose(self.movers, self.q0, self.q1), self.movers["radius"][:, None]], axis=1).astype(F32)

    def apply(self, pos, rad, world, dt):
        """gpe_apply_movers: advance, then the pass -> (new pos, moved)"""
        self.q0, self.q1 = advance(self.movers, self.q0, self.q1, dt)
        out, moved = CM.apply(pos, rad, self.capsules(), world)
        self.passes += 1
        self.pushed += int(moved.sum())
        return out, moved


class Twin(CM.Twin):
    """An OracleModel with movers and static colliders: step -> movers -> colliders behind every step of step() / run(),
    none after the module calls; the set and its poses survive everything but set_movers."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.m = Movers()

    def set_movers(self, movers):
        self.m.set(movers)

    def apply_movers(self, dt):
        if len(self.m) == 0:
            return
        self._pull()
        self.pos, _ = self.m.apply(self.pos, self.radius, self.world, dt)

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_movers(dt)
        self.apply_colliders()


# ---- the table tests/cpp/mover_grid_tests.cpp replays (tests/golden/mover_poses.txt) --------------------------------
def table_movers():
    return rows(linear((10, 20), (30, 25), 1.5, v=(3, 4), travel=2.5),
                linear((10, 20), (30, 25), 0.0, v=(-7, 0.25), travel=0.0),
                linear((5, 5), (5, 5), 2.0, v=(0, 0), travel=1.0),
                linear((0, 0), (1, 1), 0.5, v=(1e-3, -2e-3), travel=0.125),
                rotor((50, 50), (70, 50), 1.0, (50, 50), 3.0),
                rotor((50, 50), (70, 50), 1.0, (60, 55), -29.0),
                rotor((1, 2), (3, 4), 0.25, (1000, -2000), 0.0),
                rotor((1, 2), (3, 4), 0.25, (1000, -2000), 0.125))


TABLE_DTS = [1 / 60, 1 / 60, 1 / 120, 0.0, -1 / 60, 1 / 60] + [1 / 60] * 34


def table_text():
    """`m` lines: the 14 words of a mover's row (hex); `s` lines, one per (step, mover): the words of dt, q0, q1, ax, ay,
    bx, by after the advance"""
    m = table_movers()
    q0, q1 = fresh(m)
    lines = ["# m <mover> <the 14 binary32 / uint32 words of its gpe_mover, hex>",
             "# s <step> <mover> dt q0 q1 ax ay bx by (binary32 words, hex), after the advance by dt",
             "# written by tests/_movers_model.table_text()"]
    for j in range(len(m)):
        lines.append("m %d " % j + " ".join("%08x" % w for w in np.frombuffer(m[j].tobytes(), U32)))
    for s, dt in enumerate(TABLE_DTS):
        assert dt_allowed(m, dt)
        q0, q1 = advance(m, q0, q1, dt)
        caps = pose(m, q0, q1)
        for j in range(len(m)):
            words = np.array([dt, q0[j], q1[j], caps[j, 0], caps[j, 1], caps[j, 2], caps[j, 3]], F32).view(U32)
            lines.append("s %d %d " % (s, j) + " ".join("%08x" % w for w in words))
    return "\n".join(lines) + "\n"


# ---- the run scene of the CPU and GPU tests: the colliders' floor scene with a piston and a paddle ------------------
RUN_WORLD = CM.FLOOR_WORLD
RUN_GRAVITY = CM.FLOOR_GRAVITY
RUN_DT = CM.FLOOR_DT
RUN_FLOOR = CM.FLOOR_COLLIDERS[:1]                                     # the floor capsule alone: centres rest at y = 40


def run_movers():
    """a piston 4 thick sweeping 10 units along the floor at 0.5 per step (it turns after 20 steps), and a paddle 3
    thick turning at 0.1 rad per step (its tip moves 0.8 per step): both thicker than one step's displacement"""
    return rows(linear((5, 28), (5, 42), 2.0, v=(30.0, 0.0), travel=10.0),
                rotor((40, 32), (48, 32), 1.5, (40, 32), 6.0))


def run_reference(oracle, dts, resort_every=0, resort_first=False, n=1500, movers=None, colliders=RUN_FLOOR):
    """-> (frames of (pos, prev, poses) after every step, pushed by the movers, pushed by the colliders): the oracle's
    step, then the movers' pass, then the static colliders', as gpe_run(steps, resort_every, resort_first) takes the
    re-sorts."""
    pos, rad = CM.floor_scene(n)
    tw = Twin(oracle, pos, rad, world=RUN_WORLD, gravity=RUN_GRAVITY)
    tw.set_colliders(colliders)
    tw.set_movers(run_movers() if movers is None else movers)
    frames = []
    for s, dt in enumerate(dts):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(dt, resort=bool(resort))
        p, q, _ = tw.arrays()
        frames.append((p.copy(), q.copy(), tw.m.poses()))
    out = frames, tw.m.pushed, tw.pushed
    tw.close()
    return out
