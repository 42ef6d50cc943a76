"""The numpy float32 restatement of the swept form of the movers' pass (include/gpe.h "moving colliders",
csrc/k_mover_sweep.h): brute force over all movers, vectorised over the particles, no grid, in the exact operation order
of the header, one binary32 rounding per operation, no FMA.  The motion is tests/_movers_model.advance / pose, the
contact on a path tests/_sweep_model.contact, the surface rule tests/_surfaces_model.respond.  TEST INFRASTRUCTURE ONLY.

carry_records() is what the build writes per mover, judge() steps 1 to 4 of the rule for one mover, apply() the pass;
Movers a mover set that holds the mode; Mixin gives any twin of the _surfaces_model.Twin family the mode the way a
context holds it, Twin is the one the tests step; gate_scene() / blade_scene() the two tunnelling scenes with their
float64 checkers; table_text() the cases tests/cpp/mover_sweep_tests.cpp replays (tests/golden/mover_sweep_cases.txt)."""
import numpy as np

from tests import _colliders_model as CM
from tests import _movers_model as M
from tests import _surfaces_model as SM
from tests import _sweep_model as S

F32 = np.float32
U32 = np.uint32
ZERO, ONE = F32(0), F32(1)
STILL, SHIFT, TURN = 0, 1, 2


def _f(a):
    return np.ascontiguousarray(a, F32).reshape(-1)


def arm(movers):
    """mover_arm: max(|a - pivot|, |b - pivot|) of the rest capsule of a ROTATE mover, 0 for a LINEAR one -> f32[k]"""
    m = np.ascontiguousarray(movers, M.MOVER_DTYPE).reshape(-1)
    with np.errstate(all="ignore"):
        ex, ey = m["ax"] - m["px"], m["ay"] - m["py"]
        ea = np.sqrt(ex * ex + ey * ey)
        fx, fy = m["bx"] - m["px"], m["by"] - m["py"]
        fa = np.sqrt(fx * fx + fy * fy)
        out = np.where(fa > ea, fa, ea).astype(F32)
    return np.where(m["kind"] == M.ROTATE, out, ZERO).astype(F32)


def carry_records(movers, dt, p0, p1, q0, q1, c0, c1):
    """mover_carry_of for every mover: the states before (p0, p1) and after (q0, q1) the advance by dt, the posed capsules
    before (c0) and after (c1) -> dict(kind i64[k], cx, cy, px, py, arm f32[k])"""
    m = np.ascontiguousarray(movers, M.MOVER_DTYPE).reshape(-1)
    c0, c1 = np.asarray(c0, F32).reshape(-1, 4), np.asarray(c1, F32).reshape(-1, 4)
    p0, p1, q0, q1 = (_f(a) for a in (p0, p1, q0, q1))
    lin = m["kind"] == M.LINEAR
    with np.errstate(all="ignore"):
        same = (c1[:, 0] == c0[:, 0]) & (c1[:, 1] == c0[:, 1])
        x = m["omega"] * F32(dt)
        kind = np.where(lin, np.where(same, STILL, SHIFT), np.where(x == ZERO, STILL, TURN))
        cd = q0 * p0 + q1 * p1
        sd = q1 * p0 - q0 * p1
        cx = np.where(lin, c1[:, 0] - c0[:, 0], cd).astype(F32)
        cy = np.where(lin, c1[:, 1] - c0[:, 1], sd).astype(F32)
    zero = np.zeros(len(m), F32)
    turn = kind == TURN
    return dict(kind=kind, cx=np.where(kind == STILL, zero, cx), cy=np.where(kind == STILL, zero, cy),
                px=np.where(turn, m["px"], zero), py=np.where(turn, m["py"], zero), arm=np.where(turn, arm(m), zero))


def carry(rec, j, prev):
    """mover_carry: y0 = M_j(prev) -> f32[n, 2]"""
    q = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    kind = int(rec["kind"][j])
    if kind == STILL:
        return q.copy()
    cx, cy = F32(rec["cx"][j]), F32(rec["cy"][j])
    with np.errstate(all="ignore"):
        if kind == SHIFT:
            return np.stack([q[:, 0] + cx, q[:, 1] + cy], axis=1).astype(F32)
        px, py = F32(rec["px"][j]), F32(rec["py"][j])
        rx, ry = q[:, 0] - px, q[:, 1] - py
        tx = rx * cx - ry * cy
        ty = rx * cy + ry * cx
        return np.stack([px + tx, py + ty], axis=1).astype(F32)


def gate(rec, j, R, pos, prev, r):
    """mover_sweep_gate: sweep_measure with the pivot as the point and prev -> pos as the capsule of radius arm + R"""
    p, q, r = np.asarray(pos, F32).reshape(-1, 2), np.asarray(prev, F32).reshape(-1, 2), _f(r)
    px, py = F32(rec["px"][j]), F32(rec["py"][j])
    with np.errstate(all="ignore"):
        reach = F32(F32(rec["arm"][j]) + F32(R))
        a = np.abs(r)
        dx, dy = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1]
        fx, fy = px - q[:, 0], py - q[:, 1]
        A = dx * dx + dy * dy
        u = np.where(A > ZERO, (fx * dx + fy * dy) / np.where(A > ZERO, A, ONE), ZERO).astype(F32)
        u = np.where(u > ZERO, u, ZERO).astype(F32)
        u = np.where(u < ONE, u, ONE).astype(F32)
        qx, qy = fx - u * dx, fy - u * dy
        h = qx * qx + qy * qy
        s = (reach + a).astype(F32)
        return h < s * s


NAMES = ("t", "depth", "x", "y", "nx", "ny", "gap", "s")


def judge(rec, j, cap, pos, prev, r):
    """mover_sweep_judge: steps 1 to 4 for mover j with its new capsule cap = (ax, ay, bx, by, R) -> the contact dict of
    _sweep_model.contact, and `plain` bool[n]"""
    p, q, r = np.ascontiguousarray(pos, F32).reshape(-1, 2), np.ascontiguousarray(prev, F32).reshape(-1, 2), _f(r)
    y0 = carry(rec, j, q)
    plain = S.plain_particles(p, y0)
    k = S.contact(y0[:, 0], y0[:, 1], p[:, 0], p[:, 1], r, cap)
    touched, depth, nx, ny, _, s = S.measure(p[:, 0], p[:, 1], r, cap)
    ok = np.ones(len(r), bool) if int(rec["kind"][j]) != TURN else gate(rec, j, cap[4], p, q, r)
    flat = dict(t=np.ones(len(r), F32), depth=depth, x=p[:, 0], y=p[:, 1], nx=nx, ny=ny, gap=depth, s=s)
    out = {name: np.where(plain, flat[name], k[name]).astype(F32) for name in NAMES}
    out["has"] = np.where(plain, touched, k["has"] & ok)
    return out, plain


def search(pos, prev, r, rec, caps):
    """every mover on its own relative path to pos -> (winner dict with `who`, over_slop bool[n])"""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    n = len(p)
    best = dict(has=np.zeros(n, bool), who=np.zeros(n, np.int64))
    for name in NAMES:
        best[name] = np.zeros(n, F32)
    over = np.zeros(n, bool)
    for j, c in enumerate(np.ascontiguousarray(caps, F32).reshape(-1, 5)):
        k, _ = judge(rec, j, c, p, prev, r)
        with np.errstate(all="ignore"):
            over |= k["has"] & (k["depth"] > S.SLOP * k["s"])
        better = (k["t"] < best["t"]) | ((k["t"] == best["t"]) & (k["depth"] > best["depth"]))   # (a tie: the lower j stays)
        take = k["has"] & (~best["has"] | better)
        for name in NAMES:
            best[name] = np.where(take, k[name], best[name]).astype(F32)
        best["who"] = np.where(take, j, best["who"])
        best["has"] |= take
    return best, over


def apply(pos, prev, rad, old, caps, rec, world, surfaces=None):
    """The swept pass -> (pos', prev', info): old f32[k, 4] the capsules before the advance, caps f32[k, 5] after it with
    the radii, rec carry_records(); info = dict(moved, swept, stopped, who) of bool[n] / i64[n]."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    q0 = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    r = _f(rad)
    caps = np.ascontiguousarray(caps, F32).reshape(-1, 5)
    old = np.ascontiguousarray(old, F32).reshape(-1, 4)
    n = len(r)
    W, H = F32(world[0]), F32(world[1])
    if len(caps) == 0:
        none = np.zeros(n, bool)
        return p.copy(), q0.copy(), dict(moved=none, swept=none, stopped=none, who=np.zeros(n, np.int64))
    win, _ = search(p, q0, r, rec, caps)
    who = win["who"]
    with np.errstate(all="ignore"):
        qx = CM.clamp_f(p[:, 0] + win["nx"] * win["depth"], r, W - r)
        qy = CM.clamp_f(p[:, 1] + win["ny"] * win["depth"], r, H - r)
        q = np.stack([qx, qy], axis=1).astype(F32)
        new_prev = q0.copy()
        if surfaces is not None:
            row = np.ascontiguousarray(surfaces, SM.SURFACE_DTYPE).reshape(-1)[who]
            acts = win["has"] & ((row["flags"] & SM.PLAIN) == 0) & SM.velocity_finite(p, q0)
            at = np.stack([win["x"], win["y"]], axis=1).astype(F32)
            u = np.zeros(n, F32)
            for j in np.unique(who[acts]):
                u = np.where(who == j, SM.contact_u(at, caps[j]), u)
            wx, wy = SM.wall_move(old[who], caps[who, :4], u)
            s_pos, s_prev, _ = SM.respond(p, q0, r, win["nx"], win["ny"], win["depth"], wx, wy, row["restitution"],
                                          row["friction"], world)
            q = np.where(acts[:, None], s_pos, q).astype(F32)
            new_prev = np.where(acts[:, None], s_prev, new_prev).astype(F32)
        _, over = search(q, q0, r, rec, caps)
        g = np.where(win["gap"] > ZERO, win["gap"], ZERO).astype(F32)
        sx = CM.clamp_f(win["x"] + win["nx"] * g, r, W - r)
        sy = CM.clamp_f(win["y"] + win["ny"] * g, r, H - r)
    stopped = win["has"] & over
    swept = win["has"] & (win["t"] > ZERO) & (win["t"] < ONE)
    out = np.where(stopped[:, None], np.stack([sx, sy], axis=1), q).astype(F32)
    out = np.where(win["has"][:, None], out, p).astype(F32)
    out_prev = np.where((win["has"] & ~stopped)[:, None], new_prev, q0).astype(F32)
    return out, out_prev, dict(moved=win["has"].copy(), swept=swept, stopped=stopped, who=who)


class Movers(SM.Movers):
    """tests/_surfaces_model.Movers with the mode: the pass in its swept form while on.  The mode is not the set's: a
    new set leaves it alone."""
    sweep = False
    sweep_passes = swept = stopped = 0
    last = None                                                        # the info of the last swept pass

    def set_sweep(self, on):
        self.sweep = bool(on)
        self.sweep_passes = self.swept = self.stopped = 0

    def step_state(self, dt):
        """advance by dt -> (old f32[k, 4], caps f32[k, 5], rec)"""
        p0, p1 = self.q0.copy(), self.q1.copy()
        old = M.pose(self.movers, p0, p1)
        self.q0, self.q1 = M.advance(self.movers, p0, p1, dt)
        caps = self.capsules()
        return old, caps, carry_records(self.movers, dt, p0, p1, self.q0, self.q1, old, caps[:, :4])

    def apply_surface(self, pos, prev, rad, world, dt):
        if not self.sweep:
            return super().apply_surface(pos, prev, rad, world, dt)
        old, caps, rec = self.step_state(dt)
        out, new_prev, info = apply(pos, prev, rad, old, caps, rec, world, surfaces=self.surfaces)
        self.passes += 1
        self.sweep_passes += 1
        self.pushed += int(info["moved"].sum())
        self.swept += int(info["swept"].sum())
        self.stopped += int(info["stopped"].sum())
        self.last = info
        return out, new_prev, info["moved"], None


class Mixin:
    """set_mover_sweep for a twin whose movers are self.m (the _surfaces_model.Twin family): in front of it in the bases"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.m = Movers()

    def set_mover_sweep(self, on):
        self.m.set_sweep(on)

    def mover_sweep_info(self):
        return dict(mode=int(self.m.sweep), passes=self.m.sweep_passes, swept=self.m.swept, stopped=self.m.stopped)


class Twin(Mixin, S.Twin):
    """tests/_sweep_model.Twin (movers, static colliders, their surfaces, the static sweep, fields) with the movers' sweep"""


# ---- the two tunnelling scenes -------------------------------------------------------------------------------------------
SCENE_WORLD = (240.0, 200.0)
SCENE_DT = 1.0 / 60.0
SCENE_RADIUS = 1.0
GATE = M.rows(M.linear((50, 30), (50, 170), 0.0, v=(1200.0, 0.0)))     # R = 0, 20 units per step
BLADE = M.rows(M.rotor((100, 100), (150, 100), 0.0, (100, 100), 24.0))  # R = 0, 0.4 rad per step


def gate_scene():
    """-> (movers, pos, prev, rad): 6 x 36 particles of radius 1 on a lattice of spacing 3 inside the parallelogram the
    gate sweeps in its first step (x in 50 .. 70), every one more than 1.5 ahead of the old face and 1.5 behind the new
    one; every third drifts by up to 0.2 per step, the others rest"""
    i = np.arange(6 * 36)
    pos = np.stack([52.0 + 3.0 * (i % 6), 40.0 + 3.25 * (i // 6) + 0.5 * (i % 6)], axis=1).astype(F32)
    rng = np.random.default_rng(5)
    v = rng.uniform(-0.2, 0.2, pos.shape) * (i % 3 == 0)[:, None]
    prev = (pos - v.astype(F32)).astype(F32)
    return GATE, pos, prev, np.full(len(pos), SCENE_RADIUS, F32)


def blade_scene():
    """-> (movers, pos, prev, rad): particles of radius 1 at rest inside the sector the blade sweeps in its first step,
    each more than 1.3 ahead of the old blade and 1.3 behind the new one, 3.2 apart"""
    out = []
    for rho in np.arange(9.0, 46.0, 3.2):
        margin = np.arcsin(1.3 / rho)
        for th in np.arange(margin, 0.4 - margin, 3.2 / rho):
            out.append((100.0 + rho * np.cos(th), 100.0 + rho * np.sin(th)))
    pos = np.array(out, F32)
    return BLADE, pos, pos.copy(), np.full(len(pos), SCENE_RADIUS, F32)


def first_pose(movers, dt=SCENE_DT):
    """the posed capsule of the one mover after its first advance, float64 (ax, ay, bx, by)"""
    q0, q1 = M.fresh(movers)
    q0, q1 = M.advance(movers, q0, q1, dt)
    return M.pose(movers, q0, q1)[0].astype(np.float64)


def check_leading(cap, out, side, s=SCENE_RADIUS):
    """float64, no tolerance -> (behind bool[n], close bool[n]): the particle ended on the trailing side of the capsule
    cap (side = +1: the leading side is where cross(b - a, x - a) > 0); it ended nearer than s (1 - 2^-9) to its line"""
    a, b = np.asarray(cap[0:2], np.float64), np.asarray(cap[2:4], np.float64)
    o = np.asarray(out, np.float64)
    d = b - a
    cross = side * (d[0] * (o[:, 1] - a[1]) - d[1] * (o[:, 0] - a[0]))
    dist = cross / np.sqrt(d @ d)
    return ~(cross > 0), ~(dist >= s * (1.0 - 2.0 ** -9))


GATE_SIDE, BLADE_SIDE = -1.0, 1.0      # the gate a -> b points along +y and moves along +x; the blade turns counter-clockwise


def one_pass(movers, pos, prev, rad, sweep, world=SCENE_WORLD, dt=SCENE_DT, surfaces=None):
    """gpe_apply_movers(dt) on a fresh set -> (pos', prev', Movers)"""
    mv = Movers(movers)
    if surfaces is not None:
        mv.set_surfaces(surfaces)
    mv.set_sweep(sweep)
    out, out_prev, _, _ = mv.apply_surface(pos, prev, rad, world, dt)
    return out, out_prev, mv


# ---- the table tests/cpp/mover_sweep_tests.cpp replays (tests/golden/mover_sweep_cases.txt) ------------------------------
TABLE_WORLD = (200.0, 200.0)
TABLE_DT = 1.0 / 60.0
TABLE_RB = 1.0
TABLE_WARM = 3                                                         # advances before the judged one: no state is fresh


def table_movers():
    return M.rows(M.linear((40, 20), (40, 90), 0.0, v=(900.0, 0.0)),                      # 0 a thin gate, 15 per step
                  M.linear((150, 20), (150, 90), 0.25, v=(-540.0, 60.0)),                 # 1 closing on it from the right
                  M.linear((20, 110), (90, 110), 0.5, v=(0.0, 0.0), travel=3.0),          # 2 stationary
                  M.linear((110, 100), (110, 140), 0.0, v=(600.0, 0.0), travel=33.0),     # 3 reflects in the judged step
                  M.linear((30, 160), (30, 160), 1.0, v=(300.0, 120.0)),                  # 4 a disc (zero length)
                  M.rotor((100, 60), (135, 60), 0.0, (100, 60), 24.0),                    # 5 a blade, 0.4 rad per step
                  M.rotor((60, 150), (80, 150), 0.5, (70, 150), -18.0),                   # 6 a paddle about its middle
                  M.rotor((150, 150), (170, 150), 0.5, (150, 150), 0.0),                  # 7 a rotor that stands still
                  M.rotor((178, 40), (190, 40), 0.0, (170, 40), 15.0))                    # 8 a blade off its pivot


def table_cases():
    """400 particles around the movers' motions: resting, drifting, fast (the chord and gate cases), squeezed between
    movers 0 and 1, with radii above the lookup's bound, NaN and infinite prev, paths that leave the grid and boxes
    wider than 16 cells"""
    mv = Movers(table_movers())
    for _ in range(TABLE_WARM):
        mv.q0, mv.q1 = M.advance(mv.movers, mv.q0, mv.q1, TABLE_DT)
    start = (mv.q0.copy(), mv.q1.copy())
    rng = np.random.default_rng(77)
    n = 400
    pos = rng.uniform(5, 195, (n, 2))
    kindof = np.arange(n) % 8
    v = np.zeros((n, 2))
    v[kindof == 1] = rng.uniform(-0.3, 0.3, ((kindof == 1).sum(), 2))
    v[kindof == 2] = rng.uniform(-12, 12, ((kindof == 2).sum(), 2))
    v[kindof == 3] = rng.uniform(-60, 60, ((kindof == 3).sum(), 2))
    sq = kindof == 4                                                   # the squeeze: between the gate and mover 1
    pos[sq] = np.stack([rng.uniform(85, 130, sq.sum()), rng.uniform(25, 85, sq.sum())], axis=1)
    bl = kindof == 5                                                   # about the blade
    rho, th = rng.uniform(2, 40, bl.sum()), rng.uniform(0.8, 2.4, bl.sum())
    pos[bl] = np.stack([100 + rho * np.cos(th), 60 + rho * np.sin(th)], axis=1)
    v[bl] = rng.uniform(-4, 4, (bl.sum(), 2)) * (rng.random(bl.sum()) < 0.5)[:, None]
    pos = pos.astype(F32)
    prev = (pos - v.astype(F32)).astype(F32)
    prev[7::40, 0] = np.nan
    prev[11::40, 1] = np.inf
    prev[13::40] = (-150.0, 90.0)                                      # from far outside the grid
    rad = rng.choice(np.array([0.5, 1.0, -0.5, 0.25], F32), n)
    rad[17::40] = 2.5                                                  # above TABLE_RB
    surf = SM.scene_surfaces(len(mv.movers), seed=43)
    old, caps, rec = mv.step_state(TABLE_DT)
    plain = apply(pos, prev, rad, old, caps, rec, TABLE_WORLD)
    with_s = apply(pos, prev, rad, old, caps, rec, TABLE_WORLD, surfaces=surf)
    return dict(movers=mv.movers, start=start, surf=surf, pos=pos, prev=prev, rad=rad, plain=plain, surface=with_s, caps=caps,
                old=old, rec=rec)


def _hex(a):
    return " ".join("%08x" % w for w in np.ascontiguousarray(a, F32).reshape(-1).view(U32))


def table_text():
    """`m` lines: the 14 words of a mover's row, its state before the judged advance, its surface row; `c` lines: px py
    prevx prevy r | flags who posx posy prevx prevy without surfaces | the same with them; flags = moved + 2 swept +
    4 stopped; who the winner (0 when not moved); every float the hex word of its binary32"""
    t = table_cases()
    lines = ["# m <j> <14 words of gpe_mover> q0 q1  e mu flags", "# c <i> px py prevx prevy r  flags who posx posy prevx prevy  flags who posx posy prevx prevy",
             "# binary32 words in hex; the world is %g x %g, dt the word %s, the lookup's radius bound %g" % (TABLE_WORLD + (_hex(TABLE_DT), TABLE_RB)),
             "# written by tests/_mover_sweep_model.table_text()"]
    for j in range(len(t["movers"])):
        lines.append("m %d %s %s %s %d" % (j, " ".join("%08x" % w for w in np.frombuffer(t["movers"][j].tobytes(), U32)),
                                           _hex([t["start"][0][j], t["start"][1][j]]),
                                           _hex([t["surf"]["restitution"][j], t["surf"]["friction"][j]]), t["surf"]["flags"][j]))
    for i in range(len(t["rad"])):
        parts = ["c %d" % i, _hex(t["pos"][i]), _hex(t["prev"][i]), _hex(t["rad"][i])]
        for out, out_prev, info in (t["plain"], t["surface"]):
            flags = int(info["moved"][i]) + 2 * int(info["swept"][i]) + 4 * int(info["stopped"][i])
            parts += ["%d %d" % (flags, info["who"][i] if info["moved"][i] else 0), _hex(out[i]), _hex(out_prev[i])]
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"


# ---- the stepped scene: _sweep_model's sparse box with a thin piston and a thin blade ------------------------------------
STEP_DT = S.STEP_DT
STEP_STEPS = 48
STEP_MOVER_SURFACES = SM.rows((0.4, 0.2), (0.9, 0.0, SM.PLAIN))


def step_movers():
    """a piston of R = 0 that slides 2.5 per step (ten particle radii) and turns around every 12 steps, and a blade of
    R = 0 at 0.3 rad per step whose tip moves 4.5 per step"""
    return M.rows(M.linear((35, 30), (35, 70), 0.0, v=(150.0, 0.0), travel=30.0),
                  M.rotor((60, 50), (75, 50), 0.0, (60, 50), 18.0))


def step_twin(oracle, mover_sweep=True, collider_sweep=True, surfaces=None):
    pos, rad = S.step_scene()
    tw = Twin(oracle, pos, rad, world=S.STEP_WORLD, gravity=S.STEP_GRAVITY)
    tw.set_colliders(S.step_colliders())
    tw.set_movers(step_movers())
    tw.set_fields(S.STEP_FIELDS)
    if surfaces is not None:
        tw.set_surfaces("movers", surfaces)
    tw.set_collider_sweep(collider_sweep)
    tw.set_mover_sweep(mover_sweep)
    return tw


def step_reference(oracle, resort_every=0, resort_first=False, mover_sweep=True, surfaces=None, steps=STEP_STEPS, kick_every=4):
    """-> (frames of (pos, prev, poses) after every step, dict of the counters): _sweep_model's kick before every
    kick_every-th step, the oracle's step, then the model's passes (swept movers, swept colliders, fields)"""
    from tests._oracle_model import VEL_SET, circle_mask
    tw = step_twin(oracle, mover_sweep=mover_sweep, surfaces=surfaces)
    frames = []
    for s in range(steps):
        if s % kick_every == 0:
            p, _, _ = tw.arrays()
            tw.kick(circle_mask(p, *S.STEP_KICK_DISC), VEL_SET, *S.step_kick(s))
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(STEP_DT, resort=bool(resort))
        p, q, _ = tw.arrays()
        frames.append((p.copy(), q.copy(), tw.m.poses()))
    counts = dict(pushed=tw.m.pushed, passes=tw.m.sweep_passes, swept=tw.m.swept, stopped=tw.m.stopped, colliders=tw.pushed)
    tw.close()
    return frames, counts
