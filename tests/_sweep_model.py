"""The numpy float32 restatement of the swept form of the static colliders' pass (include/gpe.h "static colliders",
csrc/k_sweep.h): brute force over all colliders, vectorised over the particles, no grid, in the exact operation order of
the header, one binary32 rounding per operation, no FMA.  The plain parts are tests/_colliders_model.apply and
tests/_surfaces_model.apply / respond.  TEST INFRASTRUCTURE ONLY.

apply() is the pass; Twin an OracleModel that holds the sets, their surfaces and the sweep mode the way a context does;
box_scene() the closed box of the CPU and GPU tests with check_box() its float64 checker; table_text() the cases
tests/cpp/sweep_tests.cpp replays (tests/golden/sweep_cases.txt)."""
import numpy as np

from tests import _colliders_model as CM
from tests import _fields_model as FM
from tests import _surfaces_model as SM

F32 = np.float32
U32 = np.uint32
SLOP = F32(2.0 ** -10)
SLACK = F32(2.0 ** -19)
ZERO, ONE = F32(0), F32(1)


def _f(a):
    return np.ascontiguousarray(a, F32).reshape(-1)


def measure(x, y, r, c):
    """sweep_measure: one collider c = (ax, ay, bx, by, R) at the points (x, y) -> (touched, depth, nx, ny, d, s)"""
    ax, ay, bx, by, R = (F32(v) for v in c)
    with np.errstate(all="ignore"):
        a = np.abs(r)
        dx = F32(bx - ax)
        dy = F32(by - ay)
        fx = x - ax
        fy = y - ay
        A = F32(F32(dx * dx) + F32(dy * dy))
        if A > 0:
            u = (fx * dx + fy * dy) / A
        else:
            u = np.zeros_like(x)
        u = np.where(u > ZERO, u, ZERO).astype(F32)
        u = np.where(u < ONE, u, ONE).astype(F32)
        qx = fx - u * dx
        qy = fy - u * dy
        h = qx * qx + qy * qy
        s = (R + a).astype(F32)
        touched = h < s * s
        d = np.sqrt(h)
        depth = (s - d).astype(F32)
        if A > 0:
            L = np.sqrt(A)
            ex, ey = F32(F32(-dy) / L), F32(dx / L)
        else:
            ex, ey = ONE, ZERO
        on = d > ZERO
        safe = np.where(on, d, ONE)
        nx = np.where(on, qx / safe, ex).astype(F32)
        ny = np.where(on, qy / safe, ey).astype(F32)
    return touched, depth, nx, ny, d.astype(F32), s


def disc_root(fx, fy, mx, my, s):
    """sweep_disc_root -> f32[n], -1 where there is none"""
    with np.errstate(all="ignore"):
        bq = fx * mx + fy * my
        cq = (fx * fx + fy * fy) - s * s
        am = mx * mx + my * my
        disc = bq * bq - am * cq
        sq = np.sqrt(np.where(disc >= ZERO, disc, ZERO)).astype(F32)
        den = sq - bq
        root = cq / np.where(den != ZERO, den, ONE)
        out = np.full(len(fx), -1, F32)
        out = np.where(cq <= ZERO, ZERO, out)
        out = np.where((cq > ZERO) & (disc >= ZERO), root, out)
        out = np.where(bq < ZERO, out, F32(-1))
    return out.astype(F32)


def contact(x0, y0, x1, y1, r, c):
    """sweep_contact for every particle against one collider -> dict(has, t, depth, x, y, nx, ny, gap, s)"""
    x0, y0, x1, y1, r = _f(x0), _f(y0), _f(x1), _f(y1), _f(r)
    ax, ay, bx, by, R = (F32(v) for v in c)
    n = len(r)
    with np.errstate(all="ignore"):
        t0, dep0, nx0, ny0, d0, s = measure(x0, y0, r, c)
        mx = x1 - x0
        my = y1 - y0
        ext = ((np.abs(x0) + np.abs(y0)) + np.abs(x1)) + np.abs(y1)
        lim = s + SLACK * ext
        dx, dy = F32(bx - ax), F32(by - ay)
        A = F32(F32(dx * dx) + F32(dy * dy))
        fx = x0 - ax
        fy = y0 - ay
        none = np.full(n, -1, F32)
        cands = [none, disc_root(fx, fy, mx, my, s), none]
        if A > 0:
            L = np.sqrt(A)
            sL = s * L
            c0 = dx * fy - dy * fx
            cm = dx * my - dy * mx
            den = np.where(c0 >= ZERO, -cm, cm).astype(F32)
            over = np.abs(c0) - sL
            num = np.where(over > ZERO, over, ZERO).astype(F32)
            cands[0] = np.where(den > ZERO, num / np.where(den > ZERO, den, ONE), F32(-1)).astype(F32)
            cands[2] = disc_root(x0 - bx, y0 - by, mx, my, s)
        have = np.zeros(n, bool)
        t = np.zeros(n, F32)
        X, Y = x0.copy(), y0.copy()
        gap, nx, ny = dep0.copy(), nx0.copy(), ny0.copy()
        for tk in cands:
            ok = (tk >= ZERO) & (tk <= ONE) & (~have | (tk < t))
            xk = x0 + tk * mx
            yk = y0 + tk * my
            _, depk, nxk, nyk, dk, _ = measure(xk, yk, r, c)
            ok &= dk <= lim
            have |= ok
            t = np.where(ok, tk, t)
            X, Y = np.where(ok, xk, X), np.where(ok, yk, Y)
            gap, nx, ny = np.where(ok, depk, gap), np.where(ok, nxk, nx), np.where(ok, nyk, ny)
        t1, dep1, nx1, ny1, _, _ = measure(x1, y1, r, c)
        net = ~t0 & ~have & t1
        t = np.where(net, ONE, t)
        X, Y = np.where(net, x1, X), np.where(net, y1, Y)
        gap, nx, ny = np.where(net, dep1, gap), np.where(net, nx1, nx), np.where(net, ny1, ny)
        # (x0 touched: t = 0 at x0 with its own quantities, which is what the arrays were started with)
        t = np.where(t0, ZERO, t)
        X, Y = np.where(t0, x0, X), np.where(t0, y0, Y)
        gap, nx, ny = np.where(t0, dep0, gap), np.where(t0, nx0, nx), np.where(t0, ny0, ny)
        depth = gap + (nx * (X - x1) + ny * (Y - y1))
        has = (t0 | have | net) & (depth > ZERO)
    return dict(has=has, t=t.astype(F32), depth=depth.astype(F32), x=X.astype(F32), y=Y.astype(F32), nx=nx.astype(F32),
                ny=ny.astype(F32), gap=gap.astype(F32), s=s)


def search(p0, p1, r, colliders):
    """every collider on the paths p0 -> p1 -> (winner dict with `who`, over_slop bool[n])"""
    p0, p1 = np.ascontiguousarray(p0, F32).reshape(-1, 2), np.ascontiguousarray(p1, F32).reshape(-1, 2)
    n = len(p0)
    best = dict(has=np.zeros(n, bool), who=np.zeros(n, np.int64))
    for name in ("t", "depth", "x", "y", "nx", "ny", "gap", "s"):
        best[name] = np.zeros(n, F32)
    over = np.zeros(n, bool)
    for j, c in enumerate(np.ascontiguousarray(colliders, F32).reshape(-1, 5)):
        k = contact(p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1], r, c)
        with np.errstate(all="ignore"):
            over |= k["has"] & (k["depth"] > SLOP * k["s"])
        better = (k["t"] < best["t"]) | ((k["t"] == best["t"]) & (k["depth"] > best["depth"]))   # (a tie: the lower j stays)
        take = k["has"] & (~best["has"] | better)
        for name in ("t", "depth", "x", "y", "nx", "ny", "gap", "s"):
            best[name] = np.where(take, k[name], best[name]).astype(F32)
        best["who"] = np.where(take, j, best["who"])
        best["has"] |= take
    return best, over


def plain_particles(pos, prev):
    with np.errstate(all="ignore"):
        m = np.asarray(pos, F32) - np.asarray(prev, F32)
    return ~np.isfinite(m).all(axis=1) | ((m[:, 0] == 0) & (m[:, 1] == 0))


def apply(pos, prev, rad, colliders, world, surfaces=None):
    """The swept pass -> (pos', prev', info): info = dict(moved, swept, stopped, plain) of bool[n]."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    q0 = np.ascontiguousarray(prev, F32).reshape(-1, 2)
    r = _f(rad)
    cs = np.ascontiguousarray(colliders, F32).reshape(-1, 5)
    n = len(r)
    W, H = F32(world[0]), F32(world[1])
    plain = plain_particles(p, q0)
    if surfaces is None:
        pl_pos, pl_moved = CM.apply(p, r, cs, world)
        pl_prev = q0
    else:
        pl_pos, pl_prev, pl_moved, _ = SM.apply(p, q0, r, cs, surfaces, world)
    win, _ = search(q0, p, r, cs)
    with np.errstate(all="ignore"):
        qx = CM.clamp_f(p[:, 0] + win["nx"] * win["depth"], r, W - r)
        qy = CM.clamp_f(p[:, 1] + win["ny"] * win["depth"], r, H - r)
        q = np.stack([qx, qy], axis=1).astype(F32)
        new_prev = q0.copy()
        acts = np.zeros(n, bool)
        if surfaces is not None:
            row = np.ascontiguousarray(surfaces, SM.SURFACE_DTYPE).reshape(-1)[win["who"]]
            acts = win["has"] & ((row["flags"] & SM.PLAIN) == 0)
            s_pos, s_prev, _ = SM.respond(p, q0, r, win["nx"], win["ny"], win["depth"], np.zeros(n, F32), np.zeros(n, F32),
                                          row["restitution"], row["friction"], world)
            q = np.where(acts[:, None], s_pos, q).astype(F32)
            new_prev = np.where(acts[:, None], s_prev, new_prev).astype(F32)
        _, over = search(q0, q, r, cs)
        g = np.where(win["gap"] > ZERO, win["gap"], ZERO).astype(F32)
        sx = CM.clamp_f(win["x"] + win["nx"] * g, r, W - r)
        sy = CM.clamp_f(win["y"] + win["ny"] * g, r, H - r)
    stopped = win["has"] & over & ~plain
    moved = np.where(plain, pl_moved, win["has"])
    swept = win["has"] & ~plain & (win["t"] > ZERO) & (win["t"] < ONE)
    out = np.where(stopped[:, None], np.stack([sx, sy], axis=1), q).astype(F32)
    out = np.where(win["has"][:, None], out, p)
    out_prev = np.where((win["has"] & ~stopped)[:, None], new_prev, q0)
    out = np.where(plain[:, None], pl_pos, out).astype(F32)
    out_prev = np.where(plain[:, None], pl_prev, out_prev).astype(F32)
    return out, out_prev, dict(moved=moved, swept=swept, stopped=stopped, plain=plain)


class Twin(SM.Twin):
    """tests/_surfaces_model.Twin with the sweep mode: the static colliders' pass in its swept form while on"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sweep = False
        self.sweep_passes = self.swept = self.stopped = 0
        self.fields = np.zeros(0, FM.DTYPE)

    def set_collider_sweep(self, on):
        self.sweep = bool(on)
        self.sweep_passes = self.swept = self.stopped = 0

    def set_fields(self, fields):
        self.fields = FM.stored(fields)

    def step(self, dt, resort=False):
        """step -> movers -> colliders -> fields, the order of gpe_step"""
        super().step(dt, resort=resort)
        if len(self.fields):
            self._pull()
            self.prev, _ = FM.apply(self.pos, self.prev, self.fields, dt)

    def apply_colliders(self):
        if not self.sweep:
            return super().apply_colliders()
        if len(self.colliders) == 0:
            return
        self._pull()
        self.pos, self.prev, info = apply(self.pos, self.prev, self.radius, self.colliders, self.world,
                                          surfaces=self.collider_surfaces)
        self.passes += 1
        self.sweep_passes += 1
        self.pushed += int(info["moved"].sum())
        self.swept += int(info["swept"].sum())
        self.stopped += int(info["stopped"].sum())


# ---- the closed box ---------------------------------------------------------------------------------------------------
BOX_WORLD = (200.0, 200.0)
BOX_LO, BOX_HI = 40.0, 160.0
V_APEX = (100.0, 70.0)
V_ENDS = ((85.0, 96.0), (115.0, 96.0))                                 # two arms of length ~30.02, 60 degrees apart
PEG = (70.0, 80.0, 3.0)
LINE_Y, LINE_X, LINE_R = 130.0, (60.0, 90.0, 120.0, 150.0), 0.25
BOX_RADIUS = 0.5


def box_colliders(R):
    """the four walls of radius R, then the V (R = 0), the straight polyline of three segments, the disc peg"""
    lo, hi = BOX_LO, BOX_HI
    rows = [[lo, lo, hi, lo, R], [hi, lo, hi, hi, R], [hi, hi, lo, hi, R], [lo, hi, lo, lo, R]]
    rows += [[V_APEX[0], V_APEX[1], e[0], e[1], 0.0] for e in V_ENDS]
    rows += [[LINE_X[i], LINE_Y, LINE_X[i + 1], LINE_Y, LINE_R] for i in range(3)]
    rows.append([PEG[0], PEG[1], PEG[0], PEG[1], PEG[2]])
    return np.array(rows, F32)


def _seg_dist(p, c):
    a, b = c[0:2].astype(np.float64), c[2:4].astype(np.float64)
    d = b - a
    A = float(d @ d)
    f = p - a
    u = np.clip((f @ d) / A, 0, 1) if A > 0 else np.zeros(len(p))
    return np.linalg.norm(f - u[:, None] * d, axis=1)


def box_scene(R, n=4000, seed=11):
    """-> (colliders, start f32[n, 2], end f32[n, 2], rad): particles of radius 0.5 that start inside the box at least
    1.01 s from every collider and are displaced by 0.1 to 150 in every direction; the first rows are the aimed ones:
    at wall end points and box corners, grazing at offset s -/+ one ulp, parallel at distance exactly s, along an axis,
    wholly through the peg."""
    cs = box_colliders(R)
    rng = np.random.default_rng(seed)
    r = BOX_RADIUS
    start = np.zeros((0, 2))
    while len(start) < n:
        cand = rng.uniform(BOX_LO, BOX_HI, (2 * n, 2))
        ok = np.ones(len(cand), bool)
        for c in cs:
            ok &= _seg_dist(cand.astype(F32).astype(np.float64), c) >= 1.01 * (float(c[4]) + r) + 1e-3
        start = np.concatenate([start, cand[ok]])
    start = start[:n].astype(F32)
    ang = rng.uniform(0, 2 * np.pi, n)
    length = np.exp(rng.uniform(np.log(0.1), np.log(150.0), n))
    end = (start.astype(np.float64) + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(F32)
    # the aimed rows
    targets = [(BOX_LO, BOX_LO), (BOX_HI, BOX_LO), (BOX_HI, BOX_HI), (BOX_LO, BOX_HI), V_APEX, V_ENDS[0], V_ENDS[1],
               (LINE_X[0], LINE_Y), (LINE_X[1], LINE_Y), (LINE_X[2], LINE_Y), (LINE_X[3], LINE_Y), PEG[:2]]
    i = 0
    for k in range(40):                                                # at end points, corners, joints and through the peg
        for tx, ty in targets:
            v = np.array([tx, ty]) - start[i].astype(np.float64)
            end[i] = (start[i].astype(np.float64) + v * (1.0 + 0.35 * k)).astype(F32)
            i += 1
    s = F32(R) + F32(r)
    top = F32(F32(BOX_LO) + s)                                         # the centre line at distance exactly s of wall 0
    for k, y in enumerate((top, np.nextafter(top, F32(0)), np.nextafter(top, F32(1e9)))):
        for x0, x1 in ((50.0, 150.0), (150.0, 50.0), (50.0, 159.0), (41.0, 150.0)):
            # parallel to wall 0 at s, s - ulp, s + ulp (the start is moved in to y: these few start closer than 1.01 s)
            start[i] = (x0, y)
            end[i] = (x1, y)
            i += 1
            # grazing: tangent to the peg inflated by 0.5, at offset s, s - ulp, s + ulp of its centre
            yt = F32(F32(PEG[1]) + F32(PEG[2] + r))
            yt = (yt, np.nextafter(yt, F32(0)), np.nextafter(yt, F32(1e9)))[k]
            start[i] = (PEG[0] + (x0 - 100.0) * 0.3, yt)
            end[i] = (PEG[0] + (x1 - 100.0) * 0.3, yt)
            i += 1
    for x0, x1 in ((45.0, 155.0), (155.0, 45.0)):                      # along the polyline's axis into its end, and along y
        start[i], end[i] = (x0, LINE_Y), (x1, LINE_Y)
        i += 1
        start[i], end[i] = (50.0, 100.0), (50.0, 100.0 + (x1 - x0))
        i += 1
    for k in range(16):                                                # not finite: the plain rule
        end[i] = start[i] + F32(3)
        i += 1
    rad = np.full(n, r, F32)
    return cs, start, end, rad


def box_prev(start, n_odd=16):
    """the scene's prev: its start, the last aimed rows NaN or infinite"""
    prev = start.copy()
    first = 40 * 12 + 3 * 4 * 2 + 4
    for k in range(n_odd):
        prev[first + k, k % 2] = np.nan if k % 4 < 2 else np.inf
    return prev


def _cross(o, a, b):
    return (a[..., 0] - o[..., 0]) * (b[..., 1] - o[..., 1]) - (a[..., 1] - o[..., 1]) * (b[..., 0] - o[..., 0])


def check_box(start, out, finite):
    """float64, no tolerance -> (outside bool[n], crossed bool[n]): ended outside the box polygon; the segment start ->
    out crosses an arm of the V"""
    s, o = np.asarray(start, np.float64), np.asarray(out, np.float64)
    inside = (o[:, 0] > BOX_LO) & (o[:, 0] < BOX_HI) & (o[:, 1] > BOX_LO) & (o[:, 1] < BOX_HI)
    crossed = np.zeros(len(s), bool)
    a = np.array(V_APEX, np.float64)
    for e in V_ENDS:
        b = np.array(e, np.float64)
        d1, d2 = _cross(a, b, s), _cross(a, b, o)
        d3, d4 = _cross(s, o, a[None, :]), _cross(s, o, b[None, :])
        crossed |= (d1 * d2 < 0) & (d3 * d4 < 0)
    return finite & ~inside, finite & crossed


# ---- the table tests/cpp/sweep_tests.cpp replays (tests/golden/sweep_cases.txt) ----------------------------------------
TABLE_N = 600


def table_cases():
    """the first TABLE_N rows of the box scene (R = 0.05; the aimed rows and some random ones), against all its
    colliders with mixed surfaces, and without"""
    cs, start, end, rad = box_scene(0.05)
    prev = box_prev(start)
    sl = slice(0, TABLE_N)
    surf = SM.scene_surfaces(len(cs), seed=41)
    plain = apply(end[sl], prev[sl], rad[sl], cs, BOX_WORLD)
    with_s = apply(end[sl], prev[sl], rad[sl], cs, BOX_WORLD, surfaces=surf)
    return dict(cs=cs, surf=surf, pos=end[sl], prev=prev[sl], rad=rad[sl], plain=plain, surface=with_s)


def _hex(a):
    return " ".join("%08x" % w for w in np.ascontiguousarray(a, F32).reshape(-1).view(U32))


def table_text():
    """`k` lines: one collider with its surface row; `c` lines: px py prevx prevy r | flags posx posy prevx prevy without
    surfaces | the same with them; flags = moved + 2 swept + 4 stopped; every float the hex word of its binary32"""
    t = table_cases()
    lines = ["# k <j> ax ay bx by R  e mu flags", "# c <i> px py prevx prevy r  flags posx posy prevx prevy  flags posx posy prevx prevy",
             "# binary32 words in hex; the world is %g x %g" % BOX_WORLD, "# written by tests/_sweep_model.table_text()"]
    for j, c in enumerate(t["cs"]):
        lines.append("k %d %s %s %d" % (j, _hex(c), _hex([t["surf"]["restitution"][j], t["surf"]["friction"][j]]),
                                        t["surf"]["flags"][j]))
    for i in range(len(t["rad"])):
        parts = ["c %d" % i, _hex(t["pos"][i]), _hex(t["prev"][i]), _hex(t["rad"][i])]
        for out, out_prev, info in (t["plain"], t["surface"]):
            flags = int(info["moved"][i]) + 2 * int(info["swept"][i]) + 4 * int(info["stopped"][i])
            parts += ["%d" % flags, _hex(out[i]), _hex(out_prev[i])]
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"


# ---- the stepped scene: a sparse box of thin walls, gravity, a kick every step, a piston and a field ---------------------
STEP_WORLD = (100.0, 100.0)
STEP_GRAVITY = (0.0, 60.0)
STEP_DT = 1.0 / 60.0
STEP_LO, STEP_HI = 20.0, 80.0
STEP_STEPS = 60
STEP_KICK_DISC = (50.0, 45.0, 14.0)                                      # the particles in it are kicked: no lockstep piles
STEP_FIELDS = FM.rows(FM.field(FM.BOX, FM.UNIFORM, FM.NONE, (20, 20, 80, 45), f=(40.0, 0.0)))


def step_colliders(R=0.25):
    lo, hi = STEP_LO, STEP_HI
    return np.array([[lo, lo, hi, lo, R], [hi, lo, hi, hi, R], [hi, hi, lo, hi, R], [lo, hi, lo, lo, R],
                     [40, 60, 60, 60, 0.0]], F32)                      # and a thin shelf inside


def step_movers():
    from tests import _movers_model as MM
    return MM.rows(MM.linear((35, 35), (35, 45), 1.0, v=(12.0, 0.0), travel=25.0))


def step_scene(n=240, seed=23):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(STEP_LO + 3, STEP_HI - 3, (n, 2)).astype(F32)
    return pos, np.full(n, 0.25, F32)                                  # (sparse: the collision solver shoves nobody across)


def step_kick(s):
    """the kick before step s: every particle of STEP_KICK_DISC leaves with a velocity of 5 to 20 per step (GPE_VEL_SET)"""
    m = 5.0 + 15.0 * ((s * 7) % 11) / 10.0
    return (float(F32(m * np.cos(2.4 * s))), float(F32(m * np.sin(2.4 * s))))


def step_twin(oracle, sweep=True, surfaces=None):
    pos, rad = step_scene()
    tw = Twin(oracle, pos, rad, world=STEP_WORLD, gravity=STEP_GRAVITY)
    tw.set_colliders(step_colliders())
    tw.set_movers(step_movers())
    tw.set_fields(STEP_FIELDS)
    if surfaces is not None:
        tw.set_surfaces("colliders", surfaces)
    tw.set_collider_sweep(sweep)
    return tw


def step_reference(oracle, resort_every=0, resort_first=False, sweep=True, kick_every=1, surfaces=None, steps=STEP_STEPS,
                   apply_first=False):
    """-> (frames of (pos, prev) after every step, dict of the counters): the kick of step_kick(s) before every
    kick_every-th step, the oracle's step, then the model's passes (movers, swept colliders, fields); apply_first: one
    pass of the colliders before all that (two particles start touching the shelf)"""
    from tests._oracle_model import VEL_SET, circle_mask
    tw = step_twin(oracle, sweep=sweep, surfaces=surfaces)
    if apply_first:                                                    # gpe_apply_colliders before the first step
        tw.apply_colliders()
    frames = []
    for s in range(steps):
        if s % kick_every == 0:
            p, _, _ = tw.arrays()
            tw.kick(circle_mask(p, *STEP_KICK_DISC), VEL_SET, *step_kick(s))
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(STEP_DT, resort=bool(resort))
        p, q, _ = tw.arrays()
        frames.append((p.copy(), q.copy()))
    counts = dict(pushed=tw.pushed, passes=tw.sweep_passes, swept=tw.swept, stopped=tw.stopped, movers=tw.m.pushed)
    tw.close()
    return frames, counts


def inside_step_box(pos):
    p = np.asarray(pos, np.float64)
    return (p[:, 0] > STEP_LO) & (p[:, 0] < STEP_HI) & (p[:, 1] > STEP_LO) & (p[:, 1] < STEP_HI)
