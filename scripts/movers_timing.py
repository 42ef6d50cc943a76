"""Time the moving colliders (gpe_set_movers, csrc/k_movers.hip): the pass alone, the run they act in, the host route.

    python scripts/movers_timing.py [--scope N ...] [--run N] [--steps S] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), after a
warm-up run that begins with a Morton re-sort.
--scope N (repeatable): the "Movers" scope alone on N particles (gpe_apply_movers: the memset of the grid, k_movers_build
  and k_movers_pass) for
  piston              one capsule 2 % of the height thick sweeping along the bottom
  m64                 the piston and 63 random capsules, half of them sliding, half turning
  pegs1024            a 32 x 32 lattice of discs, each turning about a pivot beside it
  ms per call; the same scope on a context of 2 particles with the same world and radius bound: the memset, the build
  and the launch of a pass with nothing to do (the launches' own latency is most of it, so the difference of the two is
  not the pass's time: the pass starts while the build's launch is still being paid for); the "Colliders" scope of the
  static pass on the same capsules at rest, which is the yardstick for the pass; and a device-to-device copy of an array
  the size of pos (hipMemcpy, host clock).
--run N: gpe_run of S steps (default 2000) on N particles, resort_every 250, R repeats of each of
  none                no movers (what the parent commit runs)
  piston_paddle       a piston along the bottom and a paddle wheel's blade, as movers
  at_rest             the same two capsules at rest, as static colliders
  host_route          the route the movers replace: the host poses the two capsules itself (numpy, libm) and calls
                      gpe_set_colliders once per step, which synchronises and rebuilds the lookup grid on the host, then
                      gpe_step
  the cases alternated within each repeat, each continuing from the state the last one left; ms per step from the host
  clock around the S steps, synchronised at both ends, profiling off; then the movers once with profiling on for the
  "Movers" scope per call.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--scope", type=int, action="append", default=[])
ap.add_argument("--run", type=int, default=0)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")
L = gpe._lib

DT = 1.0 / 60.0
RESORT_EVERY = 250
GRAVITY = (0.0, -9.81)
F32 = np.float32
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def mover_rows(k):
    return np.zeros(k, gpe.MOVER_DTYPE)


def sets_for(world):
    """name -> MOVER_DTYPE rows; every motion keeps |omega * DT| <= 0.5 and speed * DT <= travel"""
    w, h = world
    rng = np.random.default_rng(0x30FE)
    piston = mover_rows(1)
    piston["ax"], piston["ay"], piston["bx"], piston["by"], piston["radius"] = 0.05 * w, 0.0, 0.05 * w, 0.1 * h, 0.01 * h
    piston["kind"], piston["vx"], piston["travel"] = L.MOVER_LINEAR, 0.3 * h, 0.5 * w
    m64 = mover_rows(64)
    m64[0] = piston[0]
    a = np.stack([rng.uniform(0, w, 63), rng.uniform(0, h, 63)], axis=1)
    b = a + rng.uniform(-0.1, 0.1, (63, 2)) * np.array([w, h])
    m64["ax"][1:], m64["ay"][1:], m64["bx"][1:], m64["by"][1:] = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    m64["radius"][1:] = rng.uniform(0, 0.004 * h, 63)
    m64["kind"][1:] = np.arange(63) % 2
    m64["vx"][1:], m64["vy"][1:] = rng.uniform(-0.2, 0.2, 63) * h, rng.uniform(-0.2, 0.2, 63) * h
    m64["travel"][1:] = np.where(np.arange(63) % 4 == 0, 0.1 * h, 0.0)
    m64["px"][1:], m64["py"][1:] = a[:, 0], a[:, 1]
    m64["omega"][1:] = rng.uniform(-6, 6, 63)
    gx, gy = np.meshgrid(np.arange(32), np.arange(32))
    c = np.stack([(gx.ravel() + 0.5) * w / 32, (gy.ravel() + 0.5) * h / 32], axis=1)
    pegs = mover_rows(1024)
    pegs["ax"] = pegs["bx"] = c[:, 0]
    pegs["ay"] = pegs["by"] = c[:, 1]
    pegs["radius"] = 0.004 * h
    pegs["kind"] = L.MOVER_ROTATE
    pegs["px"], pegs["py"] = c[:, 0] + 0.01 * h, c[:, 1]
    pegs["omega"] = 3.0 + (np.arange(1024) % 7)
    return {"piston": piston, "m64": m64, "pegs1024": pegs}


def piston_paddle(world):
    w, h = world
    m = mover_rows(2)
    m[0] = sets_for(world)["piston"][0]
    m["ax"][1], m["ay"][1], m["bx"][1], m["by"][1], m["radius"][1] = 0.5 * w, 0.1 * h, 0.5 * w + 0.1 * h, 0.1 * h, 0.01 * h
    m["kind"][1], m["px"][1], m["py"][1], m["omega"][1] = L.MOVER_ROTATE, 0.5 * w, 0.1 * h, 3.0
    return m


def rest_capsules(movers):
    return np.stack([movers[f] for f in ("ax", "ay", "bx", "by", "radius")], axis=1).astype(F32)


def new_state(n, warm, world=None):
    world = gpe.scenes.world_for(n) if world is None else world
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
    if warm:
        st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def copy_yardstick(st, n):
    """ms of a device-to-device copy of 8 n bytes (hipMemcpy between two gpe_buffer_alloc buffers, host clock around the
    copy and a device synchronisation, the best of 10), or None when the runtime library cannot be loaded"""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return None
    src, dst = C.c_void_p(), C.c_void_p()
    st.ctx.call("gpe_buffer_alloc", 8 * n, C.byref(src))
    st.ctx.call("gpe_buffer_alloc", 8 * n, C.byref(dst))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    best = None
    for _ in range(10):
        st.ctx.sync()
        t0 = time.perf_counter()
        ok = hip.hipMemcpy(dst, src, 8 * n, 3) == 0 and hip.hipDeviceSynchronize() == 0    # 3: device to device
        ms = (time.perf_counter() - t0) * 1e3
        if ok:
            best = ms if best is None else min(best, ms)
    st.ctx.call("gpe_buffer_free", src)
    st.ctx.call("gpe_buffer_free", dst)
    return best


def scope_of(st, name, call, repeats, inner):
    per_call = []
    for _ in range(repeats):
        st.ctx.reset_timings()
        for _ in range(inner):
            call()
        total, calls = st.ctx.timings()[name]
        per_call.append(total / calls)
    return spread(per_call)


def scope_cost(n, repeats):
    st = new_state(n, 20 if n > 10_000_000 else 200)
    # two particles, the same world and radii: the same view, the same memset and build, a pass with nothing to do
    rb = abs(float(st.particles.get_max_radius()))
    tiny = gpe.State(np.array([[0.3, 0.6], [0.6, 0.3]], F32) * np.array(st.world, F32), np.full(2, rb, F32), world=st.world,
                     mode=gpe.MODE_NATIVE, gravity=GRAVITY)
    sets = sets_for(st.world)
    inner = 5 if n > 10_000_000 else 20
    st.ctx.set_profiling(True)
    tiny.ctx.set_profiling(True)
    copy_ms = copy_yardstick(st, n)
    for c, movers in sets.items():
        st.clear_colliders()
        st.set_movers(movers)
        tiny.set_movers(movers)
        st.apply_movers(DT); tiny.apply_movers(DT)
        whole = scope_of(st, "Movers", lambda: st.apply_movers(DT), repeats, inner)
        build = scope_of(tiny, "Movers", lambda: tiny.apply_movers(DT), repeats, inner)
        info = st.movers_info()
        st.clear_movers()
        st.set_colliders(rest_capsules(movers))
        st.apply_colliders()                                          # builds the static grid
        static = scope_of(st, "Colliders", st.apply_colliders, repeats, inner)
        emit(n=n, case=c + "_pass", k=len(movers), repeats=repeats, inner=inner, movers_scope_ms=whole,
             two_particle_scope_ms=build, static_pass_ms=static,
             pos_gb_per_s=round(8.0 * n / (whole["median"] * 1e-3) / 1e9, 1),
             copy_ms=None if copy_ms is None else round(copy_ms, 5),
             copy_gb_per_s=None if copy_ms is None else round(16.0 * n / (copy_ms * 1e-3) / 1e9, 1),
             grid=[info["grid_x"], info["grid_y"]], mask_words=info["mask_words"], listed=info["listed"])
    st.close()
    tiny.close()


class HostPoser:
    """what a host did before: the two capsules posed with numpy and libm, one step of dt at a time"""

    def __init__(self, movers):
        self.m, self.g, self.sgn, self.angle = movers, 0.0, 1.0, 0.0

    def step(self):
        m, r = self.m[0], self.m[1]
        g = self.g + self.sgn * float(np.hypot(m["vx"], m["vy"])) * DT
        if g > m["travel"]:
            g, self.sgn = 2 * float(m["travel"]) - g, -self.sgn
        elif g < 0:
            g, self.sgn = -g, -self.sgn
        self.g = g
        self.angle += float(r["omega"]) * DT
        c, s = np.cos(self.angle), np.sin(self.angle)
        bx, by = r["bx"] - r["px"], r["by"] - r["py"]
        return np.array([[m["ax"] + g, m["ay"], m["bx"] + g, m["by"], m["radius"]],
                         [r["ax"], r["ay"], r["px"] + bx * c - by * s, r["py"] + bx * s + by * c, r["radius"]]], F32)


def run_cost(n, steps, repeats):
    st = new_state(n, 200)
    movers = piston_paddle(st.world)
    poser = HostPoser(movers)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)

    def host_route():
        for s in range(steps):
            st.set_colliders(poser.step())
            st.update(DT, resort=(s > 0 and s % RESORT_EVERY == 0))

    def arm(case):
        st.clear_movers()
        st.clear_colliders()
        if case == "piston_paddle":
            st.set_movers(movers)
        elif case == "at_rest":
            st.set_colliders(rest_capsules(movers))

    run()                                                             # warm-up of the measured shape
    walls = {"none": [], "piston_paddle": [], "at_rest": [], "host_route": []}
    for _ in range(repeats):
        for c in walls:                                               # alternated within the repeat
            arm(c)
            walls[c].append(wall_ms(st, host_route if c == "host_route" else run) / steps)
    for c in walls:
        emit(n=n, case=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    st.ctx.set_profiling(True)
    arm("piston_paddle")
    st.ctx.reset_timings()
    run()
    tim, info = st.ctx.timings(), st.movers_info()
    emit(n=n, case="piston_paddle_scope", steps=steps, scope_ms_per_call=round(tim["Movers"][0] / tim["Movers"][1], 5),
         pushed_per_pass=round(info["pushed"] / max(info["passes"], 1), 1), grid=[info["grid_x"], info["grid_y"]],
         listed=info["listed"])
    st.close()


for n in ARGS.scope:
    scope_cost(n, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.run, ARGS.steps, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
