"""Time the static colliders (gpe_set_colliders, csrc/k_colliders.hip): the run they act in, the pass alone, the host route.

    python scripts/colliders_timing.py [--run N] [--scope N ...] [--host N] [--steps S] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), after a
warm-up run that begins with a Morton re-sort.
--run N: gpe_run of S steps (default 2000) on N particles, resort_every 250, R repeats of each of
  none                no colliders (what the parent commit runs)
  floor               one capsule along the bottom, 2 % of the height thick
  c64                 the floor and 63 random capsules
  pegs4096            a 64 x 64 lattice of discs
the cases alternated within each repeat; ms per step from the host clock around the whole run, synchronised at both
ends, profiling off; then each armed case once with profiling on for the "Colliders" scope per call.
--scope N (repeatable): the "Colliders" scope alone on N particles for the same sets (gpe_apply_colliders, a hipEvent
  pair on the context's stream), ms per call, the bytes of pos it reads per second (8 B per particle; the stores of the
  moved particles and the lookups are not counted), and a device-to-device copy of an array the size of pos (hipMemcpy,
  host clock) as the yardstick.
--host N: the route a host had before: gpe_step, download of pos and radius, the numpy pass (one floor), gpe_edit_particles
  of the moved ones -- per step, over 20 steps.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--run", type=int, default=0)
ap.add_argument("--scope", type=int, action="append", default=[])
ap.add_argument("--host", type=int, default=0)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")

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


def sets_for(world):
    w, h = world
    rng = np.random.default_rng(0xC011)
    floor = np.array([[-0.05 * w, -0.03 * h, 1.05 * w, -0.03 * h, 0.05 * h]], F32)   # surface at 2 % of the height
    a = np.stack([rng.uniform(0, w, 63), rng.uniform(0, h, 63)], axis=1)
    b = a + rng.uniform(-0.1, 0.1, (63, 2)) * np.array([w, h])
    c64 = np.concatenate([floor, np.concatenate([a, b, rng.uniform(0, 0.004 * h, (63, 1))], axis=1)]).astype(F32)
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    c = np.stack([(gx.ravel() + 0.5) * w / 64, (gy.ravel() + 0.5) * h / 64], axis=1)
    pegs = np.concatenate([c, c, np.full((4096, 1), 0.004 * h)], axis=1).astype(F32)
    return {"none": None, "floor": floor, "c64": c64, "pegs4096": pegs}


def new_state(n, warm):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
    st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def arm(st, cs):
    if cs is None:
        st.clear_colliders()
    else:
        st.set_colliders(cs)


def run_cost(n, steps, repeats):
    st = new_state(n, 200)
    sets = sets_for(st.world)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    walls = {c: [] for c in sets}
    for _ in range(repeats):
        for c, cs in sets.items():                                    # alternated within the repeat
            arm(st, cs)
            walls[c].append(wall_ms(st, run) / steps)
    for c in sets:
        emit(n=n, case=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    st.ctx.set_profiling(True)
    for c, cs in sets.items():
        if cs is None:
            continue
        arm(st, cs)
        st.ctx.reset_timings()
        run()
        tim, info = st.ctx.timings(), st.colliders_info()
        emit(n=n, case=c + "_scope", steps=steps, scope_ms_per_call=round(tim["Colliders"][0] / tim["Colliders"][1], 5),
             pushed_per_pass=round(info["pushed"] / max(info["passes"], 1), 1), grid=[info["grid_x"], info["grid_y"]],
             list_entries=info["list_entries"])
    st.ctx.set_profiling(False)
    st.close()


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


def scope_cost(n, repeats):
    st = new_state(n, 20 if n > 10_000_000 else 200)
    sets = sets_for(st.world)
    inner = 5 if n > 10_000_000 else 20
    st.ctx.set_profiling(True)
    copy_ms = copy_yardstick(st, n)
    for c, cs in sets.items():
        if cs is None:
            continue
        arm(st, cs)
        st.apply_colliders()                                          # builds the grid
        per_call = []
        for _ in range(repeats):
            st.ctx.reset_timings()
            for _ in range(inner):
                st.apply_colliders()
            total, calls = st.ctx.timings()["Colliders"]
            per_call.append(total / calls)
        s = spread(per_call)
        info = st.colliders_info()
        emit(n=n, case=c + "_pass", repeats=repeats, inner=inner, scope_ms=s,
             pos_gb_per_s=round(8.0 * n / (s["median"] * 1e-3) / 1e9, 1),
             copy_ms=None if copy_ms is None else round(copy_ms, 5),
             copy_gb_per_s=None if copy_ms is None else round(16.0 * n / (copy_ms * 1e-3) / 1e9, 1),
             grid=[info["grid_x"], info["grid_y"]], list_entries=info["list_entries"])
    st.ctx.set_profiling(False)
    st.close()


def host_pass(pos, rad, floor, world):
    """the numpy pass for one horizontal floor capsule: what a host would write, not the test model"""
    ay, R = floor[1], floor[4]
    x = np.clip(pos[:, 0], floor[0], floor[2])
    q = pos - np.stack([x, np.full_like(x, ay)], axis=1)
    d = np.sqrt((q * q).sum(axis=1))
    s = R + np.abs(rad)
    hit = np.nonzero(d < s)[0]
    out = pos[hit] + q[hit] / d[hit, None] * (s[hit] - d[hit])[:, None]
    out = np.clip(out, rad[hit, None], np.array(world, F32) - rad[hit, None])
    return hit.astype(np.uint32), out.astype(F32)


def host_cost(n, steps=20):
    st = new_state(n, 200)
    floor = sets_for(st.world)["floor"][0]
    per_step = []
    for _ in range(steps):
        def one():
            st.update(DT)
            pos, rad = st.positions(), st.radii()
            hit, out = host_pass(pos, rad, floor, st.world)
            if len(hit):
                prev = st.previous_positions()[hit]
                st.edit_particles(indices=hit, positions=out, previous=prev)
        per_step.append(wall_ms(st, one))
    emit(n=n, case="host_route", steps=steps, ms_per_step=spread(per_step))
    st.close()


if ARGS.run:
    run_cost(ARGS.run, ARGS.steps, ARGS.repeats)
for n in ARGS.scope:
    scope_cost(n, ARGS.repeats)
if ARGS.host:
    host_cost(ARGS.host)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
