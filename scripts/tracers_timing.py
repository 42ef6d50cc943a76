"""Time the tracer recorder (gpe_tracers_*, csrc/k_tracers.hip) against the run it observes and the host route it replaces.

    python scripts/tracers_timing.py [N] [--steps S] [--repeats R] [--gravity] [--big N2] [--root DIR] [--out FILE]

On a uniform NATIVE cloud of N particles (default 1 000 000, 0: none; scenes.world_for / uniform_cloud: the workload of
bench.py, gravity off unless --gravity) with uids on, after a warm-up run of 200 steps that begins with a Morton re-sort,
R repeats (default 5) of each of:
  plain                   gpe_run of S steps (default 2000), resort_every 250, no recorder
  armed_k{K}_every{E}     the same run with K tracers (random uids) recorded after every E-th step: K = 1024 and 65 536
                          at E = 1, K = 1024 at E = 16; the ring holds 64 frames
  host_route_k{K}         what a host does without the recorder: gpe_step + gpe_find_uids after every step, same re-sort
                          schedule (the uid map is rebuilt by the first lookup after every re-sort)
Every case reports ms per step from the host wall clock around the whole run, synchronised at both ends (median, minimum
and maximum over the repeats).  The armed cases are then run R more times with profiling on: every scope is a hipEvent
pair on the context's stream, read after a synchronisation; per repeat the mean time per call of `tracers/sample`,
`tracers/resolve` (with the bytes per second over the 4 B per particle it reads) and of the re-sort it follows
("Particle sort" + "Particle rearranging").  The profiled runs are not used for ms per step: an event pair per kernel
costs more than some kernels.
--big N2: `tracers/resolve` alone on N2 particles (65 536 tracers), a gpe_morton_resort before each of the R frames.
--root DIR: import the package from another checkout (a parent commit without the recorder runs `plain` only).
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--gravity", action="store_true")
ap.add_argument("--big", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
gpe = importlib.import_module("gpu-physics-engine_amd")

DT = 1.0 / 60.0
RESORT_EVERY = 250
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def new_state(n):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.81 if ARGS.gravity else 0.0))
    st.enable_uids()
    st.run(DT, 200, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st


def wall_per_step(st, steps, one_run):
    st.ctx.sync()
    t0 = time.perf_counter()
    one_run()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(n, steps, repeats):
    st = new_state(n)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                           # warm-up of the measured shape
    emit(n=n, case="plain", gravity=ARGS.gravity, steps=steps, repeats=repeats,
         ms_per_step=spread([wall_per_step(st, steps, run) for _ in range(repeats)]))
    if not hasattr(st, "tracers_begin"):
        st.close()
        return
    rng = np.random.default_rng(2)
    for k, every in ((1024, 1), (65536, 1), (1024, 16)):
        uids = rng.choice(n, k, replace=False).astype(np.uint32)
        st.tracers_begin(uids, every=every, frames=64)
        run()
        walls = [wall_per_step(st, steps, run) for _ in range(repeats)]
        st.ctx.set_profiling(True)
        per_call = {}
        for _ in range(repeats):
            st.ctx.reset_timings()
            run()
            tim = st.ctx.timings()
            sort_ms = tim["Particle sort"][0] + tim["Particle rearranging"][0]
            per_call.setdefault("resort", []).append(sort_ms / tim["Particle sort"][1])
            for name in ("tracers/sample", "tracers/resolve"):
                per_call.setdefault(name, []).append(tim[name][0] / tim[name][1])
            calls = {name: tim[name][1] for name in ("tracers/sample", "tracers/resolve", "Particle sort")}
        st.ctx.set_profiling(False)
        frames = st.tracers_read()
        st.tracers_end()
        resolve = spread(per_call["tracers/resolve"])
        emit(n=n, case="armed_k%d_every%d" % (k, every), steps=steps, repeats=repeats, ms_per_step=spread(walls),
             sample_ms=spread(per_call["tracers/sample"]), resolve_ms=resolve,
             resolve_gb_per_s=round(4.0 * n / (resolve["median"] * 1e-3) / 1e9, 1), resort_ms=spread(per_call["resort"]),
             calls_per_run=calls, frames_held=int(frames.step.shape[0]), recorded=int(frames.recorded))
    for k in (1024, 65536):
        uids = rng.choice(n, k, replace=False).astype(np.uint32)

        def host_route():
            for s in range(steps):
                st.update(DT, resort=(s > 0 and s % RESORT_EVERY == 0))
                st.find_uids(uids)

        host_route()
        emit(n=n, case="host_route_k%d" % k, steps=steps, repeats=repeats,
             ms_per_step=spread([wall_per_step(st, steps, host_route) for _ in range(repeats)]))
    st.close()


def measure_resolve_alone(n, repeats):
    st = new_state(n)
    uids = np.random.default_rng(3).choice(n, 65536, replace=False).astype(np.uint32)
    st.tracers_begin(uids, every=1, frames=2)
    st.ctx.set_profiling(True)
    times = []
    for i in range(repeats + 2):
        st.particles.sort_by_cell_id(0.0)                           # gpe_morton_resort: the slot table is stale again
        st.ctx.reset_timings()
        st.tracers_sample()
        tim = st.ctx.timings()
        if i >= 2:
            times.append(tim["tracers/resolve"][0])
    st.tracers_end()
    st.close()
    ms = spread(times)
    emit(n=n, case="resolve_alone_k65536", repeats=repeats, resolve_ms=ms,
         resolve_gb_per_s=round(4.0 * n / (ms["median"] * 1e-3) / 1e9, 1))


if ARGS.n:
    measure(ARGS.n, ARGS.steps, ARGS.repeats)
if ARGS.big:
    measure_resolve_alone(ARGS.big, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
