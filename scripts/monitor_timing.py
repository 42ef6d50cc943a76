"""Time the run monitor (gpe_measure / gpe_monitor_*, csrc/k_monitor.hip): one record, the run it observes, the host route.

    python scripts/monitor_timing.py [--frame N ...] [--run N] [--steps S] [--repeats R] [--root DIR] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py, gravity on so that prev != pos)
after a warm-up run that begins with a Morton re-sort.
--frame N (repeatable): the cost of one record on N particles, R repeats, the cases alternated within each repeat:
  measure_wall        host clock around gpe_measure (it synchronises): launches, the 120-byte read-back and the wait
  circle_count_wall   the yardstick: host clock around gpe_query_circle as a count (8 B per particle against 16)
  monitor/partial, monitor/final, Query particles: the scopes of the same calls with profiling on (a hipEvent pair each
                      on the context's stream), ms per call, and the bytes per second of the partial pass over its 16 B
                      per particle as a share of the 8 TB/s HBM peak of the data sheet
  host_route_wall     gpe_sync + the downloads of pos and prev + a numpy reduction of the same fields (float32
                      differences, a finite mask, float64 np.sum, min / max / argmax; not the fsum of the test model)
--run N: gpe_run of S steps (default 2000) on N particles, resort_every 250, R repeats of each of
  plain               no recorder
  armed_every1 / 16   the monitor armed, a ring of 64 records
ms per step from the host clock around the whole run, synchronised at both ends; then the armed cases once more with
profiling on for the scopes' ms per call.  --root DIR imports the package from another checkout (a parent commit
without the monitor runs `plain` only).  One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--frame", type=int, action="append", default=[])
ap.add_argument("--run", type=int, default=0)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
gpe = importlib.import_module("gpu-physics-engine_amd")

DT = 1.0 / 60.0
RESORT_EVERY = 250
HBM_PEAK = 8.0e12
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def new_state(n, warm):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.81))
    st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def host_reduce(st):
    st.ctx.sync()
    p, q = st.positions(), st.previous_positions()
    v = p - q
    v2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    reg = np.isfinite(v2)
    w, h = st.ctx.world()
    return (int((~reg).sum()), int((v2[reg] > 0).sum()),
            int(((p[reg, 0] < 0) | (p[reg, 0] > w) | (p[reg, 1] < 0) | (p[reg, 1] > h)).sum()),
            p[reg].sum(axis=0, dtype=np.float64), v[reg].sum(axis=0, dtype=np.float64), v2[reg].sum(dtype=np.float64),
            p[reg].min(axis=0), p[reg].max(axis=0), int(np.argmax(np.where(reg, v2, -1.0))))


def frame_cost(n, repeats):
    st = new_state(n, 20 if n > 10_000_000 else 200)
    centre, radius = (st.world[0] * 0.5, st.world[1] * 0.5), st.world[1] * 0.1
    cases = {"measure_wall": lambda: st.measure(0.01), "circle_count_wall": lambda: st.count_circle(centre, radius)}
    inner = 5 if n > 10_000_000 else 20
    for call in cases.values():
        call()
    walls = {name: [] for name in cases}
    for _ in range(repeats):
        for name, call in cases.items():                              # alternated within the repeat
            walls[name].append(min(wall_ms(st, call) for _ in range(inner)))
    st.ctx.set_profiling(True)
    scopes = {}
    for _ in range(repeats):
        st.ctx.reset_timings()
        for _ in range(inner):
            for call in cases.values():
                call()
        for name, (total, calls) in st.ctx.timings().items():
            if name.startswith("monitor/") or name == "Query particles":
                scopes.setdefault(name, []).append(total / calls)
    st.ctx.set_profiling(False)
    host = [wall_ms(st, lambda: host_reduce(st)) for _ in range(2 if n > 10_000_000 else repeats)]
    rec = st.measure(0.01)
    partial = spread(scopes["monitor/partial"])
    rate = 16.0 * n / (partial["median"] * 1e-3)
    emit(n=n, case="frame", repeats=repeats, inner=inner, ms={k: spread(v) for k, v in walls.items()},
         scope_ms={k: spread(v) for k, v in scopes.items()}, partial_gb_per_s=round(rate / 1e9, 1),
         partial_share_of_hbm_peak=round(rate / HBM_PEAK, 3), host_route_wall_ms=spread(host),
         record=dict(n=rec.n, moving=rec.moving, outside=rec.outside, irregular=rec.irregular, max_v2=rec.max_v2))
    st.close()


def run_cost(n, steps, repeats):
    st = new_state(n, 200)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    armed = hasattr(st, "monitor_begin")
    cases = ["plain"] + (["armed_every1", "armed_every16"] if armed else [])
    walls = {c: [] for c in cases}
    for _ in range(repeats):
        for c in cases:                                               # alternated within the repeat
            if c != "plain":
                st.monitor_begin(every=1 if c == "armed_every1" else 16, frames=64, rest_speed=0.01)
            walls[c].append(wall_ms(st, run) / steps)
            if c != "plain":
                st.monitor_end()
    for c in cases:
        emit(n=n, case=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    if armed:
        st.monitor_begin(every=1, frames=64, rest_speed=0.01)
        st.ctx.set_profiling(True)
        st.ctx.reset_timings()
        run()
        tim = st.ctx.timings()
        st.ctx.set_profiling(False)
        records, recorded = st.monitor_read()
        emit(n=n, case="armed_every1_scopes", steps=steps, recorded=int(recorded),
             scope_ms_per_call={k: round(tim[k][0] / tim[k][1], 5) for k in ("monitor/partial", "monitor/final")},
             last=dict(step=int(records["step"][-1]), moving=int(records["moving"][-1]), max_v2=float(records["max_v2"][-1])))
        st.monitor_end()
    st.close()


for n in ARGS.frame:
    frame_cost(n, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.run, ARGS.steps, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
