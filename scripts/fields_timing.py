"""Time the force fields (gpe_set_fields, csrc/k_fields.hip): the run they act in, the pass alone, the host route.

    python scripts/fields_timing.py [--run N] [--scope N ...] [--host N] [--steps S] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), after a
warm-up run that begins with a Morton re-sort.
--run N: gpe_run of S steps (default 2000) on N particles, resort_every 250, R repeats of each of
  none                no fields (what the parent commit runs)
  circle              one small circle (a well of 2 % of the width): nearly every lookup list is empty
  everywhere          one EVERYWHERE UNIFORM field: every particle's prev is read and written
  boxes4096           a 64 x 64 tiling of boxes, the four kinds in turn
  wells64             64 overlapping RADIAL wells with LINEAR falloff, each 30 % of the width across
the cases alternated within each repeat; ms per step from the host clock around the whole run, synchronised at both
ends, profiling off; then each armed case once with profiling on for the "Fields" scope per call.
--scope N (repeatable): the "Fields" scope alone on N particles for the same sets (gpe_apply_fields, a hipEvent pair on
  the context's stream), ms per call, the particles touched per pass, the bytes the pass must move per second (8 B of pos
  per particle, 16 B of prev per touched particle; the lookups are not counted), and a device-to-device copy of 12 N
  bytes (hipMemcpy, host clock: 24 N bytes of traffic, what the everywhere case moves) as the yardstick.
--host N: the route a host had before: gpe_step, download of pos and prev, the numpy pass (one well), gpe_edit_particles of
  the touched ones -- per step, over 20 steps.
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


def sets_for(world):
    """gentle fields: they must not change the workload they are timed in"""
    w, h = world
    rng = np.random.default_rng(0xF1E1D)
    circle = np.zeros(1, gpe.FIELD_DTYPE)
    circle["shape"], circle["kind"], circle["falloff"] = L.FIELD_CIRCLE, L.FIELD_RADIAL, L.FALLOFF_LINEAR
    circle["x0"], circle["y0"], circle["x1"] = 0.5 * w, 0.5 * h, 0.01 * w
    circle["px"], circle["py"], circle["strength"], circle["reach"] = 0.5 * w, 0.5 * h, 1.0, 0.01 * w
    everywhere = np.zeros(1, gpe.FIELD_DTYPE)
    everywhere["shape"], everywhere["kind"], everywhere["fx"] = L.FIELD_EVERYWHERE, L.FIELD_UNIFORM, 0.01
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    boxes = np.zeros(4096, gpe.FIELD_DTYPE)
    boxes["shape"], boxes["kind"] = L.FIELD_BOX, np.arange(4096) % 4
    boxes["x0"], boxes["y0"] = gx.ravel() * w / 64, gy.ravel() * h / 64
    boxes["x1"], boxes["y1"] = boxes["x0"] + F32(w / 64), boxes["y0"] + F32(h / 64)
    boxes["px"], boxes["py"] = boxes["x0"] + F32(w / 128), boxes["y0"] + F32(h / 128)
    boxes["fx"], boxes["fy"] = rng.uniform(-0.5, 0.5, 4096), rng.uniform(-0.5, 0.5, 4096)
    boxes["strength"] = np.where(boxes["kind"] == L.FIELD_DRAG, 0.999, rng.uniform(-0.5, 0.5, 4096))
    wells = np.zeros(64, gpe.FIELD_DTYPE)
    wells["shape"], wells["kind"], wells["falloff"] = L.FIELD_CIRCLE, L.FIELD_RADIAL, L.FALLOFF_LINEAR
    wells["x0"], wells["y0"] = rng.uniform(0.3 * w, 0.7 * w, 64), rng.uniform(0.3 * h, 0.7 * h, 64)
    wells["x1"] = wells["reach"] = 0.15 * w
    wells["px"], wells["py"], wells["strength"] = wells["x0"], wells["y0"], 0.05
    return {"none": None, "circle": circle, "everywhere": everywhere, "boxes4096": boxes, "wells64": wells}


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


def arm(st, fs):
    if fs is None:
        st.clear_fields()
    else:
        st.set_fields(fs)


def run_cost(n, steps, repeats):
    st = new_state(n, 200)
    sets = sets_for(st.world)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    walls = {c: [] for c in sets}
    for _ in range(repeats):
        for c, fs in sets.items():                                    # alternated within the repeat
            arm(st, fs)
            if fs is not None:
                st.apply_fields(0.0)                                  # builds the grid outside the clock (dt = 0: drags only)
            walls[c].append(wall_ms(st, run) / steps)
    for c in sets:
        emit(n=n, case=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    st.ctx.set_profiling(True)
    for c, fs in sets.items():
        if fs is None:
            continue
        arm(st, fs)
        st.ctx.reset_timings()
        run()
        tim, info = st.ctx.timings(), st.fields_info()
        emit(n=n, case=c + "_scope", steps=steps, scope_ms_per_call=round(tim["Fields"][0] / tim["Fields"][1], 5),
             touched_per_pass=round(info["touched"] / max(info["passes"], 1), 1), grid=[info["grid_x"], info["grid_y"]],
             list_entries=info["list_entries"])
    st.ctx.set_profiling(False)
    st.close()


def copy_yardstick(st, n):
    """ms of a device-to-device copy of 12 n bytes -- 24 n bytes of traffic, what a pass that touches every particle
    moves (hipMemcpy between two gpe_buffer_alloc buffers, host clock around the copy and a device synchronisation, the
    best of 10), or None when the runtime library cannot be loaded"""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return None
    src, dst = C.c_void_p(), C.c_void_p()
    st.ctx.call("gpe_buffer_alloc", 12 * n, C.byref(src))
    st.ctx.call("gpe_buffer_alloc", 12 * n, C.byref(dst))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    best = None
    for _ in range(10):
        st.ctx.sync()
        t0 = time.perf_counter()
        ok = hip.hipMemcpy(dst, src, 12 * n, 3) == 0 and hip.hipDeviceSynchronize() == 0    # 3: device to device
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
    for c, fs in sets.items():
        if fs is None:
            continue
        arm(st, fs)
        st.apply_fields(DT)                                           # builds the grid
        before = st.fields_info()
        per_call = []
        for _ in range(repeats):
            st.ctx.reset_timings()
            for _ in range(inner):
                st.apply_fields(DT)
            total, calls = st.ctx.timings()["Fields"]
            per_call.append(total / calls)
        s = spread(per_call)
        info = st.fields_info()
        touched = (info["touched"] - before["touched"]) / (info["passes"] - before["passes"])
        emit(n=n, case=c + "_pass", repeats=repeats, inner=inner, scope_ms=s, touched_per_pass=round(touched, 1),
             gb_per_s=round((8.0 * n + 16.0 * touched) / (s["median"] * 1e-3) / 1e9, 1),
             copy_ms=None if copy_ms is None else round(copy_ms, 5),
             copy_gb_per_s=None if copy_ms is None else round(24.0 * n / (copy_ms * 1e-3) / 1e9, 1),
             pass_over_copy=None if copy_ms is None else round(s["median"] / copy_ms, 3),
             grid=[info["grid_x"], info["grid_y"]], list_entries=info["list_entries"])
    st.ctx.set_profiling(False)
    st.close()


def host_pass(pos, prev, well, dt):
    """the numpy pass for one well with linear falloff: what a host would write, not the test model"""
    d = np.array([well["px"], well["py"]], F32) - pos
    ln = np.sqrt((d * d).sum(axis=1))
    hit = np.nonzero((ln <= well["x1"]) & (ln > 0))[0]
    w = well["strength"] * np.maximum(1 - ln[hit] / well["reach"], 0)
    out = prev[hit] - d[hit] / ln[hit, None] * (w * dt * dt)[:, None]
    return hit.astype(np.uint32), out.astype(F32)


def host_cost(n, steps=20):
    st = new_state(n, 200)
    well = sets_for(st.world)["wells64"][0]
    per_step = []
    for _ in range(steps):
        def one():
            st.update(DT)
            pos, prev = st.positions(), st.previous_positions()
            hit, out = host_pass(pos, prev, well, DT)
            if len(hit):
                st.edit_particles(indices=hit, previous=out)
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
