"""Time the surface materials (gpe_set_surfaces; the surface forms of k_colliders_pass and k_movers_pass).

    python scripts/surfaces_timing.py [--root TREE] [--plain-only] [--pass N ...] [--run N] [--steps S] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), so that
particles keep arriving at the obstacles: a pass that touches nothing says nothing about the hit path.
--root TREE: import the package from another checkout (a build of the parent commit); with --plain-only nothing of the
  surfaces' interface is used, so the script runs on a tree that has none.
--pass N (repeatable): for each of
  floor               one capsule 2 % of the height thick along the bottom (static)
  pegs4096            a 64 x 64 lattice of discs (static)
  piston_paddle       a piston sweeping along the bottom and a paddle wheel's blade (movers)
  and each of plain (no surfaces), surface (restitution 0.5, friction 0.3 on every obstacle) and all_plain (the same
  rows with GPE_SURFACE_PLAIN: the surface kernel on the plain run's own trajectory, so the two scopes differ by the
  kernel's form alone): a fresh cloud, W steps of gpe_run with the set armed, then M steps with profiling on: the "Colliders" / "Movers" scope, ms per call, and the
  particles pushed per pass as a share of N.  R repeats (each continues the run).
--run N: gpe_run of S steps (default 2000) on N particles over the floor, resort_every 250, R repeats of the variants,
  alternated, each on its own context; then the host route the surfaces replace, on S / 20 steps: gpe_step,
  download pos and prev, the rule for a horizontal floor in numpy, gpe_edit_particles of the touched.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=None)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--pass", dest="passes", type=int, action="append", default=[])
ap.add_argument("--run", type=int, default=0)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root) if ARGS.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")
L = gpe._lib

DT = 1.0 / 60.0
RESORT_EVERY = 250
GRAVITY = (0.0, -9.81)
E, MU = 0.5, 0.3
F32 = np.float32
RECS = []
VARIANTS = ["plain"] if ARGS.plain_only else ["plain", "surface", "all_plain"]


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    rec["tree"] = "other" if ARGS.root else "this"
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def floor_of(world):
    w, h = world
    return np.array([[-0.05 * w, 0.0, 1.05 * w, 0.0, 0.02 * h]], F32)


def pegs_of(world):
    w, h = world
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    c = np.stack([(gx.ravel() + 0.5) * w / 64, (gy.ravel() + 0.5) * h / 64], axis=1)
    return np.concatenate([c, c, np.full((4096, 1), 0.004 * h)], axis=1).astype(F32)


def piston_paddle(world):
    w, h = world
    m = np.zeros(2, gpe.MOVER_DTYPE)
    m["ax"][0], m["ay"][0], m["bx"][0], m["by"][0], m["radius"][0] = 0.05 * w, 0.0, 0.05 * w, 0.1 * h, 0.01 * h
    m["kind"][0], m["vx"][0], m["travel"][0] = L.MOVER_LINEAR, 0.3 * h, 0.5 * w
    m["ax"][1], m["ay"][1], m["bx"][1], m["by"][1], m["radius"][1] = 0.5 * w, 0.1 * h, 0.5 * w + 0.1 * h, 0.1 * h, 0.01 * h
    m["kind"][1], m["px"][1], m["py"][1], m["omega"][1] = L.MOVER_ROTATE, 0.5 * w, 0.1 * h, 3.0
    return m


def new_state(n):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
    st.ctx.sync()
    return st


def arm(st, case, variant):
    k = 0
    if case == "piston_paddle":
        st.set_movers(piston_paddle(st.world))
        k, target = 2, "movers"
    else:
        caps = floor_of(st.world) if case == "floor" else pegs_of(st.world)
        st.set_colliders(caps)
        k, target = len(caps), "colliders"
    if variant == "surface":
        st.set_surfaces(target, gpe.surface_rows(k, E, MU))
    elif variant == "all_plain":
        st.set_surfaces(target, gpe.surface_rows(k, E, MU, L.SURFACE_PLAIN))


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def pass_cost(n, repeats):
    big = n > 10_000_000
    warm, measured = (20, 10) if big else (300, 100)
    for case in ("floor", "pegs4096", "piston_paddle"):
        for variant in VARIANTS:
            st = new_state(n)
            arm(st, case, variant)
            st.run(DT, warm, resort_every=0, resort_first=True)
            st.ctx.set_profiling(True)
            scope = "Movers" if case == "piston_paddle" else "Colliders"
            info_of = st.movers_info if case == "piston_paddle" else st.colliders_info
            per_call, share = [], []
            for _ in range(repeats):
                before = info_of()
                st.ctx.reset_timings()
                st.run(DT, measured, resort_every=0, resort_first=False)
                total, calls = st.ctx.timings()[scope]
                after = info_of()
                per_call.append(total / calls)
                share.append((after["pushed"] - before["pushed"]) / max(after["passes"] - before["passes"], 1) / n)
            emit(n=n, case=case, variant=variant, warm=warm, steps=measured, repeats=repeats, scope=scope,
                 scope_ms_per_call=spread(per_call), touched_share=spread(share))
            st.close()


def host_floor_rule(st, floor_top):
    """the rule for a horizontal floor whose face is at y = floor_top (normal (0, 1), w = 0), in numpy, on the touched"""
    pos, prev, rad = st.positions(), st.previous_positions(), st.radii()
    depth = (floor_top + np.abs(rad)) - pos[:, 1]
    hit = np.nonzero(depth > 0)[0]
    if len(hit) == 0:
        return 0
    p, q = pos[hit], prev[hit]
    v = p - q
    vn = v[:, 1]
    on = np.where(vn < 0, -E * vn, vn)
    jn = on - vn
    tl = np.abs(v[:, 0])
    k = np.where(MU * jn < tl, (tl - MU * jn) / np.where(tl > 0, tl, 1), 0)
    t = v[:, 0] * k
    new = np.stack([p[:, 0] - (v[:, 0] - t), p[:, 1] + depth[hit]], axis=1).astype(F32)
    old = (new - np.stack([t, on], axis=1)).astype(F32)
    st.edit_particles(indices=hit.astype(np.uint32), positions=new, previous=old)
    return len(hit)


def run_cost(n, steps, repeats):
    states = {}
    for variant in VARIANTS:
        st = new_state(n)
        arm(st, "floor", variant)
        st.run(DT, 200, resort_every=0, resort_first=True)
        states[variant] = st
    walls = {v: [] for v in VARIANTS}
    for _ in range(repeats):
        for v, st in states.items():                                  # alternated within the repeat
            walls[v].append(wall_ms(st, lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)) / steps)
    for v, st in states.items():
        info = st.colliders_info()
        emit(n=n, case="floor_run", variant=v, steps=steps, repeats=repeats, ms_per_step=spread(walls[v]),
             pushed_per_pass=round(info["pushed"] / max(info["passes"], 1), 1))
        st.close()
    # the host route: no colliders on the device at all
    st = new_state(n)
    floor_top = float(floor_of(st.world)[0, 4])
    st.run(DT, 200, resort_every=0, resort_first=True)
    few = max(steps // 20, 1)
    touched = []

    def route():
        for s in range(few):
            st.update(DT, resort=False)
            touched.append(host_floor_rule(st, floor_top))

    ms = [wall_ms(st, route) / few for _ in range(repeats)]
    emit(n=n, case="floor_run", variant="host_route", steps=few, repeats=repeats, ms_per_step=spread(ms),
         pushed_per_pass=round(float(np.mean(touched)), 1))
    st.close()


for n in ARGS.passes:
    pass_cost(n, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.run, ARGS.steps, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
