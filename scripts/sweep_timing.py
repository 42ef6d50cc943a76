"""Time the swept form of the static colliders' pass (gpe_set_collider_sweep; k_colliders_sweep against k_colliders_pass).

    python scripts/sweep_timing.py [--root TREE] [--plain-only] [--pass N ...] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), so that
particles keep arriving at the obstacles: a pass that touches nothing says nothing about the hit path.
--root TREE: import the package from another checkout (a build of the parent commit); with --plain-only nothing of the
  sweep's interface is used, so the script runs on a tree that has none.
--pass N (repeatable): for each of
  floor               one capsule 2 % of the height thick along the bottom
  pegs4096            a 64 x 64 lattice of discs
  and each of plain (the sweep off) and swept (on): a fresh cloud, W steps of gpe_run with the set armed, then M steps
  with profiling on: the "Colliders" scope, ms per call, and the particles pushed, swept and stopped per pass as a share
  of N.  R repeats (each continues the run).
One JSON line per case on stdout, all of them in --out.  Everything is reported, nothing is gated."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=None)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--pass", dest="passes", type=int, action="append", default=[])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root) if ARGS.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")

DT = 1.0 / 60.0
GRAVITY = (0.0, -9.81)
F32 = np.float32
RECS = []
VARIANTS = ["plain"] if ARGS.plain_only else ["plain", "swept"]


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


def pass_cost(n, repeats):
    big = n > 10_000_000
    warm, measured = (20, 10) if big else (300, 100)
    for case in ("floor", "pegs4096"):
        for variant in VARIANTS:
            world = gpe.scenes.world_for(n)
            pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
            st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
            st.set_colliders(floor_of(world) if case == "floor" else pegs_of(world))
            if variant == "swept":
                st.set_collider_sweep(True)
            st.run(DT, warm, resort_every=0, resort_first=True)
            st.ctx.set_profiling(True)
            per_call, pushed, swept, stopped = [], [], [], []
            for _ in range(repeats):
                before = st.colliders_info()
                sweep_before = st.sweep_info() if variant == "swept" else None
                st.ctx.reset_timings()
                st.run(DT, measured, resort_every=0, resort_first=False)
                total, calls = st.ctx.timings()["Colliders"]
                after = st.colliders_info()
                passes = max(after["passes"] - before["passes"], 1)
                per_call.append(total / calls)
                pushed.append((after["pushed"] - before["pushed"]) / passes / n)
                if sweep_before is not None:
                    sweep_after = st.sweep_info()
                    swept.append((sweep_after["swept"] - sweep_before["swept"]) / passes / n)
                    stopped.append((sweep_after["stopped"] - sweep_before["stopped"]) / passes / n)
            rec = dict(n=n, case=case, variant=variant, warm=warm, steps=measured, repeats=repeats, scope="Colliders",
                       scope_ms_per_call=spread(per_call), pushed_share=spread(pushed))
            if swept:
                rec.update(swept_share=spread(swept), stopped_share=spread(stopped))
            emit(**rec)
            st.close()


for n in ARGS.passes:
    pass_cost(n, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
