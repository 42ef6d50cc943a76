"""Time the swept form of the movers' pass (gpe_set_mover_sweep; k_movers_sweep_build + k_movers_sweep against
k_movers_build + k_movers_pass).

    python scripts/mover_sweep_timing.py [--root TREE] [--plain-only] [--pass N ...] [--repeats R] [--out FILE]

On a uniform NATIVE cloud (scenes.world_for / uniform_cloud: the workload of bench.py) under gravity (0, -9.81), so that
particles keep arriving at the obstacles: a pass that touches nothing says nothing about the hit path.
--root TREE: import the package from another checkout (a build of the parent commit); with --plain-only nothing of the
  mode's interface is used, so the script runs on a tree that has none.
--pass N (repeatable): for each of the scenes of scripts/movers_timing.py
  piston              one capsule 2 % of the height thick sweeping along the bottom
  m64                 the piston and 63 random capsules, half of them sliding, half turning
  pegs1024            a 32 x 32 lattice of discs, each turning about a pivot beside it
  and each of plain (the mode off) and swept (on): a fresh cloud, W steps of gpe_run with the set armed, then M steps
  with profiling on: the "Movers" scope (the memset of the grid, the build and the pass: the three enqueues), ms per
  call, the (cell, mover) bits the last build listed, and the particles pushed, swept and stopped per pass as a share of
  N.  R repeats (each continues the run).
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
L = gpe._lib

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


def sets_for(world):
    """name -> MOVER_DTYPE rows, the sets of scripts/movers_timing.py; every motion keeps |omega * DT| <= 0.5 and
    speed * DT <= travel"""
    w, h = world
    rng = np.random.default_rng(0x30FE)
    rows = lambda k: np.zeros(k, gpe.MOVER_DTYPE)
    piston = rows(1)
    piston["ax"], piston["ay"], piston["bx"], piston["by"], piston["radius"] = 0.05 * w, 0.0, 0.05 * w, 0.1 * h, 0.01 * h
    piston["kind"], piston["vx"], piston["travel"] = L.MOVER_LINEAR, 0.3 * h, 0.5 * w
    m64 = rows(64)
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
    pegs = rows(1024)
    pegs["ax"] = pegs["bx"] = c[:, 0]
    pegs["ay"] = pegs["by"] = c[:, 1]
    pegs["radius"] = 0.004 * h
    pegs["kind"] = L.MOVER_ROTATE
    pegs["px"], pegs["py"] = c[:, 0] + 0.01 * h, c[:, 1]
    pegs["omega"] = 3.0 + (np.arange(1024) % 7)
    return {"piston": piston, "m64": m64, "pegs1024": pegs}


def pass_cost(n, repeats):
    big = n > 10_000_000
    warm, measured = (20, 10) if big else (300, 100)
    world = gpe.scenes.world_for(n)
    for case, movers in sets_for(world).items():
        for variant in VARIANTS:
            pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
            st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
            st.set_movers(movers)
            if variant == "swept":
                st.set_mover_sweep(True)
            st.run(DT, warm, resort_every=0, resort_first=True)
            st.ctx.set_profiling(True)
            per_call, pushed, swept, stopped = [], [], [], []
            for _ in range(repeats):
                before = st.movers_info()
                sweep_before = st.mover_sweep_info() if variant == "swept" else None
                st.ctx.reset_timings()
                st.run(DT, measured, resort_every=0, resort_first=False)
                total, calls = st.ctx.timings()["Movers"]
                after = st.movers_info()
                passes = max(after["passes"] - before["passes"], 1)
                per_call.append(total / calls)
                pushed.append((after["pushed"] - before["pushed"]) / passes / n)
                if sweep_before is not None:
                    sweep_after = st.mover_sweep_info()
                    swept.append((sweep_after["swept"] - sweep_before["swept"]) / passes / n)
                    stopped.append((sweep_after["stopped"] - sweep_before["stopped"]) / passes / n)
            rec = dict(n=n, case=case, k=len(movers), variant=variant, warm=warm, steps=measured, repeats=repeats, scope="Movers",
                       scope_ms_per_call=spread(per_call), pushed_share=spread(pushed), listed=after["listed"],
                       grid=[after["grid_x"], after["grid_y"]])
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
