"""Time the bend constraints (gpe_set_bends, csrc/k_bends.hip): the pass alone beside the bonds' pass, a resolve, the run.

    python scripts/bends_timing.py [--side S] [--pass] [--run] [--steps N] [--repeats R] [--out FILE]

The scene is the sheet of scripts/bonds_timing.py: S x S particles (default 1000: 1 M particles) of radius 0.5 on a
lattice of spacing 1.25 with the structural bonds of a cloth (right and lower neighbour, stiffness 0.25, the upper row
pinned by anchors), and the bends along its rows and columns (about 2 S^2 of them, rest angle pi, stiffness 0.3), NATIVE
mode, no gravity, after a warm-up that begins with a Morton re-sort.  The sheet is at rest: the kernels do the same
work per bend and per node whatever the corrections are.
--pass: gpe_apply_bends alone with profiling on at iterations 1 and 4: the scopes "Bends", "bends/bend" and
  "bends/node" in ms per call, and the bytes each phase requests per second.  Counted per bend: state 1 + record 32 +
  three node slots 12 + three positions 24 + the correction written 16 = 85 B; per node: slot 4 + row start 4 + pos 8 +
  radius 4 + pos written 8 = 28 B, and per incidence entry 4 + state 1 + correction 16 = 21 B.  Then gpe_apply_bonds on
  the same sheet in the same process at the same iterations, and the ratio of the two passes.  Then the cost of a
  resolve: the pass after a Morton re-sort against the pass before it (host clock), with the scopes "uids/map" and
  "bends/resolve".
--run: gpe_run of N steps (default 2000), resort_every 250, R repeats of: the sheet with its bonds (4 iterations) and
  no bends, with bends at 1 iteration, with bends at 4; alternated within each repeat; ms per step from the host clock.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--pass", dest="do_pass", action="store_true")
ap.add_argument("--run", action="store_true")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")

DT = 1.0 / 60.0
RESORT_EVERY = 250
REST, BOND_STIFFNESS, BEND_STIFFNESS, BOND_ITERATIONS = 1.25, 0.25, 0.3, 4
HBM_PEAK_GB_S = 8000.0
F32 = np.float32
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def sheet(side):
    j, i = np.meshgrid(np.arange(side), np.arange(side))
    pos = np.stack([10.0 + REST * j.ravel(), 10.0 + REST * i.ravel()], axis=1).astype(F32)
    uid = (i * side + j).astype(np.uint32)
    bonds = np.concatenate([gpe.anchor_bonds(uid[0], pos[:side]),
                            gpe.pair_bonds(uid[:, :-1].ravel(), uid[:, 1:].ravel(), REST, BOND_STIFFNESS),
                            gpe.pair_bonds(uid[:-1, :].ravel(), uid[1:, :].ravel(), REST, BOND_STIFFNESS)])
    bends = np.concatenate([
        gpe.bends_from_angles(uid[:, :-2].ravel(), uid[:, 1:-1].ravel(), uid[:, 2:].ravel(), math.pi, BEND_STIFFNESS),
        gpe.bends_from_angles(uid[:-2, :].ravel(), uid[1:-1, :].ravel(), uid[2:, :].ravel(), math.pi, BEND_STIFFNESS)])
    world = (20.0 + REST * side, 20.0 + REST * side)
    return pos, np.full(side * side, 0.5, F32), bonds, bends, world


def new_state(side, warm=100):
    pos, rad, bonds, bends, world = sheet(side)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, 0.0))
    st.enable_uids()
    st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st, bonds, bends


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def scopes_of(st, apply, names, repeats, inner):
    per = {name: [] for name in names}
    for _ in range(repeats):
        st.ctx.reset_timings()
        for _ in range(inner):
            apply()
        tim = st.ctx.timings()
        for name in names:
            per[name].append(tim[name][0] / tim[name][1])              # per call; the phases: per relaxation
    return {name: spread(v) for name, v in per.items()}


def pass_cost(side, repeats, inner=20):
    st, bonds, bends = new_state(side)
    n, k = side * side, len(bends)
    st.ctx.set_profiling(True)
    for iterations in (1, 4):
        st.set_bends(bends, iterations)
        st.set_bonds(bonds, iterations)
        st.apply_bends(); st.apply_bonds()                             # both resolve
        info = st.bends_info()
        bend_bytes = 85.0 * k
        node_bytes = 28.0 * info["nodes"] + 21.0 * 3 * k
        s = scopes_of(st, st.apply_bends, ("Bends", "bends/bend", "bends/node"), repeats, inner)
        b = scopes_of(st, st.apply_bonds, ("Bonds", "bonds/bond", "bonds/node"), repeats, inner)
        emit(n=n, k=k, nodes=info["nodes"], case="pass", iterations=iterations, repeats=repeats, inner=inner,
             pass_ms=s["Bends"], bend_phase_ms=s["bends/bend"], node_phase_ms=s["bends/node"],
             bend_phase_gb_per_s=round(bend_bytes / (s["bends/bend"]["median"] * 1e-3) / 1e9, 1),
             node_phase_gb_per_s=round(node_bytes / (s["bends/node"]["median"] * 1e-3) / 1e9, 1),
             hbm_peak_gb_per_s=HBM_PEAK_GB_S, bonds_k=len(bonds), bonds_pass_ms=b["Bonds"],
             bonds_bond_phase_ms=b["bonds/bond"], bonds_node_phase_ms=b["bonds/node"],
             bends_over_bonds=round(s["Bends"]["median"] / b["Bonds"]["median"], 3))
    st.clear_bonds()
    plain, resolving, scopes = [], [], []
    for _ in range(repeats):
        plain.append(wall_ms(st, st.apply_bends))
        st.particles.sort_by_cell_id()
        st.ctx.reset_timings()
        resolving.append(wall_ms(st, st.apply_bends))
        tim = st.ctx.timings()
        scopes.append({name: round(tim[name][0], 5) for name in ("uids/map", "bends/resolve") if name in tim})
    emit(n=n, k=k, case="resolve", repeats=repeats, pass_wall_ms=spread(plain), pass_with_resolve_wall_ms=spread(resolving),
         scopes_ms=scopes, resolves=st.bends_info()["resolves"])
    st.ctx.set_profiling(False)
    st.close()


def run_cost(side, steps, repeats):
    st, bonds, bends = new_state(side)
    n = side * side
    st.set_bonds(bonds, BOND_ITERATIONS)
    cases = {"bonds_only": None, "bends_it1": 1, "bends_it4": 4}
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    walls = {c: [] for c in cases}
    for _ in range(repeats):
        for c, iterations in cases.items():                           # alternated within the repeat
            if iterations is None:
                st.clear_bends()
            else:
                st.set_bends(bends, iterations)
            walls[c].append(wall_ms(st, run) / steps)
    for c in cases:
        emit(n=n, k=len(bends), bonds_k=len(bonds), bond_iterations=BOND_ITERATIONS, case=c, steps=steps, repeats=repeats,
             ms_per_step=spread(walls[c]))
    emit(n=n, case="run_end", **st.bends_info())
    st.close()


if ARGS.do_pass:
    pass_cost(ARGS.side, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.side, ARGS.steps, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
