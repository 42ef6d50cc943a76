"""Time the distance bonds (gpe_set_bonds, csrc/k_bonds.hip): the pass alone, a resolve, the run it acts in, the host route.

    python scripts/bonds_timing.py [--side S] [--pass] [--run] [--host] [--steps N] [--repeats R] [--out FILE]

The scene is a sheet of S x S particles (default 1000: 1 M particles) of radius 0.5 on a lattice of spacing 1.25 with
the structural bonds of a cloth (right and lower neighbour: about 2 S^2 of them, stiffness 0.25, unbreakable) and its
upper row pinned by anchors, NATIVE mode, no gravity, after a warm-up that begins with a Morton re-sort.  The sheet is
at rest: both kernels do the same work per bond and per node whatever the corrections are, and the same particles
without bonds stay a lattice too (under gravity they would pile up at the bottom, denser than the native step takes),
so the difference between the runs is the pass.
--pass: gpe_apply_bonds alone with profiling on at iterations 1 and 4: the scopes "Bonds", "bonds/bond" and
  "bonds/node" in ms per call, and the bytes each phase moves per second against the HBM peak.  Counted per bond:
  state 1 + record 16 + two node slots 8 + two positions 16 + the correction written 8 = 49 B; per node: slot 4 + row
  start 4 + per incidence (entry 4 + state 1 + correction 8) + pos 8 + radius 4 + pos written 8.  Then the cost of a
  resolve: the pass after a Morton re-sort against the pass before it (host clock), with the scopes "uids/map" and
  "bonds/resolve".
--run: gpe_run of N steps (default 2000), resort_every 250, R repeats of: the same particles without bonds, the sheet
  at iterations 1, the sheet at iterations 4; alternated within each repeat; ms per step from the host clock.
--host: the route a host had before: gpe_step, download of pos, a numpy Jacobi relaxation, gpe_edit_particles of
  every bonded particle -- per step, over 10 steps.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--pass", dest="do_pass", action="store_true")
ap.add_argument("--run", action="store_true")
ap.add_argument("--host", action="store_true")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")

DT = 1.0 / 60.0
RESORT_EVERY = 250
GRAVITY = (0.0, 0.0)
REST, STIFFNESS = 1.25, 0.25
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
                            gpe.pair_bonds(uid[:, :-1].ravel(), uid[:, 1:].ravel(), REST, STIFFNESS),
                            gpe.pair_bonds(uid[:-1, :].ravel(), uid[1:, :].ravel(), REST, STIFFNESS)])
    world = (20.0 + REST * side, 20.0 + REST * side)
    return pos, np.full(side * side, 0.5, F32), bonds, world


def new_state(side, warm=100):
    pos, rad, bonds, world = sheet(side)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=GRAVITY)
    st.enable_uids()
    st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st, bonds


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def pass_cost(side, repeats, inner=20):
    st, bonds = new_state(side)
    n, k = side * side, len(bonds)
    st.ctx.set_profiling(True)
    for iterations in (1, 4):
        st.set_bonds(bonds, iterations)
        st.apply_bonds()                                              # resolves
        info = st.bonds_info()
        incidences = 2 * k - side                                      # an anchor has one end
        bond_bytes = 49.0 * k
        node_bytes = 28.0 * info["nodes"] + 13.0 * incidences
        per = {"Bonds": [], "bonds/bond": [], "bonds/node": []}
        for _ in range(repeats):
            st.ctx.reset_timings()
            for _ in range(inner):
                st.apply_bonds()
            tim = st.ctx.timings()
            per["Bonds"].append(tim["Bonds"][0] / tim["Bonds"][1])
            for name in ("bonds/bond", "bonds/node"):
                per[name].append(tim[name][0] / tim[name][1])      # per relaxation
        s = {name: spread(v) for name, v in per.items()}
        emit(n=n, k=k, case="pass", iterations=iterations, repeats=repeats, inner=inner, pass_ms=s["Bonds"],
             bond_phase_ms=s["bonds/bond"], node_phase_ms=s["bonds/node"],
             bond_phase_gb_per_s=round(bond_bytes / (s["bonds/bond"]["median"] * 1e-3) / 1e9, 1),
             node_phase_gb_per_s=round(node_bytes / (s["bonds/node"]["median"] * 1e-3) / 1e9, 1),
             hbm_peak_gb_per_s=HBM_PEAK_GB_S)
    # a resolve: the pass after a re-sort against the pass before it
    plain, resolving, scopes = [], [], []
    for _ in range(repeats):
        plain.append(wall_ms(st, st.apply_bonds))
        st.particles.sort_by_cell_id()
        st.ctx.reset_timings()
        resolving.append(wall_ms(st, st.apply_bonds))
        tim = st.ctx.timings()
        scopes.append({name: round(tim[name][0], 5) for name in ("uids/map", "bonds/resolve") if name in tim})
    emit(n=n, k=k, case="resolve", repeats=repeats, pass_wall_ms=spread(plain), pass_with_resolve_wall_ms=spread(resolving),
         scopes_ms=scopes, resolves=st.bonds_info()["resolves"])
    st.ctx.set_profiling(False)
    st.close()


def run_cost(side, steps, repeats):
    st, bonds = new_state(side)
    n = side * side
    cases = {"no_bonds": None, "sheet_it1": 1, "sheet_it4": 4}
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    walls = {c: [] for c in cases}
    for _ in range(repeats):
        for c, iterations in cases.items():                           # alternated within the repeat
            if iterations is None:
                st.clear_bonds()
            else:
                st.set_bonds(bonds, iterations)
            walls[c].append(wall_ms(st, run) / steps)
    for c in cases:
        emit(n=n, k=len(bonds), case=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    emit(n=n, case="run_end", **st.bonds_info())
    st.close()


def host_relax(pos, slot_a, slot_b, rest, w):
    """one Jacobi relaxation of the pair bonds in numpy: what a host would write, not the test model"""
    d = pos[slot_b] - pos[slot_a]
    length = np.sqrt((d * d).sum(axis=1))
    ok = length > 0
    c = np.zeros_like(d)
    c[ok] = d[ok] * ((length[ok] - rest) / length[ok] * w)[:, None]
    out = pos.copy()
    np.add.at(out, slot_a, c)
    np.add.at(out, slot_b, -c)
    return out


def host_cost(side, steps=10):
    st, bonds = new_state(side)
    n = side * side
    pairs = bonds[bonds["flags"] == 0]
    per_step = []
    for _ in range(steps):
        def one():
            st.update(DT)
            pos, uids = st.positions(), st.uids()
            slot = np.empty(n, np.int64)
            slot[uids] = np.arange(n)
            out = host_relax(pos, slot[pairs["uid_a"]], slot[pairs["uid_b"]], F32(REST), F32(0.5 * STIFFNESS))
            st.edit_particles(indices=np.arange(n, dtype=np.uint32), positions=out, previous=st.previous_positions())
        per_step.append(wall_ms(st, one))
    emit(n=n, k=len(pairs), case="host_route", steps=steps, ms_per_step=spread(per_step))
    st.close()


if ARGS.do_pass:
    pass_cost(ARGS.side, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.side, ARGS.steps, ARGS.repeats)
if ARGS.host:
    host_cost(ARGS.side)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
