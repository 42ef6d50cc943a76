"""Time the bonds' coloured solver (gpe_set_bond_solver, csrc/k_bonds.hip) against the Jacobi pass.

    python scripts/bond_solver_timing.py [--lib FILE] [--forms] [--pass] [--run] [--side S] [--steps N] [--repeats R] [--out FILE]

--lib: the library to load in place of the package's own.  The two launch forms of a coloured pass are chosen by a
  constant of the build (kBondLdsNodesMax, csrc/gpe_internal.h): a library compiled with -DGPE_BOND_LDS_NODES_MAX=0
  (GPE_EXTRA_CXXFLAGS of build.py) runs every pass in the per-colour form, and --forms on one build after the other
  gives the table the constant is read from.
--forms: chains (an anchor and m - 1 pairs: 2 colours) and sheets (right and lower neighbours: 4 colours; 8 x 8, 32 x
  32, 64 x 64 and 90 x 91, the largest that fits 8192 nodes) of m = 64, 1024, 4096, 8192 particles at rest, iterations 1
  and 8: gpe_apply_bonds with profiling on -- the scope "Bonds" in ms per pass -- and, profiling off, the host clock
  over a batch of passes enqueued back to back and one sync, which is what a run pays.  The info's `form` says which
  form the build took.
--pass: the 1000 x 1000 sheet of scripts/bonds_timing.py (1 M particles, 2 M bonds, stiffness 0.25, at rest): a pass
  under either solver at iterations 1 and 4, the scope "Bonds" in ms per pass and its kernels' scopes per launch.
--run: gpe_run of N steps (default 2000) of that sheet, resort_every 250, under either solver at iterations 1,
  alternated within each repeat; ms per step from the host clock.
One JSON line per case on stdout, all of them in --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--forms", action="store_true")
ap.add_argument("--pass", dest="do_pass", action="store_true")
ap.add_argument("--run", action="store_true")
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")
if ARGS.lib:
    gpe._lib.LIB_PATH = os.path.abspath(ARGS.lib)                      # (before the first load)

DT = 1.0 / 60.0
RESORT_EVERY = 250
REST, STIFFNESS = 1.25, 0.25
F32 = np.float32
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def sheet(rows, cols, pinned=True):
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    pos = np.stack([10.0 + REST * j.ravel(), 10.0 + REST * i.ravel()], axis=1).astype(F32)
    uid = (i * cols + j).astype(np.uint32)
    parts = [gpe.anchor_bonds(uid[0], pos[:cols])] if pinned else []
    parts += [gpe.pair_bonds(uid[:, :-1].ravel(), uid[:, 1:].ravel(), REST, STIFFNESS),
              gpe.pair_bonds(uid[:-1, :].ravel(), uid[1:, :].ravel(), REST, STIFFNESS)]
    world = (20.0 + REST * cols, 20.0 + REST * rows)
    return pos, np.full(rows * cols, 0.5, F32), np.concatenate(parts), world


def chain(m):
    """a serpentine of rows of 128 at the rest spacing: neighbours in the chain are neighbours in space"""
    i = np.arange(m)
    row, col = i // 128, i % 128
    col = np.where(row % 2 == 0, col, 127 - col)
    pos = np.stack([10.0 + REST * col, 10.0 + REST * row], axis=1).astype(F32)
    uid = i.astype(np.uint32)
    bonds = np.concatenate([gpe.anchor_bonds(uid[:1], pos[:1]), gpe.pair_bonds(uid[:-1], uid[1:], REST, STIFFNESS)])
    return pos, np.full(m, 0.5, F32), bonds, (20.0 + REST * 128, 20.0 + REST * (m // 128 + 1))


def new_state(scene, warm=0):
    pos, rad, bonds, world = scene
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, 0.0))
    st.enable_uids()
    if warm:
        st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st, bonds


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def scoped(st, repeats, inner):
    """-> {scope: spread of ms per call} over `repeats` batches of `inner` passes, profiling on"""
    st.ctx.set_profiling(True)
    per = {}
    for _ in range(repeats):
        st.ctx.reset_timings()
        for _ in range(inner):
            st.apply_bonds()
        for name, (ms, calls) in st.ctx.timings().items():
            if name == "Bonds" or name.startswith("bonds/"):
                per.setdefault(name, []).append(ms / calls)
    st.ctx.set_profiling(False)
    return {name: spread(v) for name, v in per.items()}


def forms(repeats, inner=50):
    shapes = [("chain", m, chain(m)) for m in (64, 1024, 4096, 8192)]
    shapes += [("sheet", r * c, sheet(r, c, pinned=False)) for r, c in ((8, 8), (32, 32), (64, 64), (90, 91))]
    for shape, m, scene in shapes:
        st, bonds = new_state(scene)
        st.set_bond_solver("coloured")
        for iterations in (1, 8):
            st.set_bonds(bonds, iterations)
            st.apply_bonds()                                           # resolves
            s = scoped(st, repeats, inner)
            batch = lambda: [st.apply_bonds() for _ in range(inner)]
            wall = [wall_ms(st, batch) / inner for _ in range(repeats)]
            info = st.bond_solver_info()
            emit(case="forms", shape=shape, m=m, k=len(bonds), iterations=iterations, form=info["form"],
                 colours=info["colours"], lds_nodes_max=info["lds_nodes_max"], pass_scope_ms=s["Bonds"],
                 pass_wall_ms=spread(wall), repeats=repeats, inner=inner)
        st.close()


def pass_cost(side, repeats, inner=20):
    st, bonds = new_state(sheet(side, side), warm=100)
    for solver in ("jacobi", "coloured"):
        st.set_bond_solver(solver)
        for iterations in (1, 4):
            st.set_bonds(bonds, iterations)
            st.apply_bonds()
            s = scoped(st, repeats, inner)
            info = st.bond_solver_info()
            emit(case="pass", n=side * side, k=len(bonds), solver=solver, iterations=iterations, form=info["form"],
                 colours=info["colours"], largest_colour=info["largest_colour"], pass_ms=s.pop("Bonds"),
                 kernels_ms_per_launch=s, repeats=repeats, inner=inner)
    st.close()


def run_cost(side, steps, repeats):
    st, bonds = new_state(sheet(side, side), warm=100)
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    cases = {"no_bonds": None, "jacobi_it1": "jacobi", "coloured_it1": "coloured"}
    run()
    walls = {c: [] for c in cases}
    for _ in range(repeats):
        for c, solver in cases.items():                                # alternated within the repeat
            if solver is None:
                st.clear_bonds()
            else:
                st.set_bond_solver(solver)
                st.set_bonds(bonds, 1)
            walls[c].append(wall_ms(st, run) / steps)
    for c in cases:
        emit(case=c, n=side * side, k=len(bonds), steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    st.close()


if ARGS.forms:
    forms(ARGS.repeats)
if ARGS.do_pass:
    pass_cost(ARGS.side, ARGS.repeats)
if ARGS.run:
    run_cost(ARGS.side, ARGS.steps, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
