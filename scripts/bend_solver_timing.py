"""Time the bends' coloured solver (gpe_set_bend_solver, csrc/k_bends.hip) against the Jacobi pass.

    python scripts/bend_solver_timing.py [--lib FILE] [--forms] [--pass] [--side S] [--repeats R] [--out FILE]

--lib: the library to load in place of the package's own.  The two launch forms of a coloured pass are chosen by a
  constant of the build (kBendLdsNodesMax, csrc/gpe_internal.h): a library compiled with -DGPE_BEND_LDS_NODES_MAX=0
  (GPE_EXTRA_CXXFLAGS of build.py) runs every pass in the per-colour form, one compiled with 8192 every set of up to
  8192 particles in the one-workgroup form, and --forms on one build after the other gives the table the constant is
  read from.
--forms: chains (a bend at every inner particle, listed in order: 3 colours) of m = 64, 256, 1024, 4096, 8192
  particles and sheets (bends along rows and columns: 6 colours; 8 x 8, 32 x 32, 64 x 64 and 90 x 91, the largest that
  fits 8192 nodes) at rest, iterations 1 and 8: gpe_apply_bends with profiling on -- the scope "Bends" in ms per pass
  -- and, profiling off, the host clock over a batch of passes enqueued back to back and one sync, which is what a run
  pays.  The info's `form` says which form the build took.
--pass: the 1000 x 1000 sheet of scripts/bends_timing.py (1 M particles, 2 M bends, stiffness 0.3, at rest): a pass
  under either solver at iterations 1 and 4, the scope "Bends" in ms per pass and its kernels' scopes per launch.
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
ap.add_argument("--lib", default=None)
ap.add_argument("--forms", action="store_true")
ap.add_argument("--pass", dest="do_pass", action="store_true")
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")
if ARGS.lib:
    gpe._lib.LIB_PATH = os.path.abspath(ARGS.lib)                      # (before the first load)

DT = 1.0 / 60.0
REST, STIFFNESS = 1.25, 0.3
F32 = np.float32
RECS = []


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def straight(a, b, c):
    return gpe.bends_from_angles(a, b, c, math.pi, STIFFNESS)


def sheet(rows, cols):
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    pos = np.stack([10.0 + REST * j.ravel(), 10.0 + REST * i.ravel()], axis=1).astype(F32)
    uid = (i * cols + j).astype(np.uint32)
    bends = np.concatenate([straight(uid[:, :-2].ravel(), uid[:, 1:-1].ravel(), uid[:, 2:].ravel()),
                            straight(uid[:-2, :].ravel(), uid[1:-1, :].ravel(), uid[2:, :].ravel())])
    world = (20.0 + REST * cols, 20.0 + REST * rows)
    return pos, np.full(rows * cols, 0.5, F32), bends, world


def chain(m):
    """a serpentine of rows of 128 at the rest spacing: neighbours in the chain are neighbours in space"""
    i = np.arange(m)
    row, col = i // 128, i % 128
    col = np.where(row % 2 == 0, col, 127 - col)
    pos = np.stack([10.0 + REST * col, 10.0 + REST * row], axis=1).astype(F32)
    uid = i.astype(np.uint32)
    bends = gpe.bends_from_angles(uid[:-2], uid[1:-1], uid[2:], math.pi, 0.0)     # (stiffness 0: the turns stay where they are)
    return pos, np.full(m, 0.5, F32), bends, (20.0 + REST * 128, 20.0 + REST * (m // 128 + 1))


def new_state(scene, warm=0):
    pos, rad, bends, world = scene
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, 0.0))
    st.enable_uids()
    if warm:
        st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st, bends


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
            st.apply_bends()
        for name, (ms, calls) in st.ctx.timings().items():
            if name == "Bends" or name.startswith("bends/"):
                per.setdefault(name, []).append(ms / calls)
    st.ctx.set_profiling(False)
    return {name: spread(v) for name, v in per.items()}


def forms(repeats, inner=50):
    shapes = [("chain", m, chain(m)) for m in (64, 256, 1024, 4096, 8192)]
    shapes += [("sheet", r * c, sheet(r, c)) for r, c in ((8, 8), (32, 32), (64, 64), (90, 91))]
    for shape, m, scene in shapes:
        st, bends = new_state(scene)
        st.set_bend_solver("coloured")
        for iterations in (1, 8):
            st.set_bends(bends, iterations)
            st.apply_bends()                                           # resolves
            s = scoped(st, repeats, inner)
            batch = lambda: [st.apply_bends() for _ in range(inner)]
            wall = [wall_ms(st, batch) / inner for _ in range(repeats)]
            info = st.bend_solver_info()
            emit(case="forms", shape=shape, m=m, k=len(bends), iterations=iterations, form=info["form"],
                 colours=info["colours"], lds_nodes_max=info["lds_nodes_max"], pass_scope_ms=s["Bends"],
                 pass_wall_ms=spread(wall), repeats=repeats, inner=inner)
        st.close()


def pass_cost(side, repeats, inner=20):
    st, bends = new_state(sheet(side, side), warm=100)
    for solver in ("jacobi", "coloured"):
        st.set_bend_solver(solver)
        for iterations in (1, 4):
            st.set_bends(bends, iterations)
            st.apply_bends()
            s = scoped(st, repeats, inner)
            info = st.bend_solver_info()
            emit(case="pass", n=side * side, k=len(bends), solver=solver, iterations=iterations, form=info["form"],
                 colours=info["colours"], largest_colour=info["largest_colour"], pass_ms=s.pop("Bends"),
                 kernels_ms_per_launch=s, repeats=repeats, inner=inner)
    st.close()


if ARGS.forms:
    forms(ARGS.repeats)
if ARGS.do_pass:
    pass_cost(ARGS.side, ARGS.repeats)
if ARGS.out:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(RECS, f, indent=1)
