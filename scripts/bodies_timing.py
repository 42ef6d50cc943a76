"""Time the rigid and soft bodies (gpe_set_bodies, csrc/k_bodies.hip): the pass alone, a slot lookup, the run it acts in,
the host route.

    python scripts/bodies_timing.py [--side S] [--pass] [--run] [--host] [--steps N] [--repeats R] [--out FILE]

The scene is a lattice of S x S particles (default 1000: 1 M particles) of radius 0.5 and spacing 1.25, NATIVE mode, no
gravity, after a warm-up that begins with a Morton re-sort.  The particles are at rest in their rest shape: the pass
does the same work per member whatever the corrections are, and the same particles without bodies stay a lattice too,
so the difference between two runs is the pass.  Three sets over the same particles, stiffness 1, unbreakable:
  b4     S^2 / 4 bodies of 4: the 2 x 2 blocks of the lattice (16 bodies to a wave);
  b64    S^2 / 64 bodies of 64: the 8 x 8 blocks (one body to a wave, one round);
  b4096  S^2 / 4096 bodies of 4096: runs of 4096 particles in row order, strips about four rows high (one body to a
         wave, 64 rounds per phase); the particles left over belong to no body.
--pass: gpe_apply_bodies alone with profiling on: the scope "Bodies" in ms per call and the bytes it requests per
  second against the HBM peak.  Counted per member: slot 4 + rest 8 + pos 8 + radius 4 + pos written 8 = 32 B (a body
  of more than 64 members gathers slot, rest and pos in each of its four phases: 4 + 3 x 20 + 12 = 88 B; the set is
  unbreakable, so the third phase is skipped: 68 B); per body: list entry 4 + record 16 + state 1 + pose written 16.
  Then the cost of a slot lookup: the pass after a Morton re-sort against the pass before it (host clock), with the
  scopes "uids/map" and "bodies/resolve".
--run: gpe_run of N steps (default 2000), resort_every 250, R repeats of: the same particles without bodies, then each
  set; alternated within each repeat; ms per step from the host clock.
--host: the route a host had before: gpe_step, download of pos and uids, shape matching in numpy, gpe_edit_particles of
  every member -- per step, over 5 steps, for each set.
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
SPACING = 1.25
HBM_PEAK_GB_S = 8000.0
F32 = np.float32
RECS = []
SETS = {"b4": 4, "b64": 64, "b4096": 4096}


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECS.append(rec)


def lattice(side):
    j, i = np.meshgrid(np.arange(side), np.arange(side))
    pos = np.stack([10.0 + SPACING * j.ravel(), 10.0 + SPACING * i.ravel()], axis=1).astype(F32)
    world = (20.0 + SPACING * side, 20.0 + SPACING * side)
    return pos, np.full(side * side, 0.5, F32), world


def body_set(side, pos, count):
    """(rows, member_uid, member_rest): uid = row * side + column at the start"""
    uid = np.arange(side * side, dtype=np.uint32).reshape(side, side)
    edge = {4: 2, 64: 8}.get(count)
    if edge and side % edge == 0:
        member = uid.reshape(side // edge, edge, side // edge, edge).transpose(0, 2, 1, 3).reshape(-1)
    else:
        member = uid.reshape(-1)[:(side * side // count) * count]
    return gpe.body_rows(np.full(len(member) // count, count)), member, pos[member]


def new_state(side, warm=100):
    pos, rad, world = lattice(side)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, 0.0))
    st.enable_uids()
    st.run(DT, warm, resort_every=0, resort_first=True)
    st.ctx.sync()
    return st, pos


def wall_ms(st, call):
    st.ctx.sync()
    t0 = time.perf_counter()
    call()
    st.ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def pass_cost(side, repeats, inner=20):
    st, pos = new_state(side)
    n = side * side
    st.ctx.set_profiling(True)
    for name, count in SETS.items():
        rows, member, rest = body_set(side, pos, count)
        st.set_bodies(rows, member, rest)
        st.apply_bodies()                                             # resolves
        per_member = 32.0 if count <= 64 else 68.0
        requested = per_member * len(member) + 37.0 * len(rows)
        per = []
        for _ in range(repeats):
            st.ctx.reset_timings()
            for _ in range(inner):
                st.apply_bodies()
            tim = st.ctx.timings()
            per.append(tim["Bodies"][0] / tim["Bodies"][1])
        s = spread(per)
        emit(n=n, case="pass", set=name, bodies=len(rows), members=len(member), repeats=repeats, inner=inner, pass_ms=s,
             requested_mb=round(requested / 1e6, 1), requested_gb_per_s=round(requested / (s["median"] * 1e-3) / 1e9, 1),
             hbm_peak_gb_per_s=HBM_PEAK_GB_S, acting=int((~np.isnan(st.body_poses()).any(axis=1)).sum()))
        # a slot lookup: the pass after a re-sort against the pass before it
        plain, resolving, scopes = [], [], []
        for _ in range(repeats):
            plain.append(wall_ms(st, st.apply_bodies))
            st.particles.sort_by_cell_id()
            st.ctx.reset_timings()
            resolving.append(wall_ms(st, st.apply_bodies))
            tim = st.ctx.timings()
            scopes.append({k: round(tim[k][0], 5) for k in ("uids/map", "bodies/resolve") if k in tim})
        emit(n=n, case="resolve", set=name, members=len(member), repeats=repeats, pass_wall_ms=spread(plain),
             pass_with_resolve_wall_ms=spread(resolving), scopes_ms=scopes, resolves=st.bodies_info()["resolves"])
    st.ctx.set_profiling(False)
    st.close()


def run_cost(side, steps, repeats):
    st, pos = new_state(side)
    n = side * side
    sets = {name: body_set(side, pos, count) for name, count in SETS.items()}
    run = lambda: st.run(DT, steps, resort_every=RESORT_EVERY, resort_first=False)
    run()                                                             # warm-up of the measured shape
    walls = {c: [] for c in ["no_bodies"] + list(sets)}
    for _ in range(repeats):
        for c in walls:                                               # alternated within the repeat
            if c == "no_bodies":
                st.clear_bodies()
            else:
                st.set_bodies(*sets[c])
            walls[c].append(wall_ms(st, run) / steps)
    for c in walls:
        emit(n=n, case="run", set=c, steps=steps, repeats=repeats, ms_per_step=spread(walls[c]))
    emit(n=n, case="run_end", **st.bodies_info())
    st.close()


def host_match(pos, slot, rest, count):
    """shape matching of equal-sized bodies in numpy: what a host would write, not the test model"""
    p = pos[slot].reshape(-1, count, 2)
    r = rest.reshape(-1, count, 2)
    q = r - r.mean(axis=1, keepdims=True)
    c = p.mean(axis=1, keepdims=True)
    d = p - c
    a = (q * d).sum(axis=(1, 2))
    b = (q[:, :, 0] * d[:, :, 1] - q[:, :, 1] * d[:, :, 0]).sum(axis=1)
    h = np.sqrt(a * a + b * b)
    co, si = (a / h)[:, None], (b / h)[:, None]
    goal = c + np.stack([co * q[:, :, 0] - si * q[:, :, 1], si * q[:, :, 0] + co * q[:, :, 1]], axis=2)
    return goal.reshape(-1, 2).astype(F32)


def host_cost(side, steps=5):
    st, pos0 = new_state(side)
    n = side * side
    for name, count in SETS.items():
        rows, member, rest = body_set(side, pos0, count)
        per_step = []
        for _ in range(steps):
            def one():
                st.update(DT)
                pos, uids = st.positions(), st.uids()
                slot = np.empty(n, np.int64)
                slot[uids] = np.arange(n)
                where = slot[member]
                st.edit_particles(indices=where.astype(np.uint32), positions=host_match(pos, where, rest, count),
                                  previous=st.previous_positions()[where])
            per_step.append(wall_ms(st, one))
        emit(n=n, case="host_route", set=name, bodies=len(rows), steps=steps, ms_per_step=spread(per_step))
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
