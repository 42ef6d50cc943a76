"""Time the cluster query on the device (csrc/k_clusters.hip) next to the count-only contact query it shares its first
stages with.

    python scripts/clusters_timing.py [N ...] [--calls K] [--adversarial N] [--out FILE]   (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud (scenes.world_for / uniform_cloud) after 20 steps under gravity that begin with a
Morton re-sort -- the scene of scripts/contacts_timing.py -- K timed calls after two warm-up calls of each of:
  contacts_count_only   gpe_query_contacts with every output NULL: the reference (keys, sort, records, the same walk)
  count_only            gpe_query_clusters with every array NULL (keys, sort, records, hook, flatten, sizes)
  labels_sizes          ... with the label and size arrays (adds the download of 2 n words)
  cluster_of            gpe_query_cluster_of for the particle in the middle of the storage order, all row arrays
Then two adversarial scenes of --adversarial particles, the same three cluster calls each:
  pile                  a square lattice at a spacing of 1.5 radii: every particle touches four others, one cluster
  serpentine_descending one path -- rows at a spacing of 1.5 radii joined at alternating ends -- stored from its far end
                        to its start, so that every hook points at the next lower index
Per call: host wall time of the whole entry point (median) and the mean device time of each profiler scope.  One JSON
line per (scene, N, case) on stdout, all of them in --out.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gpe = importlib.import_module("gpu-physics-engine_amd")
L = gpe._lib
F32 = np.float32
U32P = C.POINTER(C.c_uint32)


def timed(st, calls, one):
    walls = []
    for _ in range(2):
        one()
    st.ctx.set_profiling(True)
    st.ctx.reset_timings()
    for _ in range(calls):
        st.ctx.sync()
        t0 = time.perf_counter()
        r = one()
        st.ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    tim = st.ctx.timings()
    st.ctx.set_profiling(False)
    scopes = {k: round(v[0] / max(1, v[1]), 4) for k, v in tim.items()}
    return round(float(np.median(walls)), 4), scopes, r


def raw_contacts(st):
    res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=0)
    st.ctx.call("gpe_query_contacts", C.byref(res))
    return res.count


def raw_clusters(st, label=None, size=None):
    res = L.GpeClusterResult(struct_size=C.sizeof(L.GpeClusterResult))
    if label is not None:
        res.label, res.size = label.ctypes.data_as(U32P), size.ctypes.data_as(U32P)
    st.ctx.call("gpe_query_clusters", C.byref(res))
    return res.count, res.largest_size, res.largest_label


def cluster_calls(st, scene, n, calls, emit):
    wall, scopes, got = timed(st, calls, lambda: raw_clusters(st))
    emit(scene, n, "count_only", wall, scopes, clusters=got[0], largest_size=got[1], largest_label=got[2])
    label, size = np.empty(n, np.uint32), np.empty(n, np.uint32)
    wall, scopes, got = timed(st, calls, lambda: raw_clusters(st, label, size))
    emit(scene, n, "labels_sizes", wall, scopes, clusters=got[0], largest_size=got[1], largest_label=got[2])
    seed = n // 2
    wall, scopes, rows = timed(st, calls, lambda: st.cluster_of(index=seed, capacity=int(size[seed])))
    emit(scene, n, "cluster_of", wall, scopes, seed=seed, members=int(rows.index.size))
    return got


def lattice(n):
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    pos = np.stack([1.0 + 1.5 * (k % side), 1.0 + 1.5 * (k // side)], axis=1).astype(F32)
    return pos, np.ones(n, F32), (3.0 + 1.5 * side, 3.0 + 1.5 * side)


def serpentine_descending(n, per_row=1000):
    """about n particles of radius 1: rows 3.0 apart at a spacing of 1.5, every odd row running back, one particle 1.5
    above each row's last one joining it to the next row; listed along the path, then reversed"""
    rows = max(n // per_row, 1)
    col = np.arange(per_row)
    parts = []
    for r in range(rows):
        c = col[::-1] if r % 2 else col
        parts.append(np.stack([1.0 + 1.5 * c, np.full(per_row, 1.0 + 3.0 * r)], axis=1))
        if r + 1 < rows:
            parts.append(np.array([[1.0 + 1.5 * c[-1], 2.5 + 3.0 * r]]))
    pos = np.concatenate(parts).astype(F32)[::-1].copy()
    return pos, np.ones(len(pos), F32), (3.0 + 1.5 * per_row, 3.0 + 3.0 * rows)


def measure(recs, n, calls):
    def emit(scene, n, case, wall, scopes, **extra):
        rec = dict(scene=scene, n=n, case=case, calls=calls, wall_ms=wall, scope_ms=scopes, **extra)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.81))
    del pos, rad
    st.run(1.0 / 60.0, 20, resort_every=0, resort_first=True)
    st.ctx.sync()
    wall, scopes, cnt = timed(st, calls, lambda: raw_contacts(st))
    emit("uniform", n, "contacts_count_only", wall, scopes, contacts=cnt)
    cluster_calls(st, "uniform", n, calls, emit)
    st.close()


def adversarial(recs, n, calls):
    def emit(scene, n, case, wall, scopes, **extra):
        rec = dict(scene=scene, n=n, case=case, calls=calls, wall_ms=wall, scope_ms=scopes, **extra)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    for scene, (pos, rad, world) in (("pile", lattice(n)), ("serpentine_descending", serpentine_descending(n))):
        st = gpe.State(pos, rad, world=world, mode=gpe.MODE_COMPAT)
        m = len(rad)
        wall, scopes, cnt = timed(st, calls, lambda: raw_contacts(st))
        emit(scene, m, "contacts_count_only", wall, scopes, contacts=cnt)
        got = cluster_calls(st, scene, m, calls, emit)
        if got[:2] != (1, m):
            raise SystemExit("%s: expected one cluster of %d, got %r" % (scene, m, got))
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 100_000_000])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--adversarial", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for n in a.sizes:
        measure(recs, n, a.calls)
    if a.adversarial:
        adversarial(recs, a.adversarial, a.calls)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
