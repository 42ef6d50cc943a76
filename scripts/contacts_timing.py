"""Time the contact query on the device (csrc/k_contacts.hip) against the host route.

    python scripts/contacts_timing.py [N ...] [--calls K] [--host-max N] [--out FILE]   (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud (scenes.world_for / uniform_cloud) after 20 steps under gravity that begin with a
Morton re-sort, K timed calls after two warm-up calls of each of:
  count_only   gpe_query_contacts with every output NULL (keys, sort, count)
  degrees      ... with the degree array (adds the download of n words)
  full_list    ... with index_a, index_b and overlap, capacity = count (adds scan, gather and the copies)
  host_route   for N <= --host-max: download GPE_POS and GPE_RADIUS, then a numpy cell-binned search (cells of 2.2 x the
               largest radius, the 3 x 3 neighbourhood through searchsorted on the sorted cell keys, the float32
               predicate of include/gpe.h); above it only the two downloads are timed
Per call: host wall time of the whole entry point (median) and the mean device time of each profiler scope.  One JSON
line per (N, case) on stdout, all of them in --out.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel
times."""
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


def raw_contacts(st, capacity, fields, degree=None):
    keep = []
    res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=capacity)
    for f in fields:
        a = np.empty(max(capacity, 1), F32 if f == "overlap" else np.uint32)
        keep.append(a)
        setattr(res, f, a.ctypes.data_as(C.POINTER(C.c_float if f == "overlap" else C.c_uint32)))
    if degree is not None:
        res.degree = degree.ctypes.data_as(C.POINTER(C.c_uint32))
    st.ctx.call("gpe_query_contacts", C.byref(res))
    return res.count


def host_search(pos, rad):
    """the number of contacts by a numpy cell-binned search (what a host does after the two downloads)"""
    n = len(rad)
    cs = F32(np.abs(rad).max()) * F32(2.2)
    cx = np.floor(pos[:, 0] / cs).astype(np.int64)
    cy = np.floor(pos[:, 1] / cs).astype(np.int64)
    cx -= cx.min() - 1
    cy -= cy.min() - 1
    width = int(cx.max()) + 2
    key = cy * width + cx
    order = np.argsort(key, kind="stable")
    skey = key[order]
    total = 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            want = key + dy * width + dx
            lo = np.searchsorted(skey, want, "left")
            hi = np.searchsorted(skey, want, "right")
            cnt = hi - lo
            i = np.repeat(np.arange(n), cnt)
            off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            j = order[np.repeat(lo, cnt) + off]
            up = j > i
            i, j = i[up], j[up]
            ddx = pos[i, 0] - pos[j, 0]
            ddy = pos[i, 1] - pos[j, 1]
            rs = rad[i] + rad[j]
            total += int(np.count_nonzero(ddx * ddx + ddy * ddy < rs * rs))
    return total


def measure(n, calls, host_max):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.81))
    del pos, rad
    st.run(1.0 / 60.0, 20, resort_every=0, resort_first=True)
    st.ctx.sync()
    out = []

    def emit(case, wall, scopes, **extra):
        rec = dict(n=n, case=case, calls=calls, wall_ms=wall, scope_ms=scopes, **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)

    wall, scopes, cnt = timed(st, calls, lambda: raw_contacts(st, 0, ()))
    emit("count_only", wall, scopes, contacts=cnt)
    degree = np.empty(n, np.uint32)
    wall, scopes, cnt = timed(st, calls, lambda: raw_contacts(st, 0, (), degree))
    emit("degrees", wall, scopes, contacts=cnt, max_degree=int(degree.max()), mean_degree=round(float(degree.mean()), 3))
    wall, scopes, cnt2 = timed(st, calls, lambda: raw_contacts(st, cnt, ("index_a", "index_b", "overlap")))
    emit("full_list", wall, scopes, contacts=cnt2)

    walls, parts, found = [], [], None
    for _ in range(calls if n <= host_max else 3):
        st.ctx.sync()
        t0 = time.perf_counter()
        p = st.positions()
        r = st.radii()
        t1 = time.perf_counter()
        if n <= host_max:
            found = host_search(p, r)
        t2 = time.perf_counter()
        walls.append((t2 - t0) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        del p, r
    q = np.median(np.array(parts), axis=0)
    emit("host_route", round(float(np.median(walls)), 4), {}, contacts=found, download_ms=round(float(q[0]), 3),
         numpy_search_ms=round(float(q[1]), 3) if n <= host_max else None)
    if found is not None and found != cnt:
        raise SystemExit("host search found %d contacts, the device %d" % (found, cnt))
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 100_000_000])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for n in a.sizes:
        recs += measure(n, a.calls, a.host_max)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
