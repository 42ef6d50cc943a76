"""Time nearest-neighbour queries on the device (csrc/k_nearest.hip) against the host route and the circle query.

    python scripts/nearest_timing.py [N ...] [--calls K] [--host-calls K] [--out FILE]   (default N: 1000000 100000000)

For each N, on the contact profile's scene -- a uniform NATIVE cloud (scenes.world_for / uniform_cloud) after 20 steps
under gravity that begin with a Morton re-sort -- K timed calls after two warm-up calls of each of:
  nearest_k{1,65536}_m{1,16}   gpe_query_nearest of that many random points in the world, no cutoff (count, index and
                               dist2 requested)
  circle_k1                    gpe_query_circle around the one point with the radius that holds its 16 nearest (what a
                               host would do with a well-guessed radius: one full pass per point, members in index order)
  host_route_m{1,16}           download GPE_POS, then numpy: d2 to every particle and argpartition for the one point
Per call the device time of every profiler scope (hipEvent pairs around the work on the context's stream, read after a
synchronisation): `binning` = contacts/keys + contacts/sort, `nearest/rows`, `nearest/search`, `query/count`; per case
their median, minimum and maximum over the K calls and the median host wall time of the whole entry point.  One JSON
line per (N, case) on stdout, all of them in --out."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gpe = importlib.import_module("gpu-physics-engine_amd")

L = gpe._lib
F32 = np.float32


def spread(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def timed(st, calls, one):
    for _ in range(2):
        one()
    st.ctx.set_profiling(True)
    walls, scopes, r = [], {}, None
    for _ in range(calls):
        st.ctx.reset_timings()
        st.ctx.sync()
        t0 = time.perf_counter()
        r = one()
        st.ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
        tim = {k: v[0] for k, v in st.ctx.timings().items()}
        tim["binning"] = tim.get("contacts/keys", 0.0) + tim.get("contacts/sort", 0.0)
        for k, v in tim.items():
            scopes.setdefault(k, []).append(v)
    st.ctx.set_profiling(False)
    return spread(walls), {k: spread(v) for k, v in scopes.items() if len(v) == calls}, r


def nearest(st, pts, m, out):
    """gpe_query_nearest into the preallocated (count, index, dist2) of `out`"""
    count, index, dist2 = out
    q = L.GpeNearestQuery(struct_size=C.sizeof(L.GpeNearestQuery), k=len(pts), m=m, max_distance=float("inf"))
    q.point_xy = pts.ctypes.data_as(C.POINTER(C.c_float))
    q.count, q.index = count.ctypes.data_as(C.POINTER(C.c_uint32)), index.ctypes.data_as(C.POINTER(C.c_uint32))
    q.dist2 = dist2.ctypes.data_as(C.POINTER(C.c_float))
    st.ctx.call("gpe_query_nearest", C.byref(q))
    return int(q.found)


def host_nearest(p, pt, m):
    """the host route's search: float32 d2 to every particle, argpartition, then the order of (d2, index)"""
    dx = p[:, 0] - pt[0]
    dy = p[:, 1] - pt[1]
    d2 = dx * dx + dy * dy
    part = np.argpartition(d2, m - 1)[:m] if m < len(d2) else np.arange(len(d2))
    return part[np.lexsort((part, d2[part]))]


def measure(n, calls, host_calls):
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

    rng = np.random.default_rng(1)
    w = np.array(world, np.float64)
    all_pts = np.ascontiguousarray(rng.uniform(0.0, 1.0, (65536, 2)) * w, F32)
    first = {}
    for k in (1, 65536):
        pts = np.ascontiguousarray(all_pts[:k])
        for m in (1, 16):
            bufs = (np.empty(k, np.uint32), np.empty((k, m), np.uint32), np.empty((k, m), F32))
            wall, scopes, found = timed(st, calls, lambda: nearest(st, pts, m, bufs))
            emit("nearest_k%d_m%d" % (k, m), wall, scopes, found=found)
            if k == 1:
                first[m] = (bufs[1][0].copy(), bufs[2][0].copy())
    pt = all_pts[0]
    reach = float(np.sqrt(np.float64(first[16][1][-1]))) * 1.0001
    wall, scopes, cnt = timed(st, calls, lambda: st.count_circle(pt, reach))
    emit("circle_k1", wall, scopes, count=cnt, radius=reach)

    for m in (1, 16):
        walls, parts, got = [], [], None
        for _ in range(host_calls):
            st.ctx.sync()
            t0 = time.perf_counter()
            p = st.positions()
            t1 = time.perf_counter()
            got = host_nearest(p, pt, m)
            t2 = time.perf_counter()
            walls.append((t2 - t0) * 1e3)
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            del p
        parts = np.array(parts)
        # (argpartition may keep another of several particles tied at the m-th d2; the device keeps the lowest index)
        emit("host_route_m%d" % m, spread(walls), {}, host_calls=host_calls, download_ms=spread(parts[:, 0]),
             numpy_ms=spread(parts[:, 1]), index=[int(i) for i in got],
             agrees_with_device=bool(np.array_equal(got.astype(np.uint32), first[m][0])))
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 100_000_000])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for n in a.sizes:
        recs += measure(n, a.calls, a.host_calls)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
