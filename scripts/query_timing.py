"""Time the region queries and picking on the device (csrc/k_query.hip) against the host workaround.

    python scripts/query_timing.py [N ...] [--calls K] [--out FILE]     (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud (scenes.world_for / uniform_cloud), once in the generated (random) storage order
and once after a Morton re-sort, K timed calls after two warm-up calls of each of:
  count_1pct        gpe_query_circle with every output NULL, a circle of 1 % of the world's area (count + scan only)
  brush_all         gpe_query_circle of a brush of about 3000 particles with index, uid, pos, prev and radius
  box_half_index    gpe_query_box over the left half of the world (infinite y bounds), index only, capacity = n
  pick              gpe_pick at the centre of a particle near the centre of the world
  host_circle_1pct  the workaround for count_1pct: download GPE_POS, the numpy float32 predicate, np.nonzero
Per call: host wall time of the whole entry point (median) and the mean device time of each profiler scope, with the
count and pick kernels' achieved bytes/s against the 8 TB/s peak.  One JSON line per (N, order, case) on stdout, all of
them in --out.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
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

HBM_PEAK = 8.0e12          # B/s


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


def raw_query(st, name, args, capacity, fields):
    """one gpe_query_* / gpe_pick call through ctypes with the listed outputs; returns the count"""
    keep = []
    res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=capacity)
    for f in fields:
        width = 2 if f in ("pos_xy", "prev_xy") else 1
        a = np.empty(max(capacity, 1) * width, np.uint32 if f in ("index", "uid") else np.float32)
        keep.append(a)
        setattr(res, f, a.ctypes.data_as(C.POINTER(C.c_uint32 if f in ("index", "uid") else C.c_float)))
    st.ctx.call(name, *args, C.byref(res))
    return res.count


def bandwidth(bytes_, ms):
    return None if not ms else dict(bytes=bytes_, tb_per_s=round(bytes_ / (ms * 1e-3) / 1e12, 3),
                                    fraction_of_peak=round(bytes_ / (ms * 1e-3) / HBM_PEAK, 3))


def measure(n, calls):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    del pos, rad
    st.enable_uids()
    w, h = world
    cx, cy = w * 0.5, h * 0.5
    r_1pct = float(np.sqrt(0.01 * w * h / np.pi))
    r_brush = float(np.sqrt(3000.0 / (np.pi * n / (w * h))))
    out = []
    for order in ("random", "sorted"):
        if order == "sorted":
            st.particles.sort_by_cell_id()
            st.ctx.sync()

        def emit(case, wall, scopes, **extra):
            rec = dict(n=n, order=order, case=case, calls=calls, wall_ms=wall, scope_ms=scopes, **extra)
            print(json.dumps(rec), flush=True)
            out.append(rec)

        wall, scopes, cnt = timed(st, calls, lambda: raw_query(st, "gpe_query_circle", (cx, cy, r_1pct), 0, ()))
        emit("count_1pct", wall, scopes, matches=cnt, count_kernel=bandwidth(8 * n, scopes.get("query/count")))
        args = (cx + 0.123 * w, cy - 0.2 * h, r_brush)
        wall, scopes, cnt = timed(st, calls, lambda: raw_query(st, "gpe_query_circle", args, 8192,
                                                                ("index", "uid", "pos_xy", "prev_xy", "radius")))
        g, c = scopes.get("query/gather"), scopes.get("query/count")
        emit("brush_all", wall, scopes, matches=cnt, gather_over_count=round(g / c, 3) if g and c else None)
        args = (-np.inf, -np.inf, cx, np.inf)
        wall, scopes, cnt = timed(st, calls, lambda: raw_query(st, "gpe_query_box", args, n, ("index",)))
        emit("box_half_index", wall, scopes, matches=cnt, count_kernel=bandwidth(8 * n, scopes.get("query/count")))
        hit = st.query_circle((cx, cy), r_brush).pos[0]           # a point on a particle: pick finds one
        px, py = float(hit[0]), float(hit[1])
        wall, scopes, cnt = timed(st, calls, lambda: raw_query(st, "gpe_pick", (px, py), 1,
                                                                ("index", "uid", "pos_xy", "prev_xy", "radius")))
        emit("pick", wall, scopes, matches=cnt, pick_kernels=bandwidth(12 * n, scopes.get("query/pick")))

        walls, parts = [], []
        for _ in range(calls):
            st.ctx.sync()
            t0 = time.perf_counter()
            p = st.positions()
            t1 = time.perf_counter()
            dx = p[:, 0] - np.float32(cx)
            dy = p[:, 1] - np.float32(cy)
            idx = np.nonzero(dx * dx + dy * dy <= np.float32(r_1pct) * np.float32(r_1pct))[0]
            t2 = time.perf_counter()
            walls.append((t2 - t0) * 1e3)
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            del p, dx, dy
        q = np.median(np.array(parts), axis=0)
        emit("host_circle_1pct", round(float(np.median(walls)), 4), {}, matches=int(idx.size),
             download_ms=round(float(q[0]), 3), numpy_ms=round(float(q[1]), 3))
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 100_000_000])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for n in a.sizes:
        recs += measure(n, a.calls)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
