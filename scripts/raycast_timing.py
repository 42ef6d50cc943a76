"""Time ray casts and the segment query on the device (csrc/k_raycast.hip, csrc/k_query.hip) against the host route.

    python scripts/raycast_timing.py [N ...] [--calls K] [--host-calls K] [--out FILE]   (default N: 1000000 100000000)

For each N, on the contact profile's scene -- a uniform NATIVE cloud (scenes.world_for / uniform_cloud) after 20 steps
under gravity that begin with a Morton re-sort -- K timed calls after two warm-up calls of each of:
  rays_1 / rays_1024 / rays_65536   gpe_cast_rays of that many random rays of about 100 units (index and t requested)
  ray_horizontal / ray_vertical     one world-crossing ray
  segment_count                     gpe_query_segment of the horizontal ray with every output NULL
  host_route                        download GPE_POS and GPE_RADIUS, then the numpy float32 model for one ray
Per call the device time of every profiler scope (hipEvent pairs around the work on the context's stream, read after a
synchronisation): `binning` = contacts/keys + contacts/sort, `rays/rows`, `rays/cast`, `query/count`; per case their
median, minimum and maximum over the K calls and the median host wall time of the whole entry point.  One JSON line per
(N, case) on stdout, all of them in --out."""
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
from tests import _ray_model as M  # noqa: E402

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


def cast(st, o, e):
    k = len(o)
    index, t = np.empty(k, np.uint32), np.empty(k, F32)
    c = L.GpeRayCast(struct_size=C.sizeof(L.GpeRayCast), k=k)
    c.from_xy, c.to_xy = o.ctypes.data_as(C.POINTER(C.c_float)), e.ctypes.data_as(C.POINTER(C.c_float))
    c.index, c.t = index.ctypes.data_as(C.POINTER(C.c_uint32)), t.ctypes.data_as(C.POINTER(C.c_float))
    st.ctx.call("gpe_cast_rays", C.byref(c))
    return int(c.hits), index, t


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
    for k in (1, 1024, 65536):
        o = rng.uniform(0.0, 1.0, (k, 2)) * w
        ang = rng.uniform(0.0, 2 * np.pi, k)
        e = o + 100.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        o, e = np.ascontiguousarray(o, F32), np.ascontiguousarray(e, F32)
        wall, scopes, r = timed(st, calls, lambda: cast(st, o, e))
        emit("rays_%d" % k, wall, scopes, hits=r[0])
    hor = (np.array([[0.0, 0.37 * w[1]]], F32), np.array([[w[0], 0.37 * w[1]]], F32))
    ver = (np.array([[0.41 * w[0], 0.0]], F32), np.array([[0.41 * w[0], w[1]]], F32))
    first = {}
    for name, (o, e) in (("ray_horizontal", hor), ("ray_vertical", ver)):
        wall, scopes, r = timed(st, calls, lambda: cast(st, o, e))
        first[name] = (int(r[1][0]), float(r[2][0]))
        emit(name, wall, scopes, hits=r[0], index=first[name][0], t=first[name][1])
    a, b = hor[0][0], hor[1][0]
    wall, scopes, cnt = timed(st, calls, lambda: st.count_segment(a, b))
    emit("segment_count", wall, scopes, count=cnt)

    walls, parts, got = [], [], None
    for _ in range(host_calls):
        st.ctx.sync()
        t0 = time.perf_counter()
        p = st.positions()
        r = st.radii()
        t1 = time.perf_counter()
        got = M.cast(hor[0], hor[1], p, r)
        t2 = time.perf_counter()
        walls.append((t2 - t0) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        del p, r
    parts = np.array(parts)
    emit("host_route", spread(walls), {}, host_calls=host_calls, download_ms=spread(parts[:, 0]),
         numpy_model_ms=spread(parts[:, 1]), index=int(got["index"][0]), t=float(got["t"][0]))
    if (int(got["index"][0]), float(got["t"][0])) != first["ray_horizontal"]:
        raise SystemExit("the host model found %r, the device %r" % ((got["index"][0], got["t"][0]), first["ray_horizontal"]))
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
