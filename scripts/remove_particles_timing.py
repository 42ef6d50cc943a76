"""Time particle removal on the device against the host workaround it replaces.

    python scripts/remove_particles_timing.py [N ...] [--calls K] [--out FILE]     (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud: gpe_remove_particles_in_circle (an eraser disc taking ~0.2 % of the world per
call, a new centre each call) and gpe_remove_particles (a fresh ~1 % random mask each call), two warm-up calls, then K
timed ones.  Per call: host wall time of the whole entry point (it synchronises; it includes the native
reconfiguration that gpe_set_particles also runs) and the device-event scopes of its launches (remove/count,
remove/scan, remove/scatter, remove/index reset).  The kernels' sum is set against the algorithmic bytes of the
circle form -- 12 B per particle for the count pass, 20 B read + 20 B written per survivor for the scatter, 8 B per
survivor for the index reset -- at 6.3 TB/s.  Last, the workaround: download POS / PREV / RADIUS, filter on the host,
gpe_set_particles.  One JSON line per (N, form) on stdout, and all of them in --out."""
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

HBM_ACHIEVABLE = 6.3e12          # B/s
SCOPES = ("remove/count", "remove/scan", "remove/scatter", "remove/index reset", "Remove particles")


def timed_calls(st, calls, prepare, one):
    """(median wall ms, {scope: mean device ms}, mean particles before, mean survivors) over `calls` calls of
    one(prepare()) -- prepare() is not timed"""
    walls, before, after = [], [], []
    st.ctx.set_profiling(True)
    st.ctx.reset_timings()
    for _ in range(calls):
        arg = prepare()
        before.append(st.particles.len())
        st.ctx.sync()
        t0 = time.perf_counter()
        one(arg)
        walls.append((time.perf_counter() - t0) * 1e3)
        after.append(st.particles.len())
    tim = st.ctx.timings()
    st.ctx.set_profiling(False)
    scopes = {k: tim[k][0] / max(1, tim[k][1]) for k in SCOPES if k in tim}
    return float(np.median(walls)), scopes, float(np.mean(before)), float(np.mean(after))


def measure(n, calls):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    del pos, rad
    rng = np.random.default_rng(1)
    r_disc = float(np.sqrt(0.002 * world[0] * world[1] / np.pi))
    forms = {
        "circle": (lambda: (rng.uniform(r_disc, world[0] - r_disc), rng.uniform(r_disc, world[1] - r_disc)),
                   lambda c: st.remove_particles_in_circle(c, r_disc)),
        "mask": (lambda: rng.random(st.particles.len()) < 0.01,
                 lambda m: st.remove_particles(m)),
    }
    out = []
    for form, (prepare, one) in forms.items():
        for _ in range(2):
            one(prepare())                               # warm-up: workspace allocation, first launches
        wall, scopes, nb, na = timed_calls(st, calls, prepare, one)
        kernels = sum(scopes.get(k, 0.0) for k in SCOPES[:4])
        algo = 12.0 * nb + 40.0 * na + 8.0 * na
        rec = {"n": n, "form": form, "calls": calls, "particles_before": nb, "survivors": na,
               "wall_ms": round(wall, 4), "scope_ms": {k: round(v, 4) for k, v in scopes.items()},
               "kernels_ms": round(kernels, 4), "algorithmic_bytes_circle_model": algo,
               "bound_ms": round(algo / HBM_ACHIEVABLE * 1e3, 4),
               "fraction_of_bound": round(algo / HBM_ACHIEVABLE * 1e3 / kernels, 3) if kernels > 0 else None}
        print(json.dumps(rec), flush=True)
        out.append(rec)

    # the workaround the entry points replace: download, filter on the host, set again (one call)
    cur = st.particles.len()
    m = rng.random(cur) < 0.01
    st.ctx.sync()
    t0 = time.perf_counter()
    p, q, r = st.positions(), st.previous_positions(), st.radii()
    t1 = time.perf_counter()
    keep = ~m
    p, q, r = np.ascontiguousarray(p[keep]), np.ascontiguousarray(q[keep]), np.ascontiguousarray(r[keep])
    t2 = time.perf_counter()
    st.ctx.call("gpe_set_particles", p.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                r.ctypes.data_as(C.c_void_p), p.shape[0])
    t3 = time.perf_counter()
    rec = {"n": n, "form": "host_workaround", "particles_before": cur, "survivors": int(keep.sum()),
           "download_ms": round((t1 - t0) * 1e3, 2), "filter_ms": round((t2 - t1) * 1e3, 2),
           "set_particles_ms": round((t3 - t2) * 1e3, 2), "wall_ms": round((t3 - t0) * 1e3, 2)}
    print(json.dumps(rec), flush=True)
    out.append(rec)
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
