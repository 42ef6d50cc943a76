"""Time the particle-uid paths on the device (csrc/k_uids.hip) against the host workaround for removal by uid.

    python scripts/uids_timing.py [N ...] [--calls K] [--out FILE]     (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud, K timed calls after two warm-up calls of each of:
  resort_off / resort_on   gpe_morton_resort with uids off, then on: the gather is k_rearrange (44 B per particle)
                           resp. k_rearrange_uids (52 B); scope "Particle rearranging"
  map                      gpe_find_uids of one uid right after a re-sort, so that the uid -> index map is rebuilt;
                           scope "uids/map" (copy + iota, the 4-pass pair sort, the adjacent-key pass)
  find_1 / find_1000 / find_1000000   gpe_find_uids of that many random present uids with every output, map valid
  remove_1000              gpe_remove_particles_by_uid of 1000 random present uids (the map is rebuilt every call: the
                           previous removal made it stale)
  host_remove_1000         the workaround: download GPE_UIDS, numpy isin, gpe_remove_particles(mask)
Per call: host wall time of the whole entry point (median) and the mean device time of each profiler scope.  One JSON
line per (N, case) on stdout, and all of them in --out.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gpe = importlib.import_module("gpu-physics-engine_amd")

HBM_ACHIEVABLE = 6.3e12          # B/s


def timed(st, calls, prepare, one):
    walls = []
    st.ctx.set_profiling(True)
    st.ctx.reset_timings()
    for _ in range(calls):
        arg = prepare()
        st.ctx.sync()
        t0 = time.perf_counter()
        one(arg)
        st.ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    tim = st.ctx.timings()
    st.ctx.set_profiling(False)
    scopes = {k: round(v[0] / max(1, v[1]), 4) for k, v in tim.items()}
    return round(float(np.median(walls)), 4), scopes


def measure(n, calls):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    del pos, rad
    rng = np.random.default_rng(1)
    out = []

    def emit(case, wall, scopes, **extra):
        rec = dict(n=n, case=case, calls=calls, particles=st.particles.len(), wall_ms=wall, scope_ms=scopes, **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)

    nothing = lambda: None                                          # noqa: E731
    resort = lambda _: st.particles.sort_by_cell_id()               # noqa: E731
    for case in ("resort_off", "resort_on"):
        if case == "resort_on":
            st.enable_uids()
        for _ in range(2):
            resort(None)
        wall, scopes = timed(st, calls, nothing, resort)
        g = scopes.get("Particle rearranging")
        per = 52.0 if case == "resort_on" else 44.0
        emit(case, wall, scopes, gather_bytes=per * n,
             gather_fraction_of_bound=round(per * n / HBM_ACHIEVABLE * 1e3 / g, 3) if g else None)

    one_uid = np.zeros(1, np.uint32)
    for _ in range(2):
        resort(None)
        st.find_uids(one_uid)
    wall, scopes = timed(st, calls, lambda: resort(None), lambda _: st.find_uids(one_uid))
    emit("map", wall, scopes)                                       # the wall time includes the lookup of one uid

    for k in (1, 1000, 1_000_000):
        u = st.uids()
        q = rng.choice(u, k).astype(np.uint32)
        st.find_uids(q)
        st.find_uids(q)
        wall, scopes = timed(st, calls, lambda: q, lambda a: st.find_uids(a))
        emit("find_%d" % k, wall, scopes)

    def pick():
        return rng.choice(st.uids(), 1000, replace=False).astype(np.uint32)

    for _ in range(2):
        st.remove_particles_by_uid(pick())
    wall, scopes = timed(st, calls, pick, lambda a: st.remove_particles_by_uid(a))
    emit("remove_1000", wall, scopes)

    walls, parts = [], []
    for _ in range(calls):
        q = pick()
        st.ctx.sync()
        t0 = time.perf_counter()
        u = st.uids()
        t1 = time.perf_counter()
        m = np.isin(u, q)
        t2 = time.perf_counter()
        st.remove_particles(m)
        t3 = time.perf_counter()
        walls.append((t3 - t0) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    p = np.median(np.array(parts), axis=0)
    emit("host_remove_1000", round(float(np.median(walls)), 4), {}, download_ms=round(float(p[0]), 3),
         isin_ms=round(float(p[1]), 3), remove_particles_ms=round(float(p[2]), 3))
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
