"""Time the in-place edits on the device (csrc/k_edit.hip) against the host detour they replace.

    python scripts/edit_timing.py [N ...] [--calls K] [--out FILE]     (default N: 1000000 100000000)

For each N, on a uniform NATIVE cloud (scenes.world_for / uniform_cloud) after a Morton re-sort and two steps, K timed
calls after two warm-up calls of each of:
  query_count_empty   gpe_query_circle, every output NULL, a circle that holds nothing: k_query_count, R 8 B per particle
  kick_empty          gpe_kick_circle over the same circle, n_kicked NULL: k_kick reads the same 8 B per particle
  kick_empty_counted  ... with n_kicked (the COUNT instantiation, the call blocks)
  kick_brush          GPE_VEL_ADD over a brush of about 3000 particles, n_kicked NULL
  kick_all            GPE_VEL_SCALE over everything (R 8 + 8 B, W 8 B per particle), n_kicked NULL
  edit_k1 / edit_k100000   gpe_edit_particles by index with pos + prev + radius for k random particles
  refresh             gpe_refresh alone: the re-derivation of the native pipeline an edit of pos or radius ends with
  host_detour_k100000 the detour: download pos / prev / radius, edit k rows in numpy, gpe_set_particles
Per call: host wall time of the whole entry point (median) and the mean device time of each profiler scope, with the
kernels' achieved bytes/s against the 8 TB/s peak.  One JSON line per (N, case) on stdout, all of them in --out.  Run it
under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import argparse
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
DT = 1.0 / 60.0


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


def bandwidth(bytes_, ms):
    return None if not ms else dict(bytes=bytes_, tb_per_s=round(bytes_ / (ms * 1e-3) / 1e12, 3),
                                    fraction_of_peak=round(bytes_ / (ms * 1e-3) / HBM_PEAK, 3))


def measure(n, calls):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    del pos, rad
    st.update(DT, resort=True)
    st.update(DT)
    st.ctx.sync()
    w, h = world
    cx, cy = w * 0.5, h * 0.5
    r_brush = float(np.sqrt(3000.0 / (np.pi * n / (w * h))))
    nowhere = ((-1e6, -1e6), 5.0)
    out = []

    def emit(case, wall, scopes, **extra):
        rec = dict(n=n, case=case, calls=calls, wall_ms=wall, scope_ms=scopes, **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)

    # the two 8 B-per-particle passes, alternated
    for rep in range(2):
        wall, scopes, cnt = timed(st, calls, lambda: st.count_circle(*nowhere))
        emit("query_count_empty", wall, scopes, rep=rep, matches=cnt, kernel=bandwidth(8 * n, scopes.get("query/count")))
        wall, scopes, _ = timed(st, calls, lambda: st.kick_circle(nowhere[0], nowhere[1], L.VEL_ADD, (0.5, 0.0), count=False))
        emit("kick_empty", wall, scopes, rep=rep, kernel=bandwidth(8 * n, scopes.get("Kick particles")))
    wall, scopes, cnt = timed(st, calls, lambda: st.kick_circle(nowhere[0], nowhere[1], L.VEL_ADD, (0.5, 0.0)))
    emit("kick_empty_counted", wall, scopes, kicked=cnt, kernel=bandwidth(8 * n, scopes.get("Kick particles")))
    brush = (cx + 0.123 * w, cy - 0.2 * h)
    kicked = st.count_circle(brush, r_brush)
    wall, scopes, _ = timed(st, calls, lambda: st.kick_circle(brush, r_brush, L.VEL_ADD, (0.01, 0.0), count=False))
    emit("kick_brush", wall, scopes, kicked=kicked, kernel=bandwidth(8 * n + 16 * kicked, scopes.get("Kick particles")))
    everything = ((-np.inf, -np.inf), (np.inf, np.inf))
    wall, scopes, _ = timed(st, calls, lambda: st.kick_box(everything[0], everything[1], L.VEL_SCALE, (0.999, 0.999), count=False))
    emit("kick_all", wall, scopes, kicked=n, kernel=bandwidth(24 * n, scopes.get("Kick particles")))
    wall, scopes, cnt = timed(st, calls, lambda: st.kick_box(everything[0], everything[1], L.VEL_SCALE, (0.999, 0.999)))
    emit("kick_all_counted", wall, scopes, kicked=cnt, kernel=bandwidth(24 * n, scopes.get("Kick particles")))

    rng = np.random.default_rng(7)
    for k in (1, 100_000):
        idx = rng.permutation(n)[:k].astype(np.uint32)
        p = (rng.random((k, 2), dtype=np.float32) * np.array(world, np.float32)).astype(np.float32)
        r = np.full(k, 0.5, np.float32)
        wall, scopes, cnt = timed(st, calls, lambda: st.edit_particles(indices=idx, positions=p, previous=p, radii=r))
        inside = sum(scopes.get(s, 0.0) for s in ("edit/check", "edit/apply", "edit/max radius"))
        emit("edit_k%d" % k, wall, scopes, edited=cnt, reconfigure_and_host_ms=round(wall - inside, 4),
             max_radius_kernels=bandwidth(4 * n, scopes.get("edit/max radius")))
        wall, scopes, cnt = timed(st, calls, lambda: st.edit_particles(indices=idx, previous=p))
        emit("edit_prev_only_k%d" % k, wall, scopes, edited=cnt)
    wall, scopes, _ = timed(st, calls, lambda: st.ctx.call("gpe_refresh"))
    emit("refresh", wall, scopes)

    k = 100_000
    idx = rng.permutation(n)[:k]
    p = (rng.random((k, 2), dtype=np.float32) * np.array(world, np.float32)).astype(np.float32)
    walls, parts = [], []
    for _ in range(calls):
        st.ctx.sync()
        t0 = time.perf_counter()
        a, b, c = st.positions(), st.previous_positions(), st.radii()
        t1 = time.perf_counter()
        a[idx] = p
        b[idx] = p
        c[idx] = 0.5
        t2 = time.perf_counter()
        st.ctx.call("gpe_set_particles", a.ctypes.data, b.ctypes.data, c.ctypes.data, n)
        st.ctx.sync()
        t3 = time.perf_counter()
        walls.append((t3 - t0) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        del a, b, c
    q = np.median(np.array(parts), axis=0)
    emit("host_detour_k%d" % k, round(float(np.median(walls)), 4), {}, download_ms=round(float(q[0]), 3),
         numpy_ms=round(float(q[1]), 3), set_particles_ms=round(float(q[2]), 3))
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
