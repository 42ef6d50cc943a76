"""What profiling and synchronising cost the native step: python scripts/fixed_costs.py [N] [steps] [flags]
The bench scene (scenes.uniform_cloud in scenes.world_for(N), gravity off, the first step re-sorts), N = 1 M by default.
  * ms per step of gpe_run over `steps` steps (default 2000) with profiling off, gpe_set_profiling(10) and (1);
  * one gpe_sync on an idle context, median of 200 calls;
  * gpe_step + gpe_sync per frame, median of 200 frames;
  * a window of 20 and of 100 steps of gpe_run closed by gpe_sync, profiling off, median of 200 windows.
flags: gpe_config.flags (e.g. 4096 = GPE_FLAG_EVENT_SCOPES).  One line per figure, then one JSON line.
steps = "trace": 10 steps, then 40 with gpe_set_profiling(10) and nothing else -- the run to take a rocprofv3
--kernel-trace of (scripts/trace_step_gaps.py reads it)."""
import importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gpe = importlib.import_module("gpu-physics-engine_amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
steps = int(sys.argv[2]) if len(sys.argv) > 2 and not trace else 2000
flags = int(sys.argv[3]) if len(sys.argv) > 3 else 0
DT = 1.0 / 60.0
world = gpe.scenes.world_for(n)
pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
out = {"n": n, "steps": steps, "flags": flags}
if trace:
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, flags=flags)
    st.run(DT, 10, resort_every=0, resort_first=True)
    st.ctx.sync()
    st.ctx.set_profiling(10)
    st.ctx.reset_timings()
    st.run(DT, 40, resort_every=0, resort_first=False)
    st.ctx.sync()
    st.close()
    sys.exit(0)


def run_ms_per_step(every):
    """A fresh state per figure: every figure times the same steps of the run (the cloud relaxes as it goes)."""
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, flags=flags)
    st.run(DT, 10, resort_every=0, resort_first=True)
    st.ctx.sync()
    st.ctx.set_profiling(every)
    st.ctx.reset_timings()
    t0 = time.perf_counter()
    st.run(DT, steps, resort_every=0, resort_first=False)
    st.ctx.sync()
    el = time.perf_counter() - t0
    tim = st.ctx.timings()
    st.close()
    return el / steps * 1e3, {k: round(v[0] / max(1, v[1]) * 1e3, 2) for k, v in tim.items()}


for every in (0, 10, 1, 0, 10, 1):                       # twice over: the second round shows the run-to-run spread
    ms, scopes = run_ms_per_step(every)
    key = "run_ms_per_step_profiling_%d" % every
    out.setdefault(key, []).append(round(ms, 5))
    if scopes:
        out["scopes_us_profiling_%d" % every] = scopes
    print("gpe_run, profiling %2d: %.5f ms/step  %s" % (every, ms, scopes), flush=True)
p0, p10, p1 = (min(out["run_ms_per_step_profiling_%d" % e]) for e in (0, 10, 1))
out["sampled_step_extra_us_from_10"] = round((p10 - p0) * 10 * 1e3, 2)
out["sampled_step_extra_us_from_1"] = round((p1 - p0) * 1e3, 2)
print("a sampled step costs %.1f us more than a plain one (profiling 10), %.1f us (profiling 1)"
      % (out["sampled_step_extra_us_from_10"], out["sampled_step_extra_us_from_1"]), flush=True)

st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, flags=flags)
st.run(DT, 10, resort_every=0, resort_first=True)
st.ctx.sync()
t = []
for _ in range(200):
    t0 = time.perf_counter()
    st.ctx.sync()
    t.append(time.perf_counter() - t0)
out["idle_sync_us_median"] = round(statistics.median(t) * 1e6, 2)
out["idle_sync_us_min"] = round(min(t) * 1e6, 2)
print("gpe_sync, idle context: median %.2f us, min %.2f us of 200" % (out["idle_sync_us_median"], out["idle_sync_us_min"]), flush=True)
t = []
for _ in range(200):
    t0 = time.perf_counter()
    st.update(DT)
    st.ctx.sync()
    t.append(time.perf_counter() - t0)
out["frame_us_median"] = round(statistics.median(t) * 1e6, 2)
out["frame_us_min"] = round(min(t) * 1e6, 2)
print("gpe_step + gpe_sync: median %.2f us, min %.2f us of 200 frames" % (out["frame_us_median"], out["frame_us_min"]), flush=True)
# a window of k steps closed by gpe_sync, profiling off, as bench.py's value_fresh_cloud times it: what the window costs
# beyond k steps of the long run above is what its end costs when gpe_sync comes right behind the work, not idle
for k in (20, 100):
    t = []
    for _ in range(200):
        t0 = time.perf_counter()
        st.run(DT, k, resort_every=0, resort_first=False)
        st.ctx.sync()
        t.append(time.perf_counter() - t0)
    med = statistics.median(t) * 1e6
    out["window_%d_us_median" % k] = round(med, 2)
    out["window_%d_end_us" % k] = round(med - k * p0 * 1e3, 2)
    print("window of %3d steps + gpe_sync, profiling off: median %.2f us of 200 = %d steps of the long run + %.2f us"
          % (k, med, k, out["window_%d_end_us" % k]), flush=True)
st.close()
print(json.dumps(out), flush=True)
