"""Profiling scopes whose boundaries are timestamps written on the device (csrc/scope_stamps.h, the default on the
context's own stream) against the same run with hipEvents (GPE_FLAG_EVENT_SCOPES): the same scope names and call counts,
the same positions, and no top-level scope longer than under events -- a stamp may only take waiting out of a scope,
never put time into it.  4096 particles in a 400 x 300 world, 12 steps: the shape of test_gpu_profiling_boundaries.py,
whose checks of order and nesting run on the default backend as they stand.

The two sides of the duration check come from different runs, and on a scene this small host and GPU take about as long
as each other over a step: a scope's 10 us a call carries a host gap under events and a small kernel's launch and
dispatch under stamps, while the bound's tolerance is one 10 ns tick.  So each side is run ROUNDS times, alternating,
every run checked for names, counts and positions, and the bound -- unchanged -- is asked of each side's shortest
reading of a scope: what the scope costs when nothing else got in the way.

KNOWN TO BE CLOSE, and able to fail, on native/collide+verlet with profiling on every step -- the one scope both of whose
boundaries a one-thread kernel writes, since no k_collide_* kernel may carry a stamp.  Measured with one run a side in
six fresh processes, 18 pairs (profiles/fixed_costs/single_pairs_4096.txt): under events the scope read 0.1372-0.1461
ms over its 12 calls in every process; under stamps 0.1211-0.1292 in three processes, 0.1375-0.1408 in two and
0.1277-0.1344 in one, and 3 of the 18 pairs lost, by 0.0001-0.0023 ms.  A process in which the host keeps ahead of the
GPU reads the scope 10 % shorter under stamps; one in which it does not reads the two alike.  Every other scope, and
every scope when each third step is sampled, was shorter under stamps in all 18 pairs (native/hash by as little as 1 %,
native/collide+verlet of every third step by as little as 0.1 %, native/sort by two thirds)."""
import numpy as np
import pytest

from test_gpu_profiling_boundaries import DT, N, NAMES, STEPS, TOP_LEVEL, _tolerance

WORLD = (400.0, 300.0)


def _run(gpe, flags, every):
    pos, rad = gpe.scenes.uniform_cloud(N, WORLD, seed=11)
    st = gpe.State(pos, rad, world=WORLD, mode=gpe.MODE_NATIVE, flags=flags)
    st.update(DT, resort=True)
    st.ctx.sync()
    st.ctx.set_profiling(every)
    st.ctx.reset_timings()
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    out = {"timings": st.ctx.timings(), "trace": st.ctx.trace(), "pos": st.positions(), "prev": st.previous_positions(),
           "info": st.ctx.pipeline_info()}
    st.close()
    return out


@pytest.fixture(scope="module")
def unprofiled(gpe):
    return _run(gpe, 0, 0)


ROUNDS = 10


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_stamps_read_as_events_do(gpe, unprofiled, every):
    L = gpe._lib
    assert not unprofiled["timings"] and not unprofiled["trace"]
    runs = {"events": [], "stamps": []}
    for _ in range(ROUNDS):
        for side, flags in (("events", L.FLAG_EVENT_SCOPES), ("stamps", 0)):
            run = _run(gpe, flags, every)
            assert run["info"]["pipeline"] == L.PIPELINE_NATIVE and run["info"]["compat_steps"] == 0, run["info"]
            assert np.array_equal(run["pos"], unprofiled["pos"]) and np.array_equal(run["prev"], unprofiled["prev"])
            assert set(run["timings"]) == NAMES
            runs[side].append(run)
    first = runs["events"][0]
    for run in runs["events"] + runs["stamps"]:
        assert {k: v[1] for k, v in run["timings"].items()} == {k: v[1] for k, v in first["timings"].items()}
        assert [n for n, _, _ in run["trace"]] == [n for n, _, _ in first["trace"]]
    tol = _tolerance([t for run in runs["events"] + runs["stamps"] for t in run["trace"]])
    print()
    for name in TOP_LEVEL:
        for side in ("stamps", "events"):
            print("profiling %d, %-30s %s %s ms over %d calls" % (every, name, side, " ".join(
                "%.5f" % r["timings"][name][0] for r in runs[side]), first["timings"][name][1]))
    for name in TOP_LEVEL:
        s = [r["timings"][name][0] for r in runs["stamps"]]
        e = [r["timings"][name][0] for r in runs["events"]]
        assert min(s) > 0.0 and min(s) <= min(e) + tol, (every, name, s, e, tol)


def _hip_runtime(gpe):
    """The HIP runtime the loaded library itself links, whatever its version; else the unversioned name."""
    import ctypes
    gpe._lib.load()
    with open("/proc/self/maps") as maps:
        for line in maps:
            path = line.split()[-1]
            if "libamdhip64.so" in path.rsplit("/", 1)[-1]:
                return ctypes.CDLL(path)
    return ctypes.CDLL("libamdhip64.so")


@pytest.mark.gpu
def test_a_lent_stream_records_events_and_the_own_stream_stamps_again(gpe):
    """gpe_set_stream: scopes on a stream the caller lends record events, whatever the flag says; back on the context's
    own stream they are stamps again.  Either way the counts are those of the steps run and the trace starts at its
    origin."""
    import ctypes
    hip = _hip_runtime(gpe)
    pos, rad = gpe.scenes.uniform_cloud(N, WORLD, seed=11)
    st = gpe.State(pos, rad, world=WORLD, mode=gpe.MODE_NATIVE)
    st.update(DT, resort=True)
    st.ctx.sync()
    st.ctx.set_profiling(1)
    lent = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(lent), 1) == 0 and lent.value      # (1: hipStreamNonBlocking)
    for stream, steps in ((lent, 3), (None, 4), (lent, 2)):
        st.ctx.call("gpe_set_stream", stream)
        st.ctx.reset_timings()
        st.run(DT, steps, resort_every=0, resort_first=False)
        timings, trace = st.ctx.timings(), st.ctx.trace()
        assert set(timings) == NAMES
        assert all(timings[name][1] == steps for name in TOP_LEVEL), timings
        assert all(t0 >= 0.0 and d >= 0.0 for _, t0, d in trace) and len(trace) == sum(v[1] for v in timings.values())
    st.ctx.call("gpe_set_stream", None)
    st.ctx.sync()
    st.close()
    assert hip.hipStreamDestroy(lent) == 0
