"""Profiling scopes of the native step share the events at their common boundaries (csrc/scope_events.h): what
gpe_get_timings and gpe_get_trace return must read as it did when every scope recorded a pair of its own -- the same
names, the same call counts, ordered top-level scopes, nested scopes inside their parents -- every step
(gpe_set_profiling(1)) and sampled (3).  The event bookkeeping itself (who shares what, every event released once) is
counted on the CPU: tests/test_scope_events_cpu.py."""
import numpy as np
import pytest

N = 4096
STEPS = 12
DT = 1.0 / 60.0
# the scopes of a native step without a re-sort, as the parent of this change named them
TOP_LEVEL = ["native/hash", "native/sort", "native/collide+verlet", "native/collide-dense-regions"]
NESTED = {"sort/onesweep": "native/sort"}
NAMES = set(TOP_LEVEL) | set(NESTED)
# One event tick is 10 ns (the 100 MHz timestamp counter behind hipEventElapsedTime).  A start and a duration each reach
# the host as a binary32 number of milliseconds, rounded once; two sums of two such numbers are compared, so up to four
# half-ulps of the largest end time in the trace come on top of the tick.
TICK_MS = 1.0e-5


def _tolerance(trace):
    latest = max(t0 + d for _, t0, d in trace)
    return TICK_MS + 2.0 * float(np.spacing(np.float32(latest)))


def _state(gpe):
    world = (400.0, 300.0)                      # 46 x 35 blocks of 8 x 8 cells: two radix passes, so the run keeps its table
    pos, rad = gpe.scenes.uniform_cloud(N, world, seed=11)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    st.update(DT, resort=True)                  # the first step sorts and re-sorts: not what is counted below
    st.ctx.sync()
    return st


def _sampled(every, steps):
    return steps if every == 1 else (steps + every - 1) // every


def _check(st, every, steps, L):
    info = st.ctx.pipeline_info()
    assert info["pipeline"] == L.PIPELINE_NATIVE and info["compat_steps"] == 0, info
    passes = info["sort_passes"]
    sampled = _sampled(every, steps)
    timings = st.ctx.timings()
    print("profiling %d, %d steps, %d passes: %s" % (every, steps, passes, timings))
    assert set(timings) == NAMES
    for name, (total_ms, calls) in timings.items():
        assert calls == sampled * (passes if name == "sort/onesweep" else 1), (name, calls, sampled, passes)
        assert total_ms >= 0.0
    trace = st.ctx.trace()
    per_step = len(TOP_LEVEL) + passes
    assert len(trace) == sampled * per_step
    tol = _tolerance(trace)
    last_end = -1.0
    for s in range(sampled):
        group = trace[s * per_step:(s + 1) * per_step]
        assert sorted(n for n, _, _ in group) == sorted(TOP_LEVEL + ["sort/onesweep"] * passes)
        for name, start, dur in group:
            assert dur >= 0.0 and start >= 0.0, (name, start, dur)
        top = {n: (t0, d) for n, t0, d in group if n in TOP_LEVEL}
        # top-level scopes: in the order the step enqueues them, none reaching into the next, none into the next step
        for name in TOP_LEVEL:
            t0, d = top[name]
            assert t0 >= last_end - tol, (s, name, t0, last_end)
            last_end = t0 + d
        # nested scopes: inside their parent, one after the other
        p0, pd = top["native/sort"]
        inner_end = p0
        for name, t0, d in group:
            if name in NESTED:
                assert t0 >= inner_end - tol and t0 + d <= p0 + pd + tol, (s, name, t0, d, p0, pd)
                inner_end = t0 + d


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_scopes_read_as_before_with_shared_boundaries(gpe, every):
    L = gpe._lib
    st = _state(gpe)
    st.ctx.set_profiling(every)
    st.ctx.reset_timings()
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    _check(st, every, STEPS, L)
    st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_reset_and_switching_in_the_middle_of_a_run(gpe, every):
    """gpe_reset_timings between two runs, profiling off and on again with scopes pending, and a context closed with
    scopes pending: the counts afterwards are those of the steps since, and the results are the unprofiled run's."""
    L = gpe._lib
    st, plain = _state(gpe), _state(gpe)
    st.ctx.set_profiling(every)
    st.run(DT, 5, resort_every=0, resort_first=False)           # pending when the reset comes
    st.ctx.reset_timings()
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    _check(st, every, STEPS, L)
    st.ctx.set_profiling(0)                                     # (resolved by _check: nothing pending)
    st.run(DT, 4, resort_every=0, resort_first=False)
    assert {k: v[1] for k, v in st.ctx.timings().items()} == \
        {k: _sampled(every, STEPS) * (st.ctx.pipeline_info()["sort_passes"] if k == "sort/onesweep" else 1) for k in NAMES}
    st.ctx.set_profiling(every)
    st.run(DT, 3, resort_every=0, resort_first=False)           # pending when profiling goes off
    st.ctx.set_profiling(0)
    st.run(DT, 2, resort_every=0, resort_first=False)
    st.ctx.set_profiling(every)
    st.ctx.reset_timings()
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    _check(st, every, STEPS, L)
    st.run(DT, 2, resort_every=0, resort_first=False)           # pending when the context goes
    plain.run(DT, 5 + STEPS + 4 + 3 + 2 + STEPS + 2, resort_every=0, resort_first=False)
    assert np.array_equal(st.positions(), plain.positions())
    assert np.array_equal(st.previous_positions(), plain.previous_positions())
    st.ctx.set_profiling(every)
    st.run(DT, 2, resort_every=0, resort_first=False)
    st.close()
    plain.close()
