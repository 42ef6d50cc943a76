"""CPU: the plans of tests/_interactive_sequences.py run on the oracle model alone.  Every seed's sequence must reach what
tests/test_gpu_api_sequences.py::test_random_interactive_sequences_match_the_oracle relies on having reached -- these
are conditions on the inputs, checked here before any GPU time is spent -- and the plan is a function of the seed.  The
same for plan_observed / ObservedSequence and test_random_observed_sequences_match_the_oracle: the observed plan is the
plan with operations inserted, every pin of Coverage.check_observed is met in every seed, and over the seeds every k, m,
every, frames, field combination and capacity class of the recorders and the late queries is used."""
import zlib

import numpy as np
import pytest

import _interactive_sequences as seq


@pytest.fixture(scope="module")
def coverage(oracle):
    """The coverage counters of every seed's sequence, each run once on the model alone."""
    out = {}
    for seed in seq.SEEDS:
        s = seq.Sequence(seq.plan(seed), oracle)
        try:
            s.run()
        finally:
            s.close()
        out[seed] = (s.cov, len(s.model), s.log)
    return out


@pytest.mark.parametrize("seed", seq.SEEDS)
def test_the_plan_is_a_function_of_the_seed(seed):
    a, b = seq.plan(seed), seq.plan(seed)
    assert a.ops == b.ops and np.array_equal(a.pos, b.pos) and np.array_equal(a.rad, b.rad) and a.world == b.world
    n = len(a.rad)
    assert 1500 <= n <= 6000 and 90 <= a.world[0] <= 160 and 60 <= a.world[1] <= 110 and (a.rad > 0).all()
    assert 40 <= len(a.ops) <= 70, len(a.ops)
    # every block of the plan is there, in one piece
    for block in seq.BLOCKS:
        assert any(a.ops[i:i + len(block)] == block for i in range(len(a.ops))), block
    # the add that must grow the buffers is the first add of any kind
    first = next(i for i, op in enumerate(a.ops) if op in seq.ADDS)
    assert a.ops[first:first + 3] == ["add", "contacts", "clusters"]


# crc32 of each plan (operations, world, flags, positions, radii) and of the log its sequence writes on the model alone,
# taken before plan_observed was added: the plan and every draw of the existing operations have stayed where they were
PLAN_CRC = {1: 3770567184, 2: 364433860, 3: 3487877970, 4: 2115924798, 5: 4285430723, 6: 3316321399}
LOG_CRC = {1: 3213627477, 2: 1565545173, 3: 358587280, 4: 3659826909, 5: 2990961214, 6: 2668639786}


@pytest.mark.parametrize("seed", seq.SEEDS)
def test_the_plan_and_the_draws_of_its_operations_have_not_moved(coverage, seed):
    p = seq.plan(seed)
    text = ("\n".join(p.ops) + repr(p.world) + repr(p.spawn_flags)).encode()
    assert zlib.crc32(text + p.pos.tobytes() + p.rad.tobytes()) == PLAN_CRC[seed]
    assert zlib.crc32("\n".join(coverage[seed][2]).encode()) == LOG_CRC[seed]


def test_all_eight_flag_combinations_over_the_seeds():
    used = {f for seed in seq.SEEDS for f in seq.plan(seed).spawn_flags}
    assert len(used) == 8
    for seed in seq.SEEDS:
        flags = seq.plan(seed).spawn_flags
        assert (1, 0, 0) in flags and (0, 1, 0) in flags       # candidates block candidates; the world test rejects


@pytest.mark.parametrize("seed", seq.SEEDS)
def test_every_sequence_reaches_what_the_gpu_test_relies_on(coverage, seed):
    cov, n, log = coverage[seed]
    print("seed %d: %d ops, %d particles at the end, coverage %s" % (seed, len(seq.plan(seed).ops), n, dict(cov)))
    cov.check(seq.plan(seed).spawn_flags)
    # every add_free call of the plan used its own flags, and the kicks all three ops
    assert all(cov["kick_op_%d" % op] > 0 for op in (0, 1, 2)), dict(cov)
    assert sum(1 for k in cov if k.startswith("edit_fields_")) >= 4, dict(cov)


def test_the_field_subsets_and_flags_are_all_used_over_the_seeds(coverage):
    fields = {k for cov, _, _ in coverage.values() for k in cov if k.startswith("edit_fields_")}
    assert fields >= {"edit_fields_" + "_".join(f) for f in seq.FIELD_SUBSETS}, fields


# ---- the observed sequences ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def observed(oracle):
    """The coverage counters of every seed's observed sequence, each run once on the model alone."""
    out = {}
    for seed in seq.SEEDS:
        s = seq.ObservedSequence(seq.plan_observed(seed), oracle)
        try:
            s.run()
        finally:
            s.close()
        out[seed] = (s.cov, len(s.model), s.log)
    return out


@pytest.mark.parametrize("seed", seq.SEEDS)
def test_the_observed_plan_is_the_plan_with_operations_inserted(seed):
    a, b, base = seq.plan_observed(seed), seq.plan_observed(seed), seq.plan(seed)
    assert a.ops == b.ops
    assert [op for op in a.ops if op not in seq.OBSERVING] == base.ops
    assert not set(base.ops) & seq.OBSERVING and set(a.ops) - set(base.ops) == set(seq.OBSERVING)
    assert np.array_equal(a.pos, base.pos) and np.array_equal(a.rad, base.rad) and a.world == base.world
    assert a.spawn_flags == base.spawn_flags
    # both recorders are armed before anything happens, hence before the first add; a frame and a read follow every
    # operation that can leave the slot table stale
    assert a.ops[:2] == ["tracers_begin", "monitor_begin"]
    for i, op in enumerate(a.ops):
        if op in seq.STALE_MAKERS:
            assert a.ops[i + 1] in ("tracers_sample", "obs_step") and a.ops[i + 2] == "tracers_read", (i, a.ops[i:i + 3])


@pytest.mark.parametrize("seed", seq.SEEDS)
def test_every_observed_sequence_reaches_what_the_gpu_test_relies_on(observed, seed):
    cov, n, log = observed[seed]
    print("seed %d: %d ops, %d particles at the end, coverage %s" % (seed, len(seq.plan_observed(seed).ops), n, dict(cov)))
    cov.check(seq.plan(seed).spawn_flags)
    cov.check_observed()


def test_every_size_and_class_of_the_observers_is_used_over_the_seeds(observed):
    used = set()
    for cov, _, _ in observed.values():
        used |= {k for k, v in cov.items() if v > 0}
    need = (["tracer_k_%d" % k for k in seq.TRACER_K] + ["tracer_fields_%d" % f for f in seq.TRACER_FIELDS]
            + ["%s_every_%d" % (r, e) for r in ("tracer", "monitor") for e in seq.EVERY]
            + ["%s_frames_%d" % (r, f) for r in ("tracer", "monitor") for f in seq.FRAMES]
            + ["%s_read_%s" % (r, c) for r in ("tracer", "monitor") for c in seq.CAPACITY_CLASSES]
            + ["%s_read_consume_%d" % (r, c) for r in ("tracer", "monitor") for c in (0, 1)]
            + ["monitor_rest_speed_zero", "monitor_rest_speed_typical"]
            + ["ray_k_%d" % k for k in seq.RAY_K] + ["nearest_k_%d" % k for k in seq.NEAREST_K]
            + ["nearest_m_%d" % m for m in seq.NEAREST_M] + ["nearest_max_distance_finite", "nearest_max_distance_infinite"]
            + ["segment_capacity_" + c for c in seq.CAPACITY_CLASSES])
    assert not [k for k in need if k not in used], sorted(k for k in need if k not in used)
