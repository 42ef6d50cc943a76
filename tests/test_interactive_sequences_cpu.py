"""CPU: the plans of tests/_interactive_sequences.py run on the oracle model alone.  Every seed's sequence must reach what
tests/test_gpu_api_sequences.py::test_random_interactive_sequences_match_the_oracle relies on having reached -- these
are conditions on the inputs, checked here before any GPU time is spent -- and the plan is a function of the seed."""
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
