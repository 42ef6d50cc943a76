"""GPU (-m gpu): the dense tile where its waves and rounds end.

The direct-slot tile skips, wave by wave, what a wave has no work in: a slot of the gather beyond the looked-up ids, a
round of the own-particle fetch and write-back beyond the kept slots, the walk over the colour groups beyond the last
group.  Its uniform layouts count the members of a cell in a word of its own.  The scenes put the counts on either side
of every such edge (tests/_tile_diet_scenes.py; tests/test_tile_diet_scenes_cpu.py checks the counts on the CPU) and
every case is compared bit for bit with the oracle, on the uniform kernels and under GPE_FLAG_GENERAL_RADII (packed
counters), on steps that keep the block table: the roster is then the gather's source.
"""
import numpy as np
import pytest

from tests import _tile_diet_scenes as sc

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    ba, bb = _bits(a), _bits(b)
    if not np.array_equal(ba, bb):
        bad = np.flatnonzero((ba != bb).reshape(len(ba), -1).any(1))
        pytest.fail("%s: %d particles differ, first %s: %s / %s" % (what, len(bad), bad[:4], a[bad[:2]], b[bad[:2]]))


def _run(gpe, oracle, pos, rad, steps, handed_on, what, counted_steps=None):
    """Uniform and general kernels against the oracle, every step; native, table kept, tiles handed on or not -- on the
    first `counted_steps` steps (default: all), those on which the scene has the counts it was built with."""
    L = gpe._lib
    sts = {"uniform": gpe.State(pos, rad, world=sc.WORLD), "general": gpe.State(pos, rad, world=sc.WORLD, flags=L.FLAG_GENERAL_RADII)}
    sim = oracle.Sim(pos, rad, oracle.default_params(sc.WORLD[0], sc.WORLD[1], sc.RADIUS))
    over = {k: [] for k in sts}
    for s in range(steps):
        sim.step(DT, resort=(s == 0))
        want_p, want_q = sim.pos, sim.prev
        for k, st in sts.items():
            st.update(DT, resort=(s == 0))
            _same_bits(st.positions(), want_p, "%s: %s vs oracle, pos, step %d" % (what, k, s))
            _same_bits(st.previous_positions(), want_q, "%s: %s vs oracle, prev, step %d" % (what, k, s))
            st.ctx.sync()
            over[k].append(st.ctx.pipeline_info()["overflow_tiles"])
    for k, st in sts.items():
        st.ctx.sync()
        info = st.ctx.pipeline_info()
        print(what, k, "overflow tiles per step", over[k], info)
        assert info["uniform_radius"] == (1 if k == "uniform" else 0), info
        assert info["pipeline"] == L.PIPELINE_NATIVE and info["native_steps"] == steps and info["compat_steps"] == 0, info
        assert info["sort_passes"] == 2 and info["native_sorts"] < steps, info      # the table was kept: the roster path
        # (the statistics lag a step: what is read behind step s + 1 is the count of step s)
        counted = over[k] if counted_steps is None else over[k][1:1 + counted_steps]
        if handed_on:
            assert max(counted) > 0, (k, over[k])
        else:
            assert max(counted) == 0, (k, over[k])
        st.close()
    sim.close()


@pytest.mark.parametrize("p,ps", sc.P_CASES + sc.PS_CASES)
def test_round_and_wave_edges_of_the_gather_and_the_write_back(gpe, oracle, p, ps):
    """Tile (1, 1) looks up exactly p particles and keeps exactly ps, on every step: a sort and three kept tables."""
    pos, rad = sc.counted_tile(p, ps)
    assert sc.tile_counts(pos, 1, 1) == (p, ps)
    _run(gpe, oracle, pos, rad, 4, sc.hands_on(p, ps), "P %d PS %d" % (p, ps))


@pytest.mark.parametrize("halves", [False, True])
def test_the_last_populated_wave_of_the_colour_group_walk(gpe, oracle, halves):
    """Pairs in the groups 0-39 and 320-359 of the 360 and in the last group column; with the patch at 1.9 x the density
    the 32 x 16 halves take those tiles, 200 groups each."""
    pos, rad = sc.edge_groups(gpe, halves=halves)
    _run(gpe, oracle, pos, rad, 20, halves, "edge groups%s" % (", halves" if halves else ""))


@pytest.mark.parametrize("over", [False, True])
def test_cell_counters_at_the_member_slots_and_at_a_wave(gpe, oracle, over):
    """Clumps of 6, 7, 63 and 64 in one cell, 7 and 6 in two cells that share a packed counter word: resolved by the dense
    launch; a clump of 65 is handed on.  The clumps are whole on the first step alone -- the step resolves them, and what
    64 particles pushed apart over a few cells file as phantom members may well run a side list over later: there the
    bits are compared and the tiles are free to go either way."""
    pos, rad = sc.clumps(gpe, over=over)
    _run(gpe, oracle, pos, rad, 4, over, "clumps%s" % (" and 65" if over else ""), counted_steps=1)
