"""CPU: the scenes of tests/test_gpu_tile_diet.py have the counts the GPU cases rely on, and the oracle runs them.

Built with the functions the GPU cases use (tests/_tile_diet_scenes.py); P and PS per tile and the members per cell are
counted in numpy.  A scene that lost its counts fails here, before any GPU time is spent on it.
"""
import numpy as np
import pytest

from tests import _tile_diet_scenes as sc

DT = 1.0 / 60.0


def _oracle_steps(oracle, pos, rad, steps):
    sim = oracle.Sim(pos, rad, oracle.default_params(sc.WORLD[0], sc.WORLD[1], sc.RADIUS))
    for s in range(steps):
        sim.step(DT, resort=(s == 0))
    out = sim.pos.copy()
    sim.close()
    assert np.isfinite(out).all()
    return out


@pytest.mark.parametrize("p,ps", sc.P_CASES + sc.PS_CASES)
def test_counted_tile_has_its_counts_and_keeps_them(oracle, p, ps):
    pos, rad = sc.counted_tile(p, ps)
    assert len(pos) == p and len(np.unique(pos, axis=0)) == p
    counts = sc.all_tile_counts(pos)
    assert counts[(1, 1)] == (p, ps), counts[(1, 1)]
    for t, (tp, tps) in counts.items():
        if t != (1, 1):
            # every other tile's region holds a corner or a side of the lattice: sparser, and far from any capacity
            assert tp < p and tps <= 0.6 * ps and tp <= 0.75 * sc.RAW_CAP and tps <= 0.6 * sc.KEPT_CAP, (t, tp, tps)
    # which capacity the case crosses
    assert sc.hands_on(p, ps) == ((p, ps) in [(1537, 800), (1185, 929)])
    assert (p > sc.RAW_CAP) != (ps > sc.KEPT_CAP) or not sc.hands_on(p, ps)
    # the overlapping pairs: the dozen, each at least 8 cells inside the window's edges; everything else stands free
    pairs = sc.overlapping_pairs(pos)
    assert len(pairs) >= sc.DEEP_PAIRS
    touched = np.unique(np.array(pairs).ravel())
    c = sc.cells_of(pos[touched])
    assert (c[:, 0] >= 32 - sc.WIN_L + 8).all() and (c[:, 0] <= 63 + sc.WIN_R - 8).all()
    assert (c[:, 1] >= 32 - sc.WIN_D + 8).all() and (c[:, 1] <= 63 + sc.WIN_U - 8).all()
    # four steps of the oracle: the counts hold
    after = _oracle_steps(oracle, pos, rad, 4)
    assert sc.all_tile_counts(after)[(1, 1)] == (p, ps)
    # (the oracle's order is the sort's: compared as sets)
    before = set(map(tuple, pos.view(np.uint32).tolist()))
    moved = np.array([tuple(v) not in before for v in after.view(np.uint32).tolist()])
    assert moved.sum() >= 2 * sc.DEEP_PAIRS, moved.sum()
    # what the pairs pushed is still at least 4 cells inside the window's edges; the ring and the window's rim stand still
    c = sc.cells_of(after[moved])
    assert (c[:, 0] >= 32 - sc.WIN_L + 4).all() and (c[:, 0] <= 63 + sc.WIN_R - 4).all()
    assert (c[:, 1] >= 32 - sc.WIN_D + 4).all() and (c[:, 1] <= 63 + sc.WIN_U - 4).all()


def _groups_hit(pos, tx, y0, rows):
    """Colour groups (row-major, 20 a row) of the tile at cells (32 tx, y0), `rows` high, that hold an overlapping pair
    inside one cell."""
    zx0, zy0 = 32 * tx - 4, y0 - 2
    members = sc.cell_members(pos)
    hit = set()
    for (cx, cy), k in members.items():
        zx, zy = cx - zx0, cy - zy0
        if k >= 2 and 0 <= zx < 40 and 0 <= zy < rows + 4:
            hit.add((zy // 2) * 20 + zx // 2)
    return hit


@pytest.mark.parametrize("halves", [False, True])
def test_edge_groups_scene(gpe, oracle, halves):
    pos, rad = sc.edge_groups(gpe, halves=halves)
    counts = sc.all_tile_counts(pos)
    for tx, ty in sc.EDGE_TILES:
        hit = _groups_hit(pos, tx, 32 * ty, 32)
        # groups of the first wave, of the last populated wave (320-359 lie in lanes 0-39 of wave 5) and of the last column
        assert {0, 19, 20, 39}.issubset(hit) and {320, 339, 340, 359}.issubset(hit), sorted(hit)
        assert any(g % 20 == 19 and 40 <= g < 320 for g in hit)
    patch = [(1, 1), (2, 1), (1, 2), (2, 2)]
    if not halves:
        # no tile near a capacity: none is handed on
        assert max(v[0] for v in counts.values()) <= 0.9 * sc.RAW_CAP, counts
        assert max(v[1] for v in counts.values()) <= 0.95 * sc.KEPT_CAP, counts
    else:
        for t in patch:
            assert counts[t][1] > sc.KEPT_CAP, (t, counts[t])                      # beyond the direct-slot tile: halves
        for tx in (1, 2):
            for hy in (2, 3, 4, 5):
                hit = _groups_hit(pos, tx, 16 * hy, 16)
                assert {0, 39, 160, 199}.issubset(hit), (tx, hy, sorted(hit))      # 200 groups: lanes 0-7 of wave 3 are the last
    _oracle_steps(oracle, pos, rad, 3)


@pytest.mark.parametrize("over", [False, True])
def test_clumps_scene(gpe, oracle, over):
    pos, rad = sc.clumps(gpe, over=over)
    members = sc.cell_members(pos)
    which = sc.CLUMPS + ([sc.CLUMP_OVER] if over else [])
    clump_cells = {c for c, _ in which}
    for (cx, cy), k in which:
        assert members[(cx, cy)] == k
        centre = (np.array([cx, cy], np.float64) + 0.5) * float(sc.CELL)
        inside = (sc.cells_of(pos) == [cx, cy]).all(1)
        assert np.hypot(*(pos[inside].astype(np.float64) - centre).T).max() <= sc.CLUMP_REACH
        assert len(np.unique(pos[inside], axis=0)) == k
        # nothing else within two cells: no phantom member of the clump's cell, and the clump reaches no neighbour
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                if (dx or dy) and (cx + dx, cy + dy) not in clump_cells:
                    assert (cx + dx, cy + dy) not in members
        assert float(sc.CELL) / 2 - sc.CLUMP_REACH > sc.RADIUS
    # every other cell is far below what a wave resolves; 64 members file 58 side-list entries, under the tile's 96
    assert max(k for c, k in members.items() if c not in clump_cells) <= 8
    assert (max(k for _, k in which) > sc.CELL_MAX) == over
    # the pair of neighbouring clumps: zone cells zc (even) and zc + 1 of tile (2, 3)
    (ax, ay), (bx, by) = sc.CLUMPS[-2][0], sc.CLUMPS[-1][0]
    assert ay == by and bx == ax + 1 and (ax - (64 - 4)) % 2 == 0 and 64 <= ax < 95 and 96 <= ay < 128
    # clumps apart, no tile near a capacity
    counts = sc.all_tile_counts(pos)
    assert max(v[0] for v in counts.values()) <= 0.9 * sc.RAW_CAP and max(v[1] for v in counts.values()) <= 0.9 * sc.KEPT_CAP, counts
    _oracle_steps(oracle, pos, rad, 3)
