"""CPU: the sharded layout has two homes -- sharded.Decomposition / sharded.quantile_cuts (Python; the torch path) and
gpe_shard_layout_build / _owner_of / gpe_shard_quantile_cuts (C, no GPU needed; the local group and
gpe_shard_run_scheduled).  They must agree, and each must hold what its definition says."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import _shard_scenes as S


@pytest.fixture(scope="module")
def homes(gpe):
    gpe.build()
    return importlib.import_module("gpu-physics-engine_amd.sharded"), importlib.import_module("gpu-physics-engine_amd.local_group"), gpe._lib


def _random_cuts(rng, parts, blocks):
    return [0] + sorted(rng.choice(np.arange(1, blocks), size=parts - 1, replace=False).tolist()) + [blocks]


def _cases():
    """(world, cell size, ws, grid, xcuts, ycuts): random ones, and worlds whose block count over the grid is an odd
    multiple of one half somewhere (round against nearbyint)."""
    rng = np.random.default_rng(0x1A70)
    out = []
    for k in range(400):
        ws = int(rng.integers(1, 27))
        for grid in S.factorisations(ws) if k % 8 == 0 else [S.factorisations(ws)[int(rng.integers(len(S.factorisations(ws))))], None]:
            cell = np.float32(rng.choice([1.1, 0.55, 6.6, 2.2 * (0.3 + 2.2 * rng.random())]))
            px, py = grid if grid is not None else (None, None)
            bx, by = int(rng.integers(px or 1, 70)), int(rng.integers(py or 1, 70))
            world = (float(np.float32((bx * 8 - rng.integers(0, 8) - rng.random()) * float(cell))),
                     float(np.float32((by * 8 - rng.integers(0, 8) - rng.random()) * float(cell))))
            out.append((world, cell, ws, grid, None, None))
    for px, py in ((2, 2), (4, 1), (1, 4), (4, 6), (8, 2), (6, 4), (12, 2)):            # i * blocks / parts ends in .5
        for bx, by in ((px + px // 2, py + py // 2), (5 * px // 2, 7 * py // 2), (9 * px // 2, 3 * py // 2)):
            if bx >= px and by >= py:
                out.append((((bx * 8 - 0.5) * 1.1, (by * 8 - 0.5) * 1.1), np.float32(1.1), px * py, (px, py), None, None))
    return out


def _both(homes, world, cell, ws, grid, xcuts, ycuts):
    """(Decomposition or the ValueError's text, layout or the GpeError)."""
    sharded, lg, L = homes
    try:
        dec = sharded.Decomposition(world, cell, ws, grid=grid, xcuts=xcuts, ycuts=ycuts)
    except ValueError as e:
        dec = str(e)
    try:
        lay = lg.build_layout(world, cell, ws, grid=grid, xcuts=xcuts, ycuts=ycuts)
    except L.GpeError as e:
        lay = e
    return dec, lay


def test_layout_build_is_the_decomposition(homes):
    sharded, lg, L = homes
    rng = np.random.default_rng(0x1A71)
    built = refused = explicit = 0
    for world, cell, ws, grid, _, _ in _cases():
        dec, lay = _both(homes, world, cell, ws, grid, None, None)
        if isinstance(dec, str):
            assert isinstance(lay, L.GpeError) and lay.status == L.GPE_ERR_INVALID_ARG, (world, cell, ws, grid, dec)
            assert dec.split(" (")[0] in str(lay) or "world too small" in dec and "world too small" in str(lay), (dec, str(lay))
            refused += 1
            continue
        assert not isinstance(lay, L.GpeError), (world, cell, ws, grid, str(lay))
        assert (lay.cells_x, lay.cells_y, lay.blocks_x, lay.blocks_y, lay.px, lay.py) == (dec.gx, dec.gy, dec.bx, dec.by, dec.px, dec.py)
        assert list(lay.xcuts[:dec.px + 1]) == dec.xcuts and list(lay.ycuts[:dec.py + 1]) == dec.ycuts, (world, cell, ws, grid)
        built += 1
        if dec.bx > dec.px and dec.by > dec.py:                       # the same grid with explicit cuts
            xc, yc = _random_cuts(rng, dec.px, dec.bx), _random_cuts(rng, dec.py, dec.by)
            d2, l2 = _both(homes, world, cell, ws, (dec.px, dec.py), xc, yc)
            assert list(l2.xcuts[:dec.px + 1]) == d2.xcuts == xc and list(l2.ycuts[:dec.py + 1]) == d2.ycuts == yc
            explicit += 1
    assert built > 300 and refused > 20 and explicit > 200, (built, refused, explicit)


def _probe_positions(rng, dec, count):
    """Random finite positions: inside, on cuts and cell edges, one ulp either side, negative, beyond the world."""
    cs = dec.cell_size
    w = np.array(dec.world, np.float32)
    p = (rng.random((count, 2), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)) * w
    edges = [(np.array(c, np.float32) * np.float32(8)) * cs for c in (dec.xcuts, dec.ycuts)]
    for ax in (0, 1):
        k = count // 6
        p[:k, ax] = rng.choice(edges[ax], k)                                          # exactly on a cut
        p[k:2 * k, ax] = np.nextafter(rng.choice(edges[ax], k), np.float32(-1e30))    # one ulp below
        p[2 * k:3 * k, ax] = np.nextafter(rng.choice(edges[ax], k), np.float32(1e30))
        cells = rng.integers(0, dec.gx if ax == 0 else dec.gy, k).astype(np.float32) * cs        # on a cell edge
        p[3 * k:4 * k, ax] = cells
        p[4 * k:4 * k + 4, ax] = np.array([-1e30, 1e30, -0.0, 3e38], np.float32)
        rng.shuffle(p[:, ax])
    return np.ascontiguousarray(p.astype(np.float32))


def test_owner_of_agrees_on_finite_positions_and_clamps_the_rest(homes):
    sharded, lg, L = homes
    rng = np.random.default_rng(0x1A72)
    checked = 0
    for world, cell, ws, grid, _, _ in _cases()[::3]:
        dec, lay = _both(homes, world, cell, ws, grid, None, None)
        if isinstance(dec, str):
            continue
        if dec.bx > dec.px and dec.by > dec.py and checked % 2:
            dec, lay = _both(homes, world, cell, ws, (dec.px, dec.py), _random_cuts(rng, dec.px, dec.bx), _random_cuts(rng, dec.py, dec.by))
        p = _probe_positions(rng, dec, 600)
        with np.errstate(over="ignore", invalid="ignore"):
            want = dec.owner_of(p)
        got = lg.owner_of(lay, p).astype(np.int64)
        assert np.array_equal(got, want), (world, cell, ws, grid, p[got != want][:4])
        # NaN and +-inf: the cast of the Python side is undefined there (numpy gives what the platform's conversion gives), so
        # it is not compared; the C side documents its clamp -- NaN and -inf to block 0, +inf to the last block
        odd = np.array([[np.nan, np.nan], [-np.inf, -np.inf], [np.inf, np.inf], [np.nan, np.inf], [np.inf, -np.inf]], np.float32)
        last = ws - 1
        corner = [0, 0, last, int(dec.owner[dec.by - 1, 0]), int(dec.owner[0, dec.bx - 1])]
        assert lg.owner_of(lay, odd).tolist() == corner, (ws, grid)
        checked += 1
    assert checked > 100


def _c_quantile_cuts(L, hist, parts, min_width=2):
    h = np.ascontiguousarray(hist, np.uint64)
    out = (C.c_int32 * (parts + 1))()
    L.check(L.load().gpe_shard_quantile_cuts(h.ctypes.data_as(C.c_void_p), len(h), parts, min_width, out))
    return list(out)


def test_quantile_cuts_agree_and_hold_their_properties(homes):
    sharded, lg, L = homes
    rng = np.random.default_rng(0x1A73)
    seen = collections_counter()
    for k in range(600):
        parts = int(rng.integers(1, 27))
        bins = int(rng.integers(parts, parts * 2 if k % 3 == 0 else 140))
        kind = ("random", "zeros", "one-bin", "sparse", "huge", "steps")[k % 6]
        if kind == "random":
            hist = rng.integers(0, 1000, bins)
        elif kind == "zeros":
            hist = np.zeros(bins, np.int64)
        elif kind == "one-bin":
            hist = np.zeros(bins, np.int64)
            hist[int(rng.integers(bins))] = int(rng.integers(1, 1 << 20))
        elif kind == "sparse":
            hist = rng.integers(0, 1000, bins) * (rng.random(bins) < 0.15)
        elif kind == "huge":
            hist = (1 << 40) - rng.integers(0, 3, bins)                     # sums near 2^46: still exact in a double
        else:
            hist = np.repeat(rng.integers(0, 50, (bins + 3) // 4), 4)[:bins] * 100      # quantiles exactly on bin edges
        min_width = int(rng.choice([1, 2, 2, 2, 3]))
        want = sharded.quantile_cuts(hist, parts, min_width=min_width)
        got = _c_quantile_cuts(L, hist, parts, min_width)
        assert got == want, (kind, parts, bins, min_width, hist.tolist())
        assert got[0] == 0 and got[-1] == bins and all(b > a for a, b in zip(got[:-1], got[1:])), (got, bins)
        if parts * min_width <= bins:
            assert min(np.diff(got)) >= min_width, (got, min_width)
        seen[kind] += 1
        seen["narrow"] += bins < 2 * parts
    assert min(seen.values()) >= 50, seen
    for bad in ((None, 4, 2), (np.ones(4), 4, 0), (np.ones(4), 4, 27), (np.ones(3), 3, 4)):
        h, bins, parts = bad
        out = (C.c_int32 * 32)()
        ptr = np.ascontiguousarray(h, np.uint64).ctypes.data_as(C.c_void_p) if h is not None else None
        assert L.load().gpe_shard_quantile_cuts(ptr, bins, parts, 2, out) == L.GPE_ERR_INVALID_ARG


def collections_counter():
    import collections
    return collections.Counter()


def test_dest_mask_is_its_definition_and_neighbours_are_symmetric(homes):
    """Rank p is named at block b iff p is not b's owner and owns a block within Chebyshev distance 1 of b."""
    sharded, lg, L = homes
    rng = np.random.default_rng(0x1A74)
    for k in range(60):
        ws = int(rng.integers(2, 27))
        px, py = S.factorisations(ws)[int(rng.integers(len(S.factorisations(ws))))]
        bx, by = int(rng.integers(px, px + 14)), int(rng.integers(py, py + 14))
        xc = _random_cuts(rng, px, bx) if k % 2 else None
        yc = _random_cuts(rng, py, by) if k % 2 else None
        dec = sharded.Decomposition(((bx * 8 - 0.5) * 1.1, (by * 8 - 0.5) * 1.1), np.float32(1.1), ws, grid=(px, py), xcuts=xc, ycuts=yc)
        want = np.zeros((by, bx), np.uint32)
        for y, x in itertools.product(range(by), range(bx)):
            near = {int(dec.owner[yy, xx]) for yy in range(max(0, y - 1), min(by, y + 2)) for xx in range(max(0, x - 1), min(bx, x + 2))}
            want[y, x] = sum(1 << p for p in near if p != int(dec.owner[y, x]))
        assert np.array_equal(dec.dest_mask, want), (ws, (px, py), xc, yc)
        nb = [dec.neighbours(r) for r in range(ws)]
        for r in range(ws):
            x0, y0, x1, y1 = dec.rect_blocks(r)
            assert (dec.owner[y0:y1, x0:x1] == r).all() and (dec.owner == r).sum() == (x1 - x0) * (y1 - y0)
            assert r not in nb[r] and len(nb[r]) <= 8
            for p in nb[r]:
                assert r in nb[p], (r, p, xc, yc)
                assert dec.border_blocks(r, p) > 0 and dec.border_blocks(p, r) > 0


def test_layout_build_refusals(homes):
    sharded, lg, L = homes
    lib = L.load()
    lay = L.GpeShardLayout()

    def refused(text, world, cell, ws, px, py, xcuts=None, ycuts=None):
        xc = (C.c_int32 * len(xcuts))(*xcuts) if xcuts is not None else None
        yc = (C.c_int32 * len(ycuts))(*ycuts) if ycuts is not None else None
        status = lib.gpe_shard_layout_build(world[0], world[1], cell, ws, px, py, xc, yc, C.byref(lay))
        assert status == L.GPE_ERR_INVALID_ARG, (text, status)
        assert text in lib.gpe_last_error(None).decode(), (text, lib.gpe_last_error(None))
    big = (500.0, 400.0)
    refused("1 .. 26 ranks", big, 1.1, 0, 0, 0)
    refused("1 .. 26 ranks", big, 1.1, 27, 0, 0)
    refused("process grid does not match world_size", big, 1.1, 6, 4, 2)
    refused("process grid does not match world_size", big, 1.1, 6, 0, 6)
    refused("world too small for this many ranks", (30.0, 400.0), 1.1, 8, 8, 1)        # 4 block columns for 8 ranks
    refused("world too small for this many ranks", (400.0, 8.0), 1.1, 4, 2, 2)         # 1 block row for 2
    refused("more than 65000 cells along an axis", (72000.0, 400.0), 1.1, 2, 0, 0)
    refused("world and cell size must be positive", big, 0.0, 2, 0, 0)
    refused("world and cell size must be positive", (-1.0, 400.0), 1.1, 2, 0, 0)
    bx = int(np.floor(np.float32(500.0) / np.float32(1.1))) // 8 + 1
    for cuts in ([0, 10, 10, bx], [0, 12, 7, bx], [1, 10, 20, bx], [0, 10, 20, bx - 1], [0, 10, 20, bx + 1], [0, -3, 20, bx]):
        refused("cuts must rise from 0 to the block count", big, 1.1, 3, 3, 1, xcuts=cuts)
    assert lib.gpe_shard_layout_build(500.0, 400.0, 1.1, 3, 3, 1, (C.c_int32 * 4)(0, 10, 20, bx), None, C.byref(lay)) == L.GPE_OK


def test_a_layout_filled_in_by_hand_must_have_rising_cuts(homes):
    """gpe_shard_layout is a plain struct: gpe_shard_layout_owner_of and gpe_shard_setup index their tables by its cuts, so
    they refuse one whose cuts do not rise (a cut beyond the block count was a write behind the host tables)."""
    sharded, lg, L = homes
    lay = lg.build_layout((500.0, 400.0), 1.1, 6, grid=(3, 2))
    pos = np.zeros((4, 2), np.float32)
    assert lg.owner_of(lay, pos).tolist() == [0, 0, 0, 0]
    for field, at, value in (("xcuts", 1, 0), ("xcuts", 1, lay.blocks_x), ("xcuts", 2, 3), ("ycuts", 1, lay.blocks_y + 9), ("xcuts", 1, 1 << 20)):
        bad = L.GpeShardLayout.from_buffer_copy(lay)
        getattr(bad, field)[at] = value
        with pytest.raises(L.GpeError, match="gpe_shard_layout_owner_of: bad argument") as e:
            lg.owner_of(bad, pos)
        assert e.value.status == L.GPE_ERR_INVALID_ARG
