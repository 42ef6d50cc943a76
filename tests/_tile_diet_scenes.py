"""Scenes for the dense tile's wave and round edges (tests/test_gpu_tile_diet.py, checked on the CPU by
tests/test_tile_diet_scenes_cpu.py), and the numpy model of what a 32 x 32 direct-slot tile counts.

Radius 0.5, cells of 1.1, a 200 x 200 world (182 x 182 cells, 6 x 6 tiles).  Tile (tx, ty) owns the cells 32 t .. 32 t + 31;
it looks up the 8 x 8-cell blocks of the cells 32 t - 8 .. 32 t + 39 (P particles) and keeps those whose home cell lies in
its 41 x 37-cell window, cells 32 tx - 5 .. 32 tx + 35 by 32 ty - 3 .. 32 ty + 33 (PS particles).  It stages at most 1536
looked-up and 928 kept particles; beyond either it hands itself on.  Memberships are filed for the 40 x 36 zone cells from
(32 tx - 4, 32 ty - 2) on; the 2 x 2 colour groups are numbered row by row from there, 20 a row, 360 in all (a 32 x 16 half:
40 x 20 zone cells, 200 groups).
"""
import numpy as np

F32 = np.float32
RADIUS = 0.5
CELL = F32(F32(RADIUS) * F32(2.2))
WORLD = (200.0, 200.0)
TILE = 32
HALO = 8
WIN_L, WIN_R, WIN_D, WIN_U = 5, 4, 3, 2          # window cells beyond the tile's own, per side
RAW_CAP, KEPT_CAP = 1536, 928
CELL_MAX = 64                                    # members of one cell the dense launch resolves
LATTICE = 1.05


def cells_of(pos):
    """Home cells, floor(p / cell) in binary32 as the engine forms them."""
    c = np.floor(np.asarray(pos, F32) / CELL)
    return c.astype(np.int64)


def tile_counts(pos, tx, ty):
    """(P, PS) of tile (tx, ty): particles in its looked-up blocks, and those of them inside its cell window."""
    c = cells_of(pos)
    x0, y0 = TILE * tx, TILE * ty
    looked = ((c[:, 0] >= x0 - HALO) & (c[:, 0] < x0 + TILE + HALO) & (c[:, 1] >= y0 - HALO) & (c[:, 1] < y0 + TILE + HALO))
    kept = (looked & (c[:, 0] >= x0 - WIN_L) & (c[:, 0] < x0 + TILE + WIN_R) & (c[:, 1] >= y0 - WIN_D) & (c[:, 1] < y0 + TILE + WIN_U))
    return int(looked.sum()), int(kept.sum())


def all_tile_counts(pos):
    n = int(np.ceil(np.floor(F32(WORLD[0]) / CELL) / TILE))
    return {(tx, ty): tile_counts(pos, tx, ty) for ty in range(n) for tx in range(n)}


def cell_members(pos):
    """{(cx, cy): home-cell population}."""
    c = cells_of(pos)
    keys, counts = np.unique(c, axis=0, return_counts=True)
    return {(int(k[0]), int(k[1])): int(v) for k, v in zip(keys, counts)}


def overlapping_pairs(pos):
    """Index pairs closer than 2 r (brute force: scenes of a few thousand particles)."""
    p = np.asarray(pos, np.float64)
    out = []
    order = np.argsort(p[:, 0])
    xs = p[order, 0]
    for a, i in enumerate(order):
        b = a + 1
        while b < len(order) and xs[b] - xs[a] < 2 * RADIUS:
            j = order[b]
            if np.hypot(*(p[i] - p[j])) < 2 * RADIUS:
                out.append((int(i), int(j)))
            b += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. round and wave edges of the gather and the write-back: exactly P looked up, exactly PS kept, in tile (1, 1)

P_CASES = [(p, min(2 * p // 3, 800)) for p in (512, 513, 576, 577, 1024, 1025, 1536, 1537)]
PS_CASES = [(ps + 256, ps) for ps in (511, 512, 513, 576, 577, 928, 929)]
DEEP_PAIRS = 12


def hands_on(p, ps):
    return p > RAW_CAP or ps > KEPT_CAP


def _lattice():
    """Lattice points of the looked-up region of tile (1, 1), none within 1 % of a cell of a cell border."""
    lo, hi = float(CELL) * (TILE - HALO), float(CELL) * (2 * TILE + HALO)
    k = np.arange(int(lo / LATTICE), int(hi / LATTICE) + 2)
    gx, gy = np.meshgrid(k, k, indexing="xy")
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64) * LATTICE + 0.3
    frac = pts / float(CELL) - np.floor(pts / float(CELL))
    ok = ((frac > 0.01) & (frac < 0.99)).all(1)
    return pts[ok].astype(F32)


def counted_tile(p, ps):
    """n = p particles: a lattice of spacing 1.05 (nothing touches, nothing moves without gravity) with ps points in the
    window of tile (1, 1) and p - ps in the ring of its looked-up region around the window -- DEEP_PAIRS of the ps are
    partners half a radius beside a lattice point at the tile's centre, so that the colour passes have work."""
    pts = _lattice()
    c = cells_of(pts)
    x0 = y0 = TILE
    looked = (c >= TILE - HALO).all(1) & (c < 2 * TILE + HALO).all(1)
    inwin = (looked & (c[:, 0] >= x0 - WIN_L) & (c[:, 0] < x0 + TILE + WIN_R) & (c[:, 1] >= y0 - WIN_D) & (c[:, 1] < y0 + TILE + WIN_U))
    centre = np.array([1.5 * TILE * float(CELL)] * 2)
    win = pts[inwin]
    win = win[np.argsort(((win.astype(np.float64) - centre) ** 2).sum(1), kind="stable")]
    ring = pts[looked & ~inwin]
    assert len(win) >= ps - DEEP_PAIRS and len(ring) >= p - ps, (len(win), len(ring))
    kept = win[:ps - DEEP_PAIRS]
    # the partners: beside lattice points at most 6.5 units from the centre, 3 lattice steps apart
    d = kept.astype(np.float64) - centre
    ij = np.rint((kept.astype(np.float64) - 0.3) / LATTICE).astype(np.int64)
    deep = kept[(np.abs(d) < 6.5).all(1) & (ij % 3 == 0).all(1)][:DEEP_PAIRS]
    assert len(deep) == DEEP_PAIRS, len(deep)
    partners = (deep + np.array([0.5, 0.02], F32)).astype(F32)
    pos = np.concatenate([kept, partners, ring[:p - ps]]).astype(F32)
    return pos, np.full(len(pos), RADIUS, F32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. P4's last populated wave: pairs in the first and last colour groups of a tile, and in its last group column


def _cloud(gpe, seed):
    n = int(gpe.scenes.REF_DENSITY * WORLD[0] * WORLD[1])
    pos, _ = gpe.scenes.uniform_cloud(n, WORLD, seed=seed, radius=RADIUS)
    return pos


def edge_group_cells(tx, ty, rows=TILE):
    """Cells of the first two and the last two rows of colour groups (groups 0-39 and the last 40) and of the last group
    column of the tile whose own cells start at (32 tx, ty) and are `rows` high (32, or 16 for a half); every fourth, and the rows' last."""
    x0, y0 = TILE * tx, ty
    zx0, zy0, zw, zh = x0 - 4, y0 - 2, TILE + 8, rows + 4
    cells = [(x, y) for y in list(range(zy0, zy0 + 4)) + list(range(zy0 + zh - 4, zy0 + zh)) for x in list(range(zx0, zx0 + zw, 4)) + [zx0 + zw - 1]]
    cells += [(x, y) for x in (zx0 + zw - 2, zx0 + zw - 1) for y in range(zy0 + 5, zy0 + zh - 4, 4)]
    return cells


def pairs_in(cells, gap=0.6):
    c = (np.array(sorted(set(cells)), np.float64) + 0.5) * float(CELL)
    return np.concatenate([c - [gap / 2, 0.0], c + [gap / 2, 0.0]]).astype(F32)


EDGE_TILES = [(1, 1), (3, 2)]
PATCH_ORIGIN, PATCH_TILES = (float(CELL) * TILE, float(CELL) * TILE), 2


def edge_groups(gpe, halves=False, seed=17):
    """The bench density with pairs in the edge groups of the tiles EDGE_TILES.  halves: a patch of 2 x 2 tiles (tiles (1, 1)
    to (2, 2)) at 1.9 x the density on top -- those tiles keep more than 928 and are redone as 32 x 16 halves -- with pairs
    in the edge groups of every half of the patch as well."""
    parts = [_cloud(gpe, seed)]
    cells = []
    for tx, ty in EDGE_TILES:
        cells += edge_group_cells(tx, TILE * ty)
    if halves:
        rng = np.random.default_rng(seed + 1)
        side = F32(PATCH_TILES * TILE * float(CELL))
        extra = int(0.9 * gpe.scenes.REF_DENSITY * float(side) ** 2)
        parts.append((np.array(PATCH_ORIGIN, F32) + rng.random((extra, 2), dtype=F32) * side).astype(F32))
        for tx in (1, 2):
            for hy in (2, 3, 4, 5):
                cells += edge_group_cells(tx, 16 * hy, rows=16)
    parts.append(pairs_in(cells))
    pos = np.concatenate(parts).astype(F32)
    return pos, np.full(len(pos), RADIUS, F32)


# ---------------------------------------------------------------------------------------------------------------------
# 3. word counters: clumps in one cell

# (cell, members): two tiles' worth of sizes around the six member slots and the 64 a wave resolves; the last two sit in the
# zone cells zc (even) and zc + 1 of tile (2, 3) -- one packed counter word, two counter words
CLUMPS = [((40, 40), 6), ((46, 40), 7), ((80, 44), 63), ((110, 80), 64), ((70, 110), 7), ((71, 110), 6)]
CLUMP_OVER = ((140, 140), 65)
CLUMP_REACH = 0.04


def clumps(gpe, over=False, seed=29):
    """Clumps within 0.04 of a cell's centre -- no member reaches a neighbouring cell -- in the bench-density cloud, which
    is cleared from the 5 x 5 cells around each: a clump's cell holds the clump and nothing else.  over: with the clump
    of 65, which the dense launch hands on."""
    rng = np.random.default_rng(seed + 1)
    pos = _cloud(gpe, seed)
    which = CLUMPS + ([CLUMP_OVER] if over else [])
    c = cells_of(pos)
    clear = np.zeros(len(pos), bool)
    for (cx, cy), _ in which:
        clear |= (np.abs(c[:, 0] - cx) <= 2) & (np.abs(c[:, 1] - cy) <= 2)
    parts = [pos[~clear]]
    for (cx, cy), k in which:
        centre = (np.array([cx, cy], np.float64) + 0.5) * float(CELL)
        off = (rng.random((k, 2)) - 0.5) * (2 * CLUMP_REACH / np.sqrt(2.0)) * 0.98
        parts.append((centre + off).astype(F32))
    pos = np.concatenate(parts).astype(F32)
    return pos, np.full(len(pos), RADIUS, F32)
