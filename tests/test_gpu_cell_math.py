"""Cell membership and the Verlet step at the edges of their arithmetic, in the shape of test_gpu_pair_math.py.

Membership (which of its 8 neighbour cells a particle overlaps) exists in two forms: cell_coord / is_obj_in_cell
(gpe_internal.h; k_grid.hip, the oracle's form) and neighbour_overlap_mask (k_cells.h; the NATIVE hash kernel: 3 + 3
shared squared offsets, the clamp one v_med3_f32).  A wrong bit loses no collision, it changes how often a pair is
resolved -- silently, and only for particles within an ulp or so of "radius away from a cell edge or corner".  The
integration (verlet_one, gpe_internal.h) holds a square root, two divisions and two compare-clamps.  Whole scenes almost
never land on the values where such code breaks, so this file drives both directly:

* `reference_cells` / `reference_slots` / `reference_verlet`: orc_build_cell_ids and orc_verlet_integration
  (oracle/gpe_oracle.c) restated in numpy float32, one correctly rounded operation at a time.  Pinned to the C oracle bit
  for bit on every record (CPU).
* tests/hip/cell_probe.hip: runs both membership forms and verlet_one over seeded records of edge classes, 64 records
  per wave; every result must equal the reference bit for bit (GPU).
* The records through the compat kernels (Grid.build_cell_ids, ParticleSystem.update_positions), and edge scenes through
  the NATIVE pipeline (GPE_FLAG_NATIVE_FORCE), one context and a two-context local group, against the oracle (GPU).

Out of contract, where only the oracle's refusal to overrun is pinned: r > cell_size / 2.2 (masks of more than three
bits: the fourth and later phantom cells are dropped) and NaN positions (cell 0, no phantom cells in either form).
"""
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

import tests.test_gpu_pair_math as pm

F = np.float32
WAVE = pm.WAVE
_f, _step, _ulp, _same, _hex, _sign = pm._f, pm._step, pm._ulp, pm._same, pm._hex, pm._sign

PROBE_SRC = os.path.join(pm.ROOT, "tests", "hip", "cell_probe.hip")
PROBE_EXE = os.path.join(pm.ROOT, "tests", "hip", "cell_probe")
PER_CLASS = 64 * 1024
MAX_RS = (0.25, 0.5, 1.0, 3.0)
UNUSED = 0xFFFFFFFF
SCAN = [(y, x) for y in (-1, 0, 1) for x in (-1, 0, 1) if (x, y) != (0, 0)]     # the reference's neighbour scan
DEFAULT_STRENGTH = 150.0                                              # gpe_config_default / orc_params_default
TINY = float(np.ldexp(1.0, -149))


# ---------------------------------------------------------------------------------------------------------------------
# the references


def cell_size_of(max_r):
    """oracle.compute_cell_size, vectorised: max_radius * 2.2f in float32 (pinned to the oracle in a CPU test)."""
    return _f(max_r) * F(2.2)


def _i32_sat(q):
    """WGSL i32(f32): truncate, saturate, NaN -> 0 (f32_to_i32_sat)."""
    q = _f(q).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(q), 0.0, np.clip(q, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)


def reference_coord(p, cs):
    with np.errstate(all="ignore"):
        return _i32_sat(np.floor(_f(p) / _f(cs)))                     # a true division, then floor


def _clamp(x, lo, hi):
    """min(max(x, lo), hi) as two compares (clampf)."""
    m = np.where(x > lo, x, lo)
    return np.where(m < hi, m, hi)


def _wrap_add(c, d):
    return (c.astype(np.int64) + d).astype(np.uint32).view(np.int32)  # the add wraps as u32


def reference_cells(px, py, r, cs):
    """orc_build_cell_ids' home cell and its is_obj_in_cell over the 8 neighbours: (cx, cy, mask8), bit k = the k-th
    neighbour of the scan (y outer, x inner, centre skipped)."""
    px, py, r, cs = _f(px), _f(py), _f(r), _f(cs)
    cx, cy = reference_coord(px, cs), reference_coord(py, cs)
    mask = np.zeros(len(px), np.uint32)
    with np.errstate(all="ignore"):
        sq = r * r
        for k, (y, x) in enumerate(SCAN):
            lo_x, lo_y = _wrap_add(cx, x).astype(np.float32) * cs, _wrap_add(cy, y).astype(np.float32) * cs
            hi_x, hi_y = lo_x + cs, lo_y + cs
            dx, dy = px - _clamp(px, lo_x, hi_x), py - _clamp(py, lo_y, hi_y)
            mask |= ((dx * dx + dy * dy) < sq).astype(np.uint32) << np.uint32(k)
    return cx, cy, mask


def _split_by_bits(n):
    x = n.astype(np.uint32) & np.uint32(0x0000FFFF)
    for s, m in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        x = (x | (x << np.uint32(s))) & np.uint32(m)
    return x


def morton(x, y):
    """oracle.morton_encode, vectorised (pinned to it in a CPU test)."""
    return _split_by_bits(x.view(np.uint32)) | (_split_by_bits(y.view(np.uint32)) << np.uint32(1))


def reference_slots(cx, cy, mask):
    """The four cell ids of a particle: the home cell, then the first three set bits of the mask in scan order, the rest
    0xFFFFFFFF; the fourth and later overlaps are dropped (the oracle refuses to overrun)."""
    n = len(cx)
    out = np.full((n, 4), UNUSED, np.uint32)
    out[:, 0] = morton(cx, cy)
    count = np.zeros(n, np.int64)
    for k, (y, x) in enumerate(SCAN):
        on = ((mask >> np.uint32(k)) & np.uint32(1)).astype(bool)
        count += on
        h = morton(_wrap_add(cx, x), _wrap_add(cy, y))
        for s in (1, 2, 3):
            w = on & (count == s)
            out[w, s] = h[w]
    return out


VERLET_PARAMS = ("dt", "world_w", "world_h", "acc_x", "acc_y", "pressed", "mouse_x", "mouse_y", "strength")


def reference_verlet(cx, cy, qx, qy, r, dt2, world_w, world_h, acc_x, acc_y, pressed, mouse_x, mouse_y, strength):
    """orc_verlet_integration for one particle per element: float32 arrays (pressed: integers) in, (nx, ny) out."""
    a = [_f(v) for v in (cx, cy, qx, qy, r, dt2, world_w, world_h, acc_x, acc_y, mouse_x, mouse_y, strength)]
    cx, cy, qx, qy, r, dt2, world_w, world_h, acc_x, acc_y, mouse_x, mouse_y, strength = a
    with np.errstate(all="ignore"):
        vx, vy = cx - qx, cy - qy
        dx, dy = mouse_x - cx, mouse_y - cy
        ln = np.sqrt(dx * dx + dy * dy)
        on = np.asarray(pressed) == 1                                 # only 1 applies the force
        ax = np.where(on, acc_x + (dx / ln) * strength, acc_x)
        ay = np.where(on, acc_y + (dy / ln) * strength, acc_y)
        nx = (cx + vx) + ax * dt2
        ny = (cy + vy) + ay * dt2
        return _clamp(nx, r, world_w - r), _clamp(ny, r, world_h - r)


# ---------------------------------------------------------------------------------------------------------------------
# cell classes: each returns a dict of float32 arrays px py r cs and int8 arrays tx ty -- the neighbour (offset from the
# home cell) whose bit the placement aims at, (0, 0) where there is none


def _cs_draw(rng, n, max_r=None):
    """(max_r, cell size) per record: the four discrete radii and sixty values drawn from 0.3 to 2.5 (two thirds and
    one third of the records), or one given max_r."""
    if max_r is None:
        pick = rng.integers(0, 6, n)
        mr = np.where(pick < 4, np.array(MAX_RS)[np.minimum(pick, 3)], rng.uniform(0.3, 2.5, 60)[rng.integers(0, 60, n)])
    else:
        mr = np.full(n, max_r)
    mr = _f(mr)
    return mr, cell_size_of(mr)


def _cells(px, py, r, cs, tx=None, ty=None):
    n = len(px)
    z = np.zeros(n, np.int8)
    return dict(px=_f(px).copy(), py=_f(py).copy(), r=_f(np.broadcast_to(r, (n,))).copy(), cs=_f(cs).copy(),
                tx=z if tx is None else np.asarray(tx, np.int8), ty=z if ty is None else np.asarray(ty, np.int8))


def _radius_draw(rng, mr, cs):
    """From max_r down to 0.02 * cs, a quarter exactly max_r."""
    lo = 0.02 * cs.astype(np.float64)
    r = np.exp(rng.uniform(np.log(lo), np.log(mr.astype(np.float64))))
    return _f(np.where(rng.random(len(mr)) < 0.25, mr, r))


def _lo_of(k, cs):
    return _f(k) * cs                                                 # fl(k * cs); k below 2^24 is exact in float32


def _inside(rng, k, cs):
    """A coordinate well inside cell k."""
    return _f((k + rng.uniform(0.3, 0.7, len(k))) * cs.astype(np.float64))


def place_boundary(rng, kx, ky, cs, mr):
    """p within +-4 ulps of fl(k * cs), on x, on y or on both.  For a third of the placements the 9 neighbouring floats
    are scanned for one where fl(p / cs) and the comparisons against fl(k * cs) name different cells."""
    n = len(kx)
    mode = rng.integers(0, 3, n)                                      # 0: x, 1: y, 2: both

    def axis(k):
        b = _lo_of(k, cs)
        cand = _step(np.repeat(b[:, None], 9, 1), np.broadcast_to(np.arange(-4, 5), (n, 9)))
        c = reference_coord(cand, cs[:, None]).astype(np.float32)
        with np.errstate(all="ignore"):
            dis = (cand < c * cs[:, None]) | (cand >= (c + F(1)) * cs[:, None])
        score = dis * 2.0 + rng.random((n, 9))                        # a random one of the disagreeing, if any
        j = np.where(rng.random(n) < 1 / 3, np.argmax(score, 1), rng.integers(0, 9, n))
        return cand[np.arange(n), j]

    px = np.where(mode != 1, axis(kx), _inside(rng, kx, cs))
    py = np.where(mode != 0, axis(ky), _inside(rng, ky, cs))
    return _cells(px, py, _radius_draw(rng, mr, cs), cs)


def _edge_toward(k, s, cs):
    """The edge of cell k + s that faces cell k, as is_obj_in_cell computes it for that neighbour: its hi for s = -1
    (fl(fl((k - 1) cs) + cs)), its lo for s = +1."""
    return np.where(s < 0, _lo_of(k - 1, cs) + cs, _lo_of(k + 1, cs))


def place_touch_edge(rng, kx, ky, cs, mr):
    """The distance to one neighbour's edge within +-6 ulps of r: p = step(fl(edge + r), j) beside the lower neighbour,
    step(fl(edge - r), j) beside the upper one, on x, on y, or on both."""
    n = len(kx)
    mode = rng.integers(0, 3, n)
    r = _radius_draw(rng, mr, cs)
    sx, sy = np.where(rng.random(n) < 0.5, -1, 1), np.where(rng.random(n) < 0.5, -1, 1)

    def axis(k, s):
        e = _edge_toward(k, s, cs)
        return _step(np.where(s < 0, e + r, e - r), rng.integers(-6, 7, n))

    px = np.where(mode != 1, axis(kx, sx), _inside(rng, kx, cs))
    py = np.where(mode != 0, axis(ky, sy), _inside(rng, ky, cs))
    # the aimed neighbour: the x one, or the y one where only y touches
    return _cells(px, py, r, cs, tx=np.where(mode != 1, sx, 0), ty=np.where(mode == 1, sy, 0))


def place_touch_corner(rng, kx, ky, cs, mr):
    """fl(fl(dx^2) + fl(dy^2)) within +-6 ulps of fl(r^2) for a diagonal neighbour: the particle at a distance below
    max_r from the corner, at any angle, and r = sqrt of what the neighbour's test computes, moved by up to 3 ulps."""
    n = len(kx)
    sx, sy = np.where(rng.random(n) < 0.5, -1, 1), np.where(rng.random(n) < 0.5, -1, 1)
    ex, ey = _edge_toward(kx, sx, cs), _edge_toward(ky, sy, cs)
    d = np.exp(rng.uniform(np.log(0.02 * cs.astype(np.float64)), np.log(0.999 * mr.astype(np.float64))))
    ang = rng.uniform(0.02, np.pi / 2 - 0.02, n)
    px, py = _f(ex - sx * d * np.cos(ang)), _f(ey - sy * d * np.sin(ang))
    dx, dy = px - ex, py - ey
    q = dx * dx + dy * dy
    r = _step(np.sqrt(q), rng.integers(-3, 4, n))
    return _cells(px, py, r, cs, tx=sx, ty=sy)


def _corner_at_origin(rng, n, mr, cs):
    """... and constructed as _v_for_q does, where the corner is the origin and p - corner is exact: the home cell (0, 0)
    against (-1, -1), and its mirror images."""
    r = _radius_draw(rng, mr, cs)
    vx, vy, ok = pm._v_for_q(rng, _step(r * r, rng.integers(-6, 7, n)))
    sw = rng.random(n) < 0.5
    vx, vy = np.where(sw, vy, vx), np.where(sw, vx, vy)
    sx, sy = np.where(rng.random(n) < 0.5, -1, 1), np.where(rng.random(n) < 0.5, -1, 1)
    # a particle right of x = 0 touches the cell left of it; one left of x = 0 lies in cell -1 and touches cell 0
    return _cells(_f(-sx * vx), _f(-sy * vy), r, cs, tx=sx, ty=sy)


def _ks(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, n).astype(np.int64), rng.integers(lo, hi + 1, n).astype(np.int64)


def _c_typical(rng, n, max_r=None):
    mr, cs = _cs_draw(rng, n, max_r)
    r = np.where(rng.random(n) < 0.3, mr, _f(mr * rng.uniform(0.05, 1.0, n)))
    return _cells(_f(rng.uniform(0, 4000, n)), _f(rng.uniform(0, 4000, n)), r, cs)


def _c_boundary(rng, n, max_r=None):
    mr, cs = _cs_draw(rng, n, max_r)
    kx, ky = _ks(rng, n, 0, 63000)
    small = rng.random(n) < 0.2                                       # ... and the first cells, k = 0 included
    kx, ky = np.where(small, kx % 40, kx), np.where(small, ky % 40, ky)
    return place_boundary(rng, kx, ky, cs, mr)


def _c_touch_edge(rng, n, max_r=None):
    mr, cs = _cs_draw(rng, n, max_r)
    return place_touch_edge(rng, *_ks(rng, n, 1, 3000), cs, mr)


def _c_touch_corner(rng, n, max_r=None):
    mr, cs = _cs_draw(rng, n, max_r)
    m = n // 4
    return pm._cat(place_touch_corner(rng, *_ks(rng, n - m, 1, 3000), cs[m:], mr[m:]),
                   _corner_at_origin(rng, m, mr[:m], cs[:m]))


def _c_far(rng, n, max_r=None):
    """Cells 55 000 to 63 600, where lo + cs and k * cs round visibly: boundary and touch placements."""
    mr, cs = _cs_draw(rng, n, max_r)
    a, b = n // 3, 2 * (n // 3)
    parts = [f(rng, *_ks(rng, e - s, 55000, 63600), cs[s:e], mr[s:e])
             for f, s, e in ((place_boundary, 0, a), (place_touch_edge, a, b), (place_touch_corner, b, n))]
    return pm._cat(*parts)


def _c_origin(rng, n, max_r=None):
    """p in [-r, r]: -0, +0, components from 2^-149 to 2^-90, +-r and its neighbours: cells -1 and 0, and the (-1, -1)
    cell whose Morton id is the unused marker."""
    mr, cs = _cs_draw(rng, n, max_r)
    r = _radius_draw(rng, mr, cs)

    def comp():
        kind = rng.integers(0, 6, n)
        tiny = _f(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-149, -90, n))) * _sign(rng, n)
        tiny = np.where(tiny == 0, F(TINY), tiny)
        near_r = _step(r, rng.integers(-3, 4, n)) * _sign(rng, n)
        return _f(np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                            [np.full(n, F(-0.0)), np.zeros(n, np.float32), tiny, near_r],
                            _f(r * rng.uniform(-1, 1, n))))

    return _cells(comp(), comp(), r, cs)


def _c_radii(rng, n, max_r=None):
    """r zero, negative, subnormal, with r * r underflowing, one ulp either side of cs / 2.2, and up to 0.75 cs (out of
    contract: masks of more than three bits), half of the particles within a few r of a cell corner."""
    mr, cs = _cs_draw(rng, n, max_r)
    kind = rng.integers(0, 8, n)
    contract = _f(cs.astype(np.float64) / 2.2)
    r = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                  [np.where(rng.random(n) < 0.5, F(0.0), F(-0.0)), -_f(mr * rng.uniform(0.05, 1.0, n)),
                   _f(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-149, -126, n))),
                   _f(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-80, -70, n))),
                   _step(contract, rng.integers(-1, 2, n)), _step(mr, rng.integers(-1, 2, n))],
                  _f(cs * rng.uniform(0.4, 0.75, n)))
    r = _f(r)
    kx, ky = _ks(rng, n, 0, 100)
    reach = np.maximum(np.abs(r), _ulp(_lo_of(kx, cs))).astype(np.float64) * 1.5
    near = rng.random(n) < 0.5
    px = np.where(near, _f(_lo_of(kx, cs) + reach * rng.uniform(-1, 1, n)), _f((kx + rng.random(n)) * cs))
    py = np.where(near, _f(_lo_of(ky, cs) + reach * rng.uniform(-1, 1, n)), _f((ky + rng.random(n)) * cs))
    return _cells(px, py, r, cs)


def _c_specials(rng, n, max_r=None):
    """NaN and +-inf in p or r, |p / cs| at and beyond 2^31 (the cast saturates, the neighbour's coordinate wraps), and
    a cell size of one ulp (2^-149)."""
    mr, cs = _cs_draw(rng, n, max_r)
    base = _c_typical(rng, n, max_r)
    base["cs"] = cs
    base["r"] = _radius_draw(rng, mr, cs)
    kind = rng.integers(0, 6, n)
    edge = _f(cs.astype(np.float64) * 2147483648.0)
    with np.errstate(all="ignore"):
        huge = np.select([rng.random(n) < 0.4, rng.random(n) < 0.5],
                         [_step(edge, rng.integers(-4, 5, n)), _f(edge * rng.uniform(1.0, 4.0, n))], F(3e38))
    huge = _f(huge) * _sign(rng, n)
    odd = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, n)]
    for key in ("px", "py"):
        hit = rng.random(n) < 0.6
        base[key] = np.where((kind == 0) & hit, odd, base[key])
        base[key] = np.where((kind == 1) & hit, huge, base[key])
    base["r"] = np.where(kind == 2, np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, n)], base["r"])
    base["r"] = np.where((kind == 3) & (rng.random(n) < 0.5), F(3e38), base["r"])       # r * r overflows
    one = kind >= 4                                                    # cs = 2^-149: p = m * cs, r = m' * cs, or ordinary
    m = rng.integers(-40, 41, (3, n))
    base["cs"] = np.where(one, F(TINY), base["cs"])
    for i, key in enumerate(("px", "py")):
        base[key] = np.where(one & (rng.random(n) < 0.7), _f(m[i] * TINY), base[key])
    base["r"] = np.where(one & (rng.random(n) < 0.5), _f(np.abs(m[2]) * TINY), base["r"])
    return {k: (_f(v) if v.dtype != np.int8 else v) for k, v in base.items()}


CELL_CLASSES = {"typical": _c_typical, "boundary": _c_boundary, "touch_edge": _c_touch_edge,
                "touch_corner": _c_touch_corner, "far": _c_far, "origin": _c_origin, "radii": _c_radii,
                "specials": _c_specials}


def _with_mixed(rng, parts, names, per_class):
    pool = pm._cat(*parts)
    pick = rng.permutation(len(next(iter(pool.values()))))[:per_class]
    parts.append({k: v[pick] for k, v in pool.items()})
    names.append("mixed")
    return pm._cat(*parts), names, np.repeat(np.arange(len(names)), per_class)


def make_cell_records(per_class=PER_CLASS, seed=2025, max_r=None, specials=True):
    """All cell classes, per_class records each (a multiple of 64: every wave holds one class), then `mixed`: the
    others shuffled together.  Returns (records, class names, class index per record)."""
    assert per_class % WAVE == 0
    rng = np.random.default_rng(seed)
    names = [k for k in CELL_CLASSES if specials or k != "specials"]
    parts = [CELL_CLASSES[k](rng, per_class, max_r) for k in names]
    return _with_mixed(rng, parts, names, per_class)


_CACHE = {}


def cell_records():
    """The records every cell test shares, with their reference: computed once, never modified."""
    if "cells" not in _CACHE:
        rec, names, cls = make_cell_records()
        ref = reference_cells(rec["px"], rec["py"], rec["r"], rec["cs"])
        for v in list(rec.values()) + list(ref):
            v.setflags(write=False)
        _CACHE["cells"] = (rec, names, cls, ref)
    return _CACHE["cells"]


def _bit_of(tx, ty):
    """Scan index of the neighbour at offset (tx, ty) != (0, 0)."""
    idx = (ty.astype(np.int64) + 1) * 3 + (tx.astype(np.int64) + 1)
    return np.where(idx > 4, idx - 1, idx)


# ---------------------------------------------------------------------------------------------------------------------
# verlet classes: each returns (per-particle dict cx cy qx qy r and `group`, list of parameter sets); a parameter set is
# a dict of VERLET_PARAMS -- what one context holds: few per class, so that one oracle call serves many records


def _pset(dt=1 / 60, world=(3048.0, 1048.0), acc=(0.0, 0.0), pressed=0, mouse=(0.0, 0.0), strength=DEFAULT_STRENGTH):
    return dict(dt=F(dt), world_w=F(world[0]), world_h=F(world[1]), acc_x=F(acc[0]), acc_y=F(acc[1]),
                pressed=int(pressed), mouse_x=F(mouse[0]), mouse_y=F(mouse[1]), strength=F(strength))


def _parts(cx, cy, qx, qy, r, group):
    return dict(cx=_f(cx).copy(), cy=_f(cy).copy(), qx=_f(qx).copy(), qy=_f(qy).copy(), r=_f(r).copy(),
                group=np.asarray(group, np.int32).copy())


def _groups(rng, n, k):
    return rng.integers(0, k, n)


def _in_world(rng, n, sets, g):
    w = np.array([[float(s["world_w"]), float(s["world_h"])] for s in sets])[g]
    return _f(rng.random(n) * w[:, 0]), _f(rng.random(n) * w[:, 1])


def _v_typical(rng, n):
    sets = [_pset(acc=(rng.uniform(-12, 12), rng.uniform(-12, 12)), pressed=i % 2,
                  mouse=(rng.uniform(0, 3048), rng.uniform(0, 1048)),
                  world=((3048.0, 1048.0) if i < 4 else (rng.uniform(50, 4000), rng.uniform(50, 4000)))) for i in range(8)]
    g = _groups(rng, n, len(sets))
    cx, cy = _in_world(rng, n, sets, g)
    v = rng.normal(0, 0.05, (2, n))
    return _parts(cx, cy, _f(cx - v[0]), _f(cy - v[1]), _f(rng.uniform(0.25, 3.0, n)), g), sets


def _v_at_mouse(rng, n):
    """c == mouse exactly (0 / 0), |mouse - c| from 2^-149 to 2^-60 (the length underflows to 0 or a subnormal) and of
    1e20 (its square overflows); mouse_pressed 0, 1 and 2."""
    m = (500.25, 300.5)
    sets = [_pset(pressed=1, mouse=m, acc=(0.0, -9.81)), _pset(pressed=1, mouse=(0.0, 0.0)),
            _pset(pressed=1, mouse=(0.0, 0.0), world=(1e30, 1e30)), _pset(pressed=1, mouse=m, world=(1e30, 1e30)),
            _pset(pressed=0, mouse=m), _pset(pressed=2, mouse=m)]
    g = _groups(rng, n, len(sets))
    at = rng.random(n) < 0.5
    jx, jy = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    cx = np.where(at, F(m[0]), _step(np.full(n, F(m[0])), jx))
    cy = np.where(at, F(m[1]), _step(np.full(n, F(m[1])), jy))
    tiny = _f(np.ldexp(rng.uniform(1.0, 2.0, (2, n)), rng.integers(-149, -59, (2, n)))) * _sign(rng, 2 * n).reshape(2, n)
    tiny = np.where(rng.random((2, n)) < 0.25, F(0.0) * _sign(rng, 2 * n).reshape(2, n), tiny)    # +-0: c == mouse again
    far = F(1e20) * _sign(rng, 2 * n).reshape(2, n) * (rng.random((2, n)) < 0.7)
    origin = (g == 1) | (g == 2)
    use_far = origin & (rng.random(n) < 0.3)
    cx = np.where(origin, np.where(use_far, far[0], tiny[0]), cx)
    cy = np.where(origin, np.where(use_far, far[1], tiny[1]), cy)
    r = np.where(rng.random(n) < 0.5, F(0.5), np.array([0.0, -0.5, 1e-30, 3.0], np.float32)[rng.integers(0, 4, n)])
    still = rng.random(n) < 0.7
    v = rng.normal(0, 0.05, (2, n))
    return _parts(cx, cy, np.where(still, cx, _f(cx - v[0])), np.where(still, cy, _f(cy - v[1])), r, g), sets


def _v_clamp(rng, n):
    """The unclamped result within +-4 ulps of r and of fl(W - r) on each axis; W - r < r; r negative, 0 or NaN; results
    of -0."""
    sets = [_pset(acc=(2.5, -9.81)), _pset(acc=(0.0, 0.0), world=(400.0, 300.0)),
            _pset(acc=(2.5, -9.81), world=(1.0, 6.0)),                 # narrower than the particles, one 3-radius cell high
            _pset(acc=(-0.0, -0.0), world=(100.0, 100.0)),
            _pset(acc=(2.5, -9.81), world=(2.0, 1.5))]                 # narrower and lower than most of its particles
    g = _groups(rng, n, len(sets))
    S = {k: np.array([s[k] for s in sets])[g] for k in VERLET_PARAMS}
    r = _f(rng.uniform(0.25, 3.0, n))
    odd = (g < 2) & (rng.random(n) < 0.15)
    r = np.where(odd, np.array([0.0, -0.0, -0.5, -2.0, np.nan], np.float32)[rng.integers(0, 5, n)], r)
    dt2 = S["dt"] * S["dt"]

    def axis(world, acc):
        with np.errstate(all="ignore"):
            shift = acc * dt2
            target = np.where(rng.random(n) < 0.5, r, world - r)
            c = _step(np.nan_to_num(target - shift), rng.integers(-4, 5, n))
            inside = _f(rng.random(n) * world)
        c = np.where(rng.random(n) < 0.8, c, inside)
        still = rng.random(n) < 0.6
        return c, np.where(still, c, _f(c - rng.normal(0, 1e-3, n)))

    cx, qx = axis(_f(S["world_w"]), _f(S["acc_x"]))
    cy, qy = axis(_f(S["world_h"]), _f(S["acc_y"]))
    zero = g == 3                                                      # -0 + (-0 - +0) + (-0 * dt^2) = -0
    z = lambda: np.where(rng.random(n) < 0.7, F(-0.0), F(0.0))
    cx, cy = np.where(zero, z(), cx), np.where(zero, z(), cy)
    qx, qy = np.where(zero, -z(), qx), np.where(zero, -z(), qy)
    r = np.where(zero, np.array([0.0, -0.0, -0.5, 0.5], np.float32)[rng.integers(0, 4, n)], r)
    return _parts(cx, cy, qx, qy, r, g), sets


def _v_dt(rng, n):
    """dt^2 of 0, subnormal (2^-140), underflowing (1e-46) and 1e6; dt of 1/60, 1/30, 1/144 and -1/60, each squared in
    float32 as verlet_params does."""
    dts = [0.0, float(np.ldexp(1.0, -70)), 1e-23, 1000.0, 1 / 60, 1 / 30, 1 / 144, -1 / 60]
    sets = [_pset(dt=d, acc=(3.0, -9.81), pressed=i % 2, mouse=(1500.0, 500.0)) for i, d in enumerate(dts)]
    sets += [_pset(dt=d, acc=(3.0, -9.81), pressed=1 - i % 2, mouse=(1500.0, 500.0)) for i, d in enumerate(dts)]
    g = _groups(rng, n, len(sets))
    cx, cy = _in_world(rng, n, sets, g)
    v = rng.normal(0, 0.05, (2, n))
    return _parts(cx, cy, _f(cx - v[0]), _f(cy - v[1]), _f(rng.uniform(0.25, 3.0, n)), g), sets


def _v_velocity(rng, n):
    """prev == cur; prev far away (a velocity of 1e4); prev = 0.4 c, so that c - prev and c + v both round; NaN and
    +-inf in prev."""
    sets = [_pset(acc=(0.0, -9.81)), _pset(acc=(1.0, 2.0), pressed=1, mouse=(100.0, 900.0), world=(1e5, 1e5))]
    g = _groups(rng, n, len(sets))
    cx, cy = _in_world(rng, n, sets, g)
    kind = rng.integers(0, 4, n)
    odd = np.array([np.nan, np.inf, -np.inf], np.float32)

    def prev(c):
        return _f(np.select([kind == 0, kind == 1, kind == 2],
                            [c, _f(c - F(1e4) * _sign(rng, n)), _f(c * F(0.4))],
                            np.where(rng.random(n) < 0.6, odd[rng.integers(0, 3, n)], c)))

    return _parts(cx, cy, prev(cx), prev(cy), _f(rng.uniform(0.25, 3.0, n)), g), sets


def _v_strength(rng, n):
    sets = [_pset(pressed=1, mouse=(1500.0, 500.0), acc=(0.0, -9.81), strength=s)
            for s in (0.0, -0.0, -DEFAULT_STRENGTH, 1e30, DEFAULT_STRENGTH, np.inf)]
    g = _groups(rng, n, len(sets))
    cx, cy = _in_world(rng, n, sets, g)
    at = rng.random(n) < 0.05                                          # 0 / 0 times a strength of 0 or inf
    cx, cy = np.where(at, F(1500.0), cx), np.where(at, F(500.0), cy)
    return _parts(cx, cy, cx, cy, _f(rng.uniform(0.25, 3.0, n)), g), sets


VERLET_CLASSES = {"typical": _v_typical, "at_mouse": _v_at_mouse, "clamp": _v_clamp, "dt": _v_dt,
                  "velocity": _v_velocity, "strength": _v_strength}


def make_verlet_records(per_class=PER_CLASS, seed=2026):
    """All verlet classes and `mixed`.  Returns (records: the particles and the parameters of each, expanded; class
    names; class index per record; the parameter sets; the set of each record)."""
    assert per_class % WAVE == 0
    rng = np.random.default_rng(seed)
    names, parts, sets = list(VERLET_CLASSES), [], []
    for k in names:
        p, s = VERLET_CLASSES[k](rng, per_class)
        p["group"] = p["group"] + len(sets)
        parts.append(p)
        sets += s
    rec, names, cls = _with_mixed(rng, parts, names, per_class)
    for k in VERLET_PARAMS:
        rec[k] = np.array([s[k] for s in sets])[rec["group"]]
    rec["dt2"] = rec["dt"] * rec["dt"]                               # float32, as the host squares it
    return rec, names, cls, sets


def reference_verlet_of(rec):
    return reference_verlet(rec["cx"], rec["cy"], rec["qx"], rec["qy"], rec["r"], rec["dt2"], rec["world_w"],
                            rec["world_h"], rec["acc_x"], rec["acc_y"], rec["pressed"], rec["mouse_x"], rec["mouse_y"],
                            rec["strength"])


def verlet_records():
    if "verlet" not in _CACHE:
        rec, names, cls, sets = make_verlet_records()
        ref = reference_verlet_of(rec)
        for v in list(rec.values()) + list(ref):
            v.setflags(write=False)
        _CACHE["verlet"] = (rec, names, cls, sets, ref)
    return _CACHE["verlet"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the references against the C oracle, and what the generators promise


def test_vectorised_helpers_equal_the_oracle(oracle):
    rng = np.random.default_rng(1)
    for mr in list(MAX_RS) + list(rng.uniform(0.3, 2.5, 200)):
        assert float(cell_size_of(F(mr))) == oracle.compute_cell_size(float(F(mr)))
    xy = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, (300, 2)), [[-1, -1], [0, 0], [65535, 65535], [-1, 0]]])
    xy = xy.astype(np.int64).astype(np.int32)
    got = morton(xy[:, 0].copy(), xy[:, 1].copy())
    assert [int(v) for v in got] == [oracle.morton_encode(int(x), int(y)) for x, y in xy]
    assert got[300] == UNUSED                                          # the (-1, -1) cell aliases the unused marker
    assert oracle.default_params(1.0, 1.0, 1.0).mouse_strength == DEFAULT_STRENGTH


def test_reference_cells_equal_the_oracle_on_every_record(oracle):
    """Every cell record through oracle.build_cell_ids, one call per class and cell size: all four slots, bit for bit."""
    rec, names, cls, (cx, cy, mask) = cell_records()
    want = reference_slots(cx, cy, mask)
    checked = 0
    # grouped by cell size over all records: one oracle call per size (each class draws some sixty of them)
    order = np.argsort(rec["cs"], kind="stable")
    cs_sorted = rec["cs"][order]
    starts = np.flatnonzero(np.concatenate([[True], cs_sorted[1:] != cs_sorted[:-1]]))
    ends = np.concatenate([starts[1:], [len(order)]])
    pos = np.stack([rec["px"], rec["py"]], 1)
    got = np.empty_like(want)
    lib = oracle.lib()
    for s, e in zip(starts, ends):
        idx = order[s:e]
        p, r = np.ascontiguousarray(pos[idx]).reshape(-1), np.ascontiguousarray(rec["r"][idx])
        ids = np.full(4 * len(idx), UNUSED, np.uint32)
        lib.orc_build_cell_ids(p, r, len(idx), float(cs_sorted[s]), ids, np.zeros(4 * len(idx), np.uint32))
        got[idx] = ids.reshape(-1, 4)
        checked += len(idx)
    assert checked == len(want)
    bad = (got != want).any(1)
    lines = ["%-12s %6d of %d" % (name, (bad & (cls == c)).sum(), (cls == c).sum()) for c, name in enumerate(names)
             if (bad & (cls == c)).any()]
    for i in np.flatnonzero(bad)[:8]:
        lines.append("  [%s] p (%s, %s) r %s cs %s: oracle %s, reference %s" % (
            names[cls[i]], *[_hex(rec[k][i]) for k in ("px", "py", "r", "cs")], got[i], want[i]))
    assert not bad.any(), "reference_slots differs from the oracle:\n" + "\n".join(lines)


def _oracle_params(oracle, s):
    p = oracle.default_params(float(s["world_w"]), float(s["world_h"]), 1.0, gravity=(float(s["acc_x"]), float(s["acc_y"])))
    p.mouse_pressed, p.mouse_x, p.mouse_y = s["pressed"], float(s["mouse_x"]), float(s["mouse_y"])
    p.mouse_strength = float(s["strength"])
    return p


def _oracle_verlet(oracle, rec, sets, idx, s):
    pos = np.stack([rec["cx"][idx], rec["cy"][idx]], 1)
    prev = np.stack([rec["qx"][idx], rec["qy"][idx]], 1)
    return oracle.verlet_integration(pos, prev, rec["r"][idx], _oracle_params(oracle, sets[s]), float(sets[s]["dt"]))


def test_reference_verlet_equals_the_oracle_on_every_record(oracle):
    """Every verlet record through oracle.verlet_integration, one call per parameter set; NaN as _same treats it."""
    rec, names, cls, sets, (nx, ny) = verlet_records()
    bad = np.zeros(len(nx), bool)
    checked = 0
    for s in range(len(sets)):
        idx = np.flatnonzero(rec["group"] == s)
        got, prev = _oracle_verlet(oracle, rec, sets, idx, s)
        bad[idx] = ~(_same(got[:, 0], nx[idx]) & _same(got[:, 1], ny[idx]))
        assert _same(prev, np.stack([rec["cx"][idx], rec["cy"][idx]], 1)).all()
        checked += len(idx)
    assert checked == len(nx)
    lines = ["%-10s %6d of %d" % (name, (bad & (cls == c)).sum(), (cls == c).sum()) for c, name in enumerate(names)
             if (bad & (cls == c)).any()]
    assert not bad.any(), "reference_verlet differs from the oracle:\n" + "\n".join(lines)


def test_cell_generators_reach_their_edges():
    """No class passes vacuously -- from the reference alone."""
    rec, names, cls, (cx, cy, mask) = cell_records()
    for name in ("touch_edge", "touch_corner"):
        m = cls == names.index(name)
        bit = (mask[m] >> _bit_of(rec["tx"][m], rec["ty"][m]).astype(np.uint32)) & 1
        assert 0.2 <= bit.mean() <= 0.8, (name, bit.mean())
    m = cls == names.index("boundary")
    with np.errstate(all="ignore"):
        dis = lambda p, c: (p < c.astype(np.float32) * rec["cs"][m]) | (p >= (c + 1).astype(np.float32) * rec["cs"][m])
        disagree = dis(rec["px"][m], cx[m]) | dis(rec["py"][m], cy[m])
    assert disagree.sum() >= 1000, disagree.sum()
    m = cls == names.index("radii")
    bits = np.array([bin(v).count("1") for v in range(256)])[mask[m]]
    assert (bits >= 4).sum() >= 1000, (bits >= 4).sum()
    m = cls == names.index("far")
    assert min(cx[m].min(), cy[m].min()) >= 54990 and max(cx[m].max(), cy[m].max()) <= 63610
    m = cls == names.index("origin")
    home = set(zip(cx[m].tolist(), cy[m].tolist()))
    assert home == {(-1, -1), (-1, 0), (0, -1), (0, 0)}, home
    m = cls == names.index("specials")
    assert (np.abs(cx[m].astype(np.int64)) >= 2 ** 31 - 1).sum() > 1000 and np.isnan(rec["px"][m]).sum() > 1000


def test_verlet_generators_reach_their_edges():
    rec, names, cls, sets, (nx, ny) = verlet_records()
    m = cls == names.index("clamp")
    with np.errstate(all="ignore"):
        vx, vy = rec["cx"][m] - rec["qx"][m], rec["cy"][m] - rec["qy"][m]
        raw = {"x": ((rec["cx"][m] + vx) + rec["acc_x"][m] * rec["dt2"][m], rec["world_w"][m]),
               "y": ((rec["cy"][m] + vy) + rec["acc_y"][m] * rec["dt2"][m], rec["world_h"][m])}
        for axis, (x, world) in raw.items():
            lo, hi = rec["r"][m], world - rec["r"][m]
            first = x > lo
            second = np.where(first, x, lo) < hi
            for a in (True, False):
                for b in (True, False):                                # the four outcomes of the two compares
                    assert ((first == a) & (second == b)).sum() >= 1000, (axis, a, b, ((first == a) & (second == b)).sum())
    assert (np.signbit(nx[m]) & (nx[m] == 0)).sum() > 100               # results of -0
    m = cls == names.index("at_mouse")
    with np.errstate(all="ignore"):
        dx, dy = rec["mouse_x"][m] - rec["cx"][m], rec["mouse_y"][m] - rec["cy"][m]
        q = dx * dx + dy * dy
        ln = np.sqrt(q)
        nan_acc = (rec["pressed"][m] == 1) & np.isnan(dx / ln)
    assert nan_acc.sum() >= 1000, nan_acc.sum()
    # squared lengths that are subnormal, that underflow to 0 off the mouse, and that overflow
    assert ((q > 0) & (q < F(1.1754944e-38))).sum() > 100 and np.isinf(ln).sum() > 100
    assert ((q == 0) & ((dx != 0) | (dy != 0))).sum() > 100
    assert set(np.unique(rec["pressed"][m])) == {0, 1, 2}


def build_probe():
    deps = [PROBE_SRC] + [os.path.join(pm.CSRC, h) for h in ("k_cells.h", "gpe_internal.h")]
    if not os.path.exists(PROBE_EXE) or any(os.path.getmtime(d) > os.path.getmtime(PROBE_EXE) for d in deps):
        r = subprocess.run([pm.HIPCC] + pm.PROBE_FLAGS + ["-I", pm.CSRC, PROBE_SRC, "-o", PROBE_EXE],
                           capture_output=True, text=True)
        assert r.returncode == 0, "cell_probe.hip does not compile:\n" + r.stdout + r.stderr
    return PROBE_EXE


def test_cell_probe_compiles_for_gfx950():
    """One executable, both modes (its two kernels)."""
    exe = build_probe()
    with open(exe, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"probe_cells" in blob and b"probe_verlet" in blob


def test_overlap_mask_has_one_home():
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(pm.CSRC, "*.h*"))}
    assert [k for k, v in src.items() if "uint32_t neighbour_overlap_mask(" in v] == ["k_cells.h"]
    assert '#include "k_cells.h"' in src["k_native.hip"]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the probe


def run_probe(mode, words, n_out, tmp_path):
    exe = build_probe()
    src, dst = str(tmp_path / (mode + "_in.bin")), str(tmp_path / (mode + "_out.bin"))
    np.ascontiguousarray(words).tofile(src)
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(dst, np.uint32).reshape(len(words), n_out)


# Failing records of earlier versions of the kernels, kept as named cases: (px, py, r, cell_size).  None so far.
NAMED_CELL_CASES = {}


@pytest.mark.gpu
def test_cell_membership_equals_ieee_reference_on_edge_classes(tmp_path):
    """cx, cy, the native mask and the compat mask each equal the reference on every record of every class (the two
    masks therefore equal each other everywhere, NaN positions included: both forms give them cell 0 and no bit)."""
    rec, names, cls, (cx, cy, mask) = cell_records()
    words = np.stack([rec[k] for k in ("px", "py", "r", "cs")], 1).view(np.uint32)
    out = run_probe("cells", words, 4, tmp_path)
    ok = {"cx": out[:, 0].view(np.int32) == cx, "cy": out[:, 1].view(np.int32) == cy,
          "native": out[:, 2] == mask, "compat": out[:, 3] == mask}
    lines = []
    for k, name in enumerate(names):
        m = cls == k
        if any((~v & m).any() for v in ok.values()):
            lines.append("%-12s " % name + "  ".join("%s %6d" % (w, (~v & m).sum()) for w, v in ok.items()) +
                         "  of %d" % m.sum())
    bad = np.flatnonzero(~np.logical_and.reduce(list(ok.values())))
    for i in bad[:8]:
        lines.append("  [%s] p (%s, %s) r %s cs %s: got cell (%d, %d) native %s compat %s, want (%d, %d) %s" % (
            names[cls[i]], *[_hex(rec[k][i]) for k in ("px", "py", "r", "cs")], out[i, 0].view(np.int32),
            out[i, 1].view(np.int32), bin(out[i, 2]), bin(out[i, 3]), cx[i], cy[i], bin(mask[i])))
    assert len(bad) == 0, "cell membership differs from the IEEE reference:\n" + "\n".join(lines)


@pytest.mark.gpu
def test_verlet_one_equals_ieee_reference_on_edge_classes(tmp_path):
    rec, names, cls, sets, (nx, ny) = verlet_records()
    keys = ("cx", "cy", "qx", "qy", "r", "dt2", "world_w", "world_h", "acc_x", "acc_y", None, "mouse_x", "mouse_y",
            "strength")
    words = np.stack([rec["pressed"].astype(np.uint32) if k is None else _f(rec[k]).view(np.uint32) for k in keys], 1)
    out = run_probe("verlet", words, 2, tmp_path).view(np.float32)
    ok = _same(out[:, 0], nx) & _same(out[:, 1], ny)
    lines = ["%-10s %6d of %d" % (name, (~ok & (cls == k)).sum(), (cls == k).sum()) for k, name in enumerate(names)
             if (~ok & (cls == k)).any()]
    for i in np.flatnonzero(~ok)[:8]:
        lines.append("  [%s] c (%s, %s) prev (%s, %s) r %s %s: got (%s, %s) want (%s, %s)" % (
            names[cls[i]], *[_hex(rec[k][i]) for k in ("cx", "cy", "qx", "qy", "r")],
            {k: (_hex(v) if k != "pressed" else v) for k, v in sets[rec["group"][i]].items()},
            _hex(out[i, 0]), _hex(out[i, 1]), _hex(nx[i]), _hex(ny[i])))
    assert ok.all(), "verlet_one differs from the IEEE reference:\n" + "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the records through the compat kernels


@pytest.mark.gpu
@pytest.mark.parametrize("max_r", MAX_RS)
def test_compat_grid_build_equals_oracle_on_cell_records(gpe, oracle, max_r):
    """An odd ~300 000 records of one cell size (every class but `specials`) as one particle set: Grid.build_cell_ids
    against oracle.build_cell_ids, exactly, slot order included."""
    rec, names, cls = make_cell_records(64 * 588, seed=77 + int(max_r * 4), max_r=max_r, specials=False)
    n = len(rec["px"]) - 1
    assert n % 2 == 1 and 290_000 < n < 310_000
    pos, rad = np.stack([rec["px"], rec["py"]], 1)[:n].copy(), rec["r"][:n].copy()
    cs = oracle.compute_cell_size(max_r)
    ctx = gpe.Context(world=(5e5, 5e5), mode=gpe.MODE_COMPAT)
    ps = gpe.ParticleSystem.new_from_buffers(ctx, pos, rad)
    grid = gpe.Grid.new_without_camera(ctx, max_r, ps)
    assert grid.cell_size() == cs and (rec["cs"] == F(cs)).all()
    grid.build_cell_ids()
    got = grid.download_cell_ids().reshape(n, 4)
    ctx.close()
    want = oracle.build_cell_ids(pos, rad, cs)[0].reshape(n, 4)
    bad = (got != want).any(1)
    assert not bad.any(), "%d particles' cell ids differ, first: %s" % (bad.sum(), [
        "[%s] p (%s, %s) r %s: got %s want %s" % (names[cls[i]], _hex(pos[i, 0]), _hex(pos[i, 1]), _hex(rad[i]), got[i],
                                                  want[i]) for i in np.flatnonzero(bad)[:4]])


def _api_group(s):
    """Can the API express the parameter set?  (The button is pressed or not; the strength is the default.)"""
    return s["pressed"] in (0, 1) and float(s["strength"]) == DEFAULT_STRENGTH


@pytest.mark.gpu
def test_compat_integration_equals_oracle_on_verlet_records(gpe, oracle):
    """The verlet records grouped by (dt, gravity, mouse, world), the groups the API can express, an odd count each (the
    paired path and the tail of k_verlet): update_positions against the oracle, positions and previous positions."""
    rec, names, cls, sets, _ = verlet_records()
    want_classes = {"typical": 2, "at_mouse": 4, "clamp": 4, "dt": 3, "velocity": 2}
    ran = 0
    for name, limit in want_classes.items():
        in_class = cls == names.index(name)
        groups = [s for s in np.unique(rec["group"][in_class]) if _api_group(sets[s])]
        if name == "dt":                                              # dt^2 subnormal, dt negative, dt^2 = 1e6
            groups = [s for s in groups if float(sets[s]["dt"]) in (float(F(np.ldexp(1.0, -70))), float(F(-1 / 60)), 1000.0)]
        for s in groups[:limit]:
            idx = np.flatnonzero(in_class & (rec["group"] == s))
            idx = idx[:len(idx) - 1 + len(idx) % 2]                  # odd
            P = sets[s]
            pos = np.stack([rec["cx"][idx], rec["cy"][idx]], 1)
            prev = np.stack([rec["qx"][idx], rec["qy"][idx]], 1)
            ctx = gpe.Context(world=(float(P["world_w"]), float(P["world_h"])),
                              gravity=(float(P["acc_x"]), float(P["acc_y"])), mode=gpe.MODE_COMPAT)
            ps = gpe.ParticleSystem.new_from_buffers(ctx, pos, rec["r"][idx], prev=prev)
            ps.mouse_click_callback(P["pressed"] == 1, (float(P["mouse_x"]), float(P["mouse_y"])))
            ps.update_positions(float(P["dt"]))
            got_pos, got_prev, _ = ps.download_particle_buffers()
            ctx.close()
            want_pos, want_prev = _oracle_verlet(oracle, rec, sets, idx, s)
            bad = ~(_same(got_pos, want_pos).all(1) & _same(got_prev, want_prev).all(1))
            assert len(idx) % 2 == 1 and len(idx) > 1000
            assert not bad.any(), "%s, set %s: %d of %d differ, first c (%s, %s) got %s want %s" % (
                name, P, bad.sum(), len(idx), _hex(pos[bad][0, 0]), _hex(pos[bad][0, 1]),
                [_hex(v) for v in got_pos[bad][0]], [_hex(v) for v in want_pos[bad][0]])
            ran += 1
    assert ran >= 12


# ---------------------------------------------------------------------------------------------------------------------
# GPU: edge scenes through the NATIVE pipeline, against the oracle

MEMBERSHIP_WORLDS = {"r025": (0.25, None), "r1": (1.0, None), "wide": (0.5, 70000.0)}


def membership_edge_scene(which, seed=9):
    """About 3 000 isolated overlapping pairs at sites 16 cells apart, one particle of each on a boundary, touch_edge or
    touch_corner placement of its site's cell (in the 70 000 wide world a third of the sites lie beyond cell 55 000:
    the `far` placements), a tenth of the pairs well inside a cell, and a column of pairs on x = 0 whose x run down to
    2^-140.  Returns (pos, rad, world, max_r)."""
    max_r, width = MEMBERSHIP_WORLDS[which]
    rng = np.random.default_rng(seed + int(max_r * 8))
    cs = float(cell_size_of(max_r))
    cols, rows = 60, 50
    if width is None:
        col_cell = 16 * np.arange(1, cols + 1) + 8
        world = (cs * 16 * (cols + 2), cs * 16 * (rows + 2))
    else:
        last = int(width / cs) // 16 - 2                               # 63 636 columns of cells
        far = rng.choice(np.arange(55000 // 16 + 1, last), cols // 3, replace=False)
        near = rng.choice(np.arange(1, 55000 // 16), cols - cols // 3, replace=False)
        col_cell = 16 * np.sort(np.concatenate([near, far])) + 8
        world = (width, cs * 16 * (rows + 2))
    gx, gy = np.meshgrid(col_cell, 16 * np.arange(1, rows + 1) + 8)
    kx, ky = gx.ravel().astype(np.int64), gy.ravel().astype(np.int64)
    n = len(kx)
    csa, mra = np.full(n, F(cs)), np.full(n, F(max_r))
    kind = rng.integers(0, 10, n)
    placed = [place_boundary(rng, kx, ky, csa, mra), place_touch_edge(rng, kx, ky, csa, mra),
              place_touch_corner(rng, kx, ky, csa, mra)]
    sel = np.select([kind < 3, kind < 6, kind < 9], [0, 1, 2], 3)
    ax = np.select([sel == 0, sel == 1, sel == 2], [p["px"] for p in placed], _inside(rng, kx, csa))
    ay = np.select([sel == 0, sel == 1, sel == 2], [p["py"] for p in placed], _inside(rng, ky, csa))
    ra = np.select([sel == 0, sel == 1, sel == 2], [p["r"] for p in placed], _f(0.1 * cs * rng.uniform(0.2, 1.0, n)))
    ra = np.maximum(_f(ra), F(0.02 * cs))
    rb = np.where(rng.random(n) < 0.5, ra, _f(ra * rng.uniform(0.5, 1.0, n)))
    d = rng.uniform(0.1, 0.9, n) * (ra.astype(np.float64) + rb)
    ang = rng.uniform(0, 2 * np.pi, n)
    bx, by = _f(ax + d * np.cos(ang)), _f(ay + d * np.sin(ang))
    # the origin column: pairs 4 cells apart along x = 0
    k = 4 * rows
    t = _f(np.ldexp(rng.uniform(1.0, 2.0, (2, k)), rng.integers(-140, -90, (2, k))))
    t[:, rng.random(k) < 0.25] = 0.0
    t[0, rng.random(k) < 0.1] = -0.0
    oy = _f(cs * (4 * np.arange(1, k + 1) + 0.3))
    orad = np.where(np.arange(k) % 3 == 2, _f(max_r * rng.uniform(0.05, 0.5, k)), F(max_r))
    ody = _f(orad * rng.uniform(0.2, 1.9, k))
    pos = np.concatenate([np.stack([np.stack([ax, ay], 1), np.stack([bx, by], 1)], 1).reshape(-1, 2),
                          np.stack([np.stack([t[0], oy], 1), np.stack([t[1], _f(oy + ody)], 1)], 1).reshape(-1, 2)])
    rad = np.concatenate([np.stack([ra, rb], 1).ravel(), np.repeat(orad, 2)])
    pos, rad = _f(pos), _f(rad)
    assert rad.max() == F(max_r) and (pos >= 0).all() and (pos <= np.array(world, np.float32)).all()
    return pos, rad, world, max_r


def _shared_cells(oracle, pos, rad, cs):
    ids = oracle.build_cell_ids(pos, rad, cs)[0].reshape(-1, 2, 4)
    a, b = ids[:, 0, :, None], ids[:, 1, None, :]
    return ((a == b) & (a != UNUSED)).sum((1, 2))


@pytest.mark.parametrize("which", list(MEMBERSHIP_WORLDS))
def test_membership_edge_scene_shares_one_two_and_four_cells(oracle, which):
    """CPU precondition of the scene tests: the oracle resolves the scene's pairs once, twice and four times (the
    number of cells both particles lie in), each at least 100 times."""
    pos, rad, world, max_r = membership_edge_scene(which)
    assert 6000 <= len(pos) <= 7000
    shared = _shared_cells(oracle, pos, rad, oracle.compute_cell_size(max_r))
    for k in (1, 2, 4):
        assert (shared == k).sum() >= 100, (which, k, np.bincount(shared))
    if which == "wide":
        assert (pos[:, 0] > 55000 * 1.1).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "compat"])
@pytest.mark.parametrize("which", list(MEMBERSHIP_WORLDS))
def test_membership_edge_scene_matches_oracle(gpe, oracle, which, native):
    pos, rad, world, max_r = membership_edge_scene(which)
    pm._state_vs_oracle(gpe, oracle, pos, rad, world, gpe.MODE_NATIVE if native else gpe.MODE_COMPAT, 3,
                        "membership edges, %s (%s)" % (which, "native" if native else "compat"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(MEMBERSHIP_WORLDS))
def test_membership_edge_scene_local_group_equals_single_context(gpe, which):
    """The same scene as a two-context local group: bit-identical to one context."""
    lg = importlib.import_module("gpu-physics-engine_amd.local_group")
    pos, rad, world, max_r = membership_edge_scene(which)
    steps, dt, every = 6, 1 / 60, 4
    flags = gpe._lib.FLAG_NATIVE_FORCE
    run = lg.LocalShardedRun(pos, rad, world, 2, flags=flags)
    run.run(dt, steps, resort_every=every, resort_first=True)
    owned = run.owned()
    run.close()
    ref = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, flags=flags)
    ref.run(dt, steps, resort_every=every, resort_first=True)
    want_pos, want_prev = ref.positions(), ref.previous_positions()
    ref.close()
    seen = np.zeros(len(pos), bool)
    for r, (gid, p, q) in enumerate(owned):
        seen[gid] = True
        assert _same(p, want_pos[gid]).all(), "rank %d positions" % r
        assert _same(q, want_prev[gid]).all(), "rank %d previous positions" % r
    assert seen.all()


def integration_edge_scene(seed=21):
    """A few thousand particles 4 cells apart in a 400 x 300 world, gravity (2.5, -9.81), the mouse pressed on one of
    them exactly (0 / 0) and within ulps of the column of others; along the four walls the `clamp` placements: a first step that ends
    within +-4 ulps of r or of fl(W - r).  Returns (pos, rad, world, gravity, mouse, dt)."""
    rng = np.random.default_rng(seed)
    world, gravity, dt, max_r = (400.0, 300.0), (2.5, -9.81), 1 / 60, 1.0
    cs = 2.2
    gx, gy = np.meshgrid(np.arange(2, 43), np.arange(2, 32))
    px, py = _f(gx.ravel() * 4 * cs + 1.0), _f(gy.ravel() * 4 * cs + 1.0)
    n = len(px)
    rad = _f(rng.uniform(0.3, 1.0, n))
    mouse = (float(px[n // 2]), float(py[n // 2]))                     # exactly on one particle
    near = np.arange(n // 2 + 1, n // 2 + 9)                           # ... eight more brought within ulps of its column
    px[near] = _step(np.full(8, F(mouse[0])), rng.integers(-3, 4, 8))
    py[near] = _f(mouse[1] + 4 * cs * np.arange(1, 9) + 2 * cs)       # (between the rows)
    dt2 = F(dt) * F(dt)
    walls = []
    for axis, (w, g) in enumerate(zip(world, gravity)):
        along = _f(np.arange(2, int((world[1 - axis]) / (4 * cs)) - 1) * 4 * cs + 2.0)
        for high in (False, True):
            r = _f(rng.uniform(0.3, 1.0, len(along)))
            target = (F(w) - r) if high else r
            c = target
            for _ in range(4):                                         # gravity and the mouse's pull, which depends on c
                d, e = F(mouse[axis]) - c, F(mouse[1 - axis]) - along
                acc = F(g) + (d / np.sqrt(d * d + e * e)) * F(DEFAULT_STRENGTH)
                c = target - acc * dt2
            c = _step(c, rng.integers(-4, 5, len(along)))
            walls.append((np.stack([c, along] if axis == 0 else [along, c], 1), r))
    pos = np.concatenate([np.stack([px, py], 1)] + [w[0] for w in walls])
    rad = np.concatenate([rad] + [w[1] for w in walls])
    rad[0] = max_r
    return _f(np.clip(pos, 0, np.array(world, np.float32))), _f(rad), world, gravity, mouse, dt


def _run_against_oracle(gpe, oracle, pos, rad, world, gravity, mouse, dt, steps, mode, flags):
    st = gpe.State(pos, rad, world=world, gravity=gravity, mode=mode, flags=flags)
    st.particles.mouse_click_callback(True, mouse)
    p = oracle.default_params(world[0], world[1], float(rad.max()), gravity=gravity)
    p.mouse_pressed, p.mouse_x, p.mouse_y = 1, mouse[0], mouse[1]
    sim = oracle.Sim(pos, rad, p)
    st.run(dt, steps, resort_every=0, resort_first=True)
    for s in range(steps):
        sim.step(dt, resort=(s == 0))
    got = (st.positions(), st.previous_positions())
    want = (sim.pos, sim.prev)
    info = st.ctx.pipeline_info()
    st.close(); sim.close()
    return got, want, info


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "compat"])
def test_integration_edge_scene_matches_oracle(gpe, oracle, native):
    """Two fused steps (gpe_run) of the write-backs' verlet_one: a particle exactly at the mouse, results at the clamp's
    thresholds."""
    pos, rad, world, gravity, mouse, dt = integration_edge_scene()
    assert 1000 < len(pos) < 5000 and ((pos[:, 0] == F(mouse[0])) & (pos[:, 1] == F(mouse[1]))).sum() == 1
    got, want, info = _run_against_oracle(gpe, oracle, pos, rad, world, gravity, mouse, dt, 2,
                                          gpe.MODE_NATIVE if native else gpe.MODE_COMPAT,
                                          gpe._lib.FLAG_NATIVE_FORCE if native else 0)
    for g, w, what in zip(got, want, ("positions", "previous positions")):
        bad = ~_same(g, w).all(1)
        assert not bad.any(), "%s: %d differ, first %s: got %s want %s" % (
            what, bad.sum(), np.flatnonzero(bad)[:4], [[_hex(v) for v in p] for p in g[bad][:2]],
            [[_hex(v) for v in p] for p in w[bad][:2]])
    if native:
        assert info["native_steps"] == 2, info


@pytest.mark.gpu
def test_world_narrower_than_its_particles_matches_oracle(gpe, oracle):
    """A world one cell high and narrower than its largest particle (W - r < r: the order of the clamp's two compares
    decides).  native_configure accepts the scene, every particle lies in [0, W] x [0, H], and the first NATIVE step is
    exact: its write-back puts every particle at x = W - r < 0.  That is outside the NATIVE cell box, so the next NATIVE
    step refuses (GPE_ERR_STATE, a particle left the world box between steps); a context configured with those
    positions says GPE_REASON_OUT_OF_BOX and runs the compat kernels, exactly; so does a COMPAT context from the start."""
    L = gpe._lib
    rng = np.random.default_rng(5)
    world, gravity, dt = (1.0, 6.0), (2.5, -9.81), 1 / 60
    n = 41
    pos = _f(np.stack([rng.uniform(0, 1, n), rng.uniform(0, 6, n)], 1))
    rad = _f(rng.uniform(1.2, 3.0, n))
    rad[0] = 3.0                                                       # cell size 6.6: one cell holds the world
    mouse = (float(pos[3, 0]), float(pos[3, 1]))                       # exactly on a particle
    p = oracle.default_params(world[0], world[1], 3.0, gravity=gravity)
    p.mouse_pressed, p.mouse_x, p.mouse_y = 1, mouse[0], mouse[1]
    sim = oracle.Sim(pos, rad, p)
    sim.step(dt, resort=True)
    pos1, prev1, rad1 = sim.pos, sim.prev, sim.radius
    sim.step(dt)
    pos2, prev2 = sim.pos, sim.prev
    sim.close()
    assert (pos1[:, 0] == F(1.0) - rad1).all() and (pos1[:, 0] < 0).all()

    def state(at, radii, prev, mode, flags):
        st = gpe.State(at, radii, world=world, gravity=gravity, mode=mode, prev=prev, flags=flags)
        st.particles.mouse_click_callback(True, mouse)
        return st

    st = state(pos, rad, None, gpe.MODE_NATIVE, L.FLAG_NATIVE_FORCE)
    info = st.ctx.pipeline_info()
    assert (info["pipeline"], info["reason"]) == (L.PIPELINE_NATIVE, L.REASON_NONE), info
    st.run(dt, 1, resort_every=0, resort_first=True)
    assert _same(st.positions(), pos1).all() and _same(st.previous_positions(), prev1).all()
    assert st.ctx.pipeline_info()["native_steps"] == 1
    with pytest.raises(L.GpeError, match="left the world box") as err:
        st.update(dt)
        st.positions()
    assert err.value.status == L.GPE_ERR_STATE
    st.close()

    st = state(pos1, rad1, prev1, gpe.MODE_NATIVE, L.FLAG_NATIVE_FORCE)
    info = st.ctx.pipeline_info()
    assert (info["pipeline"], info["reason"]) == (L.PIPELINE_COMPAT, L.REASON_OUT_OF_BOX), info
    st.update(dt)
    assert _same(st.positions(), pos2).all() and _same(st.previous_positions(), prev2).all()
    st.close()

    st = state(pos, rad, None, gpe.MODE_COMPAT, 0)
    st.run(dt, 2, resort_every=0, resort_first=True)
    assert _same(st.positions(), pos2).all() and _same(st.previous_positions(), prev2).all()
    st.close()
