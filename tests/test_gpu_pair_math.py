"""pair_response (gpu-physics-engine_amd/csrc/k_pair.h) at the edges of its arithmetic.

Every collide form of the NATIVE pipeline resolves its pairs in that one device function, whose square root and
quotients are hand-written sequences (v_sqrt_f32 / v_rcp_f32 plus corrections) rather than hipcc's IEEE ones, with a
prefilter and an equal-radius shortcut in front.  Whole-scene parity tests almost never land on the values where such
sequences break, so this file drives it directly:

* `reference_pair`: the oracle's pair (oracle/gpe_oracle.c, resolve_cell_collisions) restated in numpy float32, one
  correctly rounded operation at a time, subnormals kept.  Pinned to the C oracle bit for bit (CPU).
* tests/hip/pair_probe.hip: runs pair_response<true> and both pair_response<false> halves over seeded records of edge
  classes, 64 records per wave; every result must equal the reference bit for bit (GPU).
* Edge scenes through the real pipeline (GPE_FLAG_NATIVE_FORCE), one context and a two-context local group, against
  the oracle (GPU).
"""
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "pair_probe.hip")
PROBE_EXE = os.path.join(ROOT, "tests", "hip", "pair_probe")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wall"]

F = np.float32
EPS = F(1e-4)
STIFFNESS = F(0.6)
WAVE = 64


# ---------------------------------------------------------------------------------------------------------------------
# the reference


def reference_pair(p1x, p1y, p2x, p2y, r1, r2, stiffness, active):
    """oracle/gpe_oracle.c resolve_cell_collisions, one pair: float32 arrays in, (p1x, p1y, p2x, p2y, hit) out.
    numpy's float32 +, -, *, / and sqrt are correctly rounded and keep subnormals; nothing here is fused."""
    with np.errstate(all="ignore"):
        vx, vy = p1x - p2x, p1y - p2y
        distance = np.sqrt(vx * vx + vy * vy)
        radius_sum = r1 + r2
        sq_radius_sum = radius_sum * radius_sum
        hit = active & (sq_radius_sum > distance * distance) & (distance > EPS)
        depth = (r1 + r2) - distance
        cx = ((vx / distance) * depth) * stiffness
        cy = ((vy / distance) * depth) * stiffness
        inv1, inv2 = F(1.0) / r1, F(1.0) / r2
        w1 = inv1 / (inv1 + inv2)
        w2 = inv2 / (inv1 + inv2)
        return (np.where(hit, p1x + cx * w1, p1x), np.where(hit, p1y + cy * w1, p1y),
                np.where(hit, p2x - cx * w2, p2x), np.where(hit, p2y - cy * w2, p2y), hit)


# ---------------------------------------------------------------------------------------------------------------------
# edge classes: each returns a dict of float32 arrays p1x p1y p2x p2y r1 r2 st and a bool array active


def _f(a):
    return np.asarray(a, dtype=np.float32)


def _step(x, k):
    """x moved by k ulps (toward +inf for k > 0) -- for finite x of either sign, zero included."""
    x = _f(x)
    k = np.asarray(k, dtype=np.int64)
    b = x.view(np.int32).astype(np.int64)
    key = np.where(b < 0, -(b & 0x7FFFFFFF), b) + k               # monotone integer order of the floats
    out = np.where(key < 0, (-key) | -0x80000000, key)
    return out.astype(np.int64).astype(np.int32).view(np.float32)


def _ulp(x):
    x = np.abs(_f(x))
    return (_step(x, 1) - x).astype(np.float32)


def _pairs(p1x, p1y, p2x, p2y, r1, r2, st=None, active=None):
    n = len(_f(p1x))
    full = lambda v, d: _f(np.broadcast_to(d if v is None else v, (n,))).copy()
    return dict(p1x=full(p1x, 0), p1y=full(p1y, 0), p2x=full(p2x, 0), p2y=full(p2y, 0), r1=full(r1, 0),
                r2=full(r2, 0), st=full(st, STIFFNESS),
                active=np.ones(n, bool) if active is None else np.asarray(active, bool).copy())


def _cat(*ds):
    return {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, F(-1.0), F(1.0))


def _orient(rng, vx, vy):
    """Random signs and a random exchange of the axes."""
    n = len(vx)
    vx, vy = vx * _sign(rng, n), vy * _sign(rng, n)
    sw = rng.random(n) < 0.5
    return _f(np.where(sw, vy, vx)), _f(np.where(sw, vx, vy))


def _at_origin(rng, vx, vy):
    """p1 - p2 == v exactly: one of the two particles sits at 0."""
    n = len(vx)
    first = rng.random(n) < 0.5
    z = np.zeros(n, np.float32)
    return (np.where(first, vx, z), np.where(first, vy, z), np.where(first, z, -vx), np.where(first, z, -vy))


def _v_for_q(rng, qt):
    """(vx, vy) with fl(fl(vx^2) + fl(vy^2)) == qt wherever that can be arranged (returned mask)."""
    qt = _f(qt)
    with np.errstate(all="ignore"):
        vx = _step(np.sqrt(qt), -rng.integers(1, 9, len(qt)))
        a = vx * vx
        b = qt - a                                                    # exact (Sterbenz)
        vy = np.sqrt(np.maximum(b, F(0)))
        ok = (b >= 0) & (vx * vx + vy * vy == qt)
    return vx, _f(vy), ok


def _typical(rng, n):
    r1 = _f(rng.uniform(0.25, 3.0, n))
    r2 = np.where(rng.random(n) < 0.3, r1, _f(rng.uniform(0.25, 3.0, n)))
    p1x, p1y = _f(rng.uniform(0, 4000, n)), _f(rng.uniform(0, 4000, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    d = rng.uniform(0, 1.2, n) * (r1.astype(np.float64) + r2)
    p2x, p2y = _f(p1x - d * np.cos(ang)), _f(p1y - d * np.sin(ang))
    st = np.where(rng.random(n) < 0.25, _f(rng.random(n)), STIFFNESS)
    return _pairs(p1x, p1y, p2x, p2y, r1, r2, st, active=rng.random(n) < 0.9)


def _contact(rng, n):
    """q within a few ulps of rs^2, or of rs^2 * 1.000001f (the prefilter's bound)."""
    p1x, p1y = _f(rng.uniform(0, 64, n)), _f(rng.uniform(0, 64, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.exp(rng.uniform(np.log(2e-4), np.log(6.0), n))
    p2x, p2y = _f(p1x - d * np.cos(ang)), _f(p1y - d * np.sin(ang))
    vx, vy = p1x - p2x, p1y - p2y
    q = (vx * vx + vy * vy).astype(np.float64)
    fac = np.where(rng.random(n) < 0.5, 1.0, float(F(1.000001)))
    rs = np.sqrt(q / fac)
    equal = rng.random(n) < 0.4
    r1 = _f(np.where(equal, rs / 2, rs * rng.uniform(0.3, 0.7, n)))
    k = rng.integers(-6, 7, n)
    r2 = _step(_f(rs - r1), k)
    r1 = np.where(equal, _step(_f(rs / 2), k), r1)
    r2 = np.where(equal, r1, r2)
    return _pairs(p1x, p1y, p2x, p2y, r1, r2)


def _cutoff(rng, n):
    """distance within a few ulps of 0.0001f, q around 9.9e-9, q == 0."""
    m = n // 3
    dt = _step(np.full(m, EPS), rng.integers(-4, 5, m))
    ang = rng.uniform(0, 2 * np.pi, m)
    axis = rng.random(m) < 0.5
    ax, ay = _f(np.where(axis, dt, dt * np.cos(ang))), _f(np.where(axis, 0, dt * np.sin(ang)))
    ax, ay = _orient(rng, ax, ay)
    qt = _step(np.full(m, F(9.9e-9)), rng.integers(-6, 7, m))
    bx, by, ok = _v_for_q(rng, qt)
    bx, by = _orient(rng, bx, by)
    vx = np.concatenate([ax, bx, np.zeros(n - 2 * m, np.float32)])
    vy = np.concatenate([ay, by, np.zeros(n - 2 * m, np.float32)])
    p = _at_origin(rng, vx, vy)
    # q == 0 also away from the origin: coincident particles
    same = np.arange(n) >= 2 * m
    c = _f(rng.uniform(0, 100, (2, n)))
    p = [np.where(same, c[i % 2], p[i]) for i in range(4)]
    r1, r2 = _f(rng.uniform(0.25, 3.0, n)), _f(rng.uniform(0.25, 3.0, n))
    return _pairs(*p, r1, r2)


def _sqrt_hard(rng, n):
    """q == s^2 exactly, fl(s^2) and its neighbours, q nearest (s + ulp/2)^2, and q == a * b for neighbouring a < b
    (4^e (1 + 2^-23) and 4^e (1 - 2^-24), the only such products that are floats: where v_sqrt_f32 returns b for
    them, the residual q - a b is exactly 0 and decides)."""
    s = _f(np.exp(rng.uniform(np.log(1.1e-4), np.log(8.0), n)))
    kind = rng.integers(0, 5, n)
    short = _f(np.ldexp(rng.integers(2048, 4096, n), np.frexp(s)[1] - 12))      # 12 significant bits: s^2 exact
    s = np.where(kind == 0, short, s)
    s64, u64 = s.astype(np.float64), _ulp(s).astype(np.float64)
    e = np.frexp(s)[1]
    pow2 = _f(np.ldexp(1.0, e - 1))
    qt = np.select([kind <= 1, kind == 2, kind == 3, kind == 4],
                   [s64 * s64, s64 * s64, (s64 + u64 / 2) ** 2,
                    np.where(rng.random(n) < 0.5, pow2.astype(np.float64) * _step(pow2, 1),
                             pow2.astype(np.float64) * _step(pow2, -1))])
    qt = _f(qt)
    qt = np.where(kind == 2, _step(qt, np.where(rng.random(n) < 0.5, -1, 1)), qt)
    vx, vy, ok = _v_for_q(rng, qt)
    # q = s^2 also as (s, 0) directly
    direct = (kind == 0) & (rng.random(n) < 0.5)
    vx, vy = np.where(direct, np.where(kind == 0, short, vx), vx), np.where(direct, F(0), vy)
    vx, vy = _orient(rng, vx, vy)
    p = _at_origin(rng, vx, vy)
    rs = s64 * rng.uniform(0.999, 1.5, n)
    r1 = _f(rs * rng.uniform(0.2, 0.8, n))
    r2 = np.where(rng.random(n) < 0.4, r1, _f(rs - r1))
    return _pairs(*p, r1, r2)


def _quot_zero(rng, n):
    """A component of (+)0, the other of +-distance: axis-aligned pairs."""
    d = _f(np.exp(rng.uniform(np.log(1.2e-4), np.log(5.0), n)))
    c = _f(rng.uniform(0, 4000, n))
    o = _f(rng.uniform(0, 4000, n))
    vx, _ = _orient(rng, d, np.zeros(n, np.float32))
    vx = np.abs(vx) * _sign(rng, n)
    ax = rng.random(n) < 0.5
    p1a, p2a = o, _f(o - vx)                                          # the moving axis
    p1x, p2x = np.where(ax, p1a, c), np.where(ax, p2a, c)
    p1y, p2y = np.where(ax, c, p1a), np.where(ax, c, p2a)
    r1 = _f(rng.uniform(0.25, 3.0, n))
    r2 = np.where(rng.random(n) < 0.5, r1, _f(rng.uniform(0.25, 3.0, n)))
    return _pairs(p1x, p1y, p2x, p2y, r1, r2)


def _quot_tiny(rng, n):
    """|component| from 2^-149 to 2^-90 beside an ordinary one: quotients whose numerators are (nearly) subnormal."""
    t = _f(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-149, -90, n)))
    t = np.where(t == 0, F(np.ldexp(1.0, -149)), t)
    t = t * _sign(rng, n)
    y = _f(np.exp(rng.uniform(np.log(1.2e-4), np.log(4.0), n)))
    y = y * _sign(rng, n)
    first = rng.random(n) < 0.5
    p1x, p2x = np.where(first, t, F(0)), np.where(first, F(0), -t)
    yc = _f(rng.uniform(0.5, 8.0, n))
    p1y, p2y = yc, _f(yc - y)
    sw = rng.random(n) < 0.5
    p1x, p1y = np.where(sw, p1y, p1x), np.where(sw, p1x, p1y)
    p2x, p2y = np.where(sw, p2y, p2x), np.where(sw, p2x, p2y)
    d = np.abs(p1y - p2y).astype(np.float64) + np.abs(p1x - p2x)
    r1 = _f(np.where(rng.random(n) < 0.5, 0.5, rng.uniform(0.25, 3.0, n)))
    r1 = np.maximum(r1, _f(d * 0.6))
    r2 = np.where(rng.random(n) < 0.5, r1, _f(np.maximum(rng.uniform(0.25, 3.0, n), d * 0.6)))
    out = _pairs(p1x, p1y, p2x, p2y, r1, r2)
    # the case the arithmetic was first emulated with: A = (0, 0.5), B = (0x1.0cp-137, 0.5137), r = 0.5
    out["p1x"][0], out["p1y"][0], out["p2x"][0], out["p2y"][0] = 0.0, 0.5, np.ldexp(0x10C / 256.0, -137), 0.5137
    out["r1"][0] = out["r2"][0] = 0.5
    return out


def _quot_mid(rng, n, tries=65):
    """Quotients v / distance within a hair of a rounding midpoint (searched in float64 over neighbouring vx)."""
    p1x, p1y = _f(rng.uniform(0, 16, n)), _f(rng.uniform(0, 16, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.exp(rng.uniform(np.log(2e-4), np.log(5.0), n))
    p2x0, p2y = _f(p1x - d * np.cos(ang)), _f(p1y - d * np.sin(ang))
    k = np.arange(tries) - tries // 2
    p2x = _step(np.repeat(p2x0[:, None], tries, 1), np.broadcast_to(k, (n, tries)))
    vx, vy = p1x[:, None] - p2x, (p1y - p2y)[:, None]
    dist = np.sqrt(vx * vx + vy * vy).astype(np.float64)

    def off(num):
        qq = num.astype(np.float64) / dist
        u = _ulp(_f(qq)).astype(np.float64)
        with np.errstate(all="ignore"):
            fr = np.abs(qq) / np.where(u > 0, u, 1.0)
        return np.abs(fr - np.floor(fr) - 0.5)

    score = np.minimum(off(vx), off(np.broadcast_to(vy, vx.shape)))
    best = np.argmin(score, axis=1)
    p2x = p2x[np.arange(n), best]
    r1 = _f(rng.uniform(0.25, 3.0, n))
    r2 = np.where(rng.random(n) < 0.5, r1, _f(rng.uniform(0.25, 3.0, n)))
    r1 = np.maximum(r1, _f(d * 0.6))
    r2 = np.maximum(r2, _f(d * 0.6))
    return _pairs(p1x, p1y, p2x, p2y, r1, r2)


def _special_radii():
    tiny = np.ldexp(1.0, -140)
    base = [0.0, -0.0, tiny, -tiny, 1e-38, 2.9e-39, 5e-39, 6e-39, 1e-30, 1e30, 0.5, -0.5, 1.0, 2.0,
            np.inf, -np.inf, np.nan, 3e38, 1e-45]
    out = []
    for b in base:
        b = F(b)
        out.append(b)
        if np.isfinite(b):
            out += [_step(b, -1), _step(b, 1)]
    return _f(out)


def _radii(rng, n):
    """Radii equal, one ulp apart, of opposite sign, zero, subnormal, 1e-30 / 1e30 and their neighbours, with
    1/r1 + 1/r2 overflowing, infinite and NaN -- beside ordinary ones."""
    sp = _special_radii()
    r1 = sp[rng.integers(0, len(sp), n)]
    how = rng.integers(0, 6, n)
    typ = _f(rng.uniform(0.25, 3.0, n))
    r2 = np.select([how == 0, how == 1, how == 2, how == 3, how == 4],
                   [r1, _step(np.nan_to_num(r1), np.where(rng.random(n) < 0.5, -1, 1)), -r1, typ,
                    sp[rng.integers(0, len(sp), n)]], typ)
    sw = rng.random(n) < 0.5
    r1, r2 = _f(np.where(sw, r2, r1)), _f(np.where(sw, r1, r2))
    with np.errstate(all="ignore"):
        rs = np.abs(r1.astype(np.float64) + r2)
    d = np.where(np.isfinite(rs) & (rs > 2e-4) & (rs < 1e4), rs * rng.uniform(0.02, 1.1, n),
                 np.exp(rng.uniform(np.log(2e-4), np.log(5.0), n)))
    p1x, p1y = _f(rng.uniform(0, 100, n)), _f(rng.uniform(0, 100, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    return _pairs(p1x, p1y, _f(p1x - d * np.cos(ang)), _f(p1y - d * np.sin(ang)), r1, r2)


def _neg_zero(rng, n):
    """Pairs that share a coordinate of 0 where at least one of the two zeros is -0: (-0, -0), (-0, +0), (+0, -0);
    radii and stiffness of both signs, so that the weights and the corrections take both signs."""
    kind = rng.integers(0, 3, n)
    z1 = np.where(kind == 2, F(0.0), F(-0.0))
    z2 = np.where(kind == 1, F(0.0), F(-0.0))
    c = _f(rng.uniform(0, 100, n))
    y = _f(rng.uniform(0.05, 2.0, n)) * _sign(rng, n)
    o1, o2 = c, _f(c - y)
    ax = rng.random(n) < 0.5
    p1x, p1y = np.where(ax, z1, o1), np.where(ax, o1, z1)
    p2x, p2y = np.where(ax, z2, o2), np.where(ax, o2, z2)
    r1 = _f(rng.uniform(0.6, 3.0, n)) * np.where(rng.random(n) < 0.3, F(-1), F(1))
    r2 = np.where(rng.random(n) < 0.4, r1, _f(rng.uniform(0.6, 3.0, n)) * np.where(rng.random(n) < 0.3, F(-1), F(1)))
    st = STIFFNESS * np.where(rng.random(n) < 0.25, F(-1), F(1))
    return _pairs(p1x, p1y, p2x, p2y, r1, r2, st)


def _garbage(rng, n):
    bits = rng.integers(0, 2 ** 32, (7, n), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return _pairs(*bits, active=np.zeros(n, bool))


def _waves_without_candidates(rng, n):
    w = n // WAVE
    out = _typical(rng, n)
    far = rng.random(w) < 0.5                                          # half: pairs far apart; half: nothing active
    farl = np.repeat(far, WAVE)
    out["p2x"] = np.where(farl, out["p1x"] - F(7.0) * (out["r1"] + out["r2"]), out["p2x"])
    out["active"] = np.where(farl, True, False)
    g = _garbage(rng, n)
    for k in ("p1x", "p1y", "p2x", "p2y", "r1", "r2", "st"):
        out[k] = np.where(farl, out[k], g[k])
    return out


def _one_general_lane(rng, n):
    """63 colliding lanes of equal radii and one of unequal radii (the general weights' wave-uniform branch)."""
    out = _typical(rng, n)
    out["active"][:] = True
    r = _f(rng.uniform(0.25, 3.0, n // WAVE))
    out["r1"] = out["r2"] = np.repeat(r, WAVE)
    lane = rng.integers(0, WAVE, n // WAVE) + np.arange(0, n, WAVE)
    out["r2"] = out["r2"].copy()
    out["r2"][lane] = _f(rng.uniform(0.25, 3.0, len(lane)))
    d = rng.uniform(0, 0.95, n) * (out["r1"].astype(np.float64) + out["r2"])
    ang = rng.uniform(0, 2 * np.pi, n)
    out["p2x"], out["p2y"] = _f(out["p1x"] - d * np.cos(ang)), _f(out["p1y"] - d * np.sin(ang))
    return out


def _sparse_masks(rng, n):
    """Alternating and single active lanes; the inactive lanes hold garbage and must come back unchanged."""
    w = n // WAVE
    lane = np.arange(n) % WAVE
    kind = np.repeat(rng.integers(0, 3, w), WAVE)
    single = np.repeat(rng.integers(0, WAVE, w), WAVE)
    active = np.select([kind == 0, kind == 1], [lane % 2 == 0, lane % 2 == 1], lane == single)
    out = _one_general_lane(rng, n) if rng.random() < 0.5 else _typical(rng, n)
    g = _garbage(rng, n)
    for k in ("p1x", "p1y", "p2x", "p2y", "r1", "r2", "st"):
        out[k] = np.where(active, out[k], g[k])
    out["active"] = active
    return out


CLASSES = {
    "typical": _typical, "contact": _contact, "cutoff": _cutoff, "sqrt": _sqrt_hard, "quot_zero": _quot_zero,
    "quot_tiny": _quot_tiny, "quot_midpoint": _quot_mid, "radii": _radii, "neg_zero": _neg_zero,
    "no_candidates": _waves_without_candidates, "one_general_lane": _one_general_lane, "sparse_masks": _sparse_masks,
}


def make_records(per_class, seed=2024):
    """All classes, per_class records each (a multiple of 64: every wave holds one class), then `mixed`: the
    records of the first nine classes shuffled together.  Returns (records dict, class names, class index per record)."""
    rng = np.random.default_rng(seed)
    assert per_class % WAVE == 0
    parts = [CLASSES[name](rng, per_class) for name in CLASSES]
    names = list(CLASSES)
    pool = _cat(*parts[:9])
    pick = rng.permutation(len(pool["r1"]))[:per_class]
    parts.append({k: v[pick] for k, v in pool.items()})
    names.append("mixed")
    cls = np.repeat(np.arange(len(names)), per_class)
    return _cat(*parts), names, cls


def reference_of(rec):
    return reference_pair(rec["p1x"], rec["p1y"], rec["p2x"], rec["p2y"], rec["r1"], rec["r2"], rec["st"],
                          rec["active"])


def _same(a, b):
    """Bit-equal, or both NaN."""
    a, b = _f(a), _f(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference against the C oracle


def _oracle_one_pair(oracle, rec, i):
    """Post-collision positions of the pair alone in an oracle scene, and how often the oracle resolved it (the number
    of cells the two particles share)."""
    pos = np.array([[rec["p1x"][i], rec["p1y"][i]], [rec["p2x"][i], rec["p2y"][i]]], np.float32)
    rad = np.array([rec["r1"][i], rec["r2"][i]], np.float32)
    p = oracle.default_params(1e6, 1e6, 1.0)
    p.stiffness = float(rec["st"][i])
    sim = oracle.Sim(pos, rad, p)
    sim.grid_build()
    ids = sim.cell_ids.reshape(2, -1)
    used = [c[c != 0xFFFFFFFF] for c in ids]
    shared = sum(int((used[1] == c).sum()) for c in used[0])
    sim.step(1.0 / 60.0)
    prev = sim.prev
    sim.close()
    return prev, shared


def test_reference_pair_equals_the_oracle(oracle):
    """At least 2 000 pairs from every class, each in an oracle scene of its own: after one step the oracle's previous
    positions (the positions after the collision pass) equal the reference applied as often as the oracle resolved
    the pair, bit for bit.  Pins the numpy restatement that the GPU tests trust."""
    rec, names, cls = make_records(64 * 8, seed=7)
    rng = np.random.default_rng(8)
    take = []
    for c in range(len(names)):
        idx = np.flatnonzero((cls == c) & rec["active"])
        take.append(rng.choice(idx, min(len(idx), 260), replace=False))
    take = np.concatenate(take)
    take = np.unique(np.concatenate([take, [int(np.flatnonzero(cls == names.index("quot_tiny"))[0])]]))
    assert len(take) >= 2000
    sub = {k: v[take] for k, v in rec.items()}
    threads = oracle.get_threads()
    oracle.set_threads(1)
    try:
        got, shared = zip(*(_oracle_one_pair(oracle, sub, i) for i in range(len(take))))
    finally:
        oracle.set_threads(threads)
    got, shared = np.stack(got), np.array(shared)
    cur = dict(sub)
    hits = np.zeros(len(take), bool)
    for k in range(1, shared.max() + 1):                               # the pair, resolved `shared` times
        cur["active"] = sub["active"] & (shared >= k)
        a, b, c, d, h = reference_of(cur)
        cur = dict(cur, p1x=a, p1y=b, p2x=c, p2y=d)
        hits |= h
    want = np.stack([cur["p1x"], cur["p1y"], cur["p2x"], cur["p2y"]], 1).reshape(-1, 2, 2)
    bad = ~_same(got, want).all(axis=(1, 2))
    assert hits.sum() > 1000 and (shared >= 1).sum() > 1500
    assert not bad.any(), "%d of %d pairs differ from the oracle, first %s" % (
        bad.sum(), len(take), [names[c] for c in cls[take][bad][:5]])
    # the case the kernel's quotient was first emulated with: one resolution moves A.x to -0x1.69c4p-133 (at the
    # origin corner both particles also sit in the cell left of x = 0, so the oracle's scene resolves them twice)
    i = int(np.flatnonzero(take == np.flatnonzero(cls == names.index("quot_tiny"))[0])[0])
    once = reference_of({k: v[i:i + 1] for k, v in sub.items()})
    assert once[0][0] == F(-np.ldexp(0x169C4 / 65536.0, -133)) and shared[i] == 2


def build_probe():
    deps = [PROBE_SRC, os.path.join(CSRC, "k_pair.h"), os.path.join(CSRC, "gpe_internal.h")]
    if not os.path.exists(PROBE_EXE) or any(os.path.getmtime(d) > os.path.getmtime(PROBE_EXE) for d in deps):
        r = subprocess.run([HIPCC] + PROBE_FLAGS + ["-I", CSRC, PROBE_SRC, "-o", PROBE_EXE], capture_output=True,
                           text=True)
        assert r.returncode == 0, "pair_probe.hip does not compile:\n" + r.stdout + r.stderr
    return PROBE_EXE


def test_pair_probe_compiles_for_gfx950():
    exe = build_probe()
    with open(exe, "rb") as f:
        assert b"gfx950" in f.read()


def test_pair_arithmetic_has_one_home():
    """The hand-written square root and reciprocal appear in k_pair.h only: every collide form runs that copy, the
    one the probe checks."""
    hits = {}
    for path in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
        src = open(path).read()
        for b in ("__builtin_amdgcn_rcpf", "__builtin_amdgcn_sqrtf"):
            if b in src:
                hits.setdefault(b, []).append(os.path.basename(path))
    assert hits == {"__builtin_amdgcn_rcpf": ["k_pair.h"], "__builtin_amdgcn_sqrtf": ["k_pair.h"]}, hits


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the probe


def _hex(x):
    return float(x).hex()


def run_probe(rec, tmp_path):
    exe = build_probe()
    n = len(rec["r1"])
    words = np.stack([rec[k] for k in ("p1x", "p1y", "p2x", "p2y", "r1", "r2", "st")], 1).view(np.uint32)
    words = np.concatenate([words, rec["active"].astype(np.uint32)[:, None]], 1)
    src, dst = str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(words).tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(dst, np.uint32).reshape(n, 11)
    return out


@pytest.mark.gpu
def test_pair_response_equals_ieee_reference_on_edge_classes(tmp_path):
    rec, names, cls = make_records(64 * 4096)                         # 262 144 records per class
    out = run_probe(rec, tmp_path)
    fl = out.view(np.float32)
    a, b, c, d, hit = reference_of(rec)
    want = np.stack([a, b, c, d], 1)
    ok = _same(fl[:, 0:4], want).all(1) & (out[:, 4] == hit)
    ok_a = _same(fl[:, 5:7], want[:, 0:2]).all(1) & (out[:, 7] == hit)
    ok_b = _same(fl[:, 8:10], want[:, 2:4]).all(1) & (out[:, 10] == hit)
    lines = []
    for k, name in enumerate(names):
        m = cls == k
        nb, na, nbb = int((~ok & m).sum()), int((~ok_a & m).sum()), int((~ok_b & m).sum())
        if nb or na or nbb:
            lines.append("%-16s both %6d  half p1 %6d  half p2 %6d  of %d (hits %d)" % (name, nb, na, nbb, m.sum(),
                                                                                       int(hit[m].sum())))
    bad = np.flatnonzero(~(ok & ok_a & ok_b))
    for i in bad[:8]:
        lines.append("  [%s] p1 (%s, %s) p2 (%s, %s) r (%s, %s) st %s active %d: got %s hit %d, halves %s %s, want %s hit %d" % (
            names[cls[i]], *[_hex(rec[k][i]) for k in ("p1x", "p1y", "p2x", "p2y", "r1", "r2", "st")], rec["active"][i],
            [_hex(v) for v in fl[i, 0:4]], out[i, 4], [_hex(v) for v in fl[i, 5:7]], [_hex(v) for v in fl[i, 8:10]],
            [_hex(v) for v in want[i]], hit[i]))
    assert len(bad) == 0, "pair_response differs from the IEEE reference:\n" + "\n".join(lines)
    for k, name in enumerate(names):                                   # every class reached the arithmetic
        assert hit[cls == k].sum() > 0 or name == "no_candidates", name


# ---------------------------------------------------------------------------------------------------------------------
# GPU: edge scenes through the pipeline, against the oracle


def isolated_pair_scene(seed=3):
    """Thousands of isolated pairs from the edge classes, each at a site of its own (no two pairs share a cell or touch),
    built in world coordinates so that the coordinates produce the wanted v: contact within ulps of rs^2 and of the
    prefilter's bound, distances at the 0.0001 cut-off, axis-aligned pairs, quotients near a rounding midpoint, radii
    one ulp apart -- and an origin corner: pairs on the lines x = 0 and y = 0 whose coordinates run down to
    2^-140, of radius 0.5 and of tiny radii.  Returns (pos, rad, world)."""
    rng = np.random.default_rng(seed)
    spacing, cols, rows = F(16.0), 60, 50
    world = (float(spacing) * (cols + 1), float(spacing) * (rows + 1))
    gx, gy = np.meshgrid(np.arange(1, cols + 1), np.arange(1, rows + 1))
    sites = (np.stack([gx.ravel(), gy.ravel()], 1) * spacing).astype(np.float32)
    sites += _f(rng.uniform(-2, 2, sites.shape))
    n = len(sites)
    kind = rng.integers(0, 6, n)
    p1x, p1y = sites[:, 0].copy(), sites[:, 1].copy()
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.exp(rng.uniform(np.log(9e-5), np.log(2.5), n))
    d = np.where(kind == 2, float(EPS) * (1 + rng.integers(-30, 31, n) * 2.0 ** -20), d)   # the cut-off
    axis = (kind == 3) | (rng.random(n) < 0.1)                                               # axis-aligned
    cx, cy = np.where(axis, np.round(np.cos(ang)), np.cos(ang)), np.where(axis, 0, np.sin(ang))
    cx = np.where(axis & (cx == 0), 1.0, cx)
    sw = axis & (rng.random(n) < 0.5)
    cx, cy = np.where(sw, cy, cx), np.where(sw, cx, cy)
    p2x, p2y = _f(p1x - d * cx), _f(p1y - d * cy)
    # quotients near a rounding midpoint: the best of 33 neighbouring p2x
    mid = kind == 4
    if mid.any():
        m = _quot_mid(rng, int(mid.sum()), tries=33)
        p1x[mid], p1y[mid] = m["p1x"] + sites[mid, 0] - F(8), m["p1y"] + sites[mid, 1] - F(8)
        p2x[mid], p2y[mid] = m["p2x"] + sites[mid, 0] - F(8), m["p2y"] + sites[mid, 1] - F(8)
    vx, vy = p1x - p2x, p1y - p2y
    q = (vx * vx + vy * vy).astype(np.float64)
    rs = np.where(kind == 1, np.sqrt(q / np.where(rng.random(n) < 0.5, 1.0, float(F(1.000001)))),
                  np.maximum(np.sqrt(q), 2e-4) * rng.uniform(0.8, 1.6, n))
    rs = np.minimum(rs, 3.0)
    r1 = _f(rs * rng.uniform(0.3, 0.7, n))
    r2 = _step(_f(rs - r1), np.where(kind == 1, rng.integers(-6, 7, n), 0))
    eq = (kind == 5) | (rng.random(n) < 0.3)
    r2 = np.where(eq, _step(r1, np.where(kind == 5, rng.integers(-1, 2, n), 0)), r2)
    r1, r2 = np.maximum(r1, F(1e-4)), np.maximum(r2, F(1e-4))
    # the origin corner: x = 0 and tiny x (down to 2^-140) beside ordinary y, and the same along y = 0; radius 0.5 or
    # tiny
    k = 600
    t = _f(np.ldexp(rng.uniform(1.0, 2.0, (2, k)), rng.integers(-140, -90, (2, k))))
    t[:, rng.random(k) < 0.25] = 0.0
    t[0, :4], t[1, :4] = [0.0, 0.0, 0.0, np.ldexp(0x10C / 256.0, -137)], [0.0, np.ldexp(1.0, -140), 1e-30, 0.0]
    oy = _f((np.arange(k) % 300) * 2.5 + 3.0)
    dy = _f(rng.uniform(0.1, 0.99, k))
    dy[0] = 0.0137
    orad = np.where(np.arange(k) % 3 == 2, _f(rng.uniform(2e-4, 0.01, k)), F(0.5))
    dy = np.where(orad < 0.5, _f(orad * rng.uniform(0.5, 1.9, k)), dy)
    ox1, oy1, ox2, oy2 = t[0], oy, t[1], _f(oy + dy)
    few = np.arange(k) >= k // 2                                      # ... and as many on y = 0
    ox1, oy1, ox2, oy2 = (np.where(few, oy1 + F(8.0), ox1), np.where(few, t[0], oy1),
                          np.where(few, oy2 + F(8.0), ox2), np.where(few, t[1], oy2))
    corner_rad = np.repeat(orad, 2)
    cp = np.stack([np.stack([ox1, oy1], 1), np.stack([ox2, oy2], 1)], 1).reshape(-1, 2)
    pos = np.concatenate([np.stack([np.stack([p1x, p1y], 1), np.stack([p2x, p2y], 1)], 1).reshape(-1, 2), cp])
    rad = np.concatenate([np.stack([r1, r2], 1).ravel(), corner_rad])
    # keep the grid of sites clear of the corner column: drop sites within 10 of either axis
    keep = np.ones(len(pos), bool)
    near = (sites[:, 0] < 10) | (sites[:, 1] < 10)
    keep[:2 * n] = ~np.repeat(near, 2)
    pos, rad = _f(pos[keep]), _f(rad[keep])
    pos = np.clip(pos, 0, np.array(world, np.float32))
    return pos, rad, world


def crushed_blob_scene(seed, negative=False):
    """Blobs of 2-3, 4-8, 9-16, 17-64, 65-1024 and over 1024 particles each pressed into one cell, radii 0.05 .. 0.5
    (some negative with `negative`), over a sparse background: every cell form with general weights."""
    rng = np.random.default_rng(seed)
    # with negative radii the Verlet clamp lets a particle past the wall, which the native pipeline refuses: that
    # scene sits in the middle of a larger world, out of the walls' reach
    off = F(48.0) if negative else F(0.0)
    world = (64.0 + 2 * float(off),) * 2
    sizes = [2, 3, 4, 6, 8, 9, 12, 16, 17, 40, 64, 65, 300, 1024, 1300]
    parts = [_f(rng.uniform(0, 64, (600, 2)))]
    for i, k in enumerate(sizes):
        c = np.array([4.4 + 7.7 * (i % 8), 6.6 + 16.5 * (i // 8) + 2.2 * (i % 3)], np.float32)
        parts.append(_f(c + rng.uniform(0.05, 1.05, (k, 2))))
    pos = (np.concatenate(parts) + off).astype(np.float32)
    rad = _f(rng.uniform(0.05, 0.5, len(pos)))
    if negative:
        rad = np.where(rng.random(len(pos)) < 0.3, -rad, rad)
    rad[0] = 0.5
    return pos, _f(rad), world


def negative_zero_wall_scene(seed=5):
    """Cells of 4 to 16 members (lane groups and DPP rows, which resolve each pair twice, one half per lane) on the wall
    x = 0, their members at x = -0 (and some at +0), radii 0.3 .. 0.5, over a sparse background."""
    rng = np.random.default_rng(seed)
    k = 60
    world = (40.0, 1.1 * 3 * k + 4.0)
    parts, zeros = [_f(np.stack([rng.uniform(2, 38, 200), rng.uniform(1, world[1] - 1, 200)], 1))], []
    for j in range(k):
        m = int(rng.integers(4, 17))
        lo = 1.1 * (3 * j + 1)
        y = _f(lo + rng.uniform(0.05, 1.05, m))
        x = np.where(rng.random(m) < (0.5 if j % 4 == 0 else 0.0), F(0.0), F(-0.0))
        parts.append(np.stack([x, y], 1).astype(np.float32))
    pos = np.concatenate(parts).astype(np.float32)
    rad = _f(rng.uniform(0.3, 0.5, len(pos)))
    rad[0] = 0.5
    return pos, rad, world


def _state_vs_oracle(gpe, oracle, pos, rad, world, mode, steps, what):
    flags = gpe._lib.FLAG_NATIVE_FORCE if mode == gpe.MODE_NATIVE else 0
    st = gpe.State(pos, rad, world=world, mode=mode, flags=flags)
    sim = oracle.Sim(pos, rad, oracle.default_params(world[0], world[1], float(rad.max())))
    for s in range(steps):
        st.update(1 / 60, resort=(s == 0)); sim.step(1 / 60, resort=(s == 0))
        got, want = st.previous_positions(), sim.prev
        bad = ~_same(got, want).all(1)
        assert not bad.any(), "%s, step %d: %d particles' collision results differ, first %s: got %s want %s" % (
            what, s, bad.sum(), np.flatnonzero(bad)[:4], [[_hex(v) for v in p] for p in got[bad][:2]],
            [[_hex(v) for v in p] for p in want[bad][:2]])
        assert _same(st.positions(), sim.pos).all(), "%s, step %d: positions" % (what, s)
    info = st.ctx.pipeline_info()
    st.close(); sim.close()
    if mode == gpe.MODE_NATIVE:
        assert info["native_steps"] == steps, info
    return info


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "compat"])
def test_isolated_edge_pairs_match_oracle(gpe, oracle, native):
    pos, rad, world = isolated_pair_scene()
    assert len(pos) > 5000
    _state_vs_oracle(gpe, oracle, pos, rad, world, gpe.MODE_NATIVE if native else gpe.MODE_COMPAT, 4,
                     "isolated edge pairs (%s)" % ("native" if native else "compat"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,negative", [(11, False), (12, False), (13, True)])
def test_crushed_blobs_of_mixed_radii_match_oracle(gpe, oracle, seed, negative):
    pos, rad, world = crushed_blob_scene(seed, negative)
    info = _state_vs_oracle(gpe, oracle, pos, rad, world, gpe.MODE_NATIVE, 3, "crushed blobs, seed %d" % seed)
    assert info["overflow_tiles"] > 0, info                           # the piles run over the direct-slot windows


@pytest.mark.gpu
def test_negative_zero_wall_cells_match_oracle(gpe, oracle):
    pos, rad, world = negative_zero_wall_scene()
    assert (np.signbit(pos[:, 0]) & (pos[:, 0] == 0)).sum() > 300
    _state_vs_oracle(gpe, oracle, pos, rad, world, gpe.MODE_NATIVE, 3, "cells at x = -0")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["isolated", "blobs", "blobs_negative", "negative_zero"])
def test_edge_scenes_local_group_equals_single_context(gpe, scene):
    """The same scenes as a two-context local group (order-key builds of every cell form): bit-identical to one
    context."""
    lg = importlib.import_module("gpu-physics-engine_amd.local_group")
    if scene == "isolated":
        pos, rad, world = isolated_pair_scene()
    elif scene == "negative_zero":
        pos, rad, world = negative_zero_wall_scene()
    else:
        pos, rad, world = crushed_blob_scene(12 if scene == "blobs" else 13, scene == "blobs_negative")
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
