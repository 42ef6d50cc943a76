"""The numpy float32 restatement of the segment-against-particle function of gpe_cast_rays / gpe_query_segment
(include/gpe.h, csrc/k_ray.h): brute force, k rays x n particles, no binning, in the exact operation order of the header,
one binary32 rounding per operation, no FMA (numpy rounds every array operation once; its float32 divide and sqrt are
correctly rounded).  Ray blocks keep the memory bounded."""
import numpy as np

F32 = np.float32
U32 = np.uint32
RAY_MISS = 0xFFFFFFFF
UID_ABSENT = 0xFFFFFFFF


def touch_matrix(origins, ends, pos, rad):
    """(touched bool[k, n], t f32[k, n]); t is +0 where the origin lies inside, -0 is turned into +0, and t is
    meaningless where touched is False"""
    o = np.ascontiguousarray(origins, F32).reshape(-1, 2)
    e = np.ascontiguousarray(ends, F32).reshape(-1, 2)
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    with np.errstate(all="ignore"):
        a = np.abs(r)[None, :]
        rr = a * a
        alive = a > F32(0)
        dx = (e[:, 0] - o[:, 0])[:, None]
        dy = (e[:, 1] - o[:, 1])[:, None]
        fx = o[:, 0][:, None] - p[:, 0][None, :]
        fy = o[:, 1][:, None] - p[:, 1][None, :]
        A = dx * dx + dy * dy
        Cc = fx * fx + fy * fy
        inside = alive & (Cc <= rr)
        B = fx * dx + fy * dy
        u = (-B) / A
        qx = fx + u * dx
        qy = fy + u * dy
        h = qx * qx + qy * qy
        w = np.sqrt((rr - h) / A)
        t = (u - w).astype(F32)
        enters = alive & ~inside & (A > F32(0)) & (h <= rr) & (t >= F32(0)) & (t <= F32(1))
    touched = inside | enters
    t = np.where(inside, F32(0), t).astype(F32)
    t = np.where(t == F32(0), F32(0), t).astype(F32)          # -0 is delivered as +0
    return touched, t


def touches(o, e, c, r):
    """one pair: (touched, t or None)"""
    hit, t = touch_matrix([o], [e], [c], [r])
    return bool(hit[0, 0]), (F32(t[0, 0]) if hit[0, 0] else None)


def segment_set(a, b, pos, rad):
    """-> (index u32[m] ascending, t f32[m]) of everything the segment from a to b touches"""
    hit, t = touch_matrix([a], [b], pos, rad)
    idx = np.nonzero(hit[0])[0].astype(U32)
    return idx, t[0, idx]


def cast(origins, ends, pos, rad, uids=None, block=64):
    """-> dict(index u32[k], t f32[k], uid u32[k], pos f32[k, 2], radius f32[k], hits): the first hit of every ray -- the
    least t, the lowest index on a tie (the order of bits(t) << 32 | index; t >= +0, so its bits order as its values);
    RAY_MISS / UID_ABSENT / NaN for a miss"""
    o = np.ascontiguousarray(origins, F32).reshape(-1, 2)
    e = np.ascontiguousarray(ends, F32).reshape(-1, 2)
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    k, n = len(o), len(r)
    index = np.full(k, RAY_MISS, U32)
    t_out = np.full(k, np.nan, F32)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    for lo in range(0, k, block):
        hi = min(lo + block, k)
        if n == 0:
            break
        hit, t = touch_matrix(o[lo:hi], e[lo:hi], p, r)
        key = (np.ascontiguousarray(t).view(U32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
        key = np.where(hit, key, none)
        best = key.min(axis=1)
        got = best != none
        index[lo:hi] = np.where(got, (best & np.uint64(0xFFFFFFFF)).astype(U32), U32(RAY_MISS))
        tb = (best >> np.uint64(32)).astype(U32).view(F32)
        t_out[lo:hi] = np.where(got, tb, F32(np.nan))
    got = index != RAY_MISS
    safe = np.where(got, index, 0).astype(np.int64)
    out_pos = np.full((k, 2), np.nan, F32)
    out_rad = np.full(k, np.nan, F32)
    out_uid = np.full(k, UID_ABSENT, U32)
    if n:
        out_pos[got] = p[safe[got]]
        out_rad[got] = r[safe[got]]
        if uids is not None:
            out_uid[got] = np.asarray(uids, U32)[safe[got]]
    return dict(index=index, t=t_out, uid=out_uid, pos=out_pos, radius=out_rad, hits=int(got.sum()))


def distance_f64(o, e, c):
    """float64 geometry: the distance from each centre c[j] to each closed segment o[i] -> e[i]: f64[k, n]"""
    o = np.asarray(o, np.float64).reshape(-1, 2)
    e = np.asarray(e, np.float64).reshape(-1, 2)
    c = np.asarray(c, np.float64).reshape(-1, 2)
    d = (e - o)[:, None, :]
    f = c[None, :, :] - o[:, None, :]
    dd = (d * d).sum(axis=2)
    with np.errstate(all="ignore"):
        s = np.where(dd > 0, (f * d).sum(axis=2) / np.where(dd > 0, dd, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    near = o[:, None, :] + s[:, :, None] * d
    return np.sqrt(((c[None, :, :] - near) ** 2).sum(axis=2))
