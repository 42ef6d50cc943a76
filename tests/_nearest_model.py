"""The numpy float32 restatement of gpe_query_nearest (include/gpe.h, csrc/k_nearest.hip): brute force, k points x n
particles, no binning, in the exact operation order of the header, one binary32 rounding per operation, no FMA (numpy
rounds every array operation once), and a stable sort on bits(d2) << 32 | index.  Point blocks keep the memory bounded."""
import numpy as np

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
NEAREST_NONE = 0xFFFFFFFF
UID_ABSENT = 0xFFFFFFFF
MAX_M = 64
_NO_KEY = U64(0xFFFFFFFFFFFFFFFF)


def dist2_matrix(points, pos):
    """d2 f32[k, n] = (p.x-x)*(p.x-x) + (p.y-y)*(p.y-y)"""
    q = np.ascontiguousarray(points, F32).reshape(-1, 2)
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        dx = p[None, :, 0] - q[:, 0][:, None]
        dy = p[None, :, 1] - q[:, 1][:, None]
        return (dx * dx + dy * dy).astype(F32)


def candidates(points, pos, max_distance):
    """bool[k, n]: d2 <= rr with rr = max_distance * max_distance in float32 (a NaN compares false)"""
    md = F32(max_distance)
    with np.errstate(all="ignore"):
        rr = md * md
        return dist2_matrix(points, pos) <= rr


def nearest(points, pos, m=1, max_distance=np.inf, rad=None, uids=None, block=64):
    """-> dict(count u32[k], index u32[k, m], dist2 f32[k, m], uid u32[k, m], pos f32[k, m, 2], radius f32[k, m], found):
    per point the min(m, candidates) candidates with the least bits(d2) << 32 | index, ascending; NEAREST_NONE /
    UID_ABSENT / NaN in the slots past count"""
    assert 1 <= m <= MAX_M
    q = np.ascontiguousarray(points, F32).reshape(-1, 2)
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    k, n = len(q), len(p)
    md = F32(max_distance)
    count = np.zeros(k, U32)
    index = np.full((k, m), NEAREST_NONE, U32)
    d2_out = np.full((k, m), np.nan, F32)
    take = min(m, n)
    for lo in range(0, k, block):
        if n == 0:
            break
        hi = min(lo + block, k)
        d2 = dist2_matrix(q[lo:hi], p)
        with np.errstate(all="ignore"):
            ok = d2 <= md * md
        key = (np.ascontiguousarray(d2).view(U32).astype(U64) << U64(32)) | np.arange(n, dtype=U64)[None, :]
        key = np.where(ok, key, _NO_KEY)
        order = np.argsort(key, axis=1, kind="stable")[:, :take]
        best = np.take_along_axis(key, order, axis=1)
        got = best != _NO_KEY
        count[lo:hi] = got.sum(axis=1)
        index[lo:hi, :take] = np.where(got, (best & U64(0xFFFFFFFF)).astype(U32), U32(NEAREST_NONE))
        d2_out[lo:hi, :take] = np.where(got, (best >> U64(32)).astype(U32).view(F32), F32(np.nan))
    got = index != NEAREST_NONE
    safe = np.where(got, index, 0).astype(np.int64)
    out_pos = np.full((k, m, 2), np.nan, F32)
    out_rad = np.full((k, m), np.nan, F32)
    out_uid = np.full((k, m), UID_ABSENT, U32)
    if n:
        out_pos[got] = p[safe[got]]
        if rad is not None:
            out_rad[got] = np.ascontiguousarray(rad, F32).reshape(-1)[safe[got]]
        if uids is not None:
            out_uid[got] = np.asarray(uids, U32)[safe[got]]
    return dict(count=count, index=index, dist2=d2_out, uid=out_uid, pos=out_pos, radius=out_rad, found=int(count.sum()))


def nearest_f64(points, pos, m):
    """float64 brute force: index i64[k, min(m, n)] ordered by (d2, index), and those d2 -- for inputs whose d2 is exact
    in both precisions"""
    q = np.asarray(points, np.float64).reshape(-1, 2)
    p = np.asarray(pos, np.float64).reshape(-1, 2)
    d2 = ((p[None, :, :] - q[:, None, :]) ** 2).sum(axis=2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :m]         # stable: the lowest index first among equal d2
    return order, np.take_along_axis(d2, order, axis=1)
