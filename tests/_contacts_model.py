"""The numpy float32 restatement of gpe_query_contacts (include/gpe.h): brute force over all pairs, in the exact
operation order of the header -- dx = xi - xj, dy = yi - yj, q = dx*dx + dy*dy, rs = ri + rj, contact when
q < rs*rs, overlap = rs - sqrt(q) -- one binary32 rounding per operation, no FMA (numpy rounds every array operation
once, and its float32 sqrt is correctly rounded).  Row blocks keep the memory bounded."""
import numpy as np

F32 = np.float32


def contact_matrix_rows(pos, rad, lo, hi):
    """(hit, q, rs) of rows lo .. hi-1 against every particle: hit[i - lo, j], the diagonal excluded"""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32).reshape(-1)
    with np.errstate(all="ignore"):
        dx = p[lo:hi, 0][:, None] - p[:, 0][None, :]
        dy = p[lo:hi, 1][:, None] - p[:, 1][None, :]
        q = dx * dx + dy * dy
        rs = r[lo:hi][:, None] + r[None, :]
        hit = q < rs * rs
    hit[np.arange(hi - lo), np.arange(lo, hi)] = False
    return hit, q, rs


def contacts(pos, rad, block=512):
    """-> (count, degree u32[n], a u32[count], b u32[count], overlap f32[count]); pairs a < b, ascending by a then b"""
    n = len(np.ascontiguousarray(rad).reshape(-1))
    degree = np.zeros(n, np.uint32)
    aa, bb, ov = [], [], []
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        hit, q, rs = contact_matrix_rows(pos, rad, lo, hi)
        degree[lo:hi] = hit.sum(axis=1)
        i, j = np.nonzero(hit)                              # row-major: ascending i, then ascending j
        up = j > i + lo
        i, j = i[up], j[up]
        aa.append((i + lo).astype(np.uint32))
        bb.append(j.astype(np.uint32))
        with np.errstate(all="ignore"):
            ov.append((rs[i, j] - np.sqrt(q[i, j])).astype(F32))
    a = np.concatenate(aa) if aa else np.zeros(0, np.uint32)
    b = np.concatenate(bb) if bb else np.zeros(0, np.uint32)
    o = np.concatenate(ov) if ov else np.zeros(0, F32)
    return int(a.size), degree, a, b, o
