// k_contacts.h -- what the passes over the contact query's sorted cell records share: the tile shape, the clamped cell
// key, the contact predicate and the search for a row's run of neighbour cells.  One definition, so that the cluster
// query (k_clusters.hip) walks exactly the candidates and applies exactly the predicate of gpe_query_contacts
// (k_contacts.hip).
#pragma once

#include "gpe_internal.h"

namespace gpe {

constexpr int kContactsBlock = 256;                        // particles per workgroup of the count and gather kernels
constexpr int kContactsWaves = kContactsBlock / kWave;
constexpr int kContactsFoldBlocks = 64;
constexpr int32_t kContactsAxisMax = 65535;                // clamped cell coordinates: 0 .. 65535

// One coordinate of the clamped cell: cells below 0 share column 0, cells 0 .. 65533 keep a column of their own
// (1 .. 65534), the cells above share column 65535.  Monotone in the cell coordinate.
__device__ __forceinline__ uint32_t contacts_axis(float p, float cell_size)
{
    int32_t cc = cell_coord(p, cell_size);
    cc = cc < -1 ? -1 : cc;
    cc = cc > kContactsAxisMax - 1 ? kContactsAxisMax - 1 : cc;
    return (uint32_t)(cc + 1);
}

// The contact predicate: q = dx*dx + dy*dy < (ri + rj)*(ri + rj).  Symmetric in the two particles: the squares of
// negated differences are equal and the radius sum commutes.  A NaN anywhere compares false.
__device__ __forceinline__ bool in_contact(float xi, float yi, float ri, float xj, float yj, float rj, float *q_out,
                                           float *rs_out)
{
#pragma clang fp contract(off)
    const float dx = xi - xj;
    const float dy = yi - yj;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    const float q = dxx + dyy;
    const float rs = ri + rj;
    const float rs2 = rs * rs;
    *q_out = q;
    *rs_out = rs;
    return q < rs2;
}

// first slot t in [lo, hi) with keys[t] >= k (hi when there is none); k may be 2^32 (one past the largest key)
__device__ __forceinline__ uint32_t contacts_lower_bound(const uint32_t *__restrict__ keys, uint32_t lo, uint32_t hi,
                                                         uint64_t k)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The run of row cy + dy that holds the cells cx-1 .. cx+1 (clipped to the key box): [*s, *e); false: no such row.
// *k_mid = the key of the cell (cx, cy + dy).
__device__ __forceinline__ bool contacts_row_run(const uint32_t *__restrict__ keys, uint32_t n, uint32_t key, int dy,
                                                 uint32_t *s, uint32_t *e, uint32_t *k_mid)
{
    const int32_t cx = (int32_t)(key & 0xFFFFu), y = (int32_t)(key >> 16) + dy;
    if (y < 0 || y > kContactsAxisMax) return false;
    const uint32_t x0 = (uint32_t)(cx > 0 ? cx - 1 : 0), x1 = (uint32_t)(cx < kContactsAxisMax ? cx + 1 : kContactsAxisMax);
    const uint32_t row = (uint32_t)y << 16;
    *k_mid = row | (uint32_t)cx;
    *s = contacts_lower_bound(keys, 0, n, row | x0);
    *e = contacts_lower_bound(keys, *s, n, (uint64_t)(row | x1) + 1);
    return true;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

}  // namespace gpe
