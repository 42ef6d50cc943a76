// k_nearest.hip -- nearest neighbours (gpe_query_nearest): the m particles whose centres are closest to each of k points.
// A walk on the device (gfx950, wave64) of the contact query's sorted cell records (k_contacts.hip stages (1) and (2))
// and the ray cast's row table (k_ray_row_start) outward from each point; it reads the particles and writes only scratch
// of its own.
//
// Not on the per-step path, so the plain form: k_nearest, one wave per query point.
//   The wave searches squares that double.  (X0, Y0) = the point's clamped cell; for R = 1, 2, 4, ... the square is the
//   rows Y0-R .. Y0+R and the columns X0-R .. X0+R, clipped to 0 .. 65535.  The rows are dealt to the lanes 64 at a time;
//   each lane finds its row's run of the sorted keys by two binary searches inside [row_start[Y], row_start[Y+1]) (an
//   empty row costs those two loads), and the wave consumes the 64 runs laid end to end, 64 records at a time: an
//   inclusive scan of the run lengths, and each lane finds the (row, offset) of its record by a six-step search of the
//   scanned lengths through lane shuffles, as k_ray_cast does.  So one cell with hundreds of members and thousands of
//   near-empty rows both keep the lanes busy.  Each square starts its list afresh; the doubling bounds the re-reading to
//   about a third of the last square.  (A ring-by-ring walk over single cells would cost billions of lookups in a sparse
//   scene: tiny radii in a large world.)
//   Top-m: the wave keeps the least 64-bit keys bits(d2) << 32 | index sorted over its lanes (lane j holds the j-th
//   least; m <= 64).  For each batch of 64 records the lanes whose record is a candidate (d2 <= rr) below the current
//   m-th key are voted on and inserted one at a time: every lane compares, the lanes above the place shift up through a
//   shuffle.  Wave-uniform, no LDS, no atomics; the outcome is the set of least keys whatever the order of arrival.
//   A square is final when (a) all four sides are closed -- the clipped square reaches column / row 0 or
//   65535 there, so the whole table was read -- or, with g = the least distance from the point to the outer edge of an
//   open side minus half a cell, (b) g >= max_distance or (c) the list holds m keys and the m-th d2 < g*g.  contacts_axis
//   is monotone, so every particle outside the square has its centre at least g + cell/2 from the point along one axis;
//   the half cell covers the rounding of p / cell, of the edge arithmetic and of d2 while |coordinate| <= 131072 cells,
//   the bound gpe_query_nearest checks.  (c) is strict: an unread particle never ties with a listed one.  R is also
//   capped at ceil(max_distance / cell) + 2, after which (b) holds.  None of the stops can change a result.
//   Lane j < m then writes slot j of the point's row of every requested output, fetched by index.
#include <cmath>

#include "k_contacts.h"
#include "k_region.h"

namespace gpe {

constexpr int kNearestBlock = 256;                         // threads per workgroup: one wave per query point
constexpr int kNearestWaves = kNearestBlock / kWave;
constexpr uint32_t kNearestTop = (uint32_t)kContactsAxisMax;      // the last clamped column / row: 65535
static_assert(kRayRowWords == kNearestTop + 2u, "row_start holds one word per row and the end of the last row");
static_assert(kNearestMaxM <= (uint32_t)kWave, "one neighbour per lane");
constexpr unsigned long long kNearestNoKey = ~0ull;        // above every key: bits(d2) <= 0x7F800000

// Where the search writes: count one word per point, the rest m slots per point; NULL = not requested.
struct NearestOut {
    uint32_t *count;
    uint32_t *index;
    uint32_t *uid;
    float *dist2;
    float2 *pos;
    float *radius;
};

// lane `lane` (wave-uniform) of v, the same in every lane
__device__ __forceinline__ unsigned long long nearest_read_lane(unsigned long long v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// k points, finite and within 131072 cells of 0 (checked on the host); cs > 0 finite; md >= 0 or +inf; 1 <= m <= 64;
// n > 0 sorted slots
__global__ __launch_bounds__(kNearestBlock) void k_nearest(const float2 *__restrict__ points, uint32_t k, uint32_t m,
                                                           float md, float cs, const uint32_t *__restrict__ keys,
                                                           const uint4 *__restrict__ rec,
                                                           const uint32_t *__restrict__ row_start,
                                                           const float2 *__restrict__ pos,
                                                           const float *__restrict__ radius,
                                                           const uint32_t *__restrict__ uids, NearestOut O)
{
    const uint32_t q = blockIdx.x * kNearestWaves + (threadIdx.x >> 6);
    if (q >= k) return;                                        // wave-uniform; the kernel has no barrier
    const uint32_t lane = (uint32_t)lane_id();
    const float2 pt = points[q];
    const float rr = md * md;
    const uint32_t X0 = contacts_axis(pt.x, cs), Y0 = contacts_axis(pt.y, cs);
    const float reach = md / cs;
    const uint32_t r_cap = reach < 65536.0f ? (uint32_t)ceilf(reach) + 2u : 65536u;
    const float half = 0.5f * cs;
    unsigned long long mine = kNearestNoKey;                   // lane j: the j-th least key of the current square
    for (uint32_t R = 1;;) {                                   // everything that steers the loops is wave-uniform
        mine = kNearestNoKey;
        unsigned long long kth = kNearestNoKey;                // the m-th least key: lane m - 1
        const uint32_t x_lo = X0 > R ? X0 - R : 0u, x_hi = X0 + R < kNearestTop ? X0 + R : kNearestTop;
        const uint32_t y_lo = Y0 > R ? Y0 - R : 0u, y_hi = Y0 + R < kNearestTop ? Y0 + R : kNearestTop;
        const uint32_t rows = y_hi - y_lo + 1u;
        for (uint32_t r0 = 0; r0 < rows; r0 += kWave) {
            const uint32_t r = r0 + lane;
            uint32_t s = 0, len = 0;
            if (r < rows) {
                const uint32_t Y = y_lo + r;                   // <= 65535: row_start[Y + 1] is its last word at most
                const uint32_t lo = row_start[Y], hi = row_start[Y + 1u];
                if (lo < hi) {
                    const uint32_t row = Y << 16;
                    s = contacts_lower_bound(keys, lo, hi, row | x_lo);
                    len = contacts_lower_bound(keys, s, hi, (uint64_t)(row | x_hi) + 1u) - s;
                }
            }
            const uint32_t incl = wave_inclusive_scan(len);    // the runs are disjoint: their sum is at most n < 2^32
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            for (uint64_t off = 0; off < total; off += kWave) {
                const uint64_t item64 = off + lane;
                const uint32_t item = (uint32_t)item64;
                // j = the lane whose run holds record `item` of the concatenation: the number of lanes with incl <= item
                uint32_t j = 0;
#pragma unroll
                for (uint32_t step = kWave / 2; step; step >>= 1) {
                    const uint32_t v = (uint32_t)__shfl((int)incl, (int)(j + step - 1u), kWave);
                    j += v <= item ? step : 0u;
                }
                const uint32_t incl_j = (uint32_t)__shfl((int)incl, (int)j, kWave);
                const uint32_t len_j = (uint32_t)__shfl((int)len, (int)j, kWave);
                const uint32_t s_j = (uint32_t)__shfl((int)s, (int)j, kWave);
                unsigned long long key = kNearestNoKey;
                if (item64 < total) {
                    const uint4 p = rec[s_j + (item - (incl_j - len_j))];
                    const float d2 = dist2(make_float2(__uint_as_float(p.x), __uint_as_float(p.y)), pt.x, pt.y);
                    if (d2 <= rr) key = ((unsigned long long)__float_as_uint(d2) << 32) | p.w;
                }
                uint64_t vote = ballot64(key < kth);
                while (vote) {
                    const int from = (int)__builtin_ctzll(vote);
                    vote &= vote - 1;
                    const unsigned long long v = nearest_read_lane(key, from);
                    if (v < kth) {                             // kth may have dropped since the vote
                        // the keys of one square are distinct (one per record), so mine != v
                        const unsigned long long below = __shfl_up(mine, 1, kWave);
                        const bool here = lane == 0u || below < v;
                        mine = mine < v ? mine : (here ? v : below);
                        kth = nearest_read_lane(mine, (int)(m - 1u));
                    }
                }
            }
        }
        const bool open_l = x_lo != 0u, open_r = x_hi != kNearestTop, open_d = y_lo != 0u, open_u = y_hi != kNearestTop;
        if (!(open_l || open_r || open_d || open_u)) break;    // (a) the whole table was read
        // outside the square on an open side: x >= (X0 + R) cs on the right, x < (X0 - R - 1) cs on the left, so in y
        float g = INFINITY;
        if (open_r) g = fminf(g, (float)(X0 + R) * cs - pt.x);
        if (open_l) g = fminf(g, pt.x - (float)(X0 - R - 1u) * cs);
        if (open_u) g = fminf(g, (float)(Y0 + R) * cs - pt.y);
        if (open_d) g = fminf(g, pt.y - (float)(Y0 - R - 1u) * cs);
        g -= half;
        if (g >= md) break;                                    // (b)
        if (kth != kNearestNoKey && g > 0.0f && __uint_as_float((uint32_t)(kth >> 32)) < g * g) break;     // (c)
        R = R < r_cap && 2u * R > r_cap ? r_cap : 2u * R;      // R >= 65535 closes all four sides: the loop ends
    }
    const bool mine_out = lane < m;
    const bool filled = mine_out && mine != kNearestNoKey;
    const uint32_t cnt = (uint32_t)__popcll(ballot64(filled));
    if (lane == 0u) O.count[q] = cnt;
    if (!mine_out) return;
    const uint64_t slot = (uint64_t)q * m + lane;              // < k * m <= kNearestMaxSlots
    const uint32_t i = (uint32_t)(mine & 0xFFFFFFFFull);
    const float nan = __uint_as_float(0x7FC00000u);
    if (O.index) O.index[slot] = filled ? i : GPE_NEAREST_NONE;
    if (O.uid) O.uid[slot] = filled ? uids[i] : GPE_UID_ABSENT;
    if (O.dist2) O.dist2[slot] = filled ? __uint_as_float((uint32_t)(mine >> 32)) : nan;
    if (O.pos) O.pos[slot] = filled ? pos[i] : make_float2(nan, nan);
    if (O.radius) O.radius[slot] = filled ? radius[i] : nan;
}

gpe_status launch_nearest(gpe_ctx *c, const float2 *points, uint32_t k, uint32_t m, float max_distance, float cell_size,
                          const uint32_t *keys, const uint4 *rec, const uint32_t *row_start, uint32_t *count_out,
                          uint32_t *index_out, uint32_t *uid_out, float *dist2_out, float2 *pos_out, float *radius_out)
{
    if (k == 0 || m == 0 || m > kNearestMaxM || (uint64_t)k * m > kNearestMaxSlots || c->n == 0 || c->n > 0xFFFFFFFFull ||
        !(cell_size > 0.0f) || !std::isfinite(cell_size) || !(max_distance >= 0.0f) || !count_out)
        return fail(c, GPE_ERR_INVALID_ARG, "nearest: bad batch, cell size, cutoff or particle count");
    const NearestOut O{count_out, index_out, uid_out, dist2_out, pos_out, radius_out};
    const uint32_t g = (k + kNearestWaves - 1u) / kNearestWaves;
    hipLaunchKernelGGL(k_nearest, dim3(g), dim3(kNearestBlock), 0, c->stream, points, k, m, max_distance, cell_size, keys,
                       rec, row_start, (const float2 *)c->pos, (const float *)c->radius, (const uint32_t *)c->uid.uids, O);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
