// k_contacts.hip -- contact queries (gpe_query_contacts): which particles touch, and how many neighbours each one has.
// Passes over the live set on the device (gfx950, wave64) that read the particles and write only scratch of their own.
//
// Not on the per-step path, so the plain form:
//   (1) k_contacts_keys: key[i] = the particle's cell under the QUERY's cell size (2.2 x the largest |radius|, whatever
//       the grid's override says), each coordinate clamped monotonically into 16 bits: cy << 16 | cx.  Clamping keeps
//       equal cells equal and adjacent cells adjacent or equal, so the 3 x 3 neighbourhood of the clamped cell holds
//       every cell of the unclamped one -- for positions outside the world, at 1e30, at +-inf too.  A NaN coordinate
//       goes to cell 0 (f32_to_i32_sat); the predicate rejects such a particle anyway.  val[i] = i.
//   (2) sort_pairs (stable) on (key, val): the members of a cell lie together, in ascending storage index; rows of
//       cells lie together too (the key is row-major), so the three cells cx-1 .. cx+1 of one row are ONE run of the
//       sorted keys.  k_contacts_records then writes one 16-byte record (x, y, radius, index) per sorted slot, so that
//       a walk over a run is one sequential load per candidate and not an index followed by two dependent gathers.
//   (3) k_contacts_count: lane t takes sorted slot t (a wave's lanes share their neighbour runs), finds the three row
//       runs by binary search, applies the predicate to every member and writes degree[i] and upper[i] = #{j > i in
//       contact}.  Each workgroup writes the 64-bit sum of its `upper`; k_contacts_fold adds the workgroups' words into
//       the total with at most kContactsFoldBlocks 64-bit atomics (the pattern of k_pick_fold).
//   (4) inclusive_scan (k_scan.hip) of upper[] in storage order: particle i's pairs rank from scanned[i-1].
//   (5) k_contacts_gather, only when the host asked for a per-pair array: particle i emits its partners j > i in
//       ascending j -- a nine-way merge by smallest head over the nine cells' runs, each of which ascends -- until its
//       last partner or `capacity`.  A particle without such partners, or whose first pair ranks at or past `capacity`,
//       returns after reading its two scanned words.
// A run may be of any length (a pile): the walks are plain loops over it.
// The predicate (in_contact) is IEEE binary32, one rounding per operation, left to right, no FMA: numpy float32
// reproduces it bit for bit (tests/_contacts_model.py).
#include <algorithm>

#include "k_contacts.h"

namespace gpe {

// (1)
__global__ __launch_bounds__(kStreamBlock) void k_contacts_keys(const float2 *__restrict__ pos, uint64_t n, float cell_size,
                                                                uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t stride = (uint64_t)gridDim.x * kStreamBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kStreamBlock + threadIdx.x; i < n; i += stride) {
        const float2 p = pos[i];
        keys[i] = (contacts_axis(p.y, cell_size) << 16) | contacts_axis(p.x, cell_size);
        vals[i] = (uint32_t)i;
    }
}

// (2) rec[t] = bits of (x, y, radius) and the index of the particle in sorted slot t
__global__ __launch_bounds__(kStreamBlock) void k_contacts_records(const float2 *__restrict__ pos,
                                                                   const float *__restrict__ radius,
                                                                   const uint32_t *__restrict__ vals, uint64_t n,
                                                                   uint4 *__restrict__ rec)
{
    const uint64_t stride = (uint64_t)gridDim.x * kStreamBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kStreamBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t i = vals[t];
        const float2 p = pos[i];
        rec[t] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(radius[i]), i);
    }
}

// first slot t in [lo, hi) -- one cell's run, ascending in the index -- whose particle's index is above i
__device__ __forceinline__ uint32_t contacts_first_above(const uint4 *__restrict__ rec, uint32_t lo, uint32_t hi, uint32_t i)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rec[mid].w <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// (3) degree[i], upper[i] and the workgroup's sum of upper
__global__ __launch_bounds__(kContactsBlock) void k_contacts_count(const uint32_t *__restrict__ keys,
                                                                   const uint4 *__restrict__ rec, uint32_t n,
                                                                   uint32_t *__restrict__ degree,
                                                                   uint32_t *__restrict__ upper,
                                                                   unsigned long long *__restrict__ tile_sum)
{
    __shared__ unsigned long long s_sum[kContactsWaves];
    const uint64_t t64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    uint32_t up = 0;
    if (t64 < n) {
        const uint32_t t = (uint32_t)t64;
        const uint4 me = rec[t];
        const uint32_t key = keys[t];
        const float x = __uint_as_float(me.x), y = __uint_as_float(me.y), r = __uint_as_float(me.z);
        uint32_t deg = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            uint32_t s, e, k_mid;
            if (!contacts_row_run(keys, n, key, dy, &s, &e, &k_mid)) continue;
            for (uint32_t j = s; j < e; ++j) {
                const uint4 o = rec[j];
                float q, rs;
                const bool hit = j != t && in_contact(x, y, r, __uint_as_float(o.x), __uint_as_float(o.y),
                                                      __uint_as_float(o.z), &q, &rs);
                deg += hit ? 1u : 0u;
                up += hit && o.w > me.w ? 1u : 0u;
            }
        }
        degree[me.w] = deg;
        upper[me.w] = up;
    }
    const unsigned long long sum = wave_sum_u64(up);
    if (lane_id() == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int v = 0; v < kContactsWaves; ++v) total += s_sum[v];
        tile_sum[blockIdx.x] = total;
    }
}

// the sum of the workgroups' words into *total (zeroed before): grid-stride, one atomic per workgroup
__global__ __launch_bounds__(kContactsBlock) void k_contacts_fold(const unsigned long long *__restrict__ tile_sum,
                                                                  uint64_t tiles, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s_sum[kContactsWaves];
    unsigned long long sum = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x; t < tiles; t += (uint64_t)gridDim.x * kContactsBlock)
        sum += tile_sum[t];
    sum = wave_sum_u64(sum);
    if (lane_id() == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (int v = 0; v < kContactsWaves; ++v) all += s_sum[v];
        if (all) atomicAdd(total, all);
    }
}

// Where the gather writes: one row per pair ranked below capacity; NULL = not requested.
struct ContactsOut {
    uint32_t *index_a, *index_b, *uid_a, *uid_b;
    float *overlap;
};

// (5) the pairs ranked below capacity: ascending index_a, then ascending index_b; scanned = inclusive scan of upper[]
__global__ __launch_bounds__(kContactsBlock) void k_contacts_gather(const uint32_t *__restrict__ keys,
                                                                    const uint4 *__restrict__ rec, uint32_t n,
                                                                    const uint32_t *__restrict__ scanned,
                                                                    const uint32_t *__restrict__ uids, uint32_t capacity,
                                                                    ContactsOut O)
{
#pragma clang fp contract(off)
    const uint64_t t64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    if (t64 >= n) return;                                       // (no barrier in this kernel)
    const uint32_t t = (uint32_t)t64;
    const uint4 me = rec[t];
    const uint32_t i = me.w;
    uint32_t rank = i ? scanned[i - 1] : 0u;                    // pairs of the particles below i
    const uint32_t last = scanned[i];
    const uint32_t stop = last < capacity ? last : capacity;
    if (rank >= stop) return;
    const uint32_t key = keys[t];
    const float x = __uint_as_float(me.x), y = __uint_as_float(me.y), r = __uint_as_float(me.z);
    // the nine cells' runs, each from its first member above i; head = that member's index (~0: exhausted)
    uint32_t cur[9], end[9], head[9];
#pragma unroll
    for (int row = 0; row < 3; ++row) {
        uint32_t s = 0, e = 0, k_mid = 0;
        const bool have = contacts_row_run(keys, n, key, row - 1, &s, &e, &k_mid);
        uint32_t b1 = s, b2 = s;
        if (have) {
            b1 = contacts_lower_bound(keys, s, e, k_mid);
            b2 = contacts_lower_bound(keys, b1, e, (uint64_t)k_mid + 1);
        }
        const uint32_t lo[3] = {s, b1, b2}, hi[3] = {b1, b2, e};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = row * 3 + k;
            cur[c] = contacts_first_above(rec, lo[k], hi[k], i);
            end[c] = hi[k];
            head[c] = cur[c] < end[c] ? rec[cur[c]].w : 0xFFFFFFFFu;
        }
    }
    const uint32_t uid_i = O.uid_a ? uids[i] : 0u;
    while (rank < stop) {
        uint32_t best = 0xFFFFFFFFu;                            // (an index is at most 2^32 - 2)
#pragma unroll
        for (int c = 0; c < 9; ++c) best = head[c] < best ? head[c] : best;
        if (best == 0xFFFFFFFFu) break;                         // cannot happen before `last`: the count saw the same runs
        uint32_t slot = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            if (head[c] == best) {                              // (one run only: an index is in one cell)
                slot = cur[c];
                cur[c] += 1;
                head[c] = cur[c] < end[c] ? rec[cur[c]].w : 0xFFFFFFFFu;
            }
        }
        const uint4 o = rec[slot];
        float q, rs;
        if (in_contact(x, y, r, __uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z), &q, &rs)) {
            if (O.index_a) O.index_a[rank] = i;
            if (O.index_b) O.index_b[rank] = o.w;
            if (O.uid_a) O.uid_a[rank] = uid_i;
            if (O.uid_b) O.uid_b[rank] = uids[o.w];
            if (O.overlap) O.overlap[rank] = rs - sqrtf(q);
            rank += 1;
        }
    }
}

uint64_t contacts_tiles(uint64_t n) { return (n + kContactsBlock - 1) / kContactsBlock; }

gpe_status launch_contacts_keys(gpe_ctx *c, float cell_size, uint32_t *keys, uint32_t *vals)
{
    hipLaunchKernelGGL(k_contacts_keys, dim3(stream_grid(c->n)), dim3(kStreamBlock), 0, c->stream, c->pos, c->n, cell_size,
                       keys, vals);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_contacts_records_of(gpe_ctx *c, const float2 *pos, const float *radius, const uint32_t *vals, uint64_t n,
                                      uint4 *rec)
{
    hipLaunchKernelGGL(k_contacts_records, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, pos, radius, vals, n,
                       rec);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_contacts_records(gpe_ctx *c, const uint32_t *vals, uint4 *rec)
{
    return launch_contacts_records_of(c, c->pos, c->radius, vals, c->n, rec);
}

gpe_status launch_contacts_count(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, uint32_t *degree, uint32_t *upper,
                                 unsigned long long *tile_sum, unsigned long long *total)
{
    const uint64_t tiles = contacts_tiles(c->n);
    if (tiles == 0 || c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "contacts: bad particle count");
    hipLaunchKernelGGL(k_contacts_count, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, keys, rec,
                       (uint32_t)c->n, degree, upper, tile_sum);
    GPE_HIP(c, hipGetLastError());
    GPE_HIP(c, hipMemsetAsync(total, 0, sizeof(*total), c->stream));
    const uint64_t g = std::min<uint64_t>((tiles + 4 * kContactsBlock - 1) / (4 * kContactsBlock), kContactsFoldBlocks);
    hipLaunchKernelGGL(k_contacts_fold, dim3((uint32_t)g), dim3(kContactsBlock), 0, c->stream, tile_sum, tiles, total);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_contacts_gather(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, const uint32_t *scanned,
                                  uint32_t capacity, uint32_t *index_a, uint32_t *index_b, uint32_t *uid_a, uint32_t *uid_b,
                                  float *overlap)
{
    const uint64_t tiles = contacts_tiles(c->n);
    if (tiles == 0 || c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "contacts: bad particle count");
    const ContactsOut O{index_a, index_b, uid_a, uid_b, overlap};
    hipLaunchKernelGGL(k_contacts_gather, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, keys, rec,
                       (uint32_t)c->n, scanned, (const uint32_t *)c->uid.uids, capacity, O);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
