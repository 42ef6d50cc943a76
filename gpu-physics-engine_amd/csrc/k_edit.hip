// k_edit.hip -- editing particles in place (gpe_edit_particles, gpe_kick_circle / gpe_kick_box; gfx950, wave64).
//
// Not on the per-step path.  Two families:
//   Keyed edits, one lane per key:
//   (1) k_edit_check: key -> storage index (an index as it is, a uid through the sorted uid map of k_uids.hip); an index
//       past the end sets kEditBadIndex, an absent uid becomes GPE_UID_ABSENT; slot[i] = i; the keys that name a particle
//       are counted (one atomic per wave).
//   (2) the context's sort_pairs over the k (index, slot) pairs, then k_edit_adjacent: equal neighbours (absent ones
//       aside) set kEditDuplicate, as k_uid_adjacent finds a repeated uid.  The host reads the two flag words back; a
//       refused call has touched nothing but this workspace.
//   (3) k_edit_apply<MASK>: in sorted order (the stores ascend through the particle arrays), particle keys[j] takes row
//       slots[j] of each requested field.  A field that was not requested is neither loaded nor stored: MASK is a
//       template argument, as k_query_gather skips the outputs nobody asked for.
//   (4) a radius edit: k_edit_radius_key reduces bits(|r|) << 32 | index over each tile of kQueryTile radii -- the key of
//       k_remove_count, R 4 B per particle -- and k_remove_max_key (launch_max_key_fold) folds the tiles' keys.
//       k_remove_count itself would have cost 8 B (pos) or 1 B (a zeroed mask) per particle more for a predicate that
//       removes nothing, and a scan of counts nobody reads.
//   Bytes: check R 4 + W 8 B per key (+ ceil(log2 n) map probes for a uid); sort 4 passes over 8 B pairs; apply R 8 B
//   (key, slot) + R / W 8 + 8 + 4 B per key for pos / prev / radius (pos without prev: W 16 B); max radius R 4 B per
//   particle.
//
//   Kicks, a full pass: k_kick<KIND, OP, COUNT> takes the tiles of the region queries (k_region.h: 256 threads, 8 rounds,
//   the 8 position loads of a lane in flight together), and only the lanes whose particle lies in the region load prev
//   (GPE_VEL_SET does not), apply the operation and store it.  R 8 B per particle + R 8 B / W 8 B per kicked particle.
//   COUNT: one ballot per round, the waves' totals folded through LDS, one atomic per workgroup that kicked something.
//   The arithmetic is IEEE binary32, one rounding per operation, no FMA (named temporaries and contraction off, as
//   dist2; the build also compiles with -ffp-contract=off).
#include <algorithm>

#include "k_region.h"
#include "k_uids.h"

namespace gpe {

constexpr int kEditBlock = kStreamBlock;

// (1) one lane per key
template <bool BY_UID>
__global__ __launch_bounds__(kEditBlock) void k_edit_check(uint32_t *__restrict__ keys, uint32_t *__restrict__ slots,
                                                           uint64_t k, const uint32_t *__restrict__ map_keys,
                                                           const uint32_t *__restrict__ map_vals, uint32_t n,
                                                           uint32_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * kEditBlock + threadIdx.x;
    const bool valid = i < k;
    uint32_t idx = GPE_UID_ABSENT;
    bool bad = false;
    if (valid) {
        const uint32_t key = keys[i];
        if constexpr (BY_UID) {
            idx = uid_lookup(map_keys, map_vals, n, key);
        } else {
            bad = key >= n;
            idx = bad ? GPE_UID_ABSENT : key;
        }
        keys[i] = idx;
        slots[i] = (uint32_t)i;
    }
    const uint64_t m_bad = ballot64(bad), m_found = ballot64(idx != GPE_UID_ABSENT);
    if (lane_id() == 0) {
        if (m_bad) atomicOr(&flag[0], kEditBadIndex);
        if (m_found) atomicAdd(&flag[1], (uint32_t)__popcll(m_found));
    }
}

// (2) keys sorted ascending: two keys naming the same particle are neighbours
__global__ __launch_bounds__(kEditBlock) void k_edit_adjacent(const uint32_t *__restrict__ keys, uint64_t k,
                                                              uint32_t *__restrict__ flag)
{
    const uint64_t i = 1 + (uint64_t)blockIdx.x * kEditBlock + threadIdx.x;
    bool same = false;
    if (i < k) {
        const uint32_t a = keys[i];
        same = a == keys[i - 1] && a != GPE_UID_ABSENT;
    }
    if (ballot64(same) != 0 && lane_id() == 0) atomicOr(&flag[0], kEditDuplicate);
}

// (3) particle keys[j] takes row slots[j] of the requested fields
template <uint32_t MASK>
__global__ __launch_bounds__(kEditBlock) void k_edit_apply(const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ slots, uint64_t k,
                                                           const float2 *__restrict__ pos_rows,
                                                           const float2 *__restrict__ prev_rows,
                                                           const float *__restrict__ radius_rows,
                                                           float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                           float *__restrict__ radius)
{
    const uint64_t j = (uint64_t)blockIdx.x * kEditBlock + threadIdx.x;
    if (j >= k) return;
    const uint32_t i = keys[j];
    if (i == GPE_UID_ABSENT) return;
    const uint32_t s = slots[j];
    if constexpr ((MASK & kEditPos) != 0) {
        const float2 p = pos_rows[s];
        pos[i] = p;
        if constexpr ((MASK & kEditPrev) == 0) prev[i] = p;       // at rest, as gpe_add_particles leaves a new particle
    }
    if constexpr ((MASK & kEditPrev) != 0) prev[i] = prev_rows[s];
    if constexpr ((MASK & kEditRadius) != 0) radius[i] = radius_rows[s];
}

// (4) per tile: max of bits(|radius|) << 32 | index (ties: the larger index, the last element of largest magnitude)
__global__ __launch_bounds__(kQueryBlock) void k_edit_radius_key(const float *__restrict__ radius, uint64_t n,
                                                                 unsigned long long *__restrict__ tile_key)
{
    __shared__ unsigned long long s_key[kQueryWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    float rad[kQueryRounds];
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        rad[r] = i < n ? radius[i] : 0.f;
    }
    unsigned long long key = 0;
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        if (i < n) {
            const unsigned long long k = ((unsigned long long)(__float_as_uint(rad[r]) & 0x7FFFFFFFu) << 32) | i;
            key = k > key ? k : key;
        }
    }
    key = wave_max_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = 0;
#pragma unroll
        for (int v = 0; v < kQueryWaves; ++v) best = s_key[v] > best ? s_key[v] : best;
        tile_key[blockIdx.x] = best;
    }
}

// The new previous position of a particle at p with previous position q (per component; q unused by GPE_VEL_SET).
template <int OP>
__device__ __forceinline__ float kicked(const float p, const float q, const float a)
{
#pragma clang fp contract(off)
    if constexpr (OP == GPE_VEL_ADD) {
        return q - a;
    } else if constexpr (OP == GPE_VEL_SET) {
        return p - a;
    } else {
        const float v = p - q;
        const float w = v * a;
        return p - w;
    }
}

template <int KIND, int OP, bool COUNT>
__global__ __launch_bounds__(kQueryBlock) void k_kick(QueryRegion Q, float ax, float ay, const float2 *__restrict__ pos,
                                                      float2 *__restrict__ prev, uint64_t n,
                                                      unsigned long long *__restrict__ count)
{
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    float2 p[kQueryRounds];
    bool hit[kQueryRounds];
    matches_of_tile<KIND>(Q, pos, n, first, p, hit);
    float2 q[kQueryRounds];
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {                   // the matching lanes' loads, in flight together
        q[r] = make_float2(0.f, 0.f);
        if constexpr (OP != GPE_VEL_SET)
            if (hit[r]) q[r] = prev[first + (uint64_t)r * kQueryBlock];
    }
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r)
        if (hit[r])
            prev[first + (uint64_t)r * kQueryBlock] = make_float2(kicked<OP>(p[r].x, q[r].x, ax), kicked<OP>(p[r].y, q[r].y, ay));
    if constexpr (COUNT) {
        __shared__ uint32_t s_cnt[kQueryWaves];
        uint32_t cnt = 0;                                      // wave-uniform
#pragma unroll
        for (int r = 0; r < kQueryRounds; ++r) cnt += (uint32_t)__popcll(ballot64(hit[r]));
        if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (int v = 0; v < kQueryWaves; ++v) total += s_cnt[v];
            if (total) atomicAdd(count, (unsigned long long)total);
        }
    }
}

static uint32_t key_grid(uint64_t k) { return (uint32_t)((k + kEditBlock - 1) / kEditBlock); }

gpe_status launch_edit_check(gpe_ctx *c, bool by_uid, uint32_t *keys, uint32_t *slots, uint64_t k, uint32_t *flag)
{
    if (k == 0 || k > 0x7FFFFFFFull || c->n == 0 || c->n > 0xFFFFFFFFull)
        return fail(c, GPE_ERR_INVALID_ARG, "edit: bad key or particle count");
    const auto kern = by_uid ? k_edit_check<true> : k_edit_check<false>;
    hipLaunchKernelGGL(kern, dim3(key_grid(k)), dim3(kEditBlock), 0, c->stream, keys, slots, k,
                       (const uint32_t *)c->uid.map_keys, (const uint32_t *)c->uid.map_vals, (uint32_t)c->n, flag);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_edit_adjacent(gpe_ctx *c, const uint32_t *keys, uint64_t k, uint32_t *flag)
{
    if (k < 2) return GPE_OK;
    hipLaunchKernelGGL(k_edit_adjacent, dim3(key_grid(k - 1)), dim3(kEditBlock), 0, c->stream, keys, k, flag);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_edit_apply(gpe_ctx *c, const uint32_t *keys, const uint32_t *slots, uint64_t k, const float2 *pos_rows,
                             const float2 *prev_rows, const float *radius_rows)
{
    using Kernel = void (*)(const uint32_t *, const uint32_t *, uint64_t, const float2 *, const float2 *, const float *,
                            float2 *, float2 *, float *);
    static const Kernel table[8] = {nullptr,         k_edit_apply<1>, k_edit_apply<2>, k_edit_apply<3>,
                                    k_edit_apply<4>, k_edit_apply<5>, k_edit_apply<6>, k_edit_apply<7>};
    const uint32_t mask = (pos_rows ? kEditPos : 0u) | (prev_rows ? kEditPrev : 0u) | (radius_rows ? kEditRadius : 0u);
    if (mask == 0 || k == 0) return fail(c, GPE_ERR_INVALID_ARG, "edit: nothing to apply");
    hipLaunchKernelGGL(table[mask], dim3(key_grid(k)), dim3(kEditBlock), 0, c->stream, keys, slots, k, pos_rows,
                       prev_rows, radius_rows, c->pos, c->prev, c->radius);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

static gpe_status check_tiles(gpe_ctx *c, uint64_t tiles)
{
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "edit: bad particle count");
    return GPE_OK;
}

gpe_status launch_edit_max_radius(gpe_ctx *c, unsigned long long *tile_key, unsigned long long *max_key)
{
    const uint64_t tiles = query_tiles(c->n);
    GPE_TRY(check_tiles(c, tiles));
    hipLaunchKernelGGL(k_edit_radius_key, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream,
                       (const float *)c->radius, c->n, tile_key);
    GPE_HIP(c, hipGetLastError());
    return launch_max_key_fold(c, tile_key, tiles, max_key);
}

template <int KIND, bool COUNT>
static auto kick_kernel(uint32_t op)
{
    return op == GPE_VEL_ADD ? k_kick<KIND, GPE_VEL_ADD, COUNT>
           : op == GPE_VEL_SET ? k_kick<KIND, GPE_VEL_SET, COUNT>
                               : k_kick<KIND, GPE_VEL_SCALE, COUNT>;
}

gpe_status launch_kick(gpe_ctx *c, bool box, const float *region, uint32_t op, float ax, float ay,
                       unsigned long long *count)
{
    const uint64_t tiles = query_tiles(c->n);
    GPE_TRY(check_tiles(c, tiles));
    if (op > GPE_VEL_SCALE) return fail(c, GPE_ERR_INVALID_ARG, "kick: unknown operation");
    const QueryRegion Q{region[0], region[1], region[2], region[3], region[4]};
    if (count) GPE_HIP(c, hipMemsetAsync(count, 0, sizeof(*count), c->stream));
    const auto kern = box ? (count ? kick_kernel<kQueryBox, true>(op) : kick_kernel<kQueryBox, false>(op))
                          : (count ? kick_kernel<kQueryCircle, true>(op) : kick_kernel<kQueryCircle, false>(op));
    hipLaunchKernelGGL(kern, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, Q, ax, ay,
                       (const float2 *)c->pos, c->prev, c->n, count);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
