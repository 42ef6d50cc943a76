// k_remove.hip -- removal of particles (gpe_remove_particles / gpe_remove_particles_in_circle): a stable
// compaction of the live set (pos, prev, radius) into the copy set, on the device (gfx950, wave64).
//
// Not on the per-step path, so the plain three-launch form:
//   (1) k_remove_count: each workgroup takes one tile of kRemoveBlock x kRemoveRounds consecutive particles, in
//       rounds of kRemoveBlock (coalesced), votes on "survives" and writes its survivor count; in the same pass it
//       reduces the survivors' max-radius key (bits(|r|) << 32 | index) of the tile and writes that too.
//       k_remove_max_key folds the tiles' keys into one word: at most kMaxKeyBlocks 64-bit atomics instead of one per
//       tile (device-scope atomics on one address serialise: one per tile cost 0.35 ms at 100 M particles).
//   (2) inclusive_scan (k_scan.hip) over the per-tile counts; the host reads the total and the key back.
//   (3) k_remove_scatter: the same tiles in the same order; a survivor's slot is the tile's scanned base + the
//       survivors of the earlier rounds + those of the earlier waves of its round (LDS) + those below its lane
//       (ballot + mbcnt).  The UIDS instantiations also move each survivor's uid (gpe_enable_uids) to that slot:
//       R 4 B + W 4 B more per survivor.  The uid pointers come last, so the uid-off instantiations read their
//       arguments where they always did and never touch the two extra ones.
// Bytes (circle form): count R 8 B per particle (pos) + 4 B per survivor (radius); scatter R 8 B per particle (pos, the
// predicate) and R 12 B + W 20 B per survivor.  Mask form: the predicate reads 1 B per particle instead of pos, and the
// scatter R 20 B + W 20 B per survivor.  100 M particles: count 0.22 ms, scatter 0.79 ms (profiles/remove/).
#include <algorithm>

#include "gpe_internal.h"

namespace gpe {

constexpr int kRemoveBlock = 256;
constexpr int kRemoveWaves = kRemoveBlock / kWave;
constexpr int kRemoveRounds = 8;                           // K: rounds per tile
constexpr uint64_t kRemoveTile = (uint64_t)kRemoveBlock * kRemoveRounds;

// What decides removal: a byte per particle (mask != NULL) or the closed disc around (x, y) with rr = radius * radius.
struct RemovePredicate {
    const uint8_t *mask;
    float x, y, rr;
};

// The disc test in IEEE binary32, one rounding per operation, left to right, no FMA (the header's contract; the
// build also compiles with -ffp-contract=off).
__device__ __forceinline__ bool in_disc(const float2 p, const RemovePredicate &P)
{
#pragma clang fp contract(off)
    const float dx = p.x - P.x;
    const float dy = p.y - P.y;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    return dxx + dyy <= P.rr;
}

// survives[r] for the rounds of this thread's tile (false past n).  The inputs of all rounds are loaded first, so
// that kRemoveRounds loads per lane are in flight together.
template <bool MASK>
__device__ __forceinline__ void survivors_of_tile(const RemovePredicate &P, const float2 *__restrict__ pos, uint64_t n,
                                                  uint64_t first, bool (&keep)[kRemoveRounds])
{
    if constexpr (MASK) {
        uint8_t m[kRemoveRounds];
#pragma unroll
        for (int r = 0; r < kRemoveRounds; ++r) {
            const uint64_t i = first + (uint64_t)r * kRemoveBlock;
            m[r] = i < n ? P.mask[i] : (uint8_t)1;
        }
#pragma unroll
        for (int r = 0; r < kRemoveRounds; ++r) keep[r] = m[r] == 0;
    } else {
        float2 p[kRemoveRounds];
#pragma unroll
        for (int r = 0; r < kRemoveRounds; ++r) {
            const uint64_t i = first + (uint64_t)r * kRemoveBlock;
            p[r] = i < n ? pos[i] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int r = 0; r < kRemoveRounds; ++r) keep[r] = first + (uint64_t)r * kRemoveBlock < n && !in_disc(p[r], P);
    }
}

// (1) survivors per tile, and max over the tile's survivors of bits(|radius|) << 32 | index (ties: the larger index,
// i.e. the last element of largest magnitude, as max_abs_radius picks it; 0 for a tile without survivors)
template <bool MASK>
__global__ __launch_bounds__(kRemoveBlock) void k_remove_count(RemovePredicate P, const float2 *__restrict__ pos,
                                                               const float *__restrict__ radius, uint64_t n,
                                                               uint32_t *__restrict__ tile_count,
                                                               unsigned long long *__restrict__ tile_key)
{
    __shared__ uint32_t s_cnt[kRemoveWaves];
    __shared__ unsigned long long s_key[kRemoveWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kRemoveTile + threadIdx.x;
    bool keep[kRemoveRounds];
    survivors_of_tile<MASK>(P, pos, n, first, keep);
    uint32_t kept = 0;                                         // wave-uniform
    unsigned long long key = 0;
#pragma unroll
    for (int r = 0; r < kRemoveRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kRemoveBlock;
        kept += (uint32_t)__popcll(ballot64(keep[r]));
        if (keep[r]) {
            const unsigned long long k = ((unsigned long long)(__float_as_uint(radius[i]) & 0x7FFFFFFFu) << 32) | i;
            key = k > key ? k : key;
        }
    }
    key = wave_max_u64(key);
    const int w = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) { s_cnt[w] = kept; s_key[w] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        unsigned long long best = 0;
#pragma unroll
        for (int v = 0; v < kRemoveWaves; ++v) {
            total += s_cnt[v];
            best = s_key[v] > best ? s_key[v] : best;
        }
        tile_count[blockIdx.x] = total;
        tile_key[blockIdx.x] = best;
    }
}

// (1b) max over the tiles' keys into *max_key (zeroed before): grid-stride, one atomic per workgroup
constexpr int kMaxKeyBlocks = 64;
__global__ __launch_bounds__(kRemoveBlock) void k_remove_max_key(const unsigned long long *__restrict__ tile_key,
                                                                 uint64_t tiles, unsigned long long *__restrict__ max_key)
{
    __shared__ unsigned long long s_key[kRemoveWaves];
    unsigned long long key = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kRemoveBlock + threadIdx.x; t < tiles; t += (uint64_t)gridDim.x * kRemoveBlock)
        key = tile_key[t] > key ? tile_key[t] : key;
    key = wave_max_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = 0;
#pragma unroll
        for (int v = 0; v < kRemoveWaves; ++v) best = s_key[v] > best ? s_key[v] : best;
        atomicMax(max_key, best);
    }
}

// (3) stable scatter of the survivors into the copy set; tile_scanned = inclusive scan of (1)'s counts
template <bool MASK, bool UIDS>
__global__ __launch_bounds__(kRemoveBlock) void k_remove_scatter(RemovePredicate P, const float2 *__restrict__ pos,
                                                                 const float2 *__restrict__ prev,
                                                                 const float *__restrict__ radius, uint64_t n,
                                                                 const uint32_t *__restrict__ tile_scanned,
                                                                 float2 *__restrict__ pos_out,
                                                                 float2 *__restrict__ prev_out,
                                                                 float *__restrict__ radius_out,
                                                                 const uint32_t *__restrict__ uids,
                                                                 uint32_t *__restrict__ uids_out)
{
    __shared__ uint32_t s_cnt[kRemoveRounds][kRemoveWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kRemoveTile + threadIdx.x;
    const int w = (int)(threadIdx.x >> 6);
    bool keep[kRemoveRounds];
    survivors_of_tile<MASK>(P, pos, n, first, keep);
    uint64_t vote[kRemoveRounds];
#pragma unroll
    for (int r = 0; r < kRemoveRounds; ++r) {
        vote[r] = ballot64(keep[r]);
        if (lane_id() == 0) s_cnt[r][w] = (uint32_t)__popcll(vote[r]);
    }
    __syncthreads();
    uint32_t base = blockIdx.x ? tile_scanned[blockIdx.x - 1] : 0u;   // survivors of the earlier tiles
#pragma unroll
    for (int r = 0; r < kRemoveRounds; ++r) {
        uint32_t before = 0, round = 0;
#pragma unroll
        for (int v = 0; v < kRemoveWaves; ++v) {
            const uint32_t cnt = s_cnt[r][v];
            before += v < w ? cnt : 0u;
            round += cnt;
        }
        if (keep[r]) {
            const uint64_t i = first + (uint64_t)r * kRemoveBlock;
            const uint64_t dst = (uint64_t)base + before + popc_below_lane(vote[r]);
            pos_out[dst] = pos[i];
            prev_out[dst] = prev[i];
            radius_out[dst] = radius[i];
            if constexpr (UIDS) uids_out[dst] = uids[i];
        }
        base += round;
    }
}

uint64_t remove_tiles(uint64_t n) { return (n + kRemoveTile - 1) / kRemoveTile; }

gpe_status launch_max_key_fold(gpe_ctx *c, const unsigned long long *tile_key, uint64_t tiles, unsigned long long *max_key)
{
    GPE_HIP(c, hipMemsetAsync(max_key, 0, sizeof(*max_key), c->stream));
    const uint64_t g = std::min<uint64_t>((tiles + 4 * kRemoveBlock - 1) / (4 * kRemoveBlock), kMaxKeyBlocks);
    hipLaunchKernelGGL(k_remove_max_key, dim3((uint32_t)g), dim3(kRemoveBlock), 0, c->stream, tile_key, tiles, max_key);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_remove_count(gpe_ctx *c, const uint8_t *mask, float x, float y, float rr, uint32_t *tile_count,
                               unsigned long long *tile_key, unsigned long long *max_key)
{
    const uint64_t tiles = remove_tiles(c->n);
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "remove: bad particle count");
    const RemovePredicate P{mask, x, y, rr};
    if (mask)
        hipLaunchKernelGGL(k_remove_count<true>, dim3((uint32_t)tiles), dim3(kRemoveBlock), 0, c->stream, P, c->pos,
                           c->radius, c->n, tile_count, tile_key);
    else
        hipLaunchKernelGGL(k_remove_count<false>, dim3((uint32_t)tiles), dim3(kRemoveBlock), 0, c->stream, P, c->pos,
                           c->radius, c->n, tile_count, tile_key);
    GPE_HIP(c, hipGetLastError());
    return launch_max_key_fold(c, tile_key, tiles, max_key);
}

gpe_status launch_remove_scatter(gpe_ctx *c, const uint8_t *mask, float x, float y, float rr,
                                 const uint32_t *tile_scanned, const uint32_t *uids, uint32_t *uids_out)
{
    const uint64_t tiles = remove_tiles(c->n);
    const RemovePredicate P{mask, x, y, rr};
    const bool carry = uids != nullptr;
    const auto kern = mask ? (carry ? k_remove_scatter<true, true> : k_remove_scatter<true, false>)
                           : (carry ? k_remove_scatter<false, true> : k_remove_scatter<false, false>);
    hipLaunchKernelGGL(kern, dim3((uint32_t)tiles), dim3(kRemoveBlock), 0, c->stream, P, c->pos, c->prev, c->radius,
                       c->n, tile_scanned, c->pos_copy, c->prev_copy, c->radius_copy, uids, uids_out);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
