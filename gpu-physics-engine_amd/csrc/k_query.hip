// k_query.hip -- region queries and point picking (gpe_query_circle / gpe_query_box / gpe_query_segment / gpe_pick):
// full passes over the live set on the device (gfx950, wave64) that read the particles and change nothing.
//
// Not on the per-step path, so the plain form:
//   (1) k_query_count: each workgroup takes one tile of kQueryBlock x kQueryRounds consecutive particles, in rounds of
//       kQueryBlock (coalesced), votes on "matches" (one ballot per round) and writes its match count.
//   (2) inclusive_scan (k_scan.hip) over the per-tile counts; the host reads the total.
//   (3) k_query_gather, only when the host asked for an output: the same tiles in the same order.  A tile without
//       matches, or whose first match ranks at or past `capacity`, returns after reading its two scanned words.  The
//       others rank each match by the tile's scanned base + the matches of the earlier rounds + those of the earlier
//       waves of its round (LDS) + those below its lane (ballot + mbcnt), and write the index and each requested field
//       of the matches ranked below `capacity` into the staging rows.  A NULL output pointer means the field is not
//       loaded at all.
//   Pick: k_pick reduces min(bits(d2) << 32 | index) over each tile's containing discs into a per-tile key, and
//       k_pick_fold folds the tiles' keys into one word with at most kPickFoldBlocks 64-bit atomics (device-scope
//       atomics on one address serialise; see k_remove_max_key).
// Bytes per particle: count R 8 B (pos); gather R 8 B per particle of a tile it does not skip, plus R 4 + 8 + 8 + 4 + 4 B
// and W 4 + 8 + 8 + 4 + 4 B per written match for index / pos / prev / radius / uid; pick R 12 B (pos, radius).  The
// segment kind (gpe_query_segment: ray_touches of k_ray.h) reads the radius too: count and gather R 12 B.
// 100 M particles: count 0.124 ms, pick 0.190 ms, about 0.8 of the HBM peak (profiles/query/).
#include <algorithm>

#include "k_region.h"

namespace gpe {

// (1) matches per tile
template <int KIND>
__global__ __launch_bounds__(kQueryBlock) void k_query_count(QueryRegion Q, const float2 *__restrict__ pos,
                                                             const float *__restrict__ radius, uint64_t n,
                                                             uint32_t *__restrict__ tile_count)
{
    __shared__ uint32_t s_cnt[kQueryWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    float2 p[kQueryRounds];
    bool hit[kQueryRounds];
    matches_of_tile<KIND>(Q, pos, n, first, p, hit, radius);
    uint32_t cnt = 0;                                          // wave-uniform
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) cnt += (uint32_t)__popcll(ballot64(hit[r]));
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int v = 0; v < kQueryWaves; ++v) total += s_cnt[v];
        tile_count[blockIdx.x] = total;
    }
}

// Where the gather writes: one row per match ranked below capacity; NULL = not requested (never loaded).
struct QueryOut {
    uint32_t *index;
    uint32_t *uid;
    float2 *pos;
    float2 *prev;
    float *radius;
};

// (3) the matches ranked below capacity, in ascending storage index; tile_scanned = inclusive scan of (1)'s counts
template <int KIND>
__global__ __launch_bounds__(kQueryBlock) void k_query_gather(QueryRegion Q, const float2 *__restrict__ pos,
                                                              const float2 *__restrict__ prev,
                                                              const float *__restrict__ radius,
                                                              const uint32_t *__restrict__ uids, uint64_t n,
                                                              const uint32_t *__restrict__ tile_scanned,
                                                              uint32_t capacity, QueryOut O)
{
    __shared__ uint32_t s_cnt[kQueryRounds][kQueryWaves];
    uint32_t base = blockIdx.x ? tile_scanned[blockIdx.x - 1] : 0u;   // matches of the earlier tiles
    const uint32_t end = tile_scanned[blockIdx.x];
    if (end == base || base >= capacity) return;                      // block-uniform: before any barrier
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    const int w = (int)(threadIdx.x >> 6);
    float2 p[kQueryRounds];
    bool hit[kQueryRounds];
    matches_of_tile<KIND>(Q, pos, n, first, p, hit, radius);
    uint64_t vote[kQueryRounds];
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        vote[r] = ballot64(hit[r]);
        if (lane_id() == 0) s_cnt[r][w] = (uint32_t)__popcll(vote[r]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        uint32_t before = 0, round = 0;
#pragma unroll
        for (int v = 0; v < kQueryWaves; ++v) {
            const uint32_t cnt = s_cnt[r][v];
            before += v < w ? cnt : 0u;
            round += cnt;
        }
        if (hit[r]) {
            const uint64_t i = first + (uint64_t)r * kQueryBlock;
            const uint64_t dst = (uint64_t)base + before + popc_below_lane(vote[r]);
            if (dst < capacity) {
                if (O.index) O.index[dst] = (uint32_t)i;
                if (O.pos) O.pos[dst] = p[r];
                if (O.prev) O.prev[dst] = prev[i];
                if (O.radius) O.radius[dst] = radius[i];
                if (O.uid) O.uid[dst] = uids[i];
            }
        }
        base += round;
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

constexpr unsigned long long kNoPick = ~0ull;

// Pick: per tile, min over the particles whose own disc contains (x, y) (d2 <= r * r, binary32, no FMA) of
// bits(d2) << 32 | index.  d2 is a sum of two squares, never negative and never -0, so its bits order as its values; a
// NaN d2 or radius contains nothing.  kNoPick for a tile without such a particle.
__global__ __launch_bounds__(kQueryBlock) void k_pick(float x, float y, const float2 *__restrict__ pos,
                                                      const float *__restrict__ radius, uint64_t n,
                                                      unsigned long long *__restrict__ tile_key)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long s_key[kQueryWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    float2 p[kQueryRounds];
    float rad[kQueryRounds];
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        p[r] = i < n ? pos[i] : make_float2(0.f, 0.f);
        rad[r] = i < n ? radius[i] : -1.f;
    }
    unsigned long long key = kNoPick;
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        const float d2 = dist2(p[r], x, y);
        const float rr = rad[r] * rad[r];
        if (i < n && d2 <= rr) {
            const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | i;
            key = k < key ? k : key;
        }
    }
    key = wave_min_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = kNoPick;
#pragma unroll
        for (int v = 0; v < kQueryWaves; ++v) best = s_key[v] < best ? s_key[v] : best;
        tile_key[blockIdx.x] = best;
    }
}

// min over the tiles' keys into *pick (set to kNoPick before): grid-stride, one atomic per workgroup
constexpr int kPickFoldBlocks = 64;
__global__ __launch_bounds__(kQueryBlock) void k_pick_fold(const unsigned long long *__restrict__ tile_key,
                                                           uint64_t tiles, unsigned long long *__restrict__ pick)
{
    __shared__ unsigned long long s_key[kQueryWaves];
    unsigned long long key = kNoPick;
    for (uint64_t t = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; t < tiles; t += (uint64_t)gridDim.x * kQueryBlock)
        key = tile_key[t] < key ? tile_key[t] : key;
    key = wave_min_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = kNoPick;
#pragma unroll
        for (int v = 0; v < kQueryWaves; ++v) best = s_key[v] < best ? s_key[v] : best;
        if (best != kNoPick) atomicMin(pick, best);
    }
}

uint64_t query_tiles(uint64_t n) { return (n + kQueryTile - 1) / kQueryTile; }

static gpe_status check_tiles(gpe_ctx *c, uint64_t tiles)
{
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "query: bad particle count");
    return GPE_OK;
}

gpe_status launch_query_count(gpe_ctx *c, int kind, const float *region, uint32_t *tile_count)
{
    const uint64_t tiles = query_tiles(c->n);
    GPE_TRY(check_tiles(c, tiles));
    const QueryRegion Q{region[0], region[1], region[2], region[3], region[4]};
    const auto kern = kind == kQuerySegment ? k_query_count<kQuerySegment>
                      : kind == kQueryBox   ? k_query_count<kQueryBox>
                                            : k_query_count<kQueryCircle>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, Q, c->pos, c->radius, c->n, tile_count);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_query_gather(gpe_ctx *c, int kind, const float *region, const uint32_t *tile_scanned,
                               uint32_t capacity, uint32_t *index_out, uint32_t *uid_out, float2 *pos_out,
                               float2 *prev_out, float *radius_out)
{
    const uint64_t tiles = query_tiles(c->n);
    GPE_TRY(check_tiles(c, tiles));
    const QueryRegion Q{region[0], region[1], region[2], region[3], region[4]};
    const QueryOut O{index_out, uid_out, pos_out, prev_out, radius_out};
    const auto kern = kind == kQuerySegment ? k_query_gather<kQuerySegment>
                      : kind == kQueryBox   ? k_query_gather<kQueryBox>
                                            : k_query_gather<kQueryCircle>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, Q, c->pos, c->prev, c->radius,
                       (const uint32_t *)c->uid.uids, c->n, tile_scanned, capacity, O);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_pick(gpe_ctx *c, float x, float y, unsigned long long *tile_key, unsigned long long *pick)
{
    const uint64_t tiles = query_tiles(c->n);
    GPE_TRY(check_tiles(c, tiles));
    hipLaunchKernelGGL(k_pick, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, x, y, c->pos, c->radius, c->n,
                       tile_key);
    GPE_HIP(c, hipGetLastError());
    GPE_HIP(c, hipMemsetAsync(pick, 0xFF, sizeof(*pick), c->stream));
    const uint64_t g = std::min<uint64_t>((tiles + 4 * kQueryBlock - 1) / (4 * kQueryBlock), kPickFoldBlocks);
    hipLaunchKernelGGL(k_pick_fold, dim3((uint32_t)g), dim3(kQueryBlock), 0, c->stream, tile_key, tiles, pick);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
