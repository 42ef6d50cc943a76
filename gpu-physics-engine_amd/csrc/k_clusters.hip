// k_clusters.hip -- contact clusters (gpe_query_clusters / gpe_query_cluster_of): the connected components of the graph
// whose edges are the contacts of gpe_query_contacts.  Passes over the live set on the device (gfx950, wave64) that read
// the particles and write only scratch of their own.
//
// Not on the per-step path.  Stages (1) and (2) are the contact query's (k_contacts.hip): cell keys, sort_pairs, one
// 16-byte record per sorted slot.  Then:
//   (3) k_clusters_init: parent[i] = i -- every particle is the root of its own tree.
//   (4) k_clusters_hook: lane t takes sorted slot t and walks its three row runs as k_contacts_count does.  For every hit
//       whose partner's index is below its own it unites the two trees of a lock-free union-find: each edge once, from
//       its higher end.  To unite: find both roots; equal -- nothing to do; else compare-and-swap the LARGER root from
//       itself to the smaller one, and on failure go on from the value the CAS returned.
//       The forest keeps three properties at every instant, whatever the interleaving:
//         (a) parent[x] <= x, with equality exactly for a root -- so there is no cycle and every walk up descends;
//         (b) a particle that has stopped being a root never becomes one again: only the CAS writes a root, and it
//             writes a smaller index; path halving writes only non-roots, and only an index below their own;
//         (c) parent[x] lies in x's component -- the CAS joins two components that an edge joins, halving re-points
//             x at a particle of its own tree.
//       With (a) the root of a finished component is its lowest index, whoever won which race: the labels do not depend
//       on the launch geometry.  Every access to parent[] here is a relaxed atomic at agent scope: the L2s of the XCDs
//       and the L1s of the CUs are not coherent for plain accesses within a launch.  A stale parent only costs a retry,
//       because the CAS decides at the memory itself whether x is still a root.
//       No lane waits for another workgroup (or another lane): a loop ends by its own successful CAS, or goes on from
//       a strictly smaller index because somebody else's CAS succeeded, or follows a strictly decreasing parent.
//       find halves the path as it goes; without it a line of particles stored in descending order builds one chain of
//       length n.  The lane keeps the root it last saw for itself in a register and skips a partner whose parent is
//       that root -- in a pile almost every pair.
//   (5) k_clusters_flatten, a later launch (the kernel boundary publishes the forest): label[i] = root(i), halving on the
//       way with the same atomics (nobody hooks any more: only rule-(b) writes remain), and the number of roots per
//       workgroup; k_clusters_fold adds the workgroups' words (the pattern of k_contacts_fold).
//   (6) k_clusters_tally: root_size[label[i]] += 1 (zeroed before), aggregated per wave -- one integer atomic per distinct
//       label among a wave's lanes, so that a pile which is one cluster costs n / 64 atomics on its root, not n.
//       k_clusters_sizes, the next launch: size[i] = root_size[label[i]], label_uid[i] = uids[label[i]] when asked for,
//       and per workgroup the max over its roots of size << 32 | (0xFFFFFFFF - label): the largest cluster, the lowest
//       label on a tie.  k_clusters_max_fold folds the workgroups' keys (the pattern of k_pick_fold).
//   Members (gpe_query_cluster_of): k_clusters_member_count / _gather are k_query_count / k_query_gather with the
//       predicate label[i] == the seed's label, in the region queries' tile shape, ranked by the same scan.
// Everything here is integers and independent of order: tests/_clusters_model.py reproduces it bit for bit.
#include <algorithm>

#include "k_contacts.h"
#include "k_region.h"

namespace gpe {

constexpr int kClustersFoldBlocks = 64;

__device__ __forceinline__ uint32_t parent_load(const uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void parent_store(uint32_t *parent, uint32_t x, uint32_t v)
{
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this lane can see (it may have been hooked below since).  Path halving: x, seen to be
// no root, is re-pointed at its grandparent -- an index below parent[x], in x's tree (rules (b) and (c) above).
__device__ __forceinline__ uint32_t clusters_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = parent_load(parent, x);
    while (p != x) {                                          // p < x
        const uint32_t g = parent_load(parent, p);            // g <= p
        if (g == p) return p;
        parent_store(parent, x, g);
        x = p;
        p = g;
    }
    return x;
}

// Unite the trees of a and b; returns the root the two share afterwards as far as this lane can see.
__device__ __forceinline__ uint32_t clusters_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    uint32_t ra = clusters_find(parent, a), rb = clusters_find(parent, b);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        // hi was hooked by somebody else in the meantime: seen = its parent now, below hi
        const uint32_t r = clusters_find(parent, seen);
        ra = r;
        rb = lo;
    }
    return ra;
}

// (3)
__global__ __launch_bounds__(kStreamBlock) void k_clusters_init(uint32_t *__restrict__ parent, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kStreamBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kStreamBlock + threadIdx.x; i < n; i += stride) parent[i] = (uint32_t)i;
}

// (4) no barrier in this kernel
__global__ __launch_bounds__(kContactsBlock) void k_clusters_hook(const uint32_t *__restrict__ keys,
                                                                  const uint4 *__restrict__ rec, uint32_t n,
                                                                  uint32_t *parent)
{
    const uint64_t t64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    if (t64 >= n) return;
    const uint32_t t = (uint32_t)t64;
    const uint4 me = rec[t];
    const uint32_t key = keys[t];
    const float x = __uint_as_float(me.x), y = __uint_as_float(me.y), r = __uint_as_float(me.z);
    uint32_t root = me.w;                                     // a particle of my tree, its root when last seen
    for (int dy = -1; dy <= 1; ++dy) {
        uint32_t s, e, k_mid;
        if (!contacts_row_run(keys, n, key, dy, &s, &e, &k_mid)) continue;
        for (uint32_t j = s; j < e; ++j) {
            const uint4 o = rec[j];
            float q, rs;
            if (o.w >= me.w) continue;                        // (j == t too) the edge belongs to its higher end
            if (!in_contact(x, y, r, __uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z), &q, &rs)) continue;
            if (parent_load(parent, o.w) == root) continue;   // already below my root
            root = clusters_unite(parent, root, o.w);
        }
    }
}

// (5) label[i] and the workgroup's number of roots
__global__ __launch_bounds__(kContactsBlock) void k_clusters_flatten(uint32_t *parent, uint32_t n,
                                                                     uint32_t *__restrict__ label,
                                                                     unsigned long long *__restrict__ tile_sum)
{
    __shared__ unsigned long long s_sum[kContactsWaves];
    const uint64_t i64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    unsigned long long roots = 0;
    if (i64 < n) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t l = clusters_find(parent, i);
        label[i] = l;
        roots = l == i ? 1ull : 0ull;
    }
    const unsigned long long sum = wave_sum_u64(roots);
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
__global__ __launch_bounds__(kContactsBlock) void k_clusters_fold(const unsigned long long *__restrict__ tile_sum,
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

// (6) root_size[l] += the number of particles labelled l: one atomic per distinct label among the lanes of a wave
__global__ __launch_bounds__(kContactsBlock) void k_clusters_tally(const uint32_t *__restrict__ label, uint32_t n,
                                                                   uint32_t *__restrict__ root_size)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    bool todo = i64 < n;
    const uint32_t l = todo ? label[i64] : 0u;
    uint64_t m = ballot64(todo);
    while (m) {                                               // wave-uniform: one round per distinct label
        const int first = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m));
        const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)l, first);
        const uint64_t same = ballot64(todo && l == l0);
        if (lane_id() == first) atomicAdd(&root_size[l0], (uint32_t)__popcll(same));
        todo = todo && l != l0;
        m &= ~same;
    }
}

// size[i], label_uid[i] (NULL: not requested) and the workgroup's max of size << 32 | (0xFFFFFFFF - label) over its roots
__global__ __launch_bounds__(kContactsBlock) void k_clusters_sizes(const uint32_t *__restrict__ label,
                                                                   const uint32_t *__restrict__ root_size, uint32_t n,
                                                                   const uint32_t *__restrict__ uids,
                                                                   uint32_t *__restrict__ size,
                                                                   uint32_t *__restrict__ label_uid,
                                                                   unsigned long long *__restrict__ tile_key)
{
    __shared__ unsigned long long s_key[kContactsWaves];
    const uint64_t i64 = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x;
    unsigned long long key = 0;
    if (i64 < n) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t l = label[i];
        const uint32_t sz = root_size[l];
        size[i] = sz;
        if (label_uid) label_uid[i] = uids[l];
        if (l == i) key = ((unsigned long long)sz << 32) | (0xFFFFFFFFu - l);
    }
    key = wave_max_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = 0;
#pragma unroll
        for (int v = 0; v < kContactsWaves; ++v) best = s_key[v] > best ? s_key[v] : best;
        tile_key[blockIdx.x] = best;
    }
}

// max over the workgroups' keys into *best (zeroed before): grid-stride, one atomic per workgroup
__global__ __launch_bounds__(kContactsBlock) void k_clusters_max_fold(const unsigned long long *__restrict__ tile_key,
                                                                      uint64_t tiles, unsigned long long *__restrict__ best)
{
    __shared__ unsigned long long s_key[kContactsWaves];
    unsigned long long key = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kContactsBlock + threadIdx.x; t < tiles; t += (uint64_t)gridDim.x * kContactsBlock)
        key = tile_key[t] > key ? tile_key[t] : key;
    key = wave_max_u64(key);
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (int v = 0; v < kContactsWaves; ++v) all = s_key[v] > all ? s_key[v] : all;
        if (all) atomicMax(best, all);
    }
}

// hit[r] for the rounds of this thread's tile (false past n): the particle carries the label `want`
__device__ __forceinline__ void members_of_tile(const uint32_t *__restrict__ label, uint64_t n, uint64_t first,
                                                uint32_t want, bool (&hit)[kQueryRounds])
{
    uint32_t l[kQueryRounds];
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        l[r] = i < n ? label[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) hit[r] = first + (uint64_t)r * kQueryBlock < n && l[r] == want;
}

// members per tile (the tiles of k_query_count)
__global__ __launch_bounds__(kQueryBlock) void k_clusters_member_count(const uint32_t *__restrict__ label, uint64_t n,
                                                                       uint32_t want, uint32_t *__restrict__ tile_count)
{
    __shared__ uint32_t s_cnt[kQueryWaves];
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    bool hit[kQueryRounds];
    members_of_tile(label, n, first, want, hit);
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

// Where the member gather writes: one row per member ranked below capacity; NULL = not requested (never loaded).
struct MemberOut {
    uint32_t *index;
    uint32_t *uid;
    float2 *pos;
    float2 *prev;
    float *radius;
};

// the members ranked below capacity, in ascending storage index; tile_scanned = inclusive scan of the counts above
__global__ __launch_bounds__(kQueryBlock) void k_clusters_member_gather(const uint32_t *__restrict__ label, uint32_t want,
                                                                        const float2 *__restrict__ pos,
                                                                        const float2 *__restrict__ prev,
                                                                        const float *__restrict__ radius,
                                                                        const uint32_t *__restrict__ uids, uint64_t n,
                                                                        const uint32_t *__restrict__ tile_scanned,
                                                                        uint32_t capacity, MemberOut O)
{
    __shared__ uint32_t s_cnt[kQueryRounds][kQueryWaves];
    uint32_t base = blockIdx.x ? tile_scanned[blockIdx.x - 1] : 0u;   // members of the earlier tiles
    const uint32_t end = tile_scanned[blockIdx.x];
    if (end == base || base >= capacity) return;                      // block-uniform: before any barrier
    const uint64_t first = (uint64_t)blockIdx.x * kQueryTile + threadIdx.x;
    const int w = (int)(threadIdx.x >> 6);
    bool hit[kQueryRounds];
    members_of_tile(label, n, first, want, hit);
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
                if (O.pos) O.pos[dst] = pos[i];
                if (O.prev) O.prev[dst] = prev[i];
                if (O.radius) O.radius[dst] = radius[i];
                if (O.uid) O.uid[dst] = uids[i];
            }
        }
        base += round;
    }
}

static gpe_status clusters_check(gpe_ctx *c, uint64_t tiles)
{
    if (tiles == 0 || c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "clusters: bad particle count");
    return GPE_OK;
}

static uint32_t clusters_fold_grid(uint64_t tiles)
{
    return (uint32_t)std::min<uint64_t>((tiles + 4 * kContactsBlock - 1) / (4 * kContactsBlock), kClustersFoldBlocks);
}

gpe_status launch_clusters_hook(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, uint32_t *parent)
{
    const uint64_t tiles = contacts_tiles(c->n);
    GPE_TRY(clusters_check(c, tiles));
    hipLaunchKernelGGL(k_clusters_init, dim3(stream_grid(c->n)), dim3(kStreamBlock), 0, c->stream, parent, c->n);
    GPE_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_clusters_hook, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, keys, rec,
                       (uint32_t)c->n, parent);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_clusters_flatten(gpe_ctx *c, uint32_t *parent, uint32_t *label, unsigned long long *tile_word,
                                   unsigned long long *count)
{
    const uint64_t tiles = contacts_tiles(c->n);
    GPE_TRY(clusters_check(c, tiles));
    hipLaunchKernelGGL(k_clusters_flatten, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, parent,
                       (uint32_t)c->n, label, tile_word);
    GPE_HIP(c, hipGetLastError());
    GPE_HIP(c, hipMemsetAsync(count, 0, sizeof(*count), c->stream));
    hipLaunchKernelGGL(k_clusters_fold, dim3(clusters_fold_grid(tiles)), dim3(kContactsBlock), 0, c->stream, tile_word,
                       tiles, count);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_clusters_sizes(gpe_ctx *c, const uint32_t *label, uint32_t *root_size, uint32_t *size,
                                 uint32_t *label_uid, unsigned long long *tile_word, unsigned long long *largest)
{
    const uint64_t tiles = contacts_tiles(c->n);
    GPE_TRY(clusters_check(c, tiles));
    GPE_HIP(c, hipMemsetAsync(root_size, 0, c->n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_clusters_tally, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, label, (uint32_t)c->n,
                       root_size);
    GPE_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_clusters_sizes, dim3((uint32_t)tiles), dim3(kContactsBlock), 0, c->stream, label, root_size,
                       (uint32_t)c->n, (const uint32_t *)c->uid.uids, size, label_uid, tile_word);
    GPE_HIP(c, hipGetLastError());
    GPE_HIP(c, hipMemsetAsync(largest, 0, sizeof(*largest), c->stream));
    hipLaunchKernelGGL(k_clusters_max_fold, dim3(clusters_fold_grid(tiles)), dim3(kContactsBlock), 0, c->stream, tile_word,
                       tiles, largest);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

static gpe_status member_tiles(gpe_ctx *c, uint64_t *tiles)
{
    *tiles = query_tiles(c->n);
    if (*tiles == 0 || *tiles > 0x7FFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "clusters: bad particle count");
    return GPE_OK;
}

gpe_status launch_clusters_member_count(gpe_ctx *c, const uint32_t *label, uint32_t want, uint32_t *tile_count)
{
    uint64_t tiles = 0;
    GPE_TRY(member_tiles(c, &tiles));
    hipLaunchKernelGGL(k_clusters_member_count, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, label, c->n, want,
                       tile_count);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_clusters_member_gather(gpe_ctx *c, const uint32_t *label, uint32_t want, const uint32_t *tile_scanned,
                                         uint32_t capacity, uint32_t *index_out, uint32_t *uid_out, float2 *pos_out,
                                         float2 *prev_out, float *radius_out)
{
    uint64_t tiles = 0;
    GPE_TRY(member_tiles(c, &tiles));
    const MemberOut O{index_out, uid_out, pos_out, prev_out, radius_out};
    hipLaunchKernelGGL(k_clusters_member_gather, dim3((uint32_t)tiles), dim3(kQueryBlock), 0, c->stream, label, want,
                       c->pos, c->prev, c->radius, (const uint32_t *)c->uid.uids, c->n, tile_scanned, capacity, O);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
