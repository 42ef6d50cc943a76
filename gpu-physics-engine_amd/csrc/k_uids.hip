// k_uids.hip -- opt-in particle uids (gpe_enable_uids, gpe_find_uids, gpe_remove_particles_by_uid; gfx950, wave64).
//
// A uid is a u32 the library carries with every particle through each permutation it makes.  Nothing here runs while
// uids are off.
//   - k_rearrange_uids: K4 (k_particles.hip) plus the uid, gathered through the same sorted ids.  R 4 B (id) + 24 B
//     (pos, prev, radius) + 4 B (uid), W 24 B + 4 B: 52 B per particle against K4's 44.  The uid-off re-sort still
//     launches k_rearrange itself.
//   - the uid -> index map: (uid, index) pairs sorted by uid with the context's own sort_pairs (4 radix passes), then
//     one pass over adjacent keys for duplicates; the largest uid is the last key.  Built when a lookup needs it and
//     the map is stale (gpe_api.hip clears the flag at every set, add, removal, re-sort, enable and set_uids).
//   - k_uid_find / k_uid_mark: one lane per query, a lower_bound over the sorted keys.  The trip count is
//     ceil(log2 n) for every lane (n is uniform) and each step is a select, so a wave does not diverge.
#include "k_uids.h"

namespace gpe {

__global__ __launch_bounds__(kStreamBlock) void k_uid_iota(uint32_t *__restrict__ uids, uint64_t lo, uint64_t hi,
                                                            uint32_t first)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride)
        uids[i] = first + (uint32_t)(i - lo);
}

__global__ __launch_bounds__(kStreamBlock) void k_rearrange_uids(const float2 *__restrict__ pos,
                                                                  const float2 *__restrict__ prev,
                                                                  const float *__restrict__ radius,
                                                                  const uint32_t *__restrict__ uids,
                                                                  const uint32_t *__restrict__ ids, uint64_t n,
                                                                  float2 *__restrict__ pos_out,
                                                                  float2 *__restrict__ prev_out,
                                                                  float *__restrict__ radius_out,
                                                                  uint32_t *__restrict__ uids_out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t r = ids[i];
        const float2 p = pos[r];
        const float rad = radius[r];
        const float2 q = prev[r];
        const uint32_t u = uids[r];
        pos_out[i] = p;
        radius_out[i] = rad;
        prev_out[i] = q;
        uids_out[i] = u;
    }
}

__global__ __launch_bounds__(kStreamBlock) void k_uid_map_init(const uint32_t *__restrict__ uids, uint64_t n,
                                                                uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        keys[i] = uids[i];
        vals[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kStreamBlock) void k_uid_adjacent(const uint32_t *__restrict__ keys, uint64_t n,
                                                                uint32_t *__restrict__ dup)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool same = false;
    for (uint64_t i = 1 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        same |= keys[i] == keys[i - 1];
    if (ballot64(same) != 0 && lane_id() == 0) *dup = 1u;
}

__global__ __launch_bounds__(kStreamBlock) void k_uid_find(const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals, uint32_t n,
                                                            const uint32_t *__restrict__ query, uint64_t k,
                                                            const float2 *__restrict__ pos,
                                                            const float2 *__restrict__ prev,
                                                            const float *__restrict__ radius,
                                                            uint32_t *__restrict__ index_out,
                                                            float2 *__restrict__ pos_out,
                                                            float2 *__restrict__ prev_out,
                                                            float *__restrict__ radius_out)
{
    const float nan = __uint_as_float(0x7FC00000u);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
        const uint32_t j = uid_lookup(keys, vals, n, query[i]);
        const bool found = j != GPE_UID_ABSENT;
        index_out[i] = j;
        if (pos_out) pos_out[i] = found ? pos[j] : make_float2(nan, nan);          // (uniform pointer tests)
        if (prev_out) prev_out[i] = found ? prev[j] : make_float2(nan, nan);
        if (radius_out) radius_out[i] = found ? radius[j] : nan;
    }
}

__global__ __launch_bounds__(kStreamBlock) void k_uid_mark(const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals, uint32_t n,
                                                            const uint32_t *__restrict__ query, uint64_t k,
                                                            uint8_t *__restrict__ mask)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
        const uint32_t j = uid_lookup(keys, vals, n, query[i]);
        if (j != GPE_UID_ABSENT) mask[j] = 1;                  // a duplicate query writes the same byte again
    }
}

gpe_status launch_uid_iota(gpe_ctx *c, uint32_t *uids, uint64_t lo, uint64_t hi, uint32_t first)
{
    if (hi <= lo) return GPE_OK;
    hipLaunchKernelGGL(k_uid_iota, dim3(stream_grid(hi - lo)), dim3(kStreamBlock), 0, c->stream, uids, lo, hi, first);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_rearrange_uids(gpe_ctx *c, const float2 *pos, const float2 *prev, const float *radius,
                                 const uint32_t *uids, const uint32_t *ids, uint64_t n, float2 *pos_out,
                                 float2 *prev_out, float *radius_out, uint32_t *uids_out)
{
    if (n == 0) return GPE_OK;
    Scope s(c, "Particle rearranging");  // particle_rearrange.rs:194
    hipLaunchKernelGGL(k_rearrange_uids, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, pos, prev, radius,
                       uids, ids, n, pos_out, prev_out, radius_out, uids_out);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_uid_map_init(gpe_ctx *c, const uint32_t *uids, uint64_t n, uint32_t *keys, uint32_t *vals)
{
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(k_uid_map_init, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, uids, n, keys, vals);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_uid_adjacent(gpe_ctx *c, const uint32_t *keys, uint64_t n, uint32_t *dup)
{
    if (n < 2) return GPE_OK;
    hipLaunchKernelGGL(k_uid_adjacent, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, keys, n, dup);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_uid_find(gpe_ctx *c, const uint32_t *keys, const uint32_t *vals, uint64_t n, const uint32_t *query,
                           uint64_t k, uint32_t *index_out, float2 *pos_out, float2 *prev_out, float *radius_out)
{
    if (k == 0) return GPE_OK;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(c, GPE_ERR_STATE, "uid lookup: bad map size");
    hipLaunchKernelGGL(k_uid_find, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, keys, vals, (uint32_t)n,
                       query, k, c->pos, c->prev, c->radius, index_out, pos_out, prev_out, radius_out);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_uid_mark(gpe_ctx *c, const uint32_t *keys, const uint32_t *vals, uint64_t n, const uint32_t *query,
                           uint64_t k, uint8_t *mask)
{
    if (k == 0) return GPE_OK;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(c, GPE_ERR_STATE, "uid lookup: bad map size");
    hipLaunchKernelGGL(k_uid_mark, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, keys, vals, (uint32_t)n,
                       query, k, mask);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
