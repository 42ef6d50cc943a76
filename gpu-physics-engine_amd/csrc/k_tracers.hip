// k_tracers.hip -- the tracer recorder's device side (gpe_tracers_*, include/gpe.h; gfx950, wave64).
//
// The recorder follows k <= GPE_TRACERS_MAX particles named by uid.  Nothing here runs on a context that is not armed.
//   - k_tracers_resolve: slot_index[j] = the storage index of tracer j, for every tracer that exists.  One streaming
//     pass over the n live uids (4 B per particle), launched only when something has moved the particles or changed
//     their uids since the last frame; the table was set to 0xffffffff before it.  The tracked uids come sorted
//     ascending (keys) with the tracer each belongs to (perm), both written once at gpe_tracers_begin.
//       . the uids are read 16 bytes per lane, the n % 4 last ones one per lane: no read behind uids[n)
//       . a uid outside [keys[0], keys[k-1]] is rejected on two compares; a wave with no candidate goes on
//       . the others are searched in two levels.  Every 16th key is staged in LDS (k / 16 <= 4096 words, 16 KiB: the
//         whole list of 65 536 keys is 256 KiB and does not fit in the CU's 160 KiB): a halving search there, then at
//         most four more probes among the <= 16 keys of that group, which stay in L2 (the list is read by every
//         workgroup and written by nobody).  Both loops have the same trip count on every lane and a select per step.
//       . uids are pairwise distinct (gpe_set_uids checks it, every other source hands out fresh ones), so each slot has
//         at most one writer: a plain store, and the result does not depend on the launch order.
//     A lane searches the four uids of its 16-byte group side by side (four independent chains of dependent loads), and
//     a workgroup takes 1024 particles per pass: at 1 M particles that is four waves per SIMD.  One uid at a time and
//     4096 particles per workgroup -- a quarter of the staging -- left one wave per SIMD waiting on its own loads:
//     27 against 15 us at 1 M for 1024 tracers, 46 against 31 us for 65 536 (profiles/tracers/).
//   - k_tracers_sample: one lane per tracer.  Row j of the frame = the bits of pos / prev of particle slot_index[j] and
//     that index, or quiet NaN and GPE_UID_ABSENT.  The pointers are those that are live after the step (the native step
//     swaps pos with its copy partner), handed in at the launch.
#include <algorithm>

#include "gpe_internal.h"

namespace gpe {

constexpr int kTracerStride = 16;                                      // every 16th sorted key is staged in LDS
constexpr int kTracerCoarseMax = GPE_TRACERS_MAX / kTracerStride;      // 4096 words
constexpr int kTracerGroupsPerBlock = kStreamBlock;                    // uint4 groups per workgroup and pass: one per lane

// W uids u[e] of storage index first + e against the tracked set, searched side by side: the W chains of dependent
// loads (<= 12 from LDS, then <= 4 from L2) are independent of each other.  coarse[0 .. nc): keys[16 * c]; top: the
// largest power of two below nc (0 when nc == 1).  A uid below keys[0] stays at key 0 and one above keys[k-1] ends at
// the last key: neither equals it, so the range test in front is only the fast way out.
template <int W>
__device__ __forceinline__ void tracer_match(const uint32_t (&u)[W], const uint32_t first,
                                             const uint32_t *__restrict__ coarse, const uint32_t nc, const uint32_t top,
                                             const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                             const uint32_t k, uint32_t *__restrict__ slot_index)
{
    uint32_t g[W];                                                     // the last group whose first key is <= u
#pragma unroll
    for (int e = 0; e < W; ++e) g[e] = 0;
    for (uint32_t step = top; step; step >>= 1) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const uint32_t q = g[e] + step;
            g[e] = (q < nc && coarse[q < nc ? q : 0] <= u[e]) ? q : g[e];
        }
    }
    uint32_t p[W], val[W], end[W];                                     // keys[p] == val (<= u for a uid in range)
#pragma unroll
    for (int e = 0; e < W; ++e) {
        p[e] = g[e] * kTracerStride;
        val[e] = coarse[g[e]];
        end[e] = min(p[e] + (uint32_t)kTracerStride, k);
    }
#pragma unroll
    for (uint32_t step = kTracerStride / 2; step; step >>= 1) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const uint32_t q = p[e] + step;
            const uint32_t kq = keys[q < end[e] ? q : p[e]];           // (an in-range address for the lanes past the end)
            const bool take = q < end[e] && kq <= u[e];
            p[e] = take ? q : p[e];
            val[e] = take ? kq : val[e];
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e)
        if (val[e] == u[e]) slot_index[perm[p[e]]] = first + e;
}

__global__ __launch_bounds__(kStreamBlock) void k_tracers_resolve(const uint32_t *__restrict__ uids, const uint32_t n,
                                                                   const uint32_t *__restrict__ keys,
                                                                   const uint32_t *__restrict__ perm, const uint32_t k,
                                                                   const uint32_t lo, const uint32_t hi,
                                                                   const uint32_t top, uint32_t *__restrict__ slot_index)
{
    __shared__ uint32_t coarse[kTracerCoarseMax];
    const uint32_t nc = (k + kTracerStride - 1) / kTracerStride;
    for (uint32_t c = threadIdx.x; c < nc; c += kStreamBlock) coarse[c] = keys[c * kTracerStride];
    __syncthreads();

    const uint32_t groups = n >> 2;                                    // whole groups of four uids: 16-byte loads
    const uint4 *__restrict__ uids4 = reinterpret_cast<const uint4 *>(uids);
    for (uint32_t g = blockIdx.x * kTracerGroupsPerBlock + threadIdx.x; g < groups; g += gridDim.x * kTracerGroupsPerBlock) {
        const uint4 v = uids4[g];
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
        const bool in = (u[0] >= lo && u[0] <= hi) || (u[1] >= lo && u[1] <= hi) || (u[2] >= lo && u[2] <= hi) ||
                        (u[3] >= lo && u[3] <= hi);
        if (ballot64(in) == 0) continue;                               // wave-uniform: nothing tracked in these 256 uids
        tracer_match<4>(u, 4 * g, coarse, nc, top, keys, perm, k, slot_index);
    }
    if (blockIdx.x == 0) {                                             // the n % 4 last uids, one per lane
        const uint32_t i = 4 * groups + threadIdx.x;
        if (i < n) {
            const uint32_t u[1] = {uids[i]};
            tracer_match<1>(u, i, coarse, nc, top, keys, perm, k, slot_index);
        }
    }
}

__global__ __launch_bounds__(kStreamBlock) void k_tracers_sample(const uint32_t *__restrict__ slot_index, const uint32_t k,
                                                                  const uint32_t n, const float2 *__restrict__ pos,
                                                                  const float2 *__restrict__ prev,
                                                                  float2 *__restrict__ pos_row,
                                                                  float2 *__restrict__ prev_row,
                                                                  uint32_t *__restrict__ index_row)
{
    const float nan = __uint_as_float(0x7FC00000u);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        const uint32_t s = slot_index[j];
        const bool found = s < n;                                      // (0xffffffff: no such particle)
        if (pos_row) pos_row[j] = found ? pos[s] : make_float2(nan, nan);          // (uniform pointer tests)
        if (prev_row) prev_row[j] = found ? prev[s] : make_float2(nan, nan);
        if (index_row) index_row[j] = found ? s : GPE_UID_ABSENT;
    }
}

gpe_status launch_tracers_resolve(gpe_ctx *c, const uint32_t *uids, uint64_t n, const uint32_t *keys, const uint32_t *perm,
                                  uint32_t k, uint32_t lo, uint32_t hi, uint32_t *slot_index)
{
    if (n == 0 || k == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull || k > GPE_TRACERS_MAX) return fail(c, GPE_ERR_STATE, "tracers: bad resolve size");
    const uint32_t nc = (k + kTracerStride - 1) / kTracerStride;
    uint32_t top = 0;
    if (nc > 1) {
        top = 1;
        while (2 * top < nc) top *= 2;                                 // g + top + top/2 + ... + 1 reaches nc - 1
    }
    const uint64_t groups = std::max<uint64_t>(n >> 2, 1);
    hipLaunchKernelGGL(k_tracers_resolve, dim3(stream_grid(groups, kTracerGroupsPerBlock)), dim3(kStreamBlock), 0, c->stream,
                       uids, (uint32_t)n, keys, perm, k, lo, hi, top, slot_index);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_tracers_sample(gpe_ctx *c, const uint32_t *slot_index, uint32_t k, const float2 *pos, const float2 *prev,
                                 uint64_t n, float2 *pos_row, float2 *prev_row, uint32_t *index_row)
{
    if (k == 0) return GPE_OK;
    hipLaunchKernelGGL(k_tracers_sample, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, slot_index, k,
                       (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull), pos, prev, pos_row, prev_row, index_row);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
