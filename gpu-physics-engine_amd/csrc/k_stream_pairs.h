// k_stream_pairs.h -- the pair loop of the world-anchored passes (gfx950, wave64): the one streaming body behind the
// colliders', the movers', the two swept and the fields' pass kernels.
//
// What the template guarantees.  Every particle i < n is resolved exactly once, by one lane: lane t of the grid takes
// the pairs t, t + stride, ..., so pos (and prev where PREV) is read 16 B per lane; an odd n leaves particle n - 1 to
// thread 0 of block 0, read 8 B.  Both particles of a pair are resolved before either is stored, and the votes come
// after the stores.  Nothing else is read or written here: every other access is the pass's.  The launch is
// stream_grid((n + 1) >> 1) workgroups of kStreamBlock.
//
// What a pass supplies.
//     FLAGS                               how many flags it votes on: bit b of what resolve returns, b < FLAGS
//     resolve(i, px, py, qx, qy, o)       the rule for particle i at p with the previous position q (0, 0 without
//                                         PREV).  Returns the particle's flags -- a bool where FLAGS is 1, else a
//                                         uint32_t; 0: nothing happened to it -- and, where they are not 0, fills what
//                                         store needs of the float4 o
//     store(i, flags, o, px, py, qx, qy)  writes particle i; called only with flags that are not 0.  It decides which
//                                         bytes are written
// Both are callables inlined into the loop (the form k_uid_nodes.h settled on).  The flags keep resolve's type and the
// stores stand under them here: as a uint32_t, or under a test of the pass's own, the flag was materialised per lane
// (profiles/capsule_passes/README.md).
//
// What comes back: per flag, the number of particles of this wave that set it -- valid in lane 0 of every wave, which
// is where the kernel's epilogue (one atomic per flag and wave, or the fields' fold through LDS) reads it.
//
// first and stride are not for a pass to give: as default arguments they are read where the loop is called.  Called from
// the kernel function itself (k_fields_pass) the compiler folds blockDim to one scalar load; read inside an inlined
// body it became a dependent vector load in front of the first pos load, which cost the fields' pass 1 to 2 %.
#pragma once

#include "gpe_internal.h"

namespace gpe {

template <int FLAGS>
struct PairCounts {
    uint32_t of[FLAGS];
};

template <int FLAGS, bool PREV, class Resolve, class Store>
__device__ __forceinline__ PairCounts<FLAGS> stream_pairs(const float2 *pos, const float2 *prev, uint64_t n, Resolve resolve,
                                                          Store store,
                                                          uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x,
                                                          uint64_t stride = (uint64_t)gridDim.x * blockDim.x)
{
    const uint64_t pairs = n >> 1;
    const float4 *pos4 = reinterpret_cast<const float4 *>(pos);
    const float4 *prev4 = reinterpret_cast<const float4 *>(prev);
    // a ballot counts the lanes still in the loop, so the sums are wave-uniform among them.  Lane 0 holds the wave's
    // lowest index, leaves the loop last and so has seen every vote
    PairCounts<FLAGS> count;
#pragma unroll
    for (int b = 0; b < FLAGS; ++b) count.of[b] = 0;
    for (uint64_t i = first; i < pairs; i += stride) {
        const float4 c = pos4[i];
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (PREV) q = prev4[i];
        float4 o0, o1;
        const auto f0 = resolve(2 * i, c.x, c.y, q.x, q.y, o0);
        const auto f1 = resolve(2 * i + 1, c.z, c.w, q.z, q.w, o1);
        if (f0) store(2 * i, f0, o0, c.x, c.y, q.x, q.y);
        if (f1) store(2 * i + 1, f1, o1, c.z, c.w, q.z, q.w);
#pragma unroll
        for (int b = 0; b < FLAGS; ++b)
            count.of[b] += (uint32_t)__popcll(ballot64(f0 & (1u << b))) + (uint32_t)__popcll(ballot64(f1 & (1u << b)));
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        float2 q = make_float2(0.0f, 0.0f);
        if constexpr (PREV) q = prev[i];
        float4 o;
        const auto f = resolve(i, c.x, c.y, q.x, q.y, o);
        if (f) {
            store(i, f, o, c.x, c.y, q.x, q.y);
#pragma unroll
            for (int b = 0; b < FLAGS; ++b) count.of[b] += (f & (1u << b)) ? 1u : 0u;
        }
    }
    return count;
}

}  // namespace gpe
