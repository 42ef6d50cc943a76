// k_mover_build.h -- what k_movers_build (k_movers.hip) and k_movers_sweep_build (k_mover_sweep.hip) share: one
// workgroup of kMoverBuildBlock lanes per mover j.
//
// mover_build_advance, lane 0 alone: reads the state (pose[4], pose[5]), advances it by B.dt, poses the capsule into c1
// and writes state, pose and B.rec[2 j] back.  with_old: the capsule the OLD state poses goes to c0 and to B.old[j]
// first (a function of the state alone; c0 may be c1 where the caller needs the new one only).  Returns both states;
// the caller shares what its listing needs through LDS.  (m by value: behind a reference the two poses compiled to 22
// more instructions.)
//
// mover_build_list, the whole workgroup after the barrier: strides over the cells of the rectangle [x0, x1] x [y0, y1]
// (inside the grid), sets mover j's bit in the mask of every cell that `everywhere` or listed(cx, cy) names, the cell's
// summary bit where the mask word was zero, and adds the bits set to *B.listed, one atomic per wave.
#pragma once

#include "gpe_internal.h"
#include "k_mover.h"

namespace gpe {

constexpr int kMoverBuildBlock = 256;

struct MoverBuildStep {
    float p0, p1;                // the state before the advance
    float q0, q1;                // ... and after
};

__device__ __forceinline__ MoverBuildStep mover_build_advance(const MoverBuildArgs &B, const MoverDef m, uint32_t j,
                                                              bool with_old, float *c0, float *c1)
{
    float *pose = B.pose + 6ull * j;
    MoverBuildStep s;
    s.p0 = pose[4];
    s.p1 = pose[5];
    float q0 = s.p0, q1 = s.p1;
    if (with_old) {
        mover_pose(m, q0, q1, c0);
        B.old[j] = make_float4(c0[0], c0[1], c0[2], c0[3]);
    }
    mover_advance(m, B.dt, &q0, &q1);
    mover_pose(m, q0, q1, c1);
    pose[0] = c1[0]; pose[1] = c1[1]; pose[2] = c1[2]; pose[3] = c1[3];
    pose[4] = q0; pose[5] = q1;
    B.rec[2 * j] = make_float4(c1[0], c1[1], c1[2], c1[3]);
    s.q0 = q0;
    s.q1 = q1;
    return s;
}

template <class Listed>
__device__ __forceinline__ void mover_build_list(const MoverBuildArgs &B, uint32_t j, uint32_t x0, uint32_t y0, uint32_t x1,
                                                 uint32_t y1, bool everywhere, Listed listed)
{
    const uint32_t w = x1 - x0 + 1, total = w * (y1 - y0 + 1);  // <= 128 * 128
    const uint32_t word = j >> 6;
    const unsigned long long bit = 1ull << (j & 63u);
    uint32_t count = 0;                                         // wave-uniform
    for (uint32_t t0 = 0; t0 < total; t0 += kMoverBuildBlock) {
        const uint32_t t = t0 + threadIdx.x;
        bool hit = false;
        if (t < total) {
            const uint32_t cx = x0 + t % w, cy = y0 + t / w;    // cx <= x1 < gx, cy <= y1 < gy
            hit = everywhere || listed(cx, cy);
            if (hit) {
                const uint32_t cell = cy * B.g.view.gx + cx;
                const unsigned long long old = atomicOr(&B.masks[(uint64_t)cell * B.words + word], bit);
                if (old == 0) atomicOr(&B.summary[cell], 1u << word);
            }
        }
        count += (uint32_t)__popcll(ballot64(hit));
    }
    if (lane_id() == 0 && count) atomicAdd(B.listed, (unsigned long long)count);
}

}  // namespace gpe
