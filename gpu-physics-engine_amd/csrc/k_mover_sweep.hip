// k_mover_sweep.hip -- the swept form of the movers' build and pass (gpe_set_mover_sweep; k_mover_sweep.h says what a
// mover carries a point by, what a contact on the relative path is, who wins and when a particle stops).  A translation
// unit of its own: k_movers.hip's kernels are what a context without the mode launches, untouched.
//
// k_movers_sweep_build is k_movers_build (k_mover_build.h) with three additions: it always writes the capsule before
// the advance, it writes one carry record per mover, and it lists the mover in every cell its MOTION reaches (the
// parallelogram of a LINEAR mover, the disc of a ROTATE one) instead of the cells of the new pose alone.
//
// The pass is the pair loop of k_stream_pairs.h with prev.  The common lane has read its 32 B and the summary words of
// the cells of its path's lookup box (one word for a particle that stays in its cell), finds them zero and is done -- no
// radius load, no store.  Under a summary bit the mask words of the box are ORed, one word at a time: ascending bits are
// ascending movers, each judged once.  Three integer counters, one atomic each per wave.
#include "gpe_internal.h"
#include "k_capsule_pass.h"
#include "k_mover_build.h"
#include "k_mover_sweep.h"
#include "k_stream_pairs.h"

namespace gpe {

__global__ __launch_bounds__(kMoverBuildBlock) void k_movers_sweep_build(MoverBuildArgs B, MoverSweepArgs W)
{
    __shared__ float s_cap[8];
    const uint32_t j = blockIdx.x;                              // < B.k: the launch has B.k workgroups
    const MoverDef m = B.def[j];
    const float arm = m.pad0;                                   // mover_arm(m), at set time
    if (threadIdx.x == 0) {
        float c0[4], c1[4];
        const MoverBuildStep s = mover_build_advance(B, m, j, true, c0, c1);
        MoverCarry k;
        mover_carry_of(m, B.dt, s.p0, s.p1, s.q0, s.q1, c0, c1, arm, &k);
        W.carry[j] = k;
        for (int e = 0; e < 4; ++e) {
            s_cap[e] = c0[e];
            s_cap[4 + e] = c1[e];
        }
    }
    __syncthreads();
    const float c0[4] = {s_cap[0], s_cap[1], s_cap[2], s_cap[3]};
    const float c1[4] = {s_cap[4], s_cap[5], s_cap[6], s_cap[7]};
    uint32_t x0, y0, x1, y1;
    bool everywhere;
    if (!mover_sweep_cell_rect(B.g, m, arm, c0, c1, B.rb, &x0, &y0, &x1, &y1, &everywhere)) return;   // (workgroup-uniform)
    mover_build_list(B, j, x0, y0, x1, y1, everywhere,
                     [&](uint32_t cx, uint32_t cy) { return mover_sweep_listed(B.g, m, arm, c0, c1, B.rb, cx, cy); });
}

// the swept rule's policy (k_capsule_pass.h): the masks of a path's box, every mover judged on its own relative path
template <bool SURF>
struct MoverSweepPolicy {
    const MoverPassArgs &P;
    const MoverSweepArgs &W;

    // the candidates of one path: the masks of the cells of its lookup box, or every mover
    struct Cands {
        uint32_t cx0, cx1, cy0, cy1;
        uint32_t summary;        // the OR of the box's summary words
        bool all;
    };

    // false: the path lies in the grid and no cell of its box lists a mover
    __device__ __forceinline__ bool cands(float x0x, float x0y, float x1x, float x1y, Cands &C) const
    {
        C.cx0 = C.cx1 = C.cy0 = C.cy1 = 0;
        C.summary = 0;
        C.all = !sweep_box(P.view, x0x, x0y, x1x, x1y, &C.cx0, &C.cx1, &C.cy0, &C.cy1);
        if (C.all) return true;
        uint32_t s = 0;
        for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy)                   // (cy1 < gy, cx1 < gx: every read lies in the table)
            for (uint32_t cx = C.cx0; cx <= C.cx1; ++cx) s |= P.summary[cy * P.view.gx + cx];
        C.summary = s;
        return s != 0;
    }

    template <class F>
    __device__ __forceinline__ void each(const Cands &C, F f) const
    {
        if (C.all) {
            for (uint32_t j = 0; j < P.k; ++j) f(j);
            return;
        }
        mask_each(C.summary, [&](uint32_t w) {
            unsigned long long bits = 0;
            for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy)
                for (uint32_t cx = C.cx0; cx <= C.cx1; ++cx) bits |= P.masks[(uint64_t)(cy * P.view.gx + cx) * P.words + w];
            return bits;
        }, f);
    }

    // mover_sweep_judge takes the position, then the previous position: the end of the path, then its start
    __device__ __forceinline__ bool judge(uint32_t j, float fromx, float fromy, float tox, float toy, float r,
                                          SweepContact *c) const
    {
        const float4 s = P.rec[2 * j];
        const float cap[4] = {s.x, s.y, s.z, s.w};
        const MoverCarry k = W.carry[j];
        return mover_sweep_judge(k, cap, P.rec[2 * j + 1].x, tox, toy, fromx, fromy, r, c);
    }

    __device__ __forceinline__ void respond(uint32_t who, const SweepContact &win, float px, float py, float qx, float qy,
                                            float r, float *res) const
    {
        const float4 s = P.rec[2 * who];
        const float4 b = P.old[who];
        const float cap[4] = {s.x, s.y, s.z, s.w}, before[4] = {b.x, b.y, b.z, b.w};
        SurfaceRow row = {0.0f, 0.0f, kSurfacePlain, 0u};
        if constexpr (SURF) {
            const float4 sr = P.surf[who];
            row.e = sr.x; row.mu = sr.y; row.flags = __float_as_uint(sr.z);
        }
        mover_sweep_respond(win, before, cap, P.rec[2 * who + 1].x, SURF ? &row : nullptr, px, py, qx, qy, r, P.world_w,
                            P.world_h, res);
    }
};

// the pair loop of k_stream_pairs.h over swept_resolve.  The store skips pos[i] where the response left its bits as
// they were (a mover that only carried the particle's prev), and prev[i] likewise
template <bool SURF>
__device__ __forceinline__ void mover_sweep_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                 const MoverPassArgs &P, const MoverSweepArgs &W)
{
    float2 *__restrict__ prev = W.prev;
    const MoverSweepPolicy<SURF> S{P, W};
    const PairCounts<3> count = stream_pairs<3, true>(
        pos, prev, n,
        [&](uint64_t i, float px, float py, float qx, float qy, float4 &o) -> uint32_t {
            return swept_resolve<SURF>(S, radius, i, px, py, qx, qy, o);
        },
        [&](uint64_t i, uint32_t, const float4 &o, float px, float py, float qx, float qy) {
            if (__float_as_uint(o.x) != __float_as_uint(px) || __float_as_uint(o.y) != __float_as_uint(py))
                pos[i] = make_float2(o.x, o.y);
            if constexpr (SURF) {
                if (__float_as_uint(o.z) != __float_as_uint(qx) || __float_as_uint(o.w) != __float_as_uint(qy))
                    prev[i] = make_float2(o.z, o.w);
            }
        });
    if (lane_id() == 0) {
        if (count.of[0]) atomicAdd(P.pushed, (unsigned long long)count.of[0]);
        if (count.of[1]) atomicAdd(W.counts, (unsigned long long)count.of[1]);
        if (count.of[2]) atomicAdd(W.counts + 1, (unsigned long long)count.of[2]);
    }
}

// (pos and W.prev are different arrays; prev[i] is read and written by the lane that owns particle i alone)
__global__ __launch_bounds__(kStreamBlock) void k_movers_sweep(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                               uint64_t n, MoverPassArgs P, MoverSweepArgs W)
{
    mover_sweep_body<false>(pos, radius, n, P, W);
}

__global__ __launch_bounds__(kStreamBlock) void k_movers_sweep_surface(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                                       uint64_t n, MoverPassArgs P, MoverSweepArgs W)
{
    mover_sweep_body<true>(pos, radius, n, P, W);
}

// launch_movers_build in the swept form: B.old and W.carry (B.k rows each) are written too, and the masks list every
// mover where its motion reaches
gpe_status launch_movers_sweep_build(gpe_ctx *c, const MoverBuildArgs &B, const MoverSweepArgs &W)
{
    if (B.k == 0) return GPE_OK;
    if (!B.old || !W.carry) return fail(c, GPE_ERR_STATE, "launch_movers_sweep_build: no old capsules or no carry records");
    hipLaunchKernelGGL(k_movers_sweep_build, dim3(B.k), dim3(kMoverBuildBlock), 0, c->stream, B, W);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

// One swept pass over pos[0, n) in place, W.prev[0, n) read (and written where a surface acted).  The tables as
// launch_movers_pass takes them, built by launch_movers_sweep_build; *W.counts += the swept, W.counts[1] += the stopped
gpe_status launch_movers_sweep(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const MoverPassArgs &P,
                               const MoverSweepArgs &W)
{
    if (n == 0 || P.k == 0) return GPE_OK;
    if (!W.prev || !W.counts || !W.carry || !P.old)
        return fail(c, GPE_ERR_STATE, "launch_movers_sweep: no prev, counters, carry records or old capsules");
    if (P.surf)
        hipLaunchKernelGGL(k_movers_sweep_surface, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P, W);
    else
        hipLaunchKernelGGL(k_movers_sweep, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P, W);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
