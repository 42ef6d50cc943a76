// k_mover_sweep.hip -- the swept form of the movers' build and pass (gpe_set_mover_sweep; k_mover_sweep.h says what a
// mover carries a point by, what a contact on the relative path is, who wins and when a particle stops).  A translation
// unit of its own: k_movers.hip's kernels are what a context without the mode launches, untouched.
//
// k_movers_sweep_build is k_movers_build with three additions: it always writes the capsule before the advance, it
// writes one carry record per mover, and it lists the mover in every cell its MOTION reaches (the parallelogram of a
// LINEAR mover, the disc of a ROTATE one) instead of the cells of the new pose alone.
//
// The pass is shaped like k_colliders_sweep: two particles per lane, pos and prev each read 16 B per lane.  The common
// lane has read its 32 B and the summary words of the cells of its path's lookup box (one word for a particle that stays
// in its cell), finds them zero and is done -- no radius load, no store.  Under a summary bit the mask words of the box
// are ORed, one word at a time (no array, no scratch): ascending bits are ascending movers, each judged once.  pos is
// stored only for a particle that moved, prev only where a surface changed it.  Three integer counters, one atomic each
// per wave.
#include "gpe_internal.h"
#include "k_mover_sweep.h"

namespace gpe {

constexpr int kMoverSweepBuildBlock = 256;

__global__ __launch_bounds__(kMoverSweepBuildBlock) void k_movers_sweep_build(MoverBuildArgs B, MoverSweepArgs W)
{
    __shared__ float s_cap[8];
    const uint32_t j = blockIdx.x;                              // < B.k: the launch has B.k workgroups
    const MoverDef m = B.def[j];
    const float arm = m.pad0;                                   // mover_arm(m), at set time
    if (threadIdx.x == 0) {
        float *pose = B.pose + 6ull * j;
        const float p0 = pose[4], p1 = pose[5];
        float q0 = p0, q1 = p1;
        float c0[4], c1[4];
        mover_pose(m, q0, q1, c0);
        B.old[j] = make_float4(c0[0], c0[1], c0[2], c0[3]);
        mover_advance(m, B.dt, &q0, &q1);
        mover_pose(m, q0, q1, c1);
        pose[0] = c1[0]; pose[1] = c1[1]; pose[2] = c1[2]; pose[3] = c1[3];
        pose[4] = q0; pose[5] = q1;
        B.rec[2 * j] = make_float4(c1[0], c1[1], c1[2], c1[3]);
        MoverCarry k;
        mover_carry_of(m, B.dt, p0, p1, q0, q1, c0, c1, arm, &k);
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
    const uint32_t w = x1 - x0 + 1, total = w * (y1 - y0 + 1);  // <= 128 * 128
    const uint32_t word = j >> 6;
    const unsigned long long bit = 1ull << (j & 63u);
    uint32_t count = 0;                                         // wave-uniform
    for (uint32_t t0 = 0; t0 < total; t0 += kMoverSweepBuildBlock) {
        const uint32_t t = t0 + threadIdx.x;
        bool hit = false;
        if (t < total) {
            const uint32_t cx = x0 + t % w, cy = y0 + t / w;    // cx <= x1 < gx, cy <= y1 < gy
            hit = everywhere || mover_sweep_listed(B.g, m, arm, c0, c1, B.rb, cx, cy);
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

constexpr uint32_t kMoverSweepMoved = 1u, kMoverSweepSwept = 2u, kMoverSweepStopped = 4u;

// the candidates of one path: the masks of the cells of its lookup box, or every mover
struct MoverSweepCands {
    uint32_t cx0, cx1, cy0, cy1;
    uint32_t summary;            // the OR of the box's summary words
    bool all;
};

// false: the path lies in the grid and no cell of its box lists a mover
__device__ __forceinline__ bool mover_sweep_cands(const MoverPassArgs &P, float x0x, float x0y, float x1x, float x1y,
                                                  MoverSweepCands &C)
{
    C.cx0 = C.cx1 = C.cy0 = C.cy1 = 0;
    C.summary = 0;
    C.all = !sweep_box(P.view, x0x, x0y, x1x, x1y, &C.cx0, &C.cx1, &C.cy0, &C.cy1);
    if (C.all) return true;
    uint32_t s = 0;
    for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy)                       // (cy1 < gy, cx1 < gx: every read lies in the table)
        for (uint32_t cx = C.cx0; cx <= C.cx1; ++cx) s |= P.summary[cy * P.view.gx + cx];
    C.summary = s;
    return s != 0;
}

template <class F>
__device__ __forceinline__ void mover_sweep_each(const MoverPassArgs &P, const MoverSweepCands &C, F f)
{
    if (C.all) {
        for (uint32_t j = 0; j < P.k; ++j) f(j);
        return;
    }
    uint32_t summary = C.summary;
    while (summary) {                                                  // ascending words, ascending bits: ascending movers
        const uint32_t w = (uint32_t)__builtin_ctz(summary);           // < P.words: the build sets no other bit
        summary &= summary - 1;
        unsigned long long bits = 0;
        for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy)
            for (uint32_t cx = C.cx0; cx <= C.cx1; ++cx) bits |= P.masks[(uint64_t)(cy * P.view.gx + cx) * P.words + w];
        while (bits) {
            const uint32_t b = (uint32_t)__builtin_ctzll(bits);
            bits &= bits - 1;
            f(w * 64u + b);                                            // < P.k: the build sets bits of movers only
        }
    }
}

__device__ __forceinline__ bool mover_sweep_try(const MoverPassArgs &P, const MoverSweepArgs &W, uint32_t j, float px,
                                                float py, float qx, float qy, float r, SweepContact *c)
{
    const float4 s = P.rec[2 * j];
    const float cap[4] = {s.x, s.y, s.z, s.w};
    const MoverCarry k = W.carry[j];
    return mover_sweep_judge(k, cap, P.rec[2 * j + 1].x, px, py, qx, qy, r, c);
}

// particle i at p with the previous position q.  -> kMoverSweep* flags; moved: o = (pos', prev')
template <bool SURF>
__device__ __forceinline__ uint32_t mover_sweep_resolve(const MoverPassArgs &P, const MoverSweepArgs &W,
                                                        const float *__restrict__ radius, uint64_t i, float px, float py,
                                                        float qx, float qy, float4 &o)
{
#pragma clang fp contract(off)
    MoverSweepCands C;
    if (!mover_sweep_cands(P, qx, qy, px, py, C)) return 0;
    const float r = radius[i];
    // a radius the masks were not built for: every mover.  Exactness never rests on the grid
    const bool wide = !(fabsf(r) <= P.view.rb);
    if (wide) C.all = true;
    SweepContact win;
    uint32_t who = 0;
    bool have = false;
    mover_sweep_each(P, C, [&](uint32_t j) {
        SweepContact c;
        if (!mover_sweep_try(P, W, j, px, py, qx, qy, r, &c)) return;
        if (!have || sweep_better(c, j, win, who)) {
            win = c;
            who = j;
            have = true;
        }
    });
    if (!have) return 0;
    const uint32_t flags = kMoverSweepMoved | ((win.t > 0.0f && win.t < 1.0f) ? kMoverSweepSwept : 0u);
    float res[4];
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
    // verify once: every mover on its own relative path to q, the winner included
    MoverSweepCands V;
    bool over = false;
    if (mover_sweep_cands(P, qx, qy, res[0], res[1], V) || wide) {
        if (wide) V.all = true;
        mover_sweep_each(P, V, [&](uint32_t j) {
            SweepContact c;
            if (mover_sweep_try(P, W, j, res[0], res[1], qx, qy, r, &c) && sweep_over_slop(c)) over = true;
        });
    }
    if (over) {
        float sx, sy;
        sweep_stop(r, win, P.world_w, P.world_h, &sx, &sy);
        o = make_float4(sx, sy, qx, qy);
        return flags | kMoverSweepStopped;
    }
    o = make_float4(res[0], res[1], res[2], res[3]);
    return flags;
}

template <bool SURF>
__device__ __forceinline__ void mover_sweep_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                 const MoverPassArgs &P, const MoverSweepArgs &W)
{
    float2 *__restrict__ prev = W.prev;
    const uint64_t pairs = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float4 *pos4 = reinterpret_cast<const float4 *>(pos);
    const float4 *prev4 = reinterpret_cast<const float4 *>(prev);
    // wave-uniform among the lanes still in the loop; lane 0 holds the wave's lowest index, leaves the loop last and so
    // has seen every vote (as in k_movers.hip)
    uint32_t moved = 0, swept = 0, stopped = 0;
    auto vote = [&](uint32_t f) {
        moved += (uint32_t)__popcll(ballot64(f & kMoverSweepMoved));
        swept += (uint32_t)__popcll(ballot64(f & kMoverSweepSwept));
        stopped += (uint32_t)__popcll(ballot64(f & kMoverSweepStopped));
    };
    auto store = [&](uint64_t i, uint32_t f, const float4 &o, float px, float py, float qx, float qy) {
        if (!(f & kMoverSweepMoved)) return;
        if (__float_as_uint(o.x) != __float_as_uint(px) || __float_as_uint(o.y) != __float_as_uint(py))
            pos[i] = make_float2(o.x, o.y);
        if constexpr (SURF) {
            if (__float_as_uint(o.z) != __float_as_uint(qx) || __float_as_uint(o.w) != __float_as_uint(qy))
                prev[i] = make_float2(o.z, o.w);
        }
    };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const float4 c = pos4[i];
        const float4 q = prev4[i];
        float4 o0, o1;
        const uint32_t f0 = mover_sweep_resolve<SURF>(P, W, radius, 2 * i, c.x, c.y, q.x, q.y, o0);
        const uint32_t f1 = mover_sweep_resolve<SURF>(P, W, radius, 2 * i + 1, c.z, c.w, q.z, q.w, o1);
        store(2 * i, f0, o0, c.x, c.y, q.x, q.y);
        store(2 * i + 1, f1, o1, c.z, c.w, q.z, q.w);
        vote(f0);
        vote(f1);
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        const float2 q = prev[i];
        float4 o;
        const uint32_t f = mover_sweep_resolve<SURF>(P, W, radius, i, c.x, c.y, q.x, q.y, o);
        store(i, f, o, c.x, c.y, q.x, q.y);
        moved += (f & kMoverSweepMoved) ? 1u : 0u;
        swept += (f & kMoverSweepSwept) ? 1u : 0u;
        stopped += (f & kMoverSweepStopped) ? 1u : 0u;
    }
    if (lane_id() == 0) {
        if (moved) atomicAdd(P.pushed, (unsigned long long)moved);
        if (swept) atomicAdd(W.counts, (unsigned long long)swept);
        if (stopped) atomicAdd(W.counts + 1, (unsigned long long)stopped);
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
    hipLaunchKernelGGL(k_movers_sweep_build, dim3(B.k), dim3(kMoverSweepBuildBlock), 0, c->stream, B, W);
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
