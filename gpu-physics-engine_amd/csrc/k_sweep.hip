// k_sweep.hip -- the swept form of the static colliders' pass (gpe_set_collider_sweep; k_sweep.h says what a contact
// on a path is, who wins and when a particle stops).  A translation unit of its own: k_colliders.hip's kernels are what
// a context without the sweep launches, untouched.
//
// The pair loop of k_stream_pairs.h with prev.  The common lane has read its 32 B and, per row of the lookup box of its
// path, two words of cell_start; it finds them empty and is done -- no radius load, no store.  radius, the records, the
// surface row and the root arithmetic come only under a non-empty list.  Three integer counters, one atomic each per wave.
#include "gpe_internal.h"
#include "k_capsule_pass.h"
#include "k_stream_pairs.h"

namespace gpe {

struct SweepPassArgs {
    const uint32_t *cell_start = nullptr;        // view.gx * view.gy + 1
    const uint32_t *items = nullptr;
    const float4 *rec = nullptr;                 // 2 per collider: (ax, ay, bx, by), (R, 0, 0, 0)
    uint32_t k = 0;
    ColliderGridView view;
    float world_w = 0.f, world_h = 0.f;
    unsigned long long *pushed = nullptr;        // the colliders' own counter
    unsigned long long *counts = nullptr;        // two words: swept, stopped
    const float4 *surf = nullptr;                // the surface form: one row per collider (e, mu, flags, reserved)
};

// the candidates of one path: the lists of the cells of its lookup box, or every collider
struct SweepCands {
    uint32_t cx0, cx1, cy0, cy1;
    bool all;
};

// false: the path lies in the grid and every list of its box is empty (two words of cell_start per row say).  A box
// whose lists hold more entries than there are colliders is no shortcut: every collider is walked, the winner the same
__device__ __forceinline__ bool sweep_cands(const SweepPassArgs &P, float x0x, float x0y, float x1x, float x1y, SweepCands &C)
{
    C.cx0 = C.cx1 = C.cy0 = C.cy1 = 0;
    C.all = !sweep_box(P.view, x0x, x0y, x1x, x1y, &C.cx0, &C.cx1, &C.cy0, &C.cy1);
    if (C.all) return true;
    uint32_t total = 0;
    for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy) {                     // (cy1 < gy, cx1 < gx: both reads lie in the table)
        const uint32_t row = cy * P.view.gx;
        total += P.cell_start[row + C.cx1 + 1] - P.cell_start[row + C.cx0];
    }
    if (total == 0) return false;
    if (total > P.k) C.all = true;
    return true;
}

template <class F>
__device__ __forceinline__ void sweep_each(const SweepPassArgs &P, const SweepCands &C, F f)
{
    csr_each(P.items, P.k, C.all, C.cy0, C.cy1, [&](uint32_t cy, uint32_t &lo, uint32_t &hi) {
        const uint32_t row = cy * P.view.gx;
        hi = P.cell_start[row + C.cx1 + 1];
        lo = P.cell_start[row + C.cx0];
    }, f);
}

// the plain rule on p (capsule_resolve's, by its definition in k_collider.h / k_surface.h) for a particle the sweep does
// not take: its cell as sweep_box names it, prev already in hand, the surface's new prev returned through o
template <bool SURF>
__device__ __forceinline__ uint32_t sweep_plain(const SweepPassArgs &P, const float *__restrict__ radius, uint64_t i, float px,
                                                float py, float qx, float qy, float4 &o)
{
#pragma clang fp contract(off)
    SweepCands C;
    if (!sweep_cands(P, px, py, px, py, C)) return 0;
    const float r = radius[i];
    if (!(fabsf(r) <= P.view.rb)) C.all = true;
    unsigned long long best = 0;
    sweep_each(P, C, [&](uint32_t j) { capsule_try(P.rec, j, px, py, r, best); });
    if (best == 0) return 0;
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
    const float4 s = P.rec[2 * j];
    ColliderTouch t;
    float reach;
    (void)sweep_measure(px, py, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &t, &reach);   // the winner again: the same bits
    float nx, ny;
    collider_normal(t, &nx, &ny);
    if constexpr (SURF) {
        const float4 row = P.surf[j];
        if (!(__float_as_uint(row.z) & kSurfacePlain) && surface_velocity_finite(px, py, qx, qy)) {
            float out[4];
            surface_apply(px, py, qx, qy, r, nx, ny, t.depth, 0.0f, 0.0f, row.x, row.y, P.world_w, P.world_h, out);
            o = make_float4(out[0], out[1], out[2], out[3]);
            return kSweepMoved;
        }
    }
    const float mx = nx * t.depth;
    const float my = ny * t.depth;
    const float x = px + mx;
    const float y = py + my;
    o = make_float4(clamp_f(x, r, P.world_w - r), clamp_f(y, r, P.world_h - r), qx, qy);
    return kSweepMoved;
}

// the swept rule's policy (k_capsule_pass.h): the lists of a path's box, every collider judged where it stands
template <bool SURF>
struct ColliderSweepPolicy {
    const SweepPassArgs &P;
    using Cands = SweepCands;

    __device__ __forceinline__ bool cands(float x0x, float x0y, float x1x, float x1y, Cands &C) const
    {
        return sweep_cands(P, x0x, x0y, x1x, x1y, C);
    }

    template <class F>
    __device__ __forceinline__ void each(const Cands &C, F f) const
    {
        sweep_each(P, C, f);
    }

    // sweep_contact takes the start of the path, then its end
    __device__ __forceinline__ bool judge(uint32_t j, float fromx, float fromy, float tox, float toy, float r,
                                          SweepContact *c) const
    {
        const float4 s = P.rec[2 * j];
        return sweep_contact(fromx, fromy, tox, toy, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, c);
    }

    __device__ __forceinline__ void respond(uint32_t who, const SweepContact &win, float px, float py, float qx, float qy,
                                            float r, float *res) const
    {
        res[0] = 0.0f; res[1] = 0.0f; res[2] = qx; res[3] = qy;
        bool pushed = true;
        if constexpr (SURF) {
            const float4 row = P.surf[who];
            if (!(__float_as_uint(row.z) & kSurfacePlain)) {
                surface_apply(px, py, qx, qy, r, win.nx, win.ny, win.depth, 0.0f, 0.0f, row.x, row.y, P.world_w, P.world_h, res);
                pushed = false;
            }
        }
        if (pushed) sweep_push(px, py, r, win, P.world_w, P.world_h, &res[0], &res[1]);
    }
};

// the pair loop of k_stream_pairs.h over swept_resolve, the plain rule for a particle the sweep does not take.  The
// store writes pos[i] of every particle that moved, and prev[i] where a surface changed its bits
template <bool SURF>
__device__ __forceinline__ void sweep_pass_body(float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                const float *__restrict__ radius, uint64_t n, const SweepPassArgs &P)
{
    const ColliderSweepPolicy<SURF> S{P};
    const PairCounts<3> count = stream_pairs<3, true>(
        pos, prev, n,
        [&](uint64_t i, float px, float py, float qx, float qy, float4 &o) -> uint32_t {
            if (sweep_plain_particle(px, py, qx, qy)) return sweep_plain<SURF>(P, radius, i, px, py, qx, qy, o);
            return swept_resolve<SURF>(S, radius, i, px, py, qx, qy, o);
        },
        [&](uint64_t i, uint32_t, const float4 &o, float, float, float qx, float qy) {
            pos[i] = make_float2(o.x, o.y);
            if constexpr (SURF) {
                if (__float_as_uint(o.z) != __float_as_uint(qx) || __float_as_uint(o.w) != __float_as_uint(qy))
                    prev[i] = make_float2(o.z, o.w);
            }
        });
    if (lane_id() == 0) {
        if (count.of[0]) atomicAdd(P.pushed, (unsigned long long)count.of[0]);
        if (count.of[1]) atomicAdd(P.counts, (unsigned long long)count.of[1]);
        if (count.of[2]) atomicAdd(P.counts + 1, (unsigned long long)count.of[2]);
    }
}

// (pos and prev are different arrays; prev[i] is read and written by the lane that owns particle i alone)
__global__ __launch_bounds__(kStreamBlock) void k_colliders_sweep(float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                                  const float *__restrict__ radius, uint64_t n, SweepPassArgs P)
{
    sweep_pass_body<false>(pos, prev, radius, n, P);
}

__global__ __launch_bounds__(kStreamBlock) void k_colliders_sweep_surface(float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                                          const float *__restrict__ radius, uint64_t n,
                                                                          SweepPassArgs P)
{
    sweep_pass_body<true>(pos, prev, radius, n, P);
}

// One swept pass over pos[0, n) in place, prev[0, n) read (and written under a hit of the surface form).  The tables
// as launch_colliders_pass takes them; counts: two words, *counts += the swept, counts[1] += the stopped particles
gpe_status launch_colliders_sweep(gpe_ctx *c, float2 *pos, float2 *prev, const float *radius, uint64_t n,
                                  const uint32_t *cell_start, const uint32_t *items, const float4 *rec, uint32_t k,
                                  const ColliderGridView &view, unsigned long long *pushed, unsigned long long *counts,
                                  const float4 *surf)
{
    if (n == 0 || k == 0) return GPE_OK;
    if (!prev || !counts) return fail(c, GPE_ERR_STATE, "launch_colliders_sweep: no prev or no counters");
    SweepPassArgs P;
    P.cell_start = cell_start; P.items = items; P.rec = rec; P.k = k;
    P.view = view;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    P.pushed = pushed; P.counts = counts;
    P.surf = surf;
    if (surf)
        hipLaunchKernelGGL(k_colliders_sweep_surface, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, prev, radius, n, P);
    else
        hipLaunchKernelGGL(k_colliders_sweep, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, prev, radius, n, P);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
