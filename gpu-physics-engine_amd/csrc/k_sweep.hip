// k_sweep.hip -- the swept form of the static colliders' pass (gpe_set_collider_sweep; k_sweep.h says what a contact
// on a path is, who wins and when a particle stops).  A translation unit of its own: k_colliders.hip's kernels are what
// a context without the sweep launches, untouched.
//
// A streaming pass shaped like k_colliders.hip's: two particles per lane, pos and prev each read 16 B per lane.  The
// common lane has read its 32 B and, per row of the lookup box of its path, two words of cell_start (the lists of the
// cells of one row lie behind each other in items[]); it finds them empty and is done -- no radius load, no store.
// radius, the records, the surface row and the root arithmetic come only under a non-empty list.  pos is stored only
// for a particle that moved, prev only where a surface acted.  Three integer counters, one atomic each per wave.
#include "gpe_internal.h"
#include "k_sweep.h"

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

constexpr uint32_t kSweepMoved = 1u, kSweepSwept = 2u, kSweepStopped = 4u;

// the candidates of one path: the lists of the cells of its lookup box, or every collider
struct SweepCands {
    uint32_t cx0, cx1, cy0, cy1;
    bool all;
};

// false: the path lies in the grid and every list of its box is empty.  The lists of the cells of one row lie behind
// each other in items[]: two words of cell_start per row say where.  A box whose lists together hold more entries than
// there are colliders is no shortcut: every collider is walked instead (either way the winner is the same)
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
    if (C.all) {
        for (uint32_t j = 0; j < P.k; ++j) f(j);
    } else {
        for (uint32_t cy = C.cy0; cy <= C.cy1; ++cy) {
            const uint32_t row = cy * P.view.gx;
            const uint32_t hi = P.cell_start[row + C.cx1 + 1];
            for (uint32_t e = P.cell_start[row + C.cx0]; e < hi; ++e) f(P.items[e]);
        }
    }
}

// the plain rule on p (k_colliders.hip's collider_resolve, by its definition in k_collider.h / k_surface.h)
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
    sweep_each(P, C, [&](uint32_t j) {
        const float4 s = P.rec[2 * j];
        ColliderTouch t;
        if (!collider_touch(px, py, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &t)) return;
        const unsigned long long key = collider_key(t.depth, j);
        best = key > best ? key : best;
    });
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

// particle i at p with the previous position q.  -> kSweep* flags; moved: o = (pos', prev')
template <bool SURF>
__device__ __forceinline__ uint32_t sweep_resolve(const SweepPassArgs &P, const float *__restrict__ radius, uint64_t i, float px,
                                                  float py, float qx, float qy, float4 &o)
{
#pragma clang fp contract(off)
    if (sweep_plain_particle(px, py, qx, qy)) return sweep_plain<SURF>(P, radius, i, px, py, qx, qy, o);
    SweepCands C;
    if (!sweep_cands(P, qx, qy, px, py, C)) return 0;
    const float r = radius[i];
    // a radius the lists were not built for: every collider.  Exactness never rests on the grid
    const bool wide = !(fabsf(r) <= P.view.rb);
    if (wide) C.all = true;
    SweepContact win;
    uint32_t who = 0;
    bool have = false;
    sweep_each(P, C, [&](uint32_t j) {
        const float4 s = P.rec[2 * j];
        SweepContact c;
        if (!sweep_contact(qx, qy, px, py, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &c)) return;
        if (!have || sweep_better(c, j, win, who)) {
            win = c;
            who = j;
            have = true;
        }
    });
    if (!have) return 0;
    uint32_t flags = kSweepMoved | ((win.t > 0.0f && win.t < 1.0f) ? kSweepSwept : 0u);
    float res[4] = {0.0f, 0.0f, qx, qy};
    bool pushed = true;
    if constexpr (SURF) {
        const float4 row = P.surf[who];
        if (!(__float_as_uint(row.z) & kSurfacePlain)) {
            surface_apply(px, py, qx, qy, r, win.nx, win.ny, win.depth, 0.0f, 0.0f, row.x, row.y, P.world_w, P.world_h, res);
            pushed = false;
        }
    }
    if (pushed) sweep_push(px, py, r, win, P.world_w, P.world_h, &res[0], &res[1]);
    // verify once: prev -> q against every collider, the winner included
    SweepCands V;
    bool over = false;
    if (sweep_cands(P, qx, qy, res[0], res[1], V) || wide) {
        if (wide) V.all = true;
        sweep_each(P, V, [&](uint32_t j) {
            const float4 s = P.rec[2 * j];
            SweepContact c;
            if (sweep_contact(qx, qy, res[0], res[1], r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &c) && sweep_over_slop(c))
                over = true;
        });
    }
    if (over) {
        float sx, sy;
        sweep_stop(r, win, P.world_w, P.world_h, &sx, &sy);
        o = make_float4(sx, sy, qx, qy);
        return flags | kSweepStopped;
    }
    o = make_float4(res[0], res[1], res[2], res[3]);
    return flags;
}

template <bool SURF>
__device__ __forceinline__ void sweep_pass_body(float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                const float *__restrict__ radius, uint64_t n, const SweepPassArgs &P)
{
    const uint64_t pairs = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float4 *pos4 = reinterpret_cast<const float4 *>(pos);
    const float4 *prev4 = reinterpret_cast<const float4 *>(prev);
    // wave-uniform among the lanes still in the loop; lane 0 holds the wave's lowest index, leaves the loop last and so
    // has seen every vote (as in k_colliders.hip)
    uint32_t moved = 0, swept = 0, stopped = 0;
    auto vote = [&](uint32_t f) {
        moved += (uint32_t)__popcll(ballot64(f & kSweepMoved));
        swept += (uint32_t)__popcll(ballot64(f & kSweepSwept));
        stopped += (uint32_t)__popcll(ballot64(f & kSweepStopped));
    };
    auto store = [&](uint64_t i, uint32_t f, const float4 &o, float qx, float qy) {
        if (!(f & kSweepMoved)) return;
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
        const uint32_t f0 = sweep_resolve<SURF>(P, radius, 2 * i, c.x, c.y, q.x, q.y, o0);
        const uint32_t f1 = sweep_resolve<SURF>(P, radius, 2 * i + 1, c.z, c.w, q.z, q.w, o1);
        store(2 * i, f0, o0, q.x, q.y);
        store(2 * i + 1, f1, o1, q.z, q.w);
        vote(f0);
        vote(f1);
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        const float2 q = prev[i];
        float4 o;
        const uint32_t f = sweep_resolve<SURF>(P, radius, i, c.x, c.y, q.x, q.y, o);
        store(i, f, o, q.x, q.y);
        moved += (f & kSweepMoved) ? 1u : 0u;
        swept += (f & kSweepSwept) ? 1u : 0u;
        stopped += (f & kSweepStopped) ? 1u : 0u;
    }
    if (lane_id() == 0) {
        if (moved) atomicAdd(P.pushed, (unsigned long long)moved);
        if (swept) atomicAdd(P.counts, (unsigned long long)swept);
        if (stopped) atomicAdd(P.counts + 1, (unsigned long long)stopped);
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
