// k_colliders.hip -- the static colliders' pass: every particle against the capsules of its lookup cell, pushed out of
// the one it penetrates deepest, then K12's clamp (k_collider.h says what "deepest" and "pushed" mean).
//
// A streaming pass: two particles per lane, so pos is read 16 B per lane as k_verlet reads it.  The common lane finds
// an empty list: it has read its pos and two words of cell_start per particle and is done -- no radius load, no store.
// radius is loaded only under a non-empty list, pos stored only for a particle that moved.  The colliders are 32-byte
// records (ax, ay, bx, by | R, padding): 4096 of them are 128 KB and stay in an XCD's L2; cell_start is read at the
// particles' own locality (they are kept in Morton order).
//
// The surface form (k_colliders_pass_surface, launched only while the set holds surfaces: k_surface.h) is the same
// lookup and the same winner; under a hit it also loads the winner's surface row (one float4: 4096 rows are 64 KB) and
// prev[i], and stores prev[i] beside pos[i].  The common lane costs what it costs in the plain form.
#include "gpe_internal.h"
#include "k_collider.h"
#include "k_surface.h"

namespace gpe {

struct ColliderPassArgs {
    const uint32_t *cell_start = nullptr;        // view.gx * view.gy + 1
    const uint32_t *items = nullptr;
    const float4 *rec = nullptr;                 // 2 per collider: (ax, ay, bx, by), (R, 0, 0, 0)
    uint32_t k = 0;
    ColliderGridView view;
    float world_w = 0.f, world_h = 0.f;
    unsigned long long *pushed = nullptr;
    const float4 *surf = nullptr;                // the surface form: one row per collider (e, mu, flags, reserved) ...
    float2 *prev = nullptr;                      // ... and the previous positions it rewrites under a hit
};

__device__ __forceinline__ void collider_try(const ColliderPassArgs &P, uint32_t j, float px, float py, float r,
                                             unsigned long long &best)
{
    const float4 s = P.rec[2 * j];
    const float R = P.rec[2 * j + 1].x;
    ColliderTouch t;
    if (!collider_touch(px, py, r, s.x, s.y, s.z, s.w, R, &t)) return;
    const unsigned long long key = collider_key(t.depth, j);
    best = key > best ? key : best;
}

// particle i at (px, py).  true: it moved, (ox, oy) is its new position.  SURF: the winner's surface is applied, and
// prev[i] written here, unless the row is PLAIN or p - prev is not finite
template <bool SURF>
__device__ __forceinline__ bool collider_resolve(const ColliderPassArgs &P, const float *__restrict__ radius, uint64_t i,
                                                 float px, float py, float &ox, float &oy)
{
#pragma clang fp contract(off)
    uint32_t cell = 0, lo = 0, hi = 0;
    const bool in_grid = collider_cell_of(P.view, px, py, &cell);
    if (in_grid) {
        lo = P.cell_start[cell];
        hi = P.cell_start[cell + 1];
        if (lo == hi) return false;
    }
    const float r = radius[i];
    unsigned long long best = 0;
    // no cell (outside the grid, NaN) or a radius the lists were not built for: every collider.  Exactness never rests
    // on the grid
    if (!in_grid || !(fabsf(r) <= P.view.rb)) {
        for (uint32_t j = 0; j < P.k; ++j) collider_try(P, j, px, py, r, best);
    } else {
        for (uint32_t e = lo; e < hi; ++e) collider_try(P, P.items[e], px, py, r, best);
    }
    if (best == 0) return false;
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
    const float4 s = P.rec[2 * j];
    ColliderTouch t;
    (void)collider_touch(px, py, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &t);   // the winner again: the same bits
    float nx, ny;
    collider_normal(t, &nx, &ny);
    if constexpr (SURF) {
        const float4 row = P.surf[j];
        if (!(__float_as_uint(row.z) & kSurfacePlain)) {
            const float2 pv = P.prev[i];
            if (surface_velocity_finite(px, py, pv.x, pv.y)) {
                float o[4];
                surface_apply(px, py, pv.x, pv.y, r, nx, ny, t.depth, 0.0f, 0.0f, row.x, row.y, P.world_w, P.world_h, o);
                ox = o[0];
                oy = o[1];
                P.prev[i] = make_float2(o[2], o[3]);
                return true;
            }
        }
    }
    const float mx = nx * t.depth;
    const float my = ny * t.depth;
    const float qx = px + mx;
    const float qy = py + my;
    ox = clamp_f(qx, r, P.world_w - r);                        // particle_integration.wgsl:70-71, as verlet_one
    oy = clamp_f(qy, r, P.world_h - r);
    return true;
}

template <bool SURF>
__device__ __forceinline__ void colliders_pass_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                    const ColliderPassArgs &P)
{
    const uint64_t pairs = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float4 *pos4 = reinterpret_cast<const float4 *>(pos);
    // particles this wave moved: wave-uniform among the lanes still in the loop.  Lane 0 holds the wave's lowest
    // index, leaves the loop last and so has seen every vote
    uint32_t moved = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const float4 c = pos4[i];
        float2 o0, o1;
        const bool m0 = collider_resolve<SURF>(P, radius, 2 * i, c.x, c.y, o0.x, o0.y);
        const bool m1 = collider_resolve<SURF>(P, radius, 2 * i + 1, c.z, c.w, o1.x, o1.y);
        if (m0) pos[2 * i] = o0;
        if (m1) pos[2 * i + 1] = o1;
        moved += (uint32_t)__popcll(ballot64(m0)) + (uint32_t)__popcll(ballot64(m1));
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        float2 o;
        if (collider_resolve<SURF>(P, radius, i, c.x, c.y, o.x, o.y)) {
            pos[i] = o;
            moved += 1;
        }
    }
    if (lane_id() == 0 && moved) atomicAdd(P.pushed, (unsigned long long)moved);
}

__global__ __launch_bounds__(kStreamBlock) void k_colliders_pass(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                                 uint64_t n, ColliderPassArgs P)
{
    colliders_pass_body<false>(pos, radius, n, P);
}

// (pos and P.prev are different arrays; P.prev[i] is read and written by the lane that owns particle i alone)
__global__ __launch_bounds__(kStreamBlock) void k_colliders_pass_surface(float2 *__restrict__ pos,
                                                                         const float *__restrict__ radius, uint64_t n,
                                                                         ColliderPassArgs P)
{
    colliders_pass_body<true>(pos, radius, n, P);
}

// One pass over pos[0, n) in place.  cell_start / items / rec: device memory of view.gx * view.gy + 1 words, the
// entries cell_start's last word counts (each < k) and 2 k records.  *pushed += the particles moved.  surf != nullptr:
// the surface form, k rows of surf and prev[0, n) read and written under a hit
gpe_status launch_colliders_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const uint32_t *cell_start,
                                 const uint32_t *items, const float4 *rec, uint32_t k, const ColliderGridView &view,
                                 unsigned long long *pushed, const float4 *surf, float2 *prev)
{
    if (n == 0 || k == 0) return GPE_OK;
    ColliderPassArgs P;
    P.cell_start = cell_start; P.items = items; P.rec = rec; P.k = k;
    P.view = view;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    P.pushed = pushed;
    if (surf) {
        if (!prev) return fail(c, GPE_ERR_STATE, "launch_colliders_pass: surfaces without prev");
        P.surf = surf; P.prev = prev;
        hipLaunchKernelGGL(k_colliders_pass_surface, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P);
    } else {
        hipLaunchKernelGGL(k_colliders_pass, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P);
    }
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
