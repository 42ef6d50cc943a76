// k_colliders.hip -- the static colliders' pass: every particle against the capsules of its lookup cell, pushed out of
// the one it penetrates deepest, then K12's clamp (k_collider.h says what "deepest" and "pushed" mean).
//
// A streaming pass over the pair loop of k_stream_pairs.h.  The common lane finds an empty list: it has read its pos
// and two words of cell_start per particle and is done -- no radius load, no store.
// radius is loaded only under a non-empty list, pos stored only for a particle that moved.  The colliders are 32-byte
// records (ax, ay, bx, by | R, padding): 4096 of them are 128 KB and stay in an XCD's L2; cell_start is read at the
// particles' own locality (they are kept in Morton order).
//
// The surface form (k_colliders_pass_surface, launched only while the set holds surfaces: k_surface.h) is the same
// lookup and the same winner; under a hit it also loads the winner's surface row (one float4: 4096 rows are 64 KB) and
// prev[i], and stores prev[i] beside pos[i].  The common lane costs what it costs in the plain form.
#include "gpe_internal.h"
#include "k_capsule_pass.h"
#include "k_stream_pairs.h"

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

// the pair loop (k_stream_pairs.h) over capsule_resolve (k_capsule_pass.h): the lists of a cell, a wall that stands
template <bool SURF>
__device__ __forceinline__ void colliders_pass_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                    const ColliderPassArgs &P)
{
    const PairCounts<1> moved = stream_pairs<1, false>(
        pos, nullptr, n,
        [&](uint64_t i, float px, float py, float, float, float4 &o) -> bool {
            return capsule_resolve<SURF>(P, CsrCellLookup{P.cell_start, P.items},
                                         [](uint32_t, const float4 &, float, float *wx, float *wy) { *wx = 0.0f; *wy = 0.0f; },
                                         radius, i, px, py, o.x, o.y);
        },
        [&](uint64_t i, bool, const float4 &o, float, float, float, float) {
            pos[i] = make_float2(o.x, o.y);
        });
    if (lane_id() == 0 && moved.of[0]) atomicAdd(P.pushed, (unsigned long long)moved.of[0]);
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
