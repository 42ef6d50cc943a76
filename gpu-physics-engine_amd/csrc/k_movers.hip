// k_movers.hip -- the moving colliders on the device: k_movers_build advances every mover by one step, poses its
// capsule and lists it in the lookup grid; k_movers_pass pushes every particle out of the posed mover it penetrates
// deepest, then K12's clamp (k_mover.h and k_collider.h say what "advance", "listed", "deepest" and "pushed" mean).
// Nothing here asks the host: gpe_movers.hip enqueues a memset of the grid, the build and the pass, every step.
//
// The grid is a bit mask per cell, not CSR lists: at most 1024 movers are at most 16 64-bit words per cell of a grid
// of at most 128 x 128 cells.  A mask needs no count / scan / fill, has no capacity to run over, and an integer atomicOr
// is order-free.  One summary word per cell names the mask words that are not zero: the common lane, whose cell has no
// mover near, reads those 4 bytes and retires -- no radius load, no store.
//
// With surfaces (k_surface.h) the build also writes the capsule the OLD state poses (B.old, null otherwise), and the
// pass has a sibling, k_movers_pass_surface: the same lookup and winner; under a hit it also loads the winner's surface
// row, its old capsule and prev[i], and stores prev[i] beside pos[i].
#include "gpe_internal.h"
#include "k_mover.h"
#include "k_surface.h"

namespace gpe {

constexpr int kMoverBuildBlock = 256;

// One workgroup per mover.  Lane 0 advances the state, writes the state and the posed capsule back and shares the pose
// through LDS; the workgroup then strides over the cells of the capsule's inflated bounding rectangle.
__global__ __launch_bounds__(kMoverBuildBlock) void k_movers_build(MoverBuildArgs B)
{
    __shared__ float s_cap[4];
    const uint32_t j = blockIdx.x;                              // < B.k: the launch has B.k workgroups
    const MoverDef m = B.def[j];
    if (threadIdx.x == 0) {
        float *pose = B.pose + 6ull * j;
        float q0 = pose[4], q1 = pose[5];
        float cap[4];
        if (B.old) {                                            // the capsule before the advance: a function of the state alone
            mover_pose(m, q0, q1, cap);
            B.old[j] = make_float4(cap[0], cap[1], cap[2], cap[3]);
        }
        mover_advance(m, B.dt, &q0, &q1);
        mover_pose(m, q0, q1, cap);
        pose[0] = cap[0]; pose[1] = cap[1]; pose[2] = cap[2]; pose[3] = cap[3];
        pose[4] = q0; pose[5] = q1;
        B.rec[2 * j] = make_float4(cap[0], cap[1], cap[2], cap[3]);
        s_cap[0] = cap[0]; s_cap[1] = cap[1]; s_cap[2] = cap[2]; s_cap[3] = cap[3];
    }
    __syncthreads();
    const float cap[4] = {s_cap[0], s_cap[1], s_cap[2], s_cap[3]};
    uint32_t x0, y0, x1, y1;
    bool everywhere;
    if (!mover_cell_rect(B.g, cap, m.radius, B.rb, &x0, &y0, &x1, &y1, &everywhere)) return;   // (workgroup-uniform)
    const uint32_t w = x1 - x0 + 1, total = w * (y1 - y0 + 1);  // <= 128 * 128
    const uint32_t word = j >> 6;
    const unsigned long long bit = 1ull << (j & 63u);
    uint32_t count = 0;                                         // wave-uniform
    for (uint32_t t0 = 0; t0 < total; t0 += kMoverBuildBlock) {
        const uint32_t t = t0 + threadIdx.x;
        bool hit = false;
        if (t < total) {
            const uint32_t cx = x0 + t % w, cy = y0 + t / w;    // cx <= x1 < gx, cy <= y1 < gy
            hit = everywhere || mover_listed(B.g, cap, m.radius, B.rb, cx, cy);
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

__device__ __forceinline__ void mover_try(const MoverPassArgs &P, uint32_t j, float px, float py, float r,
                                          unsigned long long &best)
{
    const float4 s = P.rec[2 * j];
    const float R = P.rec[2 * j + 1].x;
    ColliderTouch t;
    if (!collider_touch(px, py, r, s.x, s.y, s.z, s.w, R, &t)) return;
    const unsigned long long key = collider_key(t.depth, j);
    best = key > best ? key : best;
}

// particle i at (px, py).  true: it moved, (ox, oy) is its new position.  (collider_resolve of k_colliders.hip with
// the masks in the place of the lists: the same touch, key, normal and clamp).  SURF: the winner's surface is applied
// against the wall's displacement at the contact, and prev[i] written here, unless the row is PLAIN or p - prev is not
// finite
template <bool SURF>
__device__ __forceinline__ bool mover_resolve(const MoverPassArgs &P, const float *__restrict__ radius, uint64_t i,
                                              float px, float py, float &ox, float &oy)
{
#pragma clang fp contract(off)
    uint32_t cell = 0, summary = 0;
    const bool in_grid = collider_cell_of(P.view, px, py, &cell);
    if (in_grid) {
        summary = P.summary[cell];
        if (summary == 0) return false;
    }
    const float r = radius[i];
    unsigned long long best = 0;
    // no cell (outside the grid, NaN) or a radius the masks were not built for: every mover.  Exactness never rests on
    // the grid
    if (!in_grid || !(fabsf(r) <= P.view.rb)) {
        for (uint32_t j = 0; j < P.k; ++j) mover_try(P, j, px, py, r, best);
    } else {
        const unsigned long long *mask = P.masks + (uint64_t)cell * P.words;
        while (summary) {                                       // ascending words, ascending bits: ascending movers
            const uint32_t w = (uint32_t)__builtin_ctz(summary);   // < P.words: the build sets no other bit
            summary &= summary - 1;
            unsigned long long bits = mask[w];
            while (bits) {
                const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                bits &= bits - 1;
                mover_try(P, w * 64u + b, px, py, r, best);     // < P.k: the build sets bits of movers only
            }
        }
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
                const float4 b = P.old[j];
                const float before[4] = {b.x, b.y, b.z, b.w}, after[4] = {s.x, s.y, s.z, s.w};
                float wx, wy;
                surface_wall_move(before, after, t.u, &wx, &wy);
                float o[4];
                surface_apply(px, py, pv.x, pv.y, r, nx, ny, t.depth, wx, wy, row.x, row.y, P.world_w, P.world_h, o);
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
    ox = clamp_f(qx, r, P.world_w - r);
    oy = clamp_f(qy, r, P.world_h - r);
    return true;
}

// The shape of k_colliders_pass: two particles per lane, pos read 16 B per lane, the odd tail, the wave-voted counter.
template <bool SURF>
__device__ __forceinline__ void movers_pass_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                 const MoverPassArgs &P)
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
        const bool m0 = mover_resolve<SURF>(P, radius, 2 * i, c.x, c.y, o0.x, o0.y);
        const bool m1 = mover_resolve<SURF>(P, radius, 2 * i + 1, c.z, c.w, o1.x, o1.y);
        if (m0) pos[2 * i] = o0;
        if (m1) pos[2 * i + 1] = o1;
        moved += (uint32_t)__popcll(ballot64(m0)) + (uint32_t)__popcll(ballot64(m1));
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        float2 o;
        if (mover_resolve<SURF>(P, radius, i, c.x, c.y, o.x, o.y)) {
            pos[i] = o;
            moved += 1;
        }
    }
    if (lane_id() == 0 && moved) atomicAdd(P.pushed, (unsigned long long)moved);
}

__global__ __launch_bounds__(kStreamBlock) void k_movers_pass(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                              uint64_t n, MoverPassArgs P)
{
    movers_pass_body<false>(pos, radius, n, P);
}

// (pos and P.prev are different arrays; P.prev[i] is read and written by the lane that owns particle i alone)
__global__ __launch_bounds__(kStreamBlock) void k_movers_pass_surface(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                                      uint64_t n, MoverPassArgs P)
{
    movers_pass_body<true>(pos, radius, n, P);
}

// Advances the B.k movers by B.dt and lists them: B.def 3 float4, B.pose 6 floats and B.rec 2 float4 per mover; B.masks
// gx * gy * words words and B.summary gx * gy words, both zero when the kernel starts; *B.listed += the bits set.  B.old
// (may be null): one float4 per mover, the capsule before the advance
gpe_status launch_movers_build(gpe_ctx *c, const MoverBuildArgs &B)
{
    if (B.k == 0) return GPE_OK;
    hipLaunchKernelGGL(k_movers_build, dim3(B.k), dim3(kMoverBuildBlock), 0, c->stream, B);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

// One pass over pos[0, n) in place against the posed movers P.rec, found through P.masks / P.summary.  *P.pushed += the
// particles moved.  P.surf != nullptr: the surface form, P.k rows of P.surf and of P.old, P.prev[0, n) read and written
// under a hit
gpe_status launch_movers_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const MoverPassArgs &P)
{
    if (n == 0 || P.k == 0) return GPE_OK;
    if (P.surf) {
        if (!P.old || !P.prev) return fail(c, GPE_ERR_STATE, "launch_movers_pass: surfaces without the old capsules or prev");
        hipLaunchKernelGGL(k_movers_pass_surface, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P);
    } else {
        hipLaunchKernelGGL(k_movers_pass, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, radius, n, P);
    }
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
