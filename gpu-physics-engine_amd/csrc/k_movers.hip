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
#include "k_capsule_pass.h"
#include "k_mover_build.h"
#include "k_stream_pairs.h"

namespace gpe {

// One workgroup per mover.  Lane 0 advances the state, writes the state and the posed capsule back and shares the pose
// through LDS (mover_build_advance); the workgroup then strides over the cells of the capsule's inflated bounding
// rectangle (mover_build_list).
__global__ __launch_bounds__(kMoverBuildBlock) void k_movers_build(MoverBuildArgs B)
{
    __shared__ float s_cap[4];
    const uint32_t j = blockIdx.x;                              // < B.k: the launch has B.k workgroups
    const MoverDef m = B.def[j];
    if (threadIdx.x == 0) {
        float cap[4];
        (void)mover_build_advance(B, m, j, B.old != nullptr, cap, cap);
        s_cap[0] = cap[0]; s_cap[1] = cap[1]; s_cap[2] = cap[2]; s_cap[3] = cap[3];
    }
    __syncthreads();
    const float cap[4] = {s_cap[0], s_cap[1], s_cap[2], s_cap[3]};
    uint32_t x0, y0, x1, y1;
    bool everywhere;
    if (!mover_cell_rect(B.g, cap, m.radius, B.rb, &x0, &y0, &x1, &y1, &everywhere)) return;   // (workgroup-uniform)
    mover_build_list(B, j, x0, y0, x1, y1, everywhere,
                     [&](uint32_t cx, uint32_t cy) { return mover_listed(B.g, cap, m.radius, B.rb, cx, cy); });
}

// the pair loop over capsule_resolve (k_capsule_pass.h): the masks of a cell, a wall that moved from P.old[j] to rec
template <bool SURF>
__device__ __forceinline__ void movers_pass_body(float2 *__restrict__ pos, const float *__restrict__ radius, uint64_t n,
                                                 const MoverPassArgs &P)
{
    const PairCounts<1> moved = stream_pairs<1, false>(
        pos, nullptr, n,
        [&](uint64_t i, float px, float py, float, float, float4 &o) -> bool {
            return capsule_resolve<SURF>(P, MaskCellLookup{P.masks, P.summary, P.words},
                                         [&](uint32_t j, const float4 &s, float u, float *wx, float *wy) {
                                             const float4 b = P.old[j];
                                             const float before[4] = {b.x, b.y, b.z, b.w}, after[4] = {s.x, s.y, s.z, s.w};
                                             surface_wall_move(before, after, u, wx, wy);
                                         },
                                         radius, i, px, py, o.x, o.y);
        },
        [&](uint64_t i, bool, const float4 &o, float, float, float, float) { pos[i] = make_float2(o.x, o.y); });
    if (lane_id() == 0 && moved.of[0]) atomicAdd(P.pushed, (unsigned long long)moved.of[0]);
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
