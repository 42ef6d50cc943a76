// k_bends.hip -- the bend constraints' pass (gfx950, wave64): `iterations` relaxations of the set, two launches each
// (k_bend.h says what a bend's corrections are; bend_graph.h builds the tables on the host).
//
// One relaxation must not read a position it has written itself (Jacobi), so it is two streaming kernels on the
// context's in-order stream:
//   - k_bends_bend, one lane per bend j.  Reads the 32-byte record as two 16-byte words (node a, hinge b, node c, rc /
//     rs, stiffness, padding), node_slot of its three nodes (3 x 4 B), the three positions (3 x 8 B) and state[j] (1 B).
//     Writes corr[j] = (da.x, da.y, dc.x, dc.y) as one 16-byte store when the bend acts and state[j] (1 B) when it
//     changes: 0 acted, 2 inert in this relaxation.  The bend's own lane is the only writer of both.
//   - the node phase, one lane per node v (a distinct uid the bends name): k_uid_nodes.h's kernel, which asks
//     BendPassArgs::share.  Per incidence, in ascending bend index, that reads inc (4 B: bend << 2 | role), state (1 B)
//     and for an acting bend corr (16 B).  a adds da, c adds dc, the hinge -(da + dc), formed there.  One lane walks a
//     node's whole row (at most GPE_BEND_MAX_DEGREE).
// corr cannot carry the "no correction" mark itself (every binary32 pattern is a possible product, and a correction of
// zero still counts: its particle is clamped), so the mark is the state byte.
// No LDS, no float atomics.  Slots are checked against n, indices against the count of their array, before they index
// anything.
#include "gpe_internal.h"
#include "bend_graph.h"
#include "k_bend.h"
#include "k_uid_nodes.h"

namespace gpe {

static_assert(sizeof(BendRecord) == 2 * sizeof(uint4), "the device reads a BendRecord as two 16-byte words");

struct BendPassArgs {
    const uint4 *rec = nullptr;                  // 2 per bend
    const uint32_t *node_slot = nullptr, *row_start = nullptr, *inc = nullptr;
    float4 *corr = nullptr;
    uint8_t *state = nullptr;
    uint32_t k = 0, m = 0, n = 0;
    float world_w = 0.f, world_h = 0.f;
    // the node phase's shares (k_uid_nodes.h): every bend has three incidences
    __device__ __forceinline__ uint32_t incidences() const { return 3u * k; }
    template <class Add>
    __device__ __forceinline__ void share(uint32_t e, Add add) const
    {
        const uint32_t w = inc[e];
        const uint32_t j = w >> 2, role = w & 3u;
        if (j >= k || state[j] != kBendActs) return;
        const float4 c = corr[j];
        const float sx = role == kBendRoleA ? c.x : role == kBendRoleC ? c.z : bend_hinge_share(c.x, c.z);
        const float sy = role == kBendRoleA ? c.y : role == kBendRoleC ? c.w : bend_hinge_share(c.y, c.w);
        add(sx, sy);
    }
};

__global__ __launch_bounds__(kStreamBlock) void k_bends_bend(const float2 *__restrict__ pos, BendPassArgs P)
{
#pragma clang fp contract(off)
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < P.k; j += stride) {
        const uint32_t was = P.state[j];
        const uint4 r0 = P.rec[2 * (size_t)j];                         // (a, b, c, rc)
        const uint4 r1 = P.rec[2 * (size_t)j + 1];                     // (rs, stiffness, 0, 0)
        uint32_t now = kBendInert;
        if (r0.x < P.m && r0.y < P.m && r0.z < P.m) {
            const uint32_t sa = P.node_slot[r0.x];                     // (an absent uid: 0xffffffff >= n)
            const uint32_t sb = P.node_slot[r0.y];
            const uint32_t sc = P.node_slot[r0.z];
            if (sa < P.n && sb < P.n && sc < P.n) {
                const float2 a = pos[sa];
                const float2 b = pos[sb];
                const float2 c = pos[sc];
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
                now = bend_correction(a.x, a.y, b.x, b.y, c.x, c.y, __uint_as_float(r0.w), __uint_as_float(r1.x),
                                      __uint_as_float(r1.y), &d.x, &d.y, &d.z, &d.w);
                if (now == kBendActs) P.corr[j] = d;
            }
        }
        if (now != was) P.state[j] = (uint8_t)now;
    }
}

// B's tables as gpe_set_bends uploaded them for k bends and m nodes (every node index < m, every inc entry >> 2 < k),
// node_slot resolved for the particles as they are.
gpe_status launch_bends_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BendState &B, uint32_t k,
                             uint32_t m, uint32_t iterations)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bends");
    BendPassArgs P;
    P.rec = B.rec;
    P.node_slot = B.nt.node_slot; P.row_start = B.nt.row_start; P.inc = B.inc;
    P.corr = B.corr; P.state = B.state;
    P.k = k; P.m = m; P.n = (uint32_t)n;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    for (uint32_t it = 0; it < iterations; ++it) {
        {
            Scope s(c, "bends/bend");
            hipLaunchKernelGGL(k_bends_bend, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, pos, P);
            GPE_HIP(c, hipGetLastError());
        }
        GPE_TRY(launch_uid_nodes(c, "bends/node", pos, radius, P));
    }
    return GPE_OK;
}

}  // namespace gpe
