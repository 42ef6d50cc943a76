// k_bends.hip -- the bend constraints' pass (gfx950, wave64): `iterations` relaxations of the set, two launches each
// (k_bend.h says what a bend's corrections are; bend_graph.h builds the tables on the host).
//
// One relaxation must not read a position it has written itself (Jacobi), so it is two streaming kernels on the
// context's in-order stream, as in k_bonds.hip:
//   - k_bends_bend, one lane per bend j.  Reads the 32-byte record as two 16-byte words (node a, hinge b, node c, rc /
//     rs, stiffness, padding), node_slot of its three nodes (3 x 4 B), the three positions (3 x 8 B) and state[j] (1 B).
//     Writes corr[j] = (da.x, da.y, dc.x, dc.y) as one 16-byte store when the bend acts and state[j] (1 B) when it
//     changes: 0 acted, 2 inert in this relaxation.  The bend's own lane is the only writer of both.
//   - k_bends_node, one lane per node v (a distinct uid the bends name).  Reads node_slot[v] (4 B; an absent uid ends
//     there), row_start[v], row_start[v + 1], then per incidence, in ascending bend index, inc (4 B: bend << 2 | role),
//     state (1 B) and for an acting bend corr (16 B).  a adds da, c adds dc, the hinge -(da + dc), formed there.  A
//     node with an acting bend reads pos (8 B) and radius (4 B) of its particle and writes pos (8 B) once; nothing else
//     is written.  One lane walks a node's whole row (at most GPE_BEND_MAX_DEGREE).
// corr cannot carry the "no correction" mark itself (every binary32 pattern is a possible product, and a correction of
// zero still counts: its particle is clamped), so the mark is the state byte.  Two nodes never share a particle (the
// uids of the map are distinct), so no position has two writers.
// No LDS, no float atomics.  Slots are checked against n before they index anything.
#include "gpe_internal.h"
#include "bend_graph.h"
#include "k_bend.h"

namespace gpe {

static_assert(sizeof(BendRecord) == 2 * sizeof(uint4), "the device reads a BendRecord as two 16-byte words");

struct BendPassArgs {
    const uint4 *rec = nullptr;                  // 2 per bend
    const uint32_t *node_slot = nullptr, *row_start = nullptr, *inc = nullptr;
    float4 *corr = nullptr;
    uint8_t *state = nullptr;
    uint32_t k = 0, m = 0, n = 0;
    float world_w = 0.f, world_h = 0.f;
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

__global__ __launch_bounds__(kStreamBlock) void k_bends_node(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                             BendPassArgs P)
{
#pragma clang fp contract(off)
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < P.m; v += stride) {
        const uint32_t slot = P.node_slot[v];
        if (slot >= P.n) continue;
        const uint32_t lo = P.row_start[v], hi = P.row_start[v + 1];
        float accx = 0.0f, accy = 0.0f;
        bool any = false;
        for (uint32_t e = lo; e < hi; ++e) {
            const uint32_t w = P.inc[e];
            const uint32_t j = w >> 2, role = w & 3u;
            if (j >= P.k || P.state[j] != kBendActs) continue;
            const float4 c = P.corr[j];
            const float sx = role == kBendRoleA ? c.x : role == kBendRoleC ? c.z : bend_hinge_share(c.x, c.z);
            const float sy = role == kBendRoleA ? c.y : role == kBendRoleC ? c.w : bend_hinge_share(c.y, c.w);
            accx = accx + sx;
            accy = accy + sy;
            any = true;
        }
        if (!any) continue;
        const float2 p = pos[slot];
        float2 o;
        bond_move(p.x, p.y, radius[slot], accx, accy, P.world_w, P.world_h, &o.x, &o.y);
        pos[slot] = o;
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
    P.node_slot = B.node_slot; P.row_start = B.row_start; P.inc = B.inc;
    P.corr = B.corr; P.state = B.state;
    P.k = k; P.m = m; P.n = (uint32_t)n;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    for (uint32_t it = 0; it < iterations; ++it) {
        {
            Scope s(c, "bends/bend");
            hipLaunchKernelGGL(k_bends_bend, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, pos, P);
            GPE_HIP(c, hipGetLastError());
        }
        {
            Scope s(c, "bends/node");
            hipLaunchKernelGGL(k_bends_node, dim3(stream_grid(m)), dim3(kStreamBlock), 0, c->stream, pos, radius, P);
            GPE_HIP(c, hipGetLastError());
        }
    }
    return GPE_OK;
}

}  // namespace gpe
