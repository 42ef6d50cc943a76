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
//
// Under the coloured solver (gpe_set_bend_solver; bend_colours.h colours the set on the host) a relaxation is a sweep of
// the colours in order, every bend judged from the positions as they are and moving its three particles itself: no
// corr, no node phase.  No two bends of one colour share a node, so within a colour no position has two writers, and
// the bits are those of a sequential sweep in (colour, index) order whatever the launch.  Two launch forms, one
// bend_in_place:
//   - k_bends_colour, one launch per colour and relaxation on the in-order stream, one lane per entry of
//     order[colour_start[c] .. colour_start[c + 1]).  Reads order (4 B), state (1 B), the record (32 B), three
//     node_slot, three positions and three radii; writes three positions, and state when it changes.  No LDS.
//   - k_bends_coloured, one launch of one 1024-lane workgroup for a set of at most kBendLdsNodesMax nodes (a blade of
//     grass, a hinge, one fold: launches would cost more than the work).  Stages position and radius of the set's m
//     nodes in LDS (12 B a node, static, for kBendLdsNodesMax nodes: 12 KiB), runs all iterations * colours sweeps
//     there with the bends of a colour strided over the lanes and a barrier between colours, writes the present nodes
//     back once.
// Neither uses float atomics.
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

// One bend of a coloured sweep, in place.  Nodes: where the particles of the set's nodes are read and written --
//   at(node) -> a handle; present(handle); get(handle) -> float2; rad(handle) -> float; put(handle, float2).
// Every index is checked against the count of its array before it indexes anything.
template <class Nodes>
__device__ __forceinline__ void bend_in_place(const BendPassArgs &P, uint32_t j, Nodes &N)
{
#pragma clang fp contract(off)
    if (j >= P.k) return;
    const uint32_t was = P.state[j];
    const uint4 r0 = P.rec[2 * (size_t)j];                             // (a, b, c, rc)
    const uint4 r1 = P.rec[2 * (size_t)j + 1];                         // (rs, stiffness, 0, 0)
    uint32_t now = kBendInert;
    if (r0.x < P.m && r0.y < P.m && r0.z < P.m) {
        const uint32_t ha = N.at(r0.x);
        const uint32_t hb = N.at(r0.y);
        const uint32_t hc = N.at(r0.z);
        if (N.present(ha) && N.present(hb) && N.present(hc)) {
            const float2 a = N.get(ha);
            const float2 b = N.get(hb);
            const float2 c = N.get(hc);
            float dax = 0.f, day = 0.f, dcx = 0.f, dcy = 0.f;
            now = bend_correction(a.x, a.y, b.x, b.y, c.x, c.y, __uint_as_float(r0.w), __uint_as_float(r1.x),
                                  __uint_as_float(r1.y), &dax, &day, &dcx, &dcy);
            if (now == kBendActs) {
                float2 o;
                bond_move(a.x, a.y, N.rad(ha), dax, day, P.world_w, P.world_h, &o.x, &o.y);
                N.put(ha, o);
                bond_move(c.x, c.y, N.rad(hc), dcx, dcy, P.world_w, P.world_h, &o.x, &o.y);
                N.put(hc, o);
                bond_move(b.x, b.y, N.rad(hb), bend_hinge_share(dax, dcx), bend_hinge_share(day, dcy), P.world_w,
                          P.world_h, &o.x, &o.y);
                N.put(hb, o);
            }
        }
    }
    if (now != was) P.state[j] = (uint8_t)now;
}

struct BendNodesGlobal {                         // the particles where they are stored: a handle is a storage slot
    float2 *pos;
    const float *radius;
    const uint32_t *node_slot;
    uint32_t n;
    __device__ __forceinline__ uint32_t at(uint32_t node) const { return node_slot[node]; }   // (an absent uid: 0xffffffff >= n)
    __device__ __forceinline__ bool present(uint32_t h) const { return h < n; }
    __device__ __forceinline__ float2 get(uint32_t h) const { return pos[h]; }
    __device__ __forceinline__ float rad(uint32_t h) const { return radius[h]; }
    __device__ __forceinline__ void put(uint32_t h, float2 v) const { pos[h] = v; }
};

// the bends order[lo .. hi) -- one colour -- over the particles in place.  lo <= hi <= k
__global__ __launch_bounds__(kStreamBlock) void k_bends_colour(float2 *pos, const float *__restrict__ radius,
                                                               BendPassArgs P, const uint32_t *__restrict__ order,
                                                               uint32_t lo, uint32_t hi)
{
    BendNodesGlobal N{pos, radius, P.node_slot, P.n};
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t e = lo + blockIdx.x * blockDim.x + threadIdx.x; e < hi && e < P.k; e += stride)
        bend_in_place(P, order[e], N);
}

constexpr int kBendLdsBlock = 1024;

struct BendNodesLds {                            // the particles staged by node index: a handle is a node, < m <= the cap
    float2 *lpos;
    float *lrad;
    __device__ __forceinline__ uint32_t at(uint32_t node) const { return node; }
    __device__ __forceinline__ bool present(uint32_t) const { return true; }     // (an absent node's position is NaN)
    __device__ __forceinline__ float2 get(uint32_t h) const { return lpos[h]; }
    __device__ __forceinline__ float rad(uint32_t h) const { return lrad[h]; }
    __device__ __forceinline__ void put(uint32_t h, float2 v) const { lpos[h] = v; }
};

// a whole pass of a set of P.m <= kBendLdsNodesCap nodes: one workgroup.  colour_start: colours + 1 words, ascending,
// the last one <= k.  An absent node's staged position is NaN: bend_correction calls its bends inert, which is what an
// absent uid means
__global__ __launch_bounds__(kBendLdsBlock) void k_bends_coloured(float2 *pos, const float *__restrict__ radius,
                                                                  BendPassArgs P, const uint32_t *__restrict__ order,
                                                                  const uint32_t *__restrict__ colour_start,
                                                                  uint32_t colours, uint32_t iterations)
{
    __shared__ float2 lpos[kBendLdsNodesCap];
    __shared__ float lrad[kBendLdsNodesCap];
    if (P.m > kBendLdsNodesCap) return;          // (uniform; the host never launches it so)
    for (uint32_t v = threadIdx.x; v < P.m; v += kBendLdsBlock) {
        const uint32_t slot = P.node_slot[v];
        const bool present = slot < P.n;
        lpos[v] = present ? pos[slot] : make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
        lrad[v] = present ? radius[slot] : 0.0f;
    }
    __syncthreads();
    BendNodesLds N{lpos, lrad};
    for (uint32_t it = 0; it < iterations; ++it) {
        for (uint32_t c = 0; c < colours; ++c) {
            const uint32_t lo = colour_start[c], hi = colour_start[c + 1];
            // (at the shipped limit a colour holds at most a third as many bends as there are nodes: one trip)
            for (uint32_t e = lo + threadIdx.x; e < hi && e < P.k; e += kBendLdsBlock) bend_in_place(P, order[e], N);
            __syncthreads();                     // (lo, hi, colours, iterations are uniform: every lane arrives)
        }
    }
    for (uint32_t v = threadIdx.x; v < P.m; v += kBendLdsBlock) {
        const uint32_t slot = P.node_slot[v];
        if (slot < P.n) pos[slot] = lpos[v];     // (a node no bend moved gets its own bits back)
    }
}

static BendPassArgs bend_pass_args(const gpe_ctx *c, uint64_t n, const BendState &B, uint32_t k, uint32_t m)
{
    BendPassArgs P;
    P.rec = B.rec;
    P.node_slot = B.nt.node_slot; P.row_start = B.nt.row_start; P.inc = B.inc;
    P.corr = B.corr; P.state = B.state;
    P.k = k; P.m = m; P.n = (uint32_t)n;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    return P;
}

// B's tables as gpe_set_bends uploaded them for k bends and m nodes (every node index < m, every inc entry >> 2 < k),
// node_slot resolved for the particles as they are.
gpe_status launch_bends_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BendState &B, uint32_t k,
                             uint32_t m, uint32_t iterations)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bends");
    const BendPassArgs P = bend_pass_args(c, n, B, k, m);
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

// ... and B.order (k entries, each < k), B.colour_start on the device and B.colour_begin on the host (B.colours + 1
// words, ascending from 0 to k) as the coloured solver built them
gpe_status launch_bends_coloured(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BendState &B, uint32_t k,
                                 uint32_t m, uint32_t iterations, uint32_t *form)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bends");
    if (!B.order || !B.colour_start || B.colour_begin.size() != (size_t)B.colours + 1 || B.colour_begin.back() != k)
        return fail(c, GPE_ERR_STATE, "the coloured bends' pass: no colour tables for this set");
    const BendPassArgs P = bend_pass_args(c, n, B, k, m);
    if (m <= kBendLdsNodesMax) {
        Scope s(c, "bends/coloured");
        hipLaunchKernelGGL(k_bends_coloured, dim3(1), dim3(kBendLdsBlock), 0, c->stream, pos, radius, P, B.order,
                           B.colour_start, B.colours, iterations);
        GPE_HIP(c, hipGetLastError());
        *form = 2;
        return GPE_OK;
    }
    for (uint32_t it = 0; it < iterations; ++it) {
        for (uint32_t col = 0; col < B.colours; ++col) {
            const uint32_t lo = B.colour_begin[col], hi = B.colour_begin[col + 1];
            Scope s(c, "bends/colour");
            hipLaunchKernelGGL(k_bends_colour, dim3(stream_grid(hi - lo)), dim3(kStreamBlock), 0, c->stream, pos, radius,
                               P, B.order, lo, hi);
            GPE_HIP(c, hipGetLastError());
        }
    }
    *form = 1;
    return GPE_OK;
}

}  // namespace gpe
