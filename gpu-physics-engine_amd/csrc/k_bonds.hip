// k_bonds.hip -- the distance bonds' pass (gfx950, wave64): `iterations` relaxations of the set, two launches each
// (k_bond.h says what a bond's correction is; bond_graph.h builds the tables on the host).
//
// One relaxation must not read a position it has written itself (Jacobi), so it is two streaming kernels on the
// context's in-order stream:
//   - k_bonds_bond, one lane per bond j.  Reads state[j] (1 B; a broken bond ends there), the 16-byte record (node a,
//     node b or anchor index, rest, w), node_slot of its two nodes (2 x 4 B), the two positions (2 x 8 B; an anchor:
//     one position and 8 B of anchors), max_length[j] (4 B) only when the set holds a breakable bond.  Writes corr[j]
//     (8 B) when the bond acts and state[j] (1 B) when it changes: 0 acted, 1 broken, 2 inert in this relaxation.  The
//     bond's own lane is the only writer of both.  A break adds 1 to the integer counter (atomicAdd: order-free).
//   - the node phase, one lane per node v (a distinct uid the bonds name): k_uid_nodes.h's kernel, which asks
//     BondPassArgs::share.  Per incidence, in ascending bond index, that reads inc (4 B: bond << 1 | side), state (1 B)
//     and for an acting bond corr (8 B): side a adds the correction, side b its negation.  One lane walks a node's
//     whole row (at most GPE_BOND_MAX_DEGREE).
// corr cannot carry the "no correction" mark itself: every binary32 pattern is a possible product, and a correction of
// zero still counts (its particle is clamped), so the mark is the state byte.
// Bonded particles are neighbours in space and the arrays are kept in Morton order: the gathers of a wave mostly hit
// lines it has fetched already.  No LDS, no float atomics.  Slots are checked against n, indices against the count of
// their array, before they index anything.
//
// Under the coloured solver (gpe_set_bond_solver; bond_colours.h colours the set on the host) a relaxation is a sweep of
// the colours in order, every bond judged from the positions as they are and moving its two ends itself: no corr, no
// node phase.  No two bonds of one colour share a node, so within a colour no position has two writers, and the bits
// are those of a sequential sweep in (colour, index) order whatever the launch.  Two launch forms, one bond_in_place:
//   - k_bonds_colour, one launch per colour and relaxation on the in-order stream, one lane per entry of
//     order[colour_start[c] .. colour_start[c + 1]).  Reads order (4 B), state (1 B), the record (16 B), two node_slot,
//     two positions and two radii (an anchor: one of each and 8 B of anchors), max_length only when a bond can break;
//     writes one or two positions, and state when it changes.  No LDS.
//   - k_bonds_coloured, one launch of one 1024-lane workgroup for a set of at most kBondLdsNodesMax nodes (a rope, one
//     soft body: launches would cost more than the work).  Stages position and radius of the set's m nodes in LDS
//     (12 B a node, static, for kBondLdsNodesMax nodes: 12 KiB), runs all iterations * colours sweeps there with the bonds of a
//     colour strided over the lanes and a barrier between colours, writes the present nodes back once.  An absent
//     node's staged position is NaN: bond_correction calls its bonds inert, which is what an absent uid means.
#include "gpe_internal.h"
#include "bond_graph.h"
#include "k_bond.h"
#include "k_uid_nodes.h"

namespace gpe {

static_assert(sizeof(BondRecord) == sizeof(uint4), "the device reads a BondRecord as one 16-byte word");

struct BondPassArgs {
    const uint4 *rec = nullptr;
    const float *max_length = nullptr;           // NULL: no bond can break
    const float2 *anchors = nullptr;
    const uint32_t *node_slot = nullptr, *row_start = nullptr, *inc = nullptr;
    float2 *corr = nullptr;
    uint8_t *state = nullptr;
    unsigned long long *broken = nullptr;
    uint32_t k = 0, m = 0, n = 0, n_anchors = 0;
    float world_w = 0.f, world_h = 0.f;
    // the node phase's shares (k_uid_nodes.h): a pair has two incidences, an anchor one
    __device__ __forceinline__ uint32_t incidences() const { return 2u * k - n_anchors; }
    template <class Add>
    __device__ __forceinline__ void share(uint32_t e, Add add) const
    {
        const uint32_t w = inc[e];
        const uint32_t j = w >> 1;
        if (j >= k || state[j] != kBondActs) return;
        const float2 c = corr[j];
        add((w & 1u) ? -c.x : c.x, (w & 1u) ? -c.y : c.y);
    }
};

__global__ __launch_bounds__(kStreamBlock) void k_bonds_bond(const float2 *__restrict__ pos, BondPassArgs P)
{
#pragma clang fp contract(off)
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < P.k; j += stride) {
        const uint32_t was = P.state[j];
        if (was == kBondBroken) continue;
        const uint4 r = P.rec[j];
        const bool anchor = (r.y & kBondAnchorBit) != 0;
        const uint32_t sa = P.node_slot[r.x];
        const uint32_t sb = anchor ? 0u : P.node_slot[r.y];            // (an absent uid: 0xffffffff >= n)
        const uint32_t ia = r.y & ~kBondAnchorBit;
        uint32_t now = kBondInert;
        if (sa < P.n && sb < P.n && (!anchor || ia < P.n_anchors)) {
            const float2 a = pos[sa];
            const float2 b = anchor ? P.anchors[ia] : pos[sb];
            const float max_length = P.max_length ? P.max_length[j] : 0.0f;   // (a uniform pointer test)
            float cx = 0.f, cy = 0.f;
            now = bond_correction(a.x, a.y, b.x, b.y, __uint_as_float(r.z), __uint_as_float(r.w), max_length, &cx, &cy);
            if (now == kBondActs) P.corr[j] = make_float2(cx, cy);
            if (now == kBondBroken) atomicAdd(P.broken, 1ull);
        }
        if (now != was) P.state[j] = (uint8_t)now;
    }
}

// One bond of a coloured sweep, in place.  Nodes: where the particles of the set's nodes are read and written --
//   at(node) -> a handle; present(handle); get(handle) -> float2; rad(handle) -> float; put(handle, float2).
// Every index is checked against the count of its array before it indexes anything.
template <class Nodes>
__device__ __forceinline__ void bond_in_place(const BondPassArgs &P, uint32_t j, Nodes &N)
{
#pragma clang fp contract(off)
    if (j >= P.k) return;
    const uint32_t was = P.state[j];
    if (was == kBondBroken) return;
    const uint4 r = P.rec[j];
    const bool anchor = (r.y & kBondAnchorBit) != 0;
    const uint32_t ia = r.y & ~kBondAnchorBit;
    uint32_t now = kBondInert;
    if (r.x < P.m && (anchor ? ia < P.n_anchors : r.y < P.m)) {
        const uint32_t ha = N.at(r.x);
        const uint32_t hb = anchor ? ha : N.at(r.y);
        if (N.present(ha) && N.present(hb)) {
            const float2 a = N.get(ha);
            const float2 b = anchor ? P.anchors[ia] : N.get(hb);
            const float max_length = P.max_length ? P.max_length[j] : 0.0f;   // (a uniform pointer test)
            float cx = 0.f, cy = 0.f;
            now = bond_correction(a.x, a.y, b.x, b.y, __uint_as_float(r.z), __uint_as_float(r.w), max_length, &cx, &cy);
            if (now == kBondActs) {
                float2 o;
                bond_move(a.x, a.y, N.rad(ha), cx, cy, P.world_w, P.world_h, &o.x, &o.y);
                N.put(ha, o);
                if (!anchor) {
                    bond_move(b.x, b.y, N.rad(hb), -cx, -cy, P.world_w, P.world_h, &o.x, &o.y);
                    N.put(hb, o);
                }
            }
            if (now == kBondBroken) atomicAdd(P.broken, 1ull);
        }
    }
    if (now != was) P.state[j] = (uint8_t)now;
}

struct BondNodesGlobal {                         // the particles where they are stored: a handle is a storage slot
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

// the bonds order[lo .. hi) -- one colour -- over the particles in place.  lo <= hi <= k
__global__ __launch_bounds__(kStreamBlock) void k_bonds_colour(float2 *pos, const float *__restrict__ radius,
                                                               BondPassArgs P, const uint32_t *__restrict__ order,
                                                               uint32_t lo, uint32_t hi)
{
    BondNodesGlobal N{pos, radius, P.node_slot, P.n};
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t e = lo + blockIdx.x * blockDim.x + threadIdx.x; e < hi && e < P.k; e += stride)
        bond_in_place(P, order[e], N);
}

constexpr int kBondLdsBlock = 1024;

struct BondNodesLds {                            // the particles staged by node index: a handle is a node, < m <= the cap
    float2 *lpos;
    float *lrad;
    __device__ __forceinline__ uint32_t at(uint32_t node) const { return node; }
    __device__ __forceinline__ bool present(uint32_t) const { return true; }     // (an absent node's position is NaN)
    __device__ __forceinline__ float2 get(uint32_t h) const { return lpos[h]; }
    __device__ __forceinline__ float rad(uint32_t h) const { return lrad[h]; }
    __device__ __forceinline__ void put(uint32_t h, float2 v) const { lpos[h] = v; }
};

// a whole pass of a set of P.m <= kBondLdsNodesCap nodes: one workgroup.  colour_start: colours + 1 words, ascending,
// the last one <= k
__global__ __launch_bounds__(kBondLdsBlock) void k_bonds_coloured(float2 *pos, const float *__restrict__ radius,
                                                                  BondPassArgs P, const uint32_t *__restrict__ order,
                                                                  const uint32_t *__restrict__ colour_start,
                                                                  uint32_t colours, uint32_t iterations)
{
    __shared__ float2 lpos[kBondLdsNodesCap];
    __shared__ float lrad[kBondLdsNodesCap];
    if (P.m > kBondLdsNodesCap) return;          // (uniform; the host never launches it so)
    for (uint32_t v = threadIdx.x; v < P.m; v += kBondLdsBlock) {
        const uint32_t slot = P.node_slot[v];
        const bool present = slot < P.n;
        lpos[v] = present ? pos[slot] : make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
        lrad[v] = present ? radius[slot] : 0.0f;
    }
    __syncthreads();
    BondNodesLds N{lpos, lrad};
    for (uint32_t it = 0; it < iterations; ++it) {
        for (uint32_t c = 0; c < colours; ++c) {
            const uint32_t lo = colour_start[c], hi = colour_start[c + 1];
            // (at the shipped limit of 1024 nodes a colour holds at most 1024 bonds: one trip; a timing build takes more)
            for (uint32_t e = lo + threadIdx.x; e < hi && e < P.k; e += kBondLdsBlock) bond_in_place(P, order[e], N);
            __syncthreads();                     // (lo, hi, colours, iterations are uniform: every lane arrives)
        }
    }
    for (uint32_t v = threadIdx.x; v < P.m; v += kBondLdsBlock) {
        const uint32_t slot = P.node_slot[v];
        if (slot < P.n) pos[slot] = lpos[v];     // (a node no bond moved gets its own bits back)
    }
}

static BondPassArgs bond_pass_args(const gpe_ctx *c, uint64_t n, const BondState &B, uint32_t k, uint32_t m)
{
    BondPassArgs P;
    P.rec = B.rec; P.max_length = B.max_length; P.anchors = B.anchors;
    P.node_slot = B.nt.node_slot; P.row_start = B.nt.row_start; P.inc = B.inc;
    P.corr = B.corr; P.state = B.state; P.broken = B.broken;
    P.k = k; P.m = m; P.n = (uint32_t)n; P.n_anchors = B.n_anchors;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    return P;
}

// B's tables as gpe_set_bonds uploaded them for k bonds and m nodes (every node index < m, every anchor index <
// B.n_anchors, every inc entry >> 1 < k), node_slot resolved for the particles as they are.
gpe_status launch_bonds_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BondState &B, uint32_t k,
                             uint32_t m, uint32_t iterations)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bonds");
    const BondPassArgs P = bond_pass_args(c, n, B, k, m);
    for (uint32_t it = 0; it < iterations; ++it) {
        {
            Scope s(c, "bonds/bond");
            hipLaunchKernelGGL(k_bonds_bond, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, pos, P);
            GPE_HIP(c, hipGetLastError());
        }
        GPE_TRY(launch_uid_nodes(c, "bonds/node", pos, radius, P));
    }
    return GPE_OK;
}

// ... and B.order (k entries, each < k), B.colour_start on the device and B.colour_begin on the host (B.colours + 1
// words, ascending from 0 to k) as the coloured solver built them
gpe_status launch_bonds_coloured(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BondState &B, uint32_t k,
                                 uint32_t m, uint32_t iterations, uint32_t *form)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bonds");
    if (!B.order || !B.colour_start || B.colour_begin.size() != (size_t)B.colours + 1 || B.colour_begin.back() != k)
        return fail(c, GPE_ERR_STATE, "the coloured bonds' pass: no colour tables for this set");
    const BondPassArgs P = bond_pass_args(c, n, B, k, m);
    if (m <= kBondLdsNodesMax) {
        Scope s(c, "bonds/coloured");
        hipLaunchKernelGGL(k_bonds_coloured, dim3(1), dim3(kBondLdsBlock), 0, c->stream, pos, radius, P, B.order,
                           B.colour_start, B.colours, iterations);
        GPE_HIP(c, hipGetLastError());
        *form = 2;
        return GPE_OK;
    }
    for (uint32_t it = 0; it < iterations; ++it) {
        for (uint32_t col = 0; col < B.colours; ++col) {
            const uint32_t lo = B.colour_begin[col], hi = B.colour_begin[col + 1];
            Scope s(c, "bonds/colour");
            hipLaunchKernelGGL(k_bonds_colour, dim3(stream_grid(hi - lo)), dim3(kStreamBlock), 0, c->stream, pos, radius,
                               P, B.order, lo, hi);
            GPE_HIP(c, hipGetLastError());
        }
    }
    *form = 1;
    return GPE_OK;
}

}  // namespace gpe
