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

// B's tables as gpe_set_bonds uploaded them for k bonds and m nodes (every node index < m, every anchor index <
// B.n_anchors, every inc entry >> 1 < k), node_slot resolved for the particles as they are.
gpe_status launch_bonds_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BondState &B, uint32_t k,
                             uint32_t m, uint32_t iterations)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bonds");
    BondPassArgs P;
    P.rec = B.rec; P.max_length = B.max_length; P.anchors = B.anchors;
    P.node_slot = B.nt.node_slot; P.row_start = B.nt.row_start; P.inc = B.inc;
    P.corr = B.corr; P.state = B.state; P.broken = B.broken;
    P.k = k; P.m = m; P.n = (uint32_t)n; P.n_anchors = B.n_anchors;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
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

}  // namespace gpe
