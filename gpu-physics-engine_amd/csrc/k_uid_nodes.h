// k_uid_nodes.h -- the node phase of the step sets that name their particles by uid (gfx950, wave64): the one kernel
// behind "bonds/node", "bends/node" and "areas/node" (k_bonds.hip, k_bends.hip, k_areas.hip).
//
// A relaxation's first phase leaves one correction per constraint (or per member) and a state byte that says whether
// the constraint acted; this phase gives every particle the sum of its shares.  One lane per node v (a distinct uid the
// set names; uid_nodes.h builds the nodes and the rows, UidNodeTable holds them).  The lane reads node_slot[v] (4 B; an
// absent uid ends there), row_start[v], row_start[v + 1], then asks the set's shares for every incidence of its row, in
// row order -- ascending constraint index -- whether it acts and what (sx, sy) it adds.  A node with an acting
// incidence reads pos (8 B) and radius (4 B) of its particle and writes pos (8 B) once; nothing else is written.  One
// lane walks a node's whole row (at most the set's degree cap).  Two nodes never share a particle (the uids of the map
// are distinct), so no position has two writers.  No LDS, no float atomics.
//
// Shares: the set's pass arguments, passed by value as its own phase takes them (one struct per set, filled once per
// pass), with what this phase reads of every set --
//     const uint32_t *node_slot, *row_start;  uint32_t m, n;  float world_w, world_h;
// -- and the two things only the set knows:
//     __device__ uint32_t incidences() const;                         // the entries of its incidence list
//     template <class Add> __device__ void share(uint32_t e, Add add) const;   // e < incidences()
// share checks every index it takes from incidence e against the count of its array before it indexes anything, and
// calls add(sx, sy) once when the incidence acts, not at all when it does not.  (A call-back, not a flag and two
// outputs: inlined, the sum stays inside the set's own branch, which is the code the three kernels had one by one.)
#pragma once

#include "gpe_internal.h"
#include "k_bond.h"

namespace gpe {

template <class Shares>
__global__ __launch_bounds__(kStreamBlock) void k_uid_nodes(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                            Shares P)
{
#pragma clang fp contract(off)
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < P.m; v += stride) {
        const uint32_t slot = P.node_slot[v];
        if (slot >= P.n) continue;
        const uint32_t lo = P.row_start[v], hi = P.row_start[v + 1];
        float accx = 0.0f, accy = 0.0f;
        bool any = false;
        for (uint32_t e = lo; e < hi && e < P.incidences(); ++e) {
            P.share(e, [&](float sx, float sy) {
                accx = accx + sx;
                accy = accy + sy;
                any = true;
            });
        }
        if (!any) continue;
        const float2 p = pos[slot];
        float2 o;
        bond_move(p.x, p.y, radius[slot], accx, accy, P.world_w, P.world_h, &o.x, &o.y);
        pos[slot] = o;
    }
}

template <class Shares>
gpe_status launch_uid_nodes(gpe_ctx *c, const char *scope, float2 *pos, const float *radius, const Shares &P)
{
    Scope s(c, scope);
    hipLaunchKernelGGL(k_uid_nodes<Shares>, dim3(stream_grid(P.m)), dim3(kStreamBlock), 0, c->stream, pos, radius, P);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
