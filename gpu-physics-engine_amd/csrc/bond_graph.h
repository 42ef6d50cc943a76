// bond_graph.h -- the host side of a bond set: its validation and the graph the pass walks.  Plain C++, no HIP header:
// gpe_bonds.hip includes it, and so does the CPU test program (tests/cpp/bond_graph_tests.cpp).
//
// bond_graph_build turns k bonds into
//   - nodes: the distinct uids the bonds name, ascending (m <= 2 k).  An anchor's point is no node;
//   - per bond its two ends as node indices (an anchor: its index in `anchors`, with kBondAnchorBit);
//   - a CSR of incidences per node, in ascending bond index: entry = bond << 1 | side (0: the node is the bond's a,
//     1: its b).  A bond listed twice appears twice, in both rows.  The nodes and the rows are uid_nodes.h's.
// What the pass adds up per particle, and in which order, is therefore a function of the set alone.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gpe.h"
#include "uid_nodes.h"

namespace gpe {

constexpr uint32_t kBondAnchorBit = 0x80000000u;       // in BondRecord::b: the low bits index `anchors`
constexpr uint32_t kBondKnownFlags = GPE_BOND_ANCHOR | GPE_BOND_BROKEN;

struct BondRecord {              // 16 bytes: what the bond phase reads per bond
    uint32_t a, b;               // node indices; b of an anchor: kBondAnchorBit | index into anchors
    float rest, w;               // w: 0.5f * stiffness for a pair, stiffness for an anchor
};

struct BondGraph {
    std::vector<uint32_t> nodes;         // m: the endpoint uids, ascending, distinct
    std::vector<BondRecord> rec;         // k
    std::vector<float> max_length;       // k, or empty when no bond can break
    std::vector<float> anchors;          // 2 per anchor bond, in bond order
    std::vector<uint32_t> row_start;     // m + 1
    std::vector<uint32_t> inc;           // row_start[m] entries: bond << 1 | side
    std::vector<uint8_t> state;          // k: kBondBroken for a bond given with GPE_BOND_BROKEN, else 0
    uint32_t max_degree = 0;
    uint64_t broken = 0;                 // bonds that start broken
};

// NULL: the set is valid.  Otherwise what is wrong with it (the caller names the call in front).
inline const char *bond_set_problem(const gpe_bond *bonds, uint64_t k, uint32_t iterations)
{
    if (k > 0 && !bonds) return "NULL bonds";
    if (k > GPE_BONDS_MAX) return "k must be at most GPE_BONDS_MAX";
    if (iterations < 1 || iterations > GPE_BOND_ITER_MAX) return "iterations must be 1 .. GPE_BOND_ITER_MAX";
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_bond &q = bonds[j];
        if (!isfinite(q.rest_length) || !(q.rest_length >= 0.0f)) return "a rest_length is NaN, infinite or negative";
        if (!isfinite(q.max_length) || !(q.max_length >= 0.0f)) return "a max_length is NaN, infinite or negative";
        if (!(q.stiffness >= 0.0f && q.stiffness <= 1.0f)) return "a stiffness is NaN or outside [0, 1]";
        if (q.flags & ~kBondKnownFlags) return "unknown flag bits";
        if (q.uid_a == GPE_UID_ABSENT) return "uid_a is GPE_UID_ABSENT";
        if (q.uid_a == q.uid_b) return "a bond ties a particle to itself";
        if (q.flags & GPE_BOND_ANCHOR) {
            if (q.uid_b != GPE_UID_ABSENT) return "an anchor's uid_b must be GPE_UID_ABSENT";
            if (!isfinite(q.anchor_x) || !isfinite(q.anchor_y)) return "an anchor coordinate is not finite";
        } else if (q.uid_b == GPE_UID_ABSENT) {
            return "a pair's uid_b is GPE_UID_ABSENT";
        }
    }
    return nullptr;
}

// The graph of a set bond_set_problem accepts.  false: some uid has more than GPE_BOND_MAX_DEGREE bonds (*g is then
// not to be used; g->max_degree says how many).
inline bool bond_graph_build(const gpe_bond *bonds, uint64_t k, BondGraph *g)
{
    *g = BondGraph();
    std::vector<uint32_t> uids;                                         // a, then b unless the bond is an anchor, per bond
    uids.reserve(2 * k);
    bool breakable = false;
    for (uint64_t j = 0; j < k; ++j) {
        uids.push_back(bonds[j].uid_a);
        if (!(bonds[j].flags & GPE_BOND_ANCHOR)) uids.push_back(bonds[j].uid_b);
        breakable |= bonds[j].max_length > 0.0f;
    }
    UidNodes u;
    uid_nodes_build(uids.data(), uids.size(), &u);
    g->nodes = std::move(u.nodes);
    g->row_start = std::move(u.row_start);
    g->max_degree = u.max_degree;
    if (g->max_degree > GPE_BOND_MAX_DEGREE) return false;
    g->rec.resize(k);
    g->state.assign(k, 0);
    if (breakable) g->max_length.resize(k);
    g->inc.resize(uids.size());
    size_t e = 0;
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_bond &q = bonds[j];
        BondRecord &r = g->rec[j];
        r.a = u.node_of[e];
        r.rest = plus_zero(q.rest_length);
        g->inc[u.at[e++]] = (uint32_t)(j << 1);
        if (q.flags & GPE_BOND_ANCHOR) {
            r.b = kBondAnchorBit | (uint32_t)(g->anchors.size() / 2);
            r.w = q.stiffness;
            g->anchors.push_back(q.anchor_x);
            g->anchors.push_back(q.anchor_y);
        } else {
            r.b = u.node_of[e];
            r.w = 0.5f * q.stiffness;
            g->inc[u.at[e++]] = (uint32_t)(j << 1) | 1u;
        }
        if (breakable) g->max_length[j] = plus_zero(q.max_length);
        if (q.flags & GPE_BOND_BROKEN) {
            g->state[j] = 1;
            g->broken += 1;
        }
    }
    return true;
}

}  // namespace gpe
