// bend_graph.h -- the host side of a bend set: its validation and the graph the pass walks.  Plain C++, no HIP header:
// gpe_bends.hip includes it, and so does the CPU test program (tests/cpp/bend_graph_tests.cpp).
//
// bend_graph_build turns k bends into
//   - nodes: the distinct uids the bends name, ascending (m <= 3 k);
//   - per bend its three particles as node indices, with the rest angle and the stiffness (-0.0 stored as +0);
//   - a CSR of incidences per node, in ascending bend index: entry = bend << 2 | role (0: the node is the bend's a,
//     1: its hinge b, 2: its c).  A bend listed twice appears twice, in all three rows.  The nodes and the rows are
//     uid_nodes.h's.
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

enum BendRole : uint32_t { kBendRoleA = 0, kBendRoleHinge = 1, kBendRoleC = 2 };

struct BendRecord {              // 32 bytes: what the bend phase reads per bend, as two 16-byte words
    uint32_t a, b, c;            // node indices; b is the hinge
    float rc;                    // the rest angle's cosine ...
    float rs;                    // ... and sine
    float stiffness;
    uint32_t pad0, pad1;         // 0
};

struct BendGraph {
    std::vector<uint32_t> nodes;         // m: the uids, ascending, distinct
    std::vector<BendRecord> rec;         // k
    std::vector<uint32_t> row_start;     // m + 1
    std::vector<uint32_t> inc;           // row_start[m] = 3 k entries: bend << 2 | role
    uint32_t max_degree = 0;
};

// NULL: the set is valid.  Otherwise what is wrong with it (the caller names the call in front).
inline const char *bend_set_problem(const gpe_bend *bends, uint64_t k, uint32_t iterations)
{
    if (k > 0 && !bends) return "NULL bends";
    if (k > GPE_BENDS_MAX) return "k must be at most GPE_BENDS_MAX";
    if (iterations < 1 || iterations > GPE_BEND_ITER_MAX) return "iterations must be 1 .. GPE_BEND_ITER_MAX";
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_bend &q = bends[j];
        if (q.uid_a == GPE_UID_ABSENT || q.uid_b == GPE_UID_ABSENT || q.uid_c == GPE_UID_ABSENT)
            return "a uid is GPE_UID_ABSENT";
        if (q.uid_a == q.uid_b || q.uid_b == q.uid_c || q.uid_a == q.uid_c) return "a bend names a particle twice";
        if (!isfinite(q.rest_cos) || !isfinite(q.rest_sin)) return "a rest_cos or rest_sin is not finite";
        const float cc = q.rest_cos * q.rest_cos;
        const float ss = q.rest_sin * q.rest_sin;
        const float norm = cc + ss;
        if (!(fabsf(norm - 1.0f) <= 0x1p-20f)) return "(rest_cos, rest_sin) is not a unit vector";
        if (!(q.stiffness >= 0.0f && q.stiffness <= 1.0f)) return "a stiffness is NaN or outside [0, 1]";
        if (q.flags != 0 || q.reserved != 0) return "flags and reserved must be 0";
    }
    return nullptr;
}

// The graph of a set bend_set_problem accepts.  false: some uid has more than GPE_BEND_MAX_DEGREE bends (*g is then
// not to be used; g->max_degree says how many).
inline bool bend_graph_build(const gpe_bend *bends, uint64_t k, BendGraph *g)
{
    *g = BendGraph();
    std::vector<uint32_t> uids;                                         // a, b, c per bend
    uids.reserve(3 * k);
    for (uint64_t j = 0; j < k; ++j) {
        uids.push_back(bends[j].uid_a);
        uids.push_back(bends[j].uid_b);
        uids.push_back(bends[j].uid_c);
    }
    UidNodes u;
    uid_nodes_build(uids.data(), uids.size(), &u);
    g->nodes = std::move(u.nodes);
    g->row_start = std::move(u.row_start);
    g->max_degree = u.max_degree;
    if (g->max_degree > GPE_BEND_MAX_DEGREE) return false;
    g->rec.resize(k);
    g->inc.resize(3 * k);
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_bend &q = bends[j];
        BendRecord &r = g->rec[j];
        r.a = u.node_of[3 * j];
        r.b = u.node_of[3 * j + 1];
        r.c = u.node_of[3 * j + 2];
        r.rc = plus_zero(q.rest_cos);
        r.rs = plus_zero(q.rest_sin);
        r.stiffness = plus_zero(q.stiffness);
        r.pad0 = r.pad1 = 0;
        g->inc[u.at[3 * j]] = (uint32_t)(j << 2) | kBendRoleA;
        g->inc[u.at[3 * j + 1]] = (uint32_t)(j << 2) | kBendRoleHinge;
        g->inc[u.at[3 * j + 2]] = (uint32_t)(j << 2) | kBendRoleC;
    }
    return true;
}

}  // namespace gpe
