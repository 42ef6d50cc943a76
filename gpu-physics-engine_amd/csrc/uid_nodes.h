// uid_nodes.h -- what the host sides of the step sets that name their particles by uid share (bond_graph.h,
// bend_graph.h, area_table.h).  Plain C++, no HIP header: the graph headers compile on the CPU, and so does this one's
// own test program (tests/cpp/uid_nodes_tests.cpp).
//
// An incidence is one appearance of a uid in a set.  uid_nodes_build takes the uid of every incidence, in the set's
// incidence order (ascending constraint index), and makes of them
//   - nodes: the distinct uids, ascending;
//   - per incidence its node index;
//   - row_start: a CSR over the nodes (m + 1 entries), and max_degree, the longest row;
//   - per incidence its position in the row-ordered list.  The caller writes its own incidence word there.  Incidences
//     of one node keep their order, so every row comes out in ascending constraint index.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gpe {

// -0.0 -> +0: what a set stores of a value it only compares and multiplies, so that records compare by bits
inline float plus_zero(float x) { return x == 0.0f ? 0.0f : x; }

struct UidNodes {
    std::vector<uint32_t> nodes;         // m: the uids, ascending, distinct
    std::vector<uint32_t> node_of;       // per incidence: its node index
    std::vector<uint32_t> row_start;     // m + 1
    std::vector<uint32_t> at;            // per incidence: its position in the row-ordered list
    uint32_t max_degree = 0;
};

inline void uid_nodes_build(const uint32_t *uid, uint64_t count, UidNodes *u)
{
    *u = UidNodes();
    std::vector<uint32_t> &nodes = u->nodes;
    nodes.assign(uid, uid + count);
    std::sort(nodes.begin(), nodes.end());
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    const size_t m = nodes.size();
    u->node_of.resize(count);
    u->row_start.assign(m + 1, 0);
    for (uint64_t e = 0; e < count; ++e) {
        const uint32_t v = (uint32_t)(std::lower_bound(nodes.begin(), nodes.end(), uid[e]) - nodes.begin());
        u->node_of[e] = v;
        u->row_start[v + 1] += 1;
    }
    for (size_t v = 0; v < m; ++v) {
        u->max_degree = std::max(u->max_degree, u->row_start[v + 1]);
        u->row_start[v + 1] += u->row_start[v];
    }
    u->at.resize(count);
    std::vector<uint32_t> fill(u->row_start.begin(), u->row_start.end() - 1);
    for (uint64_t e = 0; e < count; ++e) u->at[e] = fill[u->node_of[e]]++;   // ascending e: a row keeps incidence order
}

}  // namespace gpe
