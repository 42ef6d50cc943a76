// bond_colours.h -- the colouring behind the bonds' coloured solver (gpe_set_bond_solver): which bonds may be relaxed
// side by side, and in which order the rest follow.  Plain C++, no HIP header: gpe_bonds.hip includes it, and so does
// the CPU test program (tests/cpp/bond_colours_tests.cpp).
//
// Two bonds that share a particle must not be relaxed at once (both would write it), so every bond gets a colour no
// bond at either of its ends has: greedy, in ascending bond index j,
//     colour[j] = the least c >= 0 that no bond of lower index has taken at node a, nor at node b for a pair.
// An anchor occupies its node a only (its point is no node).  Every bond is coloured: a broken one, one whose uid no
// particle has, and both twins of a bond listed twice (which share two nodes, so their colours differ).  The colouring
// is a function of the records in their order alone -- of nothing on the device, and of no particle.
// Greedy needs at most 2 * degree - 1 colours.  A coloured relaxation visits the bonds in `order`: by colour, within a
// colour by index; colour c is order[colour_start[c] .. colour_start[c + 1]).
#pragma once

#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "bond_graph.h"

namespace gpe {

struct BondColours {
    std::vector<uint32_t> colour;        // k
    std::vector<uint32_t> order;         // k: the bond indices sorted by (colour, index)
    std::vector<uint32_t> colour_start;  // colours + 1
    uint32_t colours = 0;                // C: 1 + the largest colour given (0 for no bonds)
    uint32_t largest = 0;                // the bonds of the fullest colour
};

// The colours of k records over m nodes (bond_graph_build's: every node index < m; a record whose index is not is
// coloured as if it had no such end).  false: the set needs more than GPE_BOND_COLOURS_MAX colours -- out->colours says
// how many, the tables are complete all the same.
inline bool bond_colours_build(const BondRecord *rec, uint64_t k, uint64_t m, BondColours *out)
{
    *out = BondColours();
    // the colours taken at a node: colours 0 .. 63 in one word per node, the rest (a set that will be refused, but whose
    // count the refusal names) in words only the crowded nodes have
    std::vector<uint64_t> low(m, 0);
    std::unordered_map<uint64_t, std::vector<uint64_t>> high;          // node -> words 1, 2, ...
    const auto word = [&](uint64_t node, size_t w) -> uint64_t {
        if (node >= m) return 0;
        if (w == 0) return low[node];
        const auto it = high.find(node);
        return (it == high.end() || it->second.size() < w) ? 0 : it->second[w - 1];
    };
    const auto take = [&](uint64_t node, uint32_t c) {
        if (node >= m) return;
        if (c < 64) { low[node] |= 1ull << c; return; }
        std::vector<uint64_t> &v = high[node];
        if (v.size() < c / 64) v.resize(c / 64, 0);
        v[c / 64 - 1] |= 1ull << (c % 64);
    };
    out->colour.resize(k);
    std::vector<uint32_t> size;
    for (uint64_t j = 0; j < k; ++j) {
        const uint64_t a = rec[j].a;
        const uint64_t b = (rec[j].b & kBondAnchorBit) ? m : rec[j].b;  // (m: no node)
        uint32_t c = 0;
        for (size_t w = 0;; ++w) {
            const uint64_t taken = word(a, w) | word(b, w);
            if (taken != ~0ull) { c = (uint32_t)(64 * w) + (uint32_t)__builtin_ctzll(~taken); break; }
        }
        take(a, c);
        take(b, c);
        out->colour[j] = c;
        if (c >= size.size()) size.resize(c + 1, 0);
        size[c] += 1;
    }
    out->colours = (uint32_t)size.size();
    out->colour_start.assign(out->colours + 1, 0);
    for (uint32_t c = 0; c < out->colours; ++c) {
        out->colour_start[c + 1] = out->colour_start[c] + size[c];
        if (size[c] > out->largest) out->largest = size[c];
    }
    std::vector<uint32_t> at(out->colour_start.begin(), out->colour_start.end() - 1);
    out->order.resize(k);
    for (uint64_t j = 0; j < k; ++j) out->order[at[out->colour[j]]++] = (uint32_t)j;   // ascending j within a colour
    return out->colours <= GPE_BOND_COLOURS_MAX;
}

}  // namespace gpe
