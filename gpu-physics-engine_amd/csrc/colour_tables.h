// colour_tables.h -- the greedy colouring the coloured solvers share (bond_colours.h, bend_colours.h): constraints that
// name the same node get different colours, so that the constraints of one colour can be relaxed side by side.  Plain
// C++, no HIP header.
//
// In ascending constraint index j,
//     colour[j] = the least c >= 0 that no constraint of lower index has taken at any of j's nodes.
// What a constraint's nodes are is its caller's (a bond: one or two, a bend: three); a node index that is not below m
// counts as no node.  A function of the constraints in their order alone.  A coloured relaxation visits the
// constraints in `order`: by colour, within a colour by index; colour c is order[colour_start[c] .. colour_start[c + 1]).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace gpe {

struct ColourTables {
    std::vector<uint32_t> colour;        // k
    std::vector<uint32_t> order;         // k: the constraint indices sorted by (colour, index)
    std::vector<uint32_t> colour_start;  // colours + 1
    uint32_t colours = 0;                // C: 1 + the largest colour given (0 for no constraints)
    uint32_t largest = 0;                // the constraints of the fullest colour
};

constexpr size_t kColourNodesMax = 3;    // the most nodes one constraint names

// The colours of k constraints over m nodes.  nodes_of(j, v) writes constraint j's nodes into v[0 .. kColourNodesMax)
// and returns how many there are.  *out is complete whatever it takes: out->colours says how many colours, and the
// caller compares it with its limit.
template <class NodesOf>
inline void colour_tables_build(uint64_t k, uint64_t m, NodesOf nodes_of, ColourTables *out)
{
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
        uint64_t v[kColourNodesMax];
        const size_t nv = nodes_of(j, v);
        uint32_t c = 0;
        for (size_t w = 0;; ++w) {
            uint64_t taken = 0;
            for (size_t i = 0; i < nv; ++i) taken |= word(v[i], w);
            if (taken != ~0ull) { c = (uint32_t)(64 * w) + (uint32_t)__builtin_ctzll(~taken); break; }
        }
        for (size_t i = 0; i < nv; ++i) take(v[i], c);
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
}

}  // namespace gpe
