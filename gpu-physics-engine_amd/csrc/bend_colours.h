// bend_colours.h -- the colouring behind the bends' coloured solver (gpe_set_bend_solver): which bends may be relaxed
// side by side, and in which order the rest follow.  Plain C++, no HIP header: gpe_bends.hip includes it, and so does
// the CPU test program (tests/cpp/bend_colours_tests.cpp).
//
// Two bends that share a particle must not be relaxed at once (both would write it), so every bend gets a colour no
// bend at any of its three particles has: greedy, in ascending bend index j,
//     colour[j] = the least c >= 0 that no bend of lower index has taken at node a, at the hinge b or at node c.
// Every bend is coloured: one whose uid no particle has, and both twins of a bend listed twice (which share three
// nodes, so their colours differ).  The colouring is a function of the records in their order alone -- of nothing on
// the device, and of no particle.  Greedy needs at most 3 * (degree - 1) + 1 colours; a chain listed in order takes 3.
// A coloured relaxation visits the bends in `order`: by colour, within a colour by index; colour c is
// order[colour_start[c] .. colour_start[c + 1]).  The greedy core is colour_tables.h's, shared with the bonds.
#pragma once

#include <stdint.h>

#include "bend_graph.h"
#include "colour_tables.h"

namespace gpe {

using BendColours = ColourTables;        // colour, order, colour_start, colours, largest: of the bends

// The colours of k records over m nodes (bend_graph_build's: every node index < m; a record whose index is not is
// coloured as if it had no such particle).  false: the set needs more than GPE_BEND_COLOURS_MAX colours -- out->colours
// says how many, the tables are complete all the same.
inline bool bend_colours_build(const BendRecord *rec, uint64_t k, uint64_t m, BendColours *out)
{
    *out = BendColours();
    colour_tables_build(k, m, [&](uint64_t j, uint64_t *v) -> size_t {
        v[0] = rec[j].a;
        v[1] = rec[j].b;
        v[2] = rec[j].c;
        return 3;
    }, out);
    return out->colours <= GPE_BEND_COLOURS_MAX;
}

}  // namespace gpe
