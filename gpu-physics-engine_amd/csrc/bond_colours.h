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

#include "bond_graph.h"
#include "colour_tables.h"

namespace gpe {

using BondColours = ColourTables;        // colour, order, colour_start, colours, largest: of the bonds

// The colours of k records over m nodes (bond_graph_build's: every node index < m; a record whose index is not is
// coloured as if it had no such end).  false: the set needs more than GPE_BOND_COLOURS_MAX colours -- out->colours says
// how many, the tables are complete all the same.  The greedy core is colour_tables.h's, shared with the bends.
inline bool bond_colours_build(const BondRecord *rec, uint64_t k, uint64_t m, BondColours *out)
{
    *out = BondColours();
    colour_tables_build(k, m, [&](uint64_t j, uint64_t *v) -> size_t {
        v[0] = rec[j].a;
        if (rec[j].b & kBondAnchorBit) return 1;                       // (its point is no node)
        v[1] = rec[j].b;
        return 2;
    }, out);
    return out->colours <= GPE_BOND_COLOURS_MAX;
}

}  // namespace gpe
