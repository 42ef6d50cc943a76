// lookup_grid.h -- what the lookup grids of the static colliders, the force fields and the movers share on the host:
// which resolution a world gets, the grid of one cell, and the CSR table of the two that keep lists.  Pure C++ (no
// HIP): collider_grid.h, field_grid.h and mover_grid.h hold the listing rules and their completeness arguments,
// tests/cpp/lookup_grid_tests.cpp drives this header alone on the CPU.
//
// A grid is gx x gy square cells from the world's origin, at most `dim` per axis.  The pass finds a particle's cell by
// one binary32 product per axis (collider_cell_of).  The grid of one cell is always valid: it lists every item.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "k_collider.h"

namespace gpe {

struct LookupView {
    ColliderGridView view;                 // what the pass is handed
    double cell = 1.0;                     // the exact cell size: 1 / (double)view.inv_cell (one cell: unused)
};

// (a grid is kept while rb, W and H are bit for bit what it was built for)
inline uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}

// the CSR table: the item indices of a cell ascending
struct LookupGrid : LookupView {
    std::vector<uint32_t> cell_start;      // gx * gy + 1
    std::vector<uint32_t> items;
};

// The view of one cell, whatever the world and rb are.  extent: the size of the cell, twice the world's (0: there is no
// usable world).  Anything but a cell with a normal reciprocal leaves inv_cell = 0: every finite p lands in the cell,
// every other one walks all items, which is the same list.
inline LookupView lookup_grid_one_cell(float rb, double extent)
{
    LookupView v;
    v.view.rb = rb;
    const float cell = (float)extent;
    const float inv = 1.0f / cell;
    if (extent > 0.0 && isfinite(cell) && isfinite(inv) && inv >= 1e-30f) v.view.inv_cell = inv;
    v.cell = v.view.inv_cell > 0.0f ? 1.0 / (double)v.view.inv_cell : 1.0;
    return v;
}

// The view for the radius bound rb >= 0 (or NaN) and the world W x H, all as the context holds them (anything goes).
// Cells of max(4 rb, max(W, H) / dim) at first, doubled while an axis has more than dim cells or attempt(view) -- the
// caller's "try this resolution" -- says no; the one cell when both axes are down to one cell, and for a world that is
// not positive and finite, lies outside [min_world, 1e20], or comes with an rb that is not finite.
template <class Attempt>
inline LookupView lookup_grid_choose(float rb, float W, float H, uint32_t dim, double min_world, Attempt attempt)
{
    const double w = W, h = H, world = std::max(w, h);
    if (!(w > 0.0 && h > 0.0 && isfinite(world) && isfinite(rb) && world >= min_world && world <= 1e20))
        return lookup_grid_one_cell(rb, world > 0.0 && isfinite(world) ? world * 2.0 : 0.0);
    for (double want = std::max(4.0 * (double)rb, world / (double)dim);; want *= 2.0) {
        // the pass multiplies by a binary32 reciprocal: the cell IS 1 / that number
        const float inv = 1.0f / (float)want;
        const double cell = 1.0 / (double)inv;
        const double nx = floor(w / cell) + 1.0, ny = floor(h / cell) + 1.0;      // W and H lie strictly inside the grid
        if (nx <= 1.0 && ny <= 1.0) break;
        if (nx > (double)dim || ny > (double)dim) continue;
        LookupView v;
        v.view.inv_cell = inv;
        v.view.gx = (uint32_t)nx; v.view.gy = (uint32_t)ny;
        v.view.gxf = (float)v.view.gx; v.view.gyf = (float)v.view.gy;
        v.view.rb = rb;
        v.cell = cell;
        if (attempt(v)) return v;
    }
    return lookup_grid_one_cell(rb, world * 2.0);
}

// The table of g's view for k items.  cells_of(j, emit) names the cells of item j at this resolution as runs:
// emit(first, last) for the cells first .. last of one row (or of the whole grid), cell = cy * gx + cx.  It is asked
// twice per item -- to count, then to fill -- and must name the same runs both times.  Item by item, so every cell's
// list ascends.  emit returns false once more than max_entries entries are counted; cells_of may stop there.
// false: more than max_entries entries (the table is left unusable).
template <class CellsOf>
inline bool lookup_grid_fill(LookupGrid &g, uint32_t k, uint64_t max_entries, CellsOf cells_of)
{
    const uint64_t cells = (uint64_t)g.view.gx * g.view.gy;
    g.cell_start.assign(cells + 1, 0);
    g.items.clear();
    uint64_t total = 0;
    for (uint32_t j = 0; j < k && total <= max_entries; ++j)
        cells_of(j, [&](uint64_t first, uint64_t last) {
            if (total > max_entries) return false;
            total += last - first + 1;
            if (total > max_entries) return false;
            for (uint64_t c = first; c <= last; ++c) g.cell_start[c + 1] += 1;
            return true;
        });
    if (total > max_entries) return false;
    // counts -> starts; the fill advances cell_start[i] to the end of cell i, which is the start of cell i + 1:
    // shifting by one afterwards restores it
    for (uint64_t i = 0; i < cells; ++i) g.cell_start[i + 1] += g.cell_start[i];
    g.items.assign((size_t)total, 0);
    for (uint32_t j = 0; j < k; ++j)
        cells_of(j, [&](uint64_t first, uint64_t last) {
            for (uint64_t c = first; c <= last; ++c) g.items[g.cell_start[c]++] = j;
            return true;
        });
    for (uint64_t i = cells; i > 0; --i) g.cell_start[i] = g.cell_start[i - 1];
    g.cell_start[0] = 0;
    return true;
}

// The table at the first resolution whose lists hold at most max_entries entries, else the one cell with every item.
// prepare(view) readies the caller's per-item data for a resolution; cells_of as lookup_grid_fill takes it.
template <class Prepare, class CellsOf>
inline LookupGrid lookup_grid_build(uint32_t k, float rb, float W, float H, uint32_t dim, double min_world, uint64_t max_entries,
                                    Prepare prepare, CellsOf cells_of)
{
    LookupGrid g;
    const LookupView v = lookup_grid_choose(rb, W, H, dim, min_world, [&](const LookupView &at) {
        static_cast<LookupView &>(g) = at;
        prepare(at);
        return lookup_grid_fill(g, k, max_entries, cells_of);
    });
    if (v.view.gx == 1 && v.view.gy == 1) {                    // the one cell (a resolution tried has two cells at least)
        static_cast<LookupView &>(g) = v;
        g.cell_start.assign(2, 0);
        g.cell_start[1] = k;
        g.items.resize(k);
        for (uint32_t j = 0; j < k; ++j) g.items[j] = j;
    }
    return g;
}

}  // namespace gpe
