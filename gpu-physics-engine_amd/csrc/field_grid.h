// field_grid.h -- the lookup grid of the force fields, built on the host in double.  Pure C++ (no HIP), like
// collider_grid.h: gpe_fields.hip uploads what it builds, tests/cpp/field_grid_tests.cpp drives it on the CPU.
//
// The grid is a CSR table over gx x gy square cells from the world's origin: cell_start[cells + 1] and items[], the
// field indices of a cell ASCENDING -- the pass sums a particle's fields in list order, so the order is part of the
// result.  The view and the cell function are the colliders' (ColliderGridView, collider_cell_of of k_collider.h).
//
// Completeness ("Force fields").  For every point p whose cell collider_cell_of(p) lies in the grid, the
// cell's list holds every field that field_matches can accept at p.  A field is listed in a cell when the cell meets
// its region inflated by one whole cell: the box [x0 - cell, x1 + cell] x [y0 - cell, y1 + cell], the disc of radius
// R + cell.  The whole cell pays for every rounding: p lies within 2^-12 cells of the cell the binary32 cell function
// names; the box predicate compares exactly; for a circle whose M = |x0| + |y0| + R is at most 2^17 cells the binary32
// disc predicate accepts only within R (1 + 2^-21) + 2^-74 < R + cell / 8 of the centre (cells are at least 2^-40).  A
// field beyond that magnitude is listed in every cell, and so is EVERYWHERE.  A box with x0 > x1 or y0 > y1 accepts
// nothing and is listed nowhere.  The grid of one cell lists every field: it is always valid.  Matching ignores the
// particle's radius, so the grid depends on the set and the world alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "k_collider.h"
#include "k_field.h"

namespace gpe {

constexpr uint64_t kFieldGridMaxEntries = 4ull << 20;          // items[] stays at or under 4 M entries
constexpr double kFieldFarCells = 131072.0;                    // 2^17: past this many cells a field is listed everywhere

struct FieldRegion { uint32_t shape; float x0, y0, x1, y1; };

struct FieldGrid {
    ColliderGridView view;                 // what the pass is handed (rb unused: 0)
    double cell = 1.0;                     // the exact cell size: 1 / (double)view.inv_cell (one cell: unused)
    std::vector<uint32_t> cell_start;      // gx * gy + 1
    std::vector<uint32_t> items;
};

// what a field covers at one resolution
struct FieldSpan {
    uint8_t everywhere = 0;                // EVERYWHERE, or far: every cell
    uint32_t row0 = 1, row1 = 0;           // rows it can reach (row0 > row1: none)
    uint32_t col0 = 1, col1 = 0;           // BOX: the columns, the same in every row
};

inline bool field_cells_of(double lo, double hi, double cell, uint32_t g, uint32_t *c0, uint32_t *c1)
{
    if (!(lo <= hi) || hi < 0.0 || lo >= (double)g * cell) return false;
    const double a = floor(lo / cell), b = floor(hi / cell);
    *c0 = a > 0.0 ? (uint32_t)a : 0u;
    *c1 = b < (double)(g - 1) ? (uint32_t)b : g - 1;
    return *c0 <= *c1;
}

// The columns of a circle in row cy: the cells that meet the disc of radius R + cell (+ 1 % of a cell for this
// function's own double roundings).
inline bool field_circle_row(const FieldRegion &f, double cell, uint32_t cy, uint32_t gx, uint32_t *c0, uint32_t *c1)
{
    const double R = (double)f.x1 + 1.01 * cell;
    const double lo = (double)cy * cell, hi = ((double)cy + 1.0) * cell, y = f.y0;
    const double dy = y < lo ? lo - y : (y > hi ? y - hi : 0.0);
    if (dy > R) return false;
    const double hw = sqrt(R * R - dy * dy) + 0.01 * cell;
    return field_cells_of((double)f.x0 - hw, (double)f.x0 + hw, cell, gx, c0, c1);
}

// One attempt at a resolution.  false: more than max_entries entries (the grid is left unusable).
inline bool field_grid_fill(FieldGrid &g, const FieldRegion *fs, uint32_t k, uint64_t max_entries)
{
    const uint32_t gx = g.view.gx, gy = g.view.gy;
    const uint64_t cells = (uint64_t)gx * gy;
    const double cell = g.cell;
    std::vector<FieldSpan> span(k);
    for (uint32_t j = 0; j < k; ++j) {
        const FieldRegion &f = fs[j];
        FieldSpan &s = span[j];
        if (f.shape == kFieldEverywhere) { s.everywhere = 1; continue; }
        if (f.shape == kFieldBox && (f.x0 > f.x1 || f.y0 > f.y1)) continue;            // accepts nothing
        const double m = f.shape == kFieldCircle ? fabs((double)f.x0) + fabs((double)f.y0) + fabs((double)f.x1)
                                                 : std::max(std::max(fabs((double)f.x0), fabs((double)f.y0)),
                                                            std::max(fabs((double)f.x1), fabs((double)f.y1)));
        if (!(m <= kFieldFarCells * cell)) { s.everywhere = 1; continue; }
        const double pad = 1.01 * cell;
        if (f.shape == kFieldCircle) {
            const double R = (double)f.x1 + pad;
            if (!field_cells_of((double)f.y0 - R, (double)f.y0 + R, cell, gy, &s.row0, &s.row1)) { s.row0 = 1; s.row1 = 0; }
        } else {
            if (!field_cells_of((double)f.y0 - pad, (double)f.y1 + pad, cell, gy, &s.row0, &s.row1) ||
                !field_cells_of((double)f.x0 - pad, (double)f.x1 + pad, cell, gx, &s.col0, &s.col1)) { s.row0 = 1; s.row1 = 0; }
        }
    }
    // two sweeps over the same candidates: count, then fill.  Field by field, so every cell's list ascends
    g.cell_start.assign(cells + 1, 0);
    g.items.clear();
    for (int sweep = 0; sweep < 2; ++sweep) {
        uint64_t total = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const FieldSpan &s = span[j];
            if (s.everywhere) {
                total += cells;
                if (sweep == 0 && total > max_entries) return false;
                for (uint64_t cell_i = 0; cell_i < cells; ++cell_i) {
                    if (sweep == 0) g.cell_start[cell_i + 1] += 1;
                    else g.items[g.cell_start[cell_i]++] = j;
                }
                continue;
            }
            for (uint32_t cy = s.row0; cy <= s.row1 && s.row0 <= s.row1; ++cy) {
                uint32_t c0 = s.col0, c1 = s.col1;
                if (fs[j].shape == kFieldCircle && !field_circle_row(fs[j], cell, cy, gx, &c0, &c1)) continue;
                total += (uint64_t)(c1 - c0) + 1;
                if (sweep == 0 && total > max_entries) return false;
                for (uint32_t cx = c0; cx <= c1; ++cx) {
                    const uint64_t cell_i = (uint64_t)cy * gx + cx;
                    if (sweep == 0) g.cell_start[cell_i + 1] += 1;
                    else g.items[g.cell_start[cell_i]++] = j;
                }
            }
        }
        if (sweep == 0) {
            // counts -> starts; the fill advances cell_start[i] to the end of cell i, which is the start of cell i + 1:
            // shifting by one afterwards restores it
            for (uint64_t i = 0; i < cells; ++i) g.cell_start[i + 1] += g.cell_start[i];
            g.items.assign((size_t)total, 0);
        }
    }
    for (uint64_t i = cells; i > 0; --i) g.cell_start[i] = g.cell_start[i - 1];
    g.cell_start[0] = 0;
    return true;
}

// The grid of one cell: every field, whatever the world is.
// extent: the size of the cell, twice the world's (0: there is no usable world).
inline void field_grid_one_cell(FieldGrid &g, uint32_t k, double extent)
{
    g.view = ColliderGridView();
    const float cell = (float)extent;
    const float inv = 1.0f / cell;
    // anything but a cell with a normal reciprocal leaves inv_cell = 0: every finite p lands in the cell, every other
    // one walks all fields, which is the same list
    if (extent > 0.0 && isfinite(cell) && isfinite(inv) && inv >= 1e-30f) g.view.inv_cell = inv;
    g.cell = g.view.inv_cell > 0.0f ? 1.0 / (double)g.view.inv_cell : 1.0;
    g.cell_start.assign(2, 0);
    g.cell_start[1] = k;
    g.items.resize(k);
    for (uint32_t j = 0; j < k; ++j) g.items[j] = j;
}

// The grid for k <= GPE_FIELDS_MAX validated fields (finite coordinates, a circle's radius >= 0) and the world W x H
// as the context holds it (W and H may be anything).  The resolution: cells of max(W, H) / 1024, doubled until items[]
// holds at most max_entries entries.  A world outside [1e-6, 1e20] gets the one cell.
inline FieldGrid field_grid_build(const FieldRegion *fs, uint32_t k, float W, float H,
                                  uint64_t max_entries = kFieldGridMaxEntries)
{
    FieldGrid g;
    const double w = W, h = H, world = std::max(w, h);
    if (!(w > 0.0 && h > 0.0 && isfinite(world) && world >= 1e-6 && world <= 1e20)) {
        field_grid_one_cell(g, k, world > 0.0 && isfinite(world) ? world * 2.0 : 0.0);
        return g;
    }
    for (double want = world / 1024.0;; want *= 2.0) {
        // the pass multiplies by a binary32 reciprocal: the cell IS 1 / that number
        const float inv = 1.0f / (float)want;
        const double cell = 1.0 / (double)inv;
        const double nx = floor(w / cell) + 1.0, ny = floor(h / cell) + 1.0;      // W and H lie strictly inside the grid
        if (nx <= 1.0 && ny <= 1.0) break;
        if (nx > (double)kColliderGridMaxDim || ny > (double)kColliderGridMaxDim) continue;
        g.view = ColliderGridView();
        g.view.inv_cell = inv;
        g.view.gx = (uint32_t)nx; g.view.gy = (uint32_t)ny;
        g.view.gxf = (float)g.view.gx; g.view.gyf = (float)g.view.gy;
        g.cell = cell;
        if (field_grid_fill(g, fs, k, max_entries)) return g;
    }
    field_grid_one_cell(g, k, world * 2.0);
    return g;
}

}  // namespace gpe
