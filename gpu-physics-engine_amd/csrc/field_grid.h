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
#include "lookup_grid.h"

namespace gpe {

constexpr uint64_t kFieldGridMaxEntries = 4ull << 20;          // items[] stays at or under 4 M entries
constexpr double kFieldFarCells = 131072.0;                    // 2^17: past this many cells a field is listed everywhere

struct FieldRegion { uint32_t shape; float x0, y0, x1, y1; };

using FieldGrid = LookupGrid;              // (view.rb unused: 0)

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

// The grid for k <= GPE_FIELDS_MAX validated fields (finite coordinates, a circle's radius >= 0) and the world W x H
// as the context holds it (W and H may be anything).  The resolution: cells of max(W, H) / 1024, doubled until items[]
// holds at most max_entries entries (lookup_grid.h, with a radius bound of 0).  A world outside [1e-6, 1e20] gets the
// one cell.
inline FieldGrid field_grid_build(const FieldRegion *fs, uint32_t k, float W, float H,
                                  uint64_t max_entries = kFieldGridMaxEntries)
{
    std::vector<FieldSpan> span(k);
    uint32_t gx = 1, gy = 1;
    double cell = 1.0;
    auto prepare = [&](const LookupView &v) {
        gx = v.view.gx; gy = v.view.gy;
        cell = v.cell;
        for (uint32_t j = 0; j < k; ++j) {
            const FieldRegion &f = fs[j];
            FieldSpan &s = span[j] = FieldSpan();
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
    };
    auto cells_of = [&](uint32_t j, auto emit) {
        const FieldSpan &s = span[j];
        if (s.everywhere) { emit(0, (uint64_t)gx * gy - 1); return; }
        for (uint32_t cy = s.row0; cy <= s.row1 && s.row0 <= s.row1; ++cy) {
            uint32_t c0 = s.col0, c1 = s.col1;
            if (fs[j].shape == kFieldCircle && !field_circle_row(fs[j], cell, cy, gx, &c0, &c1)) continue;
            if (!emit((uint64_t)cy * gx + c0, (uint64_t)cy * gx + c1)) return;
        }
    };
    return lookup_grid_build(k, 0.0f, W, H, kColliderGridMaxDim, 1e-6, max_entries, prepare, cells_of);
}

}  // namespace gpe
