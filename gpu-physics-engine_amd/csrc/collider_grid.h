// collider_grid.h -- the lookup grid of the static colliders, built on the host in double.  Pure C++ (no HIP), like
// native_policy.h: gpe_colliders.hip uploads what it builds, tests/cpp/collider_grid_tests.cpp drives it on the CPU.
//
// The grid is a CSR table over gx x gy square cells from the world's origin: cell_start[cells + 1] and items[], the
// collider indices of a cell ascending.
//
// Completeness ("Static colliders").  For every point p whose cell collider_cell_of(p) lies in the grid, the
// cell's list holds every collider that collider_touch can report touched for any |r| <= rb.  A collider is listed in
// a cell when the distance from its segment to the cell's centre is at most R + rb + cell + half the cell's diagonal:
// the distance to the nearest point of the cell, inflated by the reach R + rb and by one whole cell.  The whole cell
// pays for every rounding: p lies within 2^-12 cells of the cell the binary32 cell function names, and for a collider
// with M = max |coordinate| + R + rb <= 2^17 cells the binary32 predicate reports touched only within
// (R + rb)(1 + 2^-22) + 17 * 2^-24 * M < R + rb + cell / 4 of the segment.  A collider beyond that magnitude is listed
// in every cell.  The grid of one cell lists every collider: it is always valid.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "k_collider.h"

namespace gpe {

constexpr uint64_t kColliderGridMaxEntries = 4ull << 20;       // items[] stays at or under 4 M entries
constexpr double kColliderFarCells = 131072.0;                 // 2^17: past this many cells a collider is listed everywhere

struct ColliderCapsule { float ax, ay, bx, by, radius; };

struct ColliderGrid {
    ColliderGridView view;                 // what the pass is handed
    double cell = 1.0;                     // the exact cell size: 1 / (double)view.inv_cell (one cell: unused)
    std::vector<uint32_t> cell_start;      // gx * gy + 1
    std::vector<uint32_t> items;
};

inline double collider_point_segment_distance(double px, double py, double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay, fx = px - ax, fy = py - ay;
    const double A = dx * dx + dy * dy;
    double u = A > 0.0 ? (fx * dx + fy * dy) / A : 0.0;
    u = u > 0.0 ? u : 0.0;
    u = u < 1.0 ? u : 1.0;
    const double qx = fx - u * dx, qy = fy - u * dy;
    return sqrt(qx * qx + qy * qy);
}

// The candidates of row cy: the cells whose x-range comes within `reach` of the part of the segment that lies in the
// row's band inflated by `reach`.  false: the segment does not come near the row.
inline bool collider_row_span(const ColliderCapsule &c, double cell, double reach, uint32_t cy, uint32_t gx, uint32_t *x0,
                              uint32_t *x1)
{
    const double lo = (double)cy * cell - reach, hi = ((double)cy + 1.0) * cell + reach;
    const double ax = c.ax, ay = c.ay, dx = (double)c.bx - ax, dy = (double)c.by - ay;
    double u0 = 0.0, u1 = 1.0;
    if (dy == 0.0) {
        if (ay < lo || ay > hi) return false;
    } else {
        double ua = (lo - ay) / dy, ub = (hi - ay) / dy;
        if (ua > ub) std::swap(ua, ub);
        u0 = std::max(u0, ua);
        u1 = std::min(u1, ub);
        if (u0 > u1) return false;
    }
    const double xa = ax + u0 * dx, xb = ax + u1 * dx;
    const double xmin = std::min(xa, xb) - reach, xmax = std::max(xa, xb) + reach;
    if (xmax < 0.0 || xmin >= (double)gx * cell) return false;
    const double c0 = floor(xmin / cell), c1 = floor(xmax / cell);
    *x0 = c0 > 0.0 ? (uint32_t)c0 : 0u;
    *x1 = c1 < (double)(gx - 1) ? (uint32_t)c1 : gx - 1;
    return *x0 <= *x1;
}

// One attempt at a resolution.  false: more than max_entries entries (the grid is left unusable).
inline bool collider_grid_fill(ColliderGrid &g, const ColliderCapsule *cs, uint32_t k, double rb, uint64_t max_entries)
{
    const uint32_t gx = g.view.gx, gy = g.view.gy;
    const uint64_t cells = (uint64_t)gx * gy;
    const double cell = g.cell, half_diag = cell * 0.70710678118654757;
    std::vector<uint8_t> far(k, 0);
    std::vector<uint32_t> row0(k, 1), row1(k, 0);              // the rows a near collider can reach (empty: none)
    for (uint32_t j = 0; j < k; ++j) {
        const ColliderCapsule &c = cs[j];
        const double m = std::max(std::max(fabs((double)c.ax), fabs((double)c.ay)), std::max(fabs((double)c.bx), fabs((double)c.by)));
        if (!(m + c.radius + rb <= kColliderFarCells * cell)) { far[j] = 1; continue; }
        const double reach = (double)c.radius + rb + cell + half_diag + 0.01 * cell;
        const double ylo = std::min((double)c.ay, (double)c.by) - reach, yhi = std::max((double)c.ay, (double)c.by) + reach;
        if (yhi < 0.0 || ylo >= (double)gy * cell) continue;
        const double r0 = floor(ylo / cell), r1 = floor(yhi / cell);
        row0[j] = r0 > 0.0 ? (uint32_t)r0 : 0u;
        row1[j] = r1 < (double)(gy - 1) ? (uint32_t)r1 : gy - 1;
    }
    // two sweeps over the same candidates: count, then fill.  Collider by collider, so every cell's list ascends
    g.cell_start.assign(cells + 1, 0);
    g.items.clear();
    for (int sweep = 0; sweep < 2; ++sweep) {
        uint64_t total = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const ColliderCapsule &c = cs[j];
            if (far[j]) {
                total += cells;
                if (sweep == 0 && total > max_entries) return false;
                for (uint64_t cell_i = 0; cell_i < cells; ++cell_i) {
                    if (sweep == 0) g.cell_start[cell_i + 1] += 1;
                    else g.items[g.cell_start[cell_i]++] = j;
                }
                continue;
            }
            const double keep = (double)c.radius + rb + cell + half_diag;
            for (uint32_t cy = row0[j]; cy <= row1[j] && row0[j] <= row1[j]; ++cy) {
                uint32_t x0, x1;
                if (!collider_row_span(c, cell, keep + 0.01 * cell, cy, gx, &x0, &x1)) continue;
                for (uint32_t cx = x0; cx <= x1; ++cx) {
                    const double d = collider_point_segment_distance(((double)cx + 0.5) * cell, ((double)cy + 0.5) * cell,
                                                                     c.ax, c.ay, c.bx, c.by);
                    if (!(d <= keep)) continue;
                    const uint64_t cell_i = (uint64_t)cy * gx + cx;
                    total += 1;
                    if (sweep == 0) {
                        if (total > max_entries) return false;
                        g.cell_start[cell_i + 1] += 1;
                    } else {
                        g.items[g.cell_start[cell_i]++] = j;
                    }
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

// The grid of one cell: every collider, whatever the world and rb are.
// extent: the size of the cell, twice the world's (0: there is no usable world).
inline void collider_grid_one_cell(ColliderGrid &g, uint32_t k, float rb, double extent)
{
    g.view = ColliderGridView();
    g.view.rb = rb;
    const float cell = (float)extent;
    const float inv = 1.0f / cell;
    // anything but a cell with a normal reciprocal leaves inv_cell = 0: every finite p lands in the cell, every other
    // one walks all colliders, which is the same list
    if (extent > 0.0 && isfinite(cell) && isfinite(inv) && inv >= 1e-30f) g.view.inv_cell = inv;
    g.cell = g.view.inv_cell > 0.0f ? 1.0 / (double)g.view.inv_cell : 1.0;
    g.cell_start.assign(2, 0);
    g.cell_start[1] = k;
    g.items.resize(k);
    for (uint32_t j = 0; j < k; ++j) g.items[j] = j;
}

// The grid for k <= GPE_COLLIDERS_MAX validated colliders (finite coordinates, finite radius >= 0), the radius bound
// rb = |gpe_max_radius| and the world W x H, all as the context holds them (rb, W and H may be anything).  The
// resolution: cells of max(4 rb, max(W, H) / 1024), doubled until items[] holds at most max_entries entries.
inline ColliderGrid collider_grid_build(const ColliderCapsule *cs, uint32_t k, float rb_in, float W, float H,
                                        uint64_t max_entries = kColliderGridMaxEntries)
{
    ColliderGrid g;
    const float rb = fabsf(rb_in);
    const double w = W, h = H, world = std::max(w, h);
    if (!(w > 0.0 && h > 0.0 && isfinite(world) && isfinite(rb) && world >= 1e-20 && world <= 1e20)) {
        collider_grid_one_cell(g, k, rb, world > 0.0 && isfinite(world) ? world * 2.0 : 0.0);
        return g;
    }
    double want = std::max(4.0 * (double)rb, world / 1024.0);
    for (;; want *= 2.0) {
        // the pass multiplies by a binary32 reciprocal: the cell IS 1 / that number
        const float inv = 1.0f / (float)want;
        const double cell = 1.0 / (double)inv;
        const double nx = floor(w / cell) + 1.0, ny = floor(h / cell) + 1.0;      // W and H lie strictly inside the grid
        if (nx <= 1.0 && ny <= 1.0) break;
        if (nx > (double)kColliderGridMaxDim || ny > (double)kColliderGridMaxDim) continue;
        g.view.inv_cell = inv;
        g.view.gx = (uint32_t)nx; g.view.gy = (uint32_t)ny;
        g.view.gxf = (float)g.view.gx; g.view.gyf = (float)g.view.gy;
        g.view.rb = rb;
        g.cell = cell;
        if (collider_grid_fill(g, cs, k, rb, max_entries)) return g;
    }
    collider_grid_one_cell(g, k, rb, world * 2.0);
    return g;
}

}  // namespace gpe
