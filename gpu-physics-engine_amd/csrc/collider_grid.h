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
#include "lookup_grid.h"

namespace gpe {

constexpr uint64_t kColliderGridMaxEntries = 4ull << 20;       // items[] stays at or under 4 M entries
constexpr double kColliderFarCells = 131072.0;                 // 2^17: past this many cells a collider is listed everywhere

struct ColliderCapsule { float ax, ay, bx, by, radius; };

using ColliderGrid = LookupGrid;

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

// what a collider can reach at one resolution
struct ColliderSpan {
    uint8_t far = 0;                       // listed in every cell
    uint32_t row0 = 1, row1 = 0;           // the rows a near collider can reach (row0 > row1: none)
};

// The grid for k <= GPE_COLLIDERS_MAX validated colliders (finite coordinates, finite radius >= 0), the radius bound
// rb = |gpe_max_radius| and the world W x H, all as the context holds them (rb, W and H may be anything).  The
// resolution: cells of max(4 rb, max(W, H) / 1024), doubled until items[] holds at most max_entries entries
// (lookup_grid.h).
inline ColliderGrid collider_grid_build(const ColliderCapsule *cs, uint32_t k, float rb_in, float W, float H,
                                        uint64_t max_entries = kColliderGridMaxEntries)
{
    const float rbf = fabsf(rb_in);
    const double rb = rbf;
    std::vector<ColliderSpan> span(k);
    uint32_t gx = 1, gy = 1;
    double cell = 1.0, half_diag = 0.0;
    auto prepare = [&](const LookupView &v) {
        gx = v.view.gx; gy = v.view.gy;
        cell = v.cell; half_diag = cell * 0.70710678118654757;
        for (uint32_t j = 0; j < k; ++j) {
            const ColliderCapsule &c = cs[j];
            ColliderSpan &s = span[j] = ColliderSpan();
            const double m = std::max(std::max(fabs((double)c.ax), fabs((double)c.ay)), std::max(fabs((double)c.bx), fabs((double)c.by)));
            if (!(m + c.radius + rb <= kColliderFarCells * cell)) { s.far = 1; continue; }
            const double reach = (double)c.radius + rb + cell + half_diag + 0.01 * cell;
            const double ylo = std::min((double)c.ay, (double)c.by) - reach, yhi = std::max((double)c.ay, (double)c.by) + reach;
            if (yhi < 0.0 || ylo >= (double)gy * cell) continue;
            const double r0 = floor(ylo / cell), r1 = floor(yhi / cell);
            s.row0 = r0 > 0.0 ? (uint32_t)r0 : 0u;
            s.row1 = r1 < (double)(gy - 1) ? (uint32_t)r1 : gy - 1;
        }
    };
    auto cells_of = [&](uint32_t j, auto emit) {
        const ColliderCapsule &c = cs[j];
        const ColliderSpan &s = span[j];
        if (s.far) { emit(0, (uint64_t)gx * gy - 1); return; }
        const double keep = (double)c.radius + rb + cell + half_diag;
        for (uint32_t cy = s.row0; cy <= s.row1 && s.row0 <= s.row1; ++cy) {
            uint32_t x0, x1;
            if (!collider_row_span(c, cell, keep + 0.01 * cell, cy, gx, &x0, &x1)) continue;
            for (uint32_t cx = x0; cx <= x1; ++cx) {
                const double d = collider_point_segment_distance(((double)cx + 0.5) * cell, ((double)cy + 0.5) * cell,
                                                                 c.ax, c.ay, c.bx, c.by);
                if (!(d <= keep)) continue;
                const uint64_t cell_i = (uint64_t)cy * gx + cx;
                if (!emit(cell_i, cell_i)) return;
            }
        }
    };
    return lookup_grid_build(k, rbf, W, H, kColliderGridMaxDim, 1e-20, max_entries, prepare, cells_of);
}

}  // namespace gpe
