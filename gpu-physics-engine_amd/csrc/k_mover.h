// k_mover.h -- the one definition of how a moving collider moves (a mover: a capsule at rest plus a motion), and of
// the cells a posed mover is listed in: what the device (k_movers.hip), the host (gpe_movers.hip, mover_grid.h) and the
// CPU test program (tests/cpp/mover_grid_tests.cpp) share.  No HIP header: plain g++ compiles it (with
// -ffp-contract=off).
//
// The arithmetic rules are k_collider.h's: IEEE binary32, one rounding per operation, left to right, no FMA; `/` and
// sqrtf correctly rounded; no libm sin / cos anywhere (device, host and numpy do not agree on those): a rotation is
// composed from a polynomial.  numpy float32 reproduces every function here bit for bit (tests/_movers_model.py).
//
// The posed capsule pushes particles exactly as a static collider does (collider_touch, collider_normal, collider_key:
// the deepest mover only, judged from the position the pass starts with).  The pass writes pos only, which in a Verlet
// engine hands the particle the wall's velocity.  This plain pass has no swept test: a mover must be thicker than one
// step's relative displacement of mover and particle, or particles are tunnelled through -- hosts make movers thick, or
// switch the movers' sweep on (gpe_set_mover_sweep; k_mover_sweep.h: the particle's path relative to each mover).
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_collider.h"

namespace gpe {

constexpr uint32_t kMoverLinear = 0, kMoverRotate = 1;         // GPE_MOVER_LINEAR, GPE_MOVER_ROTATE
constexpr float kMoverMaxTurn = 0.5f;                          // the polynomial's range: |omega * dt| <= 0.5

// A mover as the device holds it (3 float4): the capsule at rest, and the motion with what the host derived at set time
struct MoverDef {
    float ax, ay, bx, by;        // the capsule at rest
    float radius;
    uint32_t kind;
    float travel;                // LINEAR: > 0: back and forth over this distance; 0: for ever
    float rate;                  // LINEAR: speed = sqrtf(vx*vx + vy*vy); ROTATE: omega
    float ux, uy;                // LINEAR: v / speed ((0, 0) when speed == 0); ROTATE: the pivot
    float pad0, pad1;            // pad0: mover_arm (k_mover_sweep.h), read by the swept form alone; pad1: 0
};

// The dt contract's side of a set: the largest |omega|, and among the LINEAR movers that go back and forth (travel > 0;
// bounded = false: there is none) the largest speed and the smallest travel.
struct MoverLimits {
    float max_omega = 0.f, max_speed = 0.f, min_travel = 0.f;
    bool bounded = false;
};

// speed and direction of a LINEAR mover's velocity, at set time
GPE_COLLIDER_FN void mover_direction(float vx, float vy, float *speed, float *ux, float *uy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float xx = vx * vx;
    const float yy = vy * vy;
    const float h = xx + yy;
    const float sp = sqrtf(h);
    *speed = sp;
    if (sp > 0.0f) {
        *ux = vx / sp;
        *uy = vy / sp;
    } else {
        *ux = 0.0f;
        *uy = 0.0f;
    }
}

// One step of the motion: the state (q0, q1) after dt.  LINEAR: (g, sgn), the progress along u and which way it is
// going; ROTATE: (c, s), the unit vector of the orientation.  Contract (the host checks it): |omega * dt| <= 0.5, and
// speed * |dt| <= travel when travel > 0, so that one reflection suffices.  A ROTATE mover with omega * dt == 0 keeps
// its state bit for bit (the renormalisation below need not be idempotent).
GPE_COLLIDER_FN void mover_advance(const MoverDef &m, float dt, float *q0, float *q1)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (m.kind == kMoverLinear) {
        const float g = *q0;
        float sgn = *q1;
        const float d = m.rate * dt;
        const float sd = sgn * d;
        float g1 = g + sd;
        if (m.travel > 0.0f) {
            if (g1 > m.travel) {
                const float over = g1 - m.travel;
                g1 = m.travel - over;
                sgn = -sgn;
            } else if (g1 < 0.0f) {
                g1 = -g1;
                sgn = -sgn;
            }
            g1 = (g1 < 0.0f) ? 0.0f : g1;
            g1 = (g1 > m.travel) ? m.travel : g1;
        }
        *q0 = g1;
        *q1 = sgn;
        return;
    }
    const float x = m.rate * dt;
    if (x == 0.0f) return;
    const float c = *q0, s = *q1;
    const float x2 = x * x;
    const float S0 = -0x1.555556p-3f, S1 = 0x1.111112p-7f, S2 = -0x1.a01a02p-13f, S3 = 0x1.71de3ap-19f;
    const float C0 = -0.5f, C1 = 0x1.555556p-5f, C2 = -0x1.6c16c2p-10f, C3 = 0x1.a01a02p-16f, C4 = -0x1.27e4fcp-22f;
    // Horner, innermost first: every line is one product and one sum
    float ps = x2 * S3;
    ps = S2 + ps;
    ps = x2 * ps;
    ps = S1 + ps;
    ps = x2 * ps;
    ps = S0 + ps;
    ps = x2 * ps;
    ps = x * ps;
    const float sa = x + ps;
    float pc = x2 * C4;
    pc = C3 + pc;
    pc = x2 * pc;
    pc = C2 + pc;
    pc = x2 * pc;
    pc = C1 + pc;
    pc = x2 * pc;
    pc = C0 + pc;
    pc = x2 * pc;
    const float ca = 1.0f + pc;
    const float cc = c * ca;
    const float ss = s * sa;
    const float c2 = cc - ss;
    const float sc = s * ca;
    const float cs = c * sa;
    const float s2 = sc + cs;
    const float c22 = c2 * c2;
    const float s22 = s2 * s2;
    const float mm = c22 + s22;
    const float mag = sqrtf(mm);
    *q0 = c2 / mag;
    *q1 = s2 / mag;
}

// The posed capsule of the state (q0, q1): out = (ax, ay, bx, by)
GPE_COLLIDER_FN void mover_pose(const MoverDef &m, float q0, float q1, float *out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (m.kind == kMoverLinear) {
        const float ox = q0 * m.ux;
        const float oy = q0 * m.uy;
        out[0] = m.ax + ox;
        out[1] = m.ay + oy;
        out[2] = m.bx + ox;
        out[3] = m.by + oy;
        return;
    }
    const float rest[4] = {m.ax, m.ay, m.bx, m.by};
    for (int e = 0; e < 2; ++e) {
        const float rx = rest[2 * e] - m.ux;
        const float ry = rest[2 * e + 1] - m.uy;
        const float xc = rx * q0;
        const float ys = ry * q1;
        const float tx = xc - ys;
        const float xs = rx * q1;
        const float yc = ry * q0;
        const float ty = xs + yc;
        out[2 * e] = m.ux + tx;
        out[2 * e + 1] = m.uy + ty;
    }
}

// ---- the lookup grid: a bit mask of the movers per cell -------------------------------------------------------------
// gx x gy <= 128 x 128 cells of `cell` = 1 / (double)view.inv_cell world units; `words` 64-bit words per cell, bit
// j % 64 of word j / 64 is mover j; one summary word per cell, bit w set when mask word w is not zero.  The device builds
// it every step from the posed capsules (k_movers_build), the test program builds the same masks on the CPU.
//
// Completeness is collider_grid.h's argument word for word: a mover is listed in a cell when the distance (in double)
// from its posed segment to the cell's centre is at most R + rb + cell + half the cell's diagonal; a mover of magnitude
// beyond 2^17 cells, or with a coordinate that is not finite, is listed in every cell; the grid of one cell lists
// every mover.  No result of the pass depends on the grid.
constexpr uint32_t kMoverGridMaxDim = 128;
constexpr uint32_t kMoversMax = 1024;                          // GPE_MOVERS_MAX
constexpr double kMoverFarCells = 131072.0;                    // 2^17

struct MoverGridView {
    ColliderGridView view;       // collider_cell_of names a particle's cell
    double cell = 1.0;           // 1 / (double)view.inv_cell (one cell: unused)
};

GPE_COLLIDER_FN double mover_segment_distance(double px, double py, double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay, fx = px - ax, fy = py - ay;
    const double A = dx * dx + dy * dy;
    double u = A > 0.0 ? (fx * dx + fy * dy) / A : 0.0;
    u = u > 0.0 ? u : 0.0;
    u = u < 1.0 ? u : 1.0;
    const double qx = fx - u * dx, qy = fy - u * dy;
    return sqrt(qx * qx + qy * qy);
}

GPE_COLLIDER_FN double mover_max_nan(double a, double b) { return (a > b || a != a) ? a : b; }   // a NaN wins

// The cells the posed capsule cap = (ax, ay, bx, by), R can be listed in: the rectangle [x0, x1] x [y0, y1] of its
// inflated bounding box, cut to the grid.  false: none.  *everywhere: listed in every cell without a distance test
// (far, not finite, or the grid of one cell); the rectangle is then the whole grid.
GPE_COLLIDER_FN bool mover_cell_rect(const MoverGridView &g, const float *cap, float R, float rb, uint32_t *x0, uint32_t *y0,
                                     uint32_t *x1, uint32_t *y1, bool *everywhere)
{
    const uint32_t gx = g.view.gx, gy = g.view.gy;
    const double cell = g.cell;
    const double ax = cap[0], ay = cap[1], bx = cap[2], by = cap[3];
    const double m = mover_max_nan(mover_max_nan(fabs(ax), fabs(ay)), mover_max_nan(fabs(bx), fabs(by)));
    *x0 = 0; *y0 = 0; *x1 = gx - 1; *y1 = gy - 1;
    *everywhere = (gx == 1 && gy == 1) || !(m + (double)R + (double)rb <= kMoverFarCells * cell);
    if (*everywhere) return true;
    const double reach = (double)R + (double)rb + cell + cell * 0.70710678118654757 + 0.01 * cell;
    const double xlo = fmin(ax, bx) - reach, xhi = fmax(ax, bx) + reach;
    const double ylo = fmin(ay, by) - reach, yhi = fmax(ay, by) + reach;
    if (xhi < 0.0 || yhi < 0.0 || xlo >= (double)gx * cell || ylo >= (double)gy * cell) return false;
    const double c0 = floor(xlo / cell), c1 = floor(xhi / cell), r0 = floor(ylo / cell), r1 = floor(yhi / cell);
    *x0 = c0 > 0.0 ? (uint32_t)c0 : 0u;
    *x1 = c1 < (double)(gx - 1) ? (uint32_t)c1 : gx - 1;
    *y0 = r0 > 0.0 ? (uint32_t)r0 : 0u;
    *y1 = r1 < (double)(gy - 1) ? (uint32_t)r1 : gy - 1;
    return *x0 <= *x1 && *y0 <= *y1;
}

// Is the posed capsule listed in cell (cx, cy) of its rectangle?  (The rule of collider_grid_fill.)
GPE_COLLIDER_FN bool mover_listed(const MoverGridView &g, const float *cap, float R, float rb, uint32_t cx, uint32_t cy)
{
    const double cell = g.cell;
    const double keep = (double)R + (double)rb + cell + cell * 0.70710678118654757;
    const double d = mover_segment_distance(((double)cx + 0.5) * cell, ((double)cy + 0.5) * cell, cap[0], cap[1], cap[2], cap[3]);
    return d <= keep;
}

}  // namespace gpe
