// k_mover_sweep.h -- the one definition of the swept form of the movers' pass (gpe_set_mover_sweep): a particle is judged
// by its path RELATIVE TO EACH MOVER over this step, not by pos against the new pose alone, so a thin piston or blade no
// longer jumps across the particles it should push.  What the build and the pass (k_mover_sweep.hip), the host
// (gpe_movers.hip, mover_grid.h), the CPU test program (tests/cpp/mover_sweep_tests.cpp) and the docs share.  No HIP
// header: plain g++ compiles it (with -ffp-contract=off).
//
// The arithmetic rules are k_collider.h's: IEEE binary32, one rounding per operation, left to right, no FMA; `/` and
// sqrtf correctly rounded; no libm trigonometry.  numpy float32 reproduces every function here bit for bit
// (tests/_mover_sweep_model.py).
//
// The rule, for a particle (p, prev, r) and the movers j with their capsules C0_j (posed from the state before
// mover_advance) and C1_j (after it), radius R_j:
//   1. CARRY.  y0_j = M_j(prev): prev moved rigidly with mover j over this step (mover_carry_of writes one record per
//      mover, mover_carry applies it).  LINEAR: y0 = prev + (a1 - a0), component-wise from the posed capsules; ROTATE:
//      cd = c1*c0 + s1*s0, sd = s1*c0 - c1*s0 from the orientation states, y0 = pivot + Rot(cd, sd)(prev - pivot) in
//      mover_pose's order.  A mover whose state did not change (LINEAR with a1 == a0, ROTATE with omega*dt == 0) is
//      STILL: y0 = prev bit for bit.  The relative path of the particle is taken as the chord y0_j -> p.
//   2. PLAIN.  If p - y0_j is not finite, or exactly zero in both components, mover j judges the particle by the plain
//      touch at p (collider_touch against C1_j): a contact with t = 1, the touch's normal and depth.  A particle at
//      rest under a mover at rest gets the plain pass's contact; a particle at rest under a MOVING mover is swept.
//   3. GATE (a turning ROTATE mover only).  Mover j is considered only if the WORLD path prev -> p comes within
//      rho_j = (arm_j + R_j) + |r| of the pivot: sweep_measure with the pivot as the point, prev -> p as the capsule and
//      arm_j + R_j as its radius says "touched".  arm_j = max(|a - pivot|, |b - pivot|) of the rest capsule (mover_arm,
//      at set time).  The chord is exact at both ends and off by up to |omega dt| * |m| / 4 between them: for a particle
//      that flies in from afar it can cut through the disc its true path never enters, and the blade never leaves it.
//   4. CONTACT.  sweep_contact(y0_j, p, r, C1_j, R_j), unchanged: normal and depth are in the world frame at the end of
//      the step.
//   5. WINNER.  sweep_better: the least t, then the greatest depth, then the lowest j; a plain touch takes part with
//      t = 1.  A total order: judging a mover twice changes nothing.
//   6. RESPONSE.  Without a surface, on a row flagged GPE_SURFACE_PLAIN, or when p - prev is not finite:
//      q = sweep_push(p, n, depth).  With one: u re-measured at the contact point (the same bits),
//      w = surface_wall_move(C0, C1, u), surface_apply(p, prev, r, n, depth, w, e, mu) -> q, prev'.
//   7. ONE VERIFICATION.  If any mover j has a contact (steps 1 to 4 with q in the place of p) deeper than
//      2^-10 * s_j (sweep_over_slop), the particle stops at its first contact instead: pos = sweep_stop(winner), prev
//      untouched, no surface.  Otherwise pos = q, and prev = prev' where a surface acted.
//
// WHAT IS GUARANTEED.  A particle that starts the step on one side of a blade RELATIVE TO THE BLADE (y0_j on that side of
// C1_j), and whose chord y0_j -> p crosses the blade's stretch, does not end on the other side.  WHAT IS NOT.  The chord
// error of step 3 applies to particles that are fast themselves (|m| large): the rule sweeps the chord, not the curved
// relative path.  The collision solver's own pushes are not swept (prev is the position after the step's collision
// response).  A particle that starts inside the capsule is pushed as by the plain pass.  Two movers closing on one
// particle are resolved by the first contact plus the one verification: the rule goes no further, a squeezed particle
// stops at its first contact.
//
// THE LOOKUP (mover_sweep_cell_rect, mover_sweep_listed; no result depends on it).  A mover is listed in every cell its
// MOTION can reach: LINEAR: the cells within `keep` (k_mover.h) of the parallelogram hull(C0, C1) -- the cell's centre
// inside it, or within keep of one of its four edges, in double; ROTATE: within keep of the disc of radius arm about the
// pivot.  A particle's candidates are the OR of the masks over sweep_box(prev, p).  Completeness: w(t) = prev + t m lies
// in the box.  LINEAR: the contact point on the chord is w(t) + (1 - t) D, so w(t) is within s + slack of C1 translated
// back by (1 - t) D, which lies inside the hull.  ROTATE: the gate puts a point of the world path within rho_j of the
// pivot: within R + |r| of the disc; a plain touch at p lies within s of C1, inside the disc.  The half-cell border rule
// and the slack bound are k_sweep.h's.
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_mover.h"
#include "k_sweep.h"

namespace gpe {

constexpr uint32_t kCarryStill = 0, kCarryShift = 1, kCarryTurn = 2;

// What one mover carries a point by in this step (2 float4 on the device)
struct alignas(16) MoverCarry {
    uint32_t kind;              // kCarry*
    float cx, cy;                // SHIFT: a1 - a0;  TURN: (cd, sd)
    float px, py;                // TURN: the pivot
    float arm;                   // TURN: the farthest end point of the rest capsule from the pivot
    float pad0, pad1;
};

// max(|a - pivot|, |b - pivot|) of a ROTATE mover's rest capsule (MoverDef::pad0, at set time); a LINEAR mover: 0
GPE_COLLIDER_FN float mover_arm(const MoverDef &m)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (m.kind != kMoverRotate) return 0.0f;
    const float ex = m.ax - m.ux;
    const float ey = m.ay - m.uy;
    const float exx = ex * ex;
    const float eyy = ey * ey;
    const float eh = exx + eyy;
    const float ea = sqrtf(eh);
    const float fx = m.bx - m.ux;
    const float fy = m.by - m.uy;
    const float fxx = fx * fx;
    const float fyy = fy * fy;
    const float fh = fxx + fyy;
    const float fa = sqrtf(fh);
    return (fa > ea) ? fa : ea;
}

// The carry record of mover m for the step dt that took its state from (p0, p1) to (q0, q1) and its posed capsule from
// c0 to c1 (4 floats each); arm = mover_arm(m)
GPE_COLLIDER_FN void mover_carry_of(const MoverDef &m, float dt, float p0, float p1, float q0, float q1, const float *c0,
                                    const float *c1, float arm, MoverCarry *k)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    k->kind = kCarryStill;
    k->cx = 0.0f; k->cy = 0.0f; k->px = 0.0f; k->py = 0.0f; k->arm = 0.0f; k->pad0 = 0.0f; k->pad1 = 0.0f;
    if (m.kind == kMoverLinear) {
        if (c1[0] == c0[0] && c1[1] == c0[1]) return;
        k->kind = kCarryShift;
        k->cx = c1[0] - c0[0];
        k->cy = c1[1] - c0[1];
        return;
    }
    const float x = m.rate * dt;
    if (x == 0.0f) return;                                     // (mover_advance kept the state bit for bit)
    const float cc = q0 * p0;
    const float ss = q1 * p1;
    const float sc = q1 * p0;
    const float cs = q0 * p1;
    k->kind = kCarryTurn;
    k->cx = cc + ss;
    k->cy = sc - cs;
    k->px = m.ux; k->py = m.uy;
    k->arm = arm;
}

// Step 1: y0 = M(prev)
GPE_COLLIDER_FN void mover_carry(const MoverCarry &k, float prevx, float prevy, float *yx, float *yy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (k.kind == kCarryShift) {
        *yx = prevx + k.cx;
        *yy = prevy + k.cy;
        return;
    }
    if (k.kind == kCarryTurn) {
        const float rx = prevx - k.px;
        const float ry = prevy - k.py;
        const float xc = rx * k.cx;
        const float ys = ry * k.cy;
        const float tx = xc - ys;
        const float xs = rx * k.cy;
        const float yc = ry * k.cx;
        const float ty = xs + yc;
        *yx = k.px + tx;
        *yy = k.py + ty;
        return;
    }
    *yx = prevx;
    *yy = prevy;
}

// Step 3: does the world path prev -> p come within (arm + R) + |r| of the pivot?
GPE_COLLIDER_FN bool mover_sweep_gate(const MoverCarry &k, float R, float px, float py, float prevx, float prevy, float r)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float reach = k.arm + R;
    ColliderTouch T;
    float s;
    return sweep_measure(k.px, k.py, r, prevx, prevy, px, py, reach, &T, &s);
}

// Steps 1 to 4: the contact of one mover (its carry record, its new capsule cap = (ax, ay, bx, by), R) on the particle
// that ends at p.  false: none.
GPE_COLLIDER_FN bool mover_sweep_judge(const MoverCarry &k, const float *cap, float R, float px, float py, float prevx,
                                       float prevy, float r, SweepContact *c)
{
    float yx, yy;
    mover_carry(k, prevx, prevy, &yx, &yy);
    if (sweep_plain_particle(px, py, yx, yy)) {
        ColliderTouch T;
        float s;
        if (!sweep_measure(px, py, r, cap[0], cap[1], cap[2], cap[3], R, &T, &s)) return false;
        float nx, ny;
        collider_normal(T, &nx, &ny);
        c->t = 1.0f; c->depth = T.depth;
        c->x = px; c->y = py;
        c->nx = nx; c->ny = ny;
        c->gap = T.depth;
        c->s = s;
        return true;
    }
    if (k.kind == kCarryTurn && !mover_sweep_gate(k, R, px, py, prevx, prevy, r)) return false;
    return sweep_contact(yx, yy, px, py, r, cap[0], cap[1], cap[2], cap[3], R, c);
}

// Step 6: the winner's response -> res = (q, prev').  surf: its row (null: none); old: C0, cap: C1
GPE_COLLIDER_FN void mover_sweep_respond(const SweepContact &win, const float *old, const float *cap, float R,
                                         const SurfaceRow *surf, float px, float py, float prevx, float prevy, float r,
                                         float W, float H, float *res)
{
    res[2] = prevx; res[3] = prevy;
    if (surf && !(surf->flags & kSurfacePlain) && surface_velocity_finite(px, py, prevx, prevy)) {
        ColliderTouch T;
        float s, wx, wy;
        (void)sweep_measure(win.x, win.y, r, cap[0], cap[1], cap[2], cap[3], R, &T, &s);   // the contact point again: the same u
        surface_wall_move(old, cap, T.u, &wx, &wy);
        surface_apply(px, py, prevx, prevy, r, win.nx, win.ny, win.depth, wx, wy, surf->e, surf->mu, W, H, res);
        return;
    }
    sweep_push(px, py, r, win, W, H, &res[0], &res[1]);
}

// ---- the lookup: the cells a mover's motion can reach ------------------------------------------------------------------
GPE_COLLIDER_FN double mover_sweep_cross(double ox, double oy, double ax, double ay, double bx, double by)
{
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

// mover_cell_rect for the motion: the inflated bounding box of hull(c0, c1), or of the disc (arm about the pivot) for a
// ROTATE mover; *everywhere as there, judged over both capsules, the pivot and the arm
GPE_COLLIDER_FN bool mover_sweep_cell_rect(const MoverGridView &g, const MoverDef &m, float arm, const float *c0,
                                           const float *c1, float rb, uint32_t *x0, uint32_t *y0, uint32_t *x1,
                                           uint32_t *y1, bool *everywhere)
{
    const uint32_t gx = g.view.gx, gy = g.view.gy;
    const double cell = g.cell;
    double mag = 0.0;
    for (int e = 0; e < 4; ++e) mag = mover_max_nan(mover_max_nan(fabs((double)c0[e]), fabs((double)c1[e])), mag);
    double xlo, xhi, ylo, yhi;
    if (m.kind == kMoverRotate) {
        mag = mover_max_nan(mover_max_nan(fabs((double)m.ux), fabs((double)m.uy)) + (double)arm, mag);
        xlo = (double)m.ux - (double)arm; xhi = (double)m.ux + (double)arm;
        ylo = (double)m.uy - (double)arm; yhi = (double)m.uy + (double)arm;
    } else {
        xlo = fmin(fmin(c0[0], c0[2]), fmin(c1[0], c1[2])); xhi = fmax(fmax(c0[0], c0[2]), fmax(c1[0], c1[2]));
        ylo = fmin(fmin(c0[1], c0[3]), fmin(c1[1], c1[3])); yhi = fmax(fmax(c0[1], c0[3]), fmax(c1[1], c1[3]));
    }
    *x0 = 0; *y0 = 0; *x1 = gx - 1; *y1 = gy - 1;
    *everywhere = (gx == 1 && gy == 1) || !(mag + (double)m.radius + (double)rb <= kMoverFarCells * cell);
    if (*everywhere) return true;
    const double reach = (double)m.radius + (double)rb + cell + cell * 0.70710678118654757 + 0.01 * cell;
    xlo -= reach; xhi += reach; ylo -= reach; yhi += reach;
    if (xhi < 0.0 || yhi < 0.0 || xlo >= (double)gx * cell || ylo >= (double)gy * cell) return false;
    const double a0 = floor(xlo / cell), a1 = floor(xhi / cell), r0 = floor(ylo / cell), r1 = floor(yhi / cell);
    *x0 = a0 > 0.0 ? (uint32_t)a0 : 0u;
    *x1 = a1 < (double)(gx - 1) ? (uint32_t)a1 : gx - 1;
    *y0 = r0 > 0.0 ? (uint32_t)r0 : 0u;
    *y1 = r1 < (double)(gy - 1) ? (uint32_t)r1 : gy - 1;
    return *x0 <= *x1 && *y0 <= *y1;
}

// Is the mover's motion listed in cell (cx, cy) of its rectangle?
GPE_COLLIDER_FN bool mover_sweep_listed(const MoverGridView &g, const MoverDef &m, float arm, const float *c0,
                                        const float *c1, float rb, uint32_t cx, uint32_t cy)
{
    const double cell = g.cell;
    const double keep = (double)m.radius + (double)rb + cell + cell * 0.70710678118654757;
    const double x = ((double)cx + 0.5) * cell, y = ((double)cy + 0.5) * cell;
    if (m.kind == kMoverRotate) {
        const double dx = x - (double)m.ux, dy = y - (double)m.uy;
        return sqrt(dx * dx + dy * dy) - (double)arm <= keep;
    }
    // the parallelogram a0 -> b0 -> b1 -> a1: strictly inside (all four turns the same way), or near an edge
    const double qx[4] = {c0[0], c0[2], c1[2], c1[0]}, qy[4] = {c0[1], c0[3], c1[3], c1[1]};
    int pos = 0, neg = 0;
    double d = 1.7976931348623157e308;
    for (int e = 0; e < 4; ++e) {
        const int f = (e + 1) & 3;
        const double t = mover_sweep_cross(qx[e], qy[e], qx[f], qy[f], x, y);
        pos += t > 0.0;
        neg += t < 0.0;
        d = fmin(d, mover_segment_distance(x, y, qx[e], qy[e], qx[f], qy[f]));
    }
    return pos == 4 || neg == 4 || d <= keep;
}

}  // namespace gpe
