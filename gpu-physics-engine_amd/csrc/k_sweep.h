// k_sweep.h -- the one definition of the swept form of the static colliders' pass (gpe_set_collider_sweep): a particle is
// judged by the path prev -> pos of this step, not by pos alone, so a wall thinner than the step's displacement is no
// longer tunnelled through.  What the pass (k_sweep.hip), the CPU test program (tests/cpp/sweep_tests.cpp) and the docs
// share.  No HIP header: plain g++ compiles it (with -ffp-contract=off).
//
// The arithmetic rules are k_collider.h's: IEEE binary32, one rounding per operation, left to right, no FMA; `/` and
// sqrtf correctly rounded.  numpy float32 reproduces every function here bit for bit (tests/_sweep_model.py).
//
// The rule, for a particle (p, prev, r) with m = p - prev:
//   1. m not finite, or exactly zero in both components: the plain rule of k_collider.h / k_surface.h on p.
//   2. every collider j gives at most one contact on prev -> p (sweep_contact): where the path first meets the capsule
//      inflated by s_j = R_j + |r|, with depth_j = (s_j - d_j) + n_j . (x_j - p) > 0.
//   3. the least t_j wins, then the greatest depth_j, then the lowest j (sweep_better).
//   4. q = clamp(p + n * depth) (sweep_push), or surface_apply(p, prev, r, n, depth, 0, 0, e, mu, W, H) -> q, prev'.
//   5. if any collider has a contact on prev -> q deeper than 2^-10 * s_j (sweep_over_slop), the particle stops at its
//      first contact instead: pos = clamp(x_1 + n_1 * max(s_1 - d_1, 0)) (sweep_stop), prev untouched, no surface.
//      Otherwise pos = q, and prev = prev' where a surface acted.
// So a particle ends at a point whose path from prev enters nothing deeper than the slop, or at the first point where it
// touched anything.  What is not swept: the movers, and the collision solver's own pushes (prev is the position after
// the step's collision response); a particle that starts on the wrong side of a wall stays there.
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_collider.h"
#include "k_surface.h"

namespace gpe {

constexpr float kSweepSlop = 0.0009765625f;                    // 2^-10: step 5's bound, as a share of s_j
constexpr float kSweepSlack = 1.9073486328125e-06f;            // 2^-19: sweep_contact's bound on d_j - s_j, see there
constexpr uint32_t kSweepBoxCells = 16;                        // a path's lookup box spans at most 16 x 16 cells

// collider_touch without its early return: *t is always filled (depth = s - d may be negative or NaN).  The same
// operations in the same order, so `true` here is `true` there with the same bits.  *s_out = R + |r|.
GPE_COLLIDER_FN bool sweep_measure(float px, float py, float r, float ax, float ay, float bx, float by, float R,
                                   ColliderTouch *t, float *s_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = fabsf(r);
    const float dx = bx - ax;
    const float dy = by - ay;
    const float fx = px - ax;
    const float fy = py - ay;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    const float A = dxx + dyy;
    float u = 0.0f;
    if (A > 0.0f) {
        const float ex = fx * dx;
        const float ey = fy * dy;
        const float B = ex + ey;
        u = B / A;
    }
    u = (u > 0.0f) ? u : 0.0f;                                 // NaN -> 0
    u = (u < 1.0f) ? u : 1.0f;
    const float ux = u * dx;
    const float uy = u * dy;
    const float qx = fx - ux;
    const float qy = fy - uy;
    const float qxx = qx * qx;
    const float qyy = qy * qy;
    const float h = qxx + qyy;
    const float s = R + a;
    const float ss = s * s;
    const float d = sqrtf(h);
    t->depth = s - d;
    t->qx = qx; t->qy = qy; t->d = d;
    t->dx = dx; t->dy = dy; t->A = A;
    t->u = u;
    *s_out = s;
    return h < ss;
}

// Is the particle outside the sweep (step 1)?
GPE_COLLIDER_FN bool sweep_plain_particle(float px, float py, float prevx, float prevy)
{
    if (!surface_velocity_finite(px, py, prevx, prevy)) return true;
    const float mx = px - prevx;
    const float my = py - prevy;
    return mx == 0.0f && my == 0.0f;
}

struct SweepContact {
    float t;                     // where on the path: 0 at x0, 1 at x1
    float depth;                 // (s - d) + n . (x - x1): how far x1 is pushed along n.  > 0
    float x, y;                  // the contact point x0 + t (x1 - x0)
    float nx, ny;                // collider_normal at the contact point
    float gap;                   // s - d at the contact point
    float s;                     // R + |r|
};

// The earliest t >= 0 at which x0 + t m, approaching, is at distance s of the point c (f = x0 - c), or -1.  A start on
// or inside the circle counts as t = 0: a particle resting at distance s as the last pass left it has its entry there.
GPE_COLLIDER_FN float sweep_disc_root(float fx, float fy, float mx, float my, float s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float bxx = fx * mx;
    const float byy = fy * my;
    const float bq = bxx + byy;
    if (!(bq < 0.0f)) return -1.0f;                            // not approaching (or a NaN)
    const float fxx = fx * fx;
    const float fyy = fy * fy;
    const float ff = fxx + fyy;
    const float ss = s * s;
    const float cq = ff - ss;
    if (!(cq > 0.0f)) return (cq <= 0.0f) ? 0.0f : -1.0f;
    const float mxx = mx * mx;
    const float myy = my * my;
    const float am = mxx + myy;
    const float bb = bq * bq;
    const float ac = am * cq;
    const float disc = bb - ac;
    if (!(disc >= 0.0f)) return -1.0f;
    const float sq = sqrtf(disc);
    const float den = sq - bq;                                 // > 0: both terms are
    return cq / den;                                           // the smaller root, without cancellation
}

// The contact of one collider (a -> b, R) on the path x0 -> x1 of a particle of stored radius r.  false: none.
//   x0 touched (collider_touch):           t = 0.
//   else the least accepted candidate of:  the band's side (|cross(b - a, x - a)| = s |b - a|, approaching), the disc
//                                          about a, the disc about b (sweep_disc_root), tried in that order, each in
//                                          [0, 1]; a later one replaces an earlier one only when strictly smaller.
//                                          A candidate is accepted when the capsule's distance at x = x0 + t m obeys
//                                              d <= s + 2^-19 (|x0x| + |x0y| + |x1x| + |x1y|)
//                                          (32 ulps of the path's coordinates: what the rounding of t, x and d can
//                                          amount to, and no more -- a looser test would take a point beside the
//                                          capsule's end for a contact); it also keeps a band root to the segment's
//                                          own stretch.
//   else x1 touched:                       t = 1 (a grazing root lost to rounding never leaves a particle touching).
//   depth = (s - d) + n . (x - x1) must be > 0: a path that leaves the capsule it started in has no contact.
// THE SLACK.  At an accepted contact point d_j <= s_j + 2^-19 * (|x0x| + |x0y| + |x1x| + |x1y|).  For a path whose end
// points lie in the lookup grid (coordinates below 1025 cells) that is at most s_j + 0.008 cells: with the quarter cell
// collider_grid.h grants the rounding of d itself, well inside the whole cell its lists are inflated by.
GPE_COLLIDER_FN bool sweep_contact(float x0x, float x0y, float x1x, float x1y, float r, float ax, float ay, float bx,
                                   float by, float R, SweepContact *c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    ColliderTouch T;
    float s;
    float t = 0.0f, X = x0x, Y = x0y;
    if (!sweep_measure(x0x, x0y, r, ax, ay, bx, by, R, &T, &s)) {
        const float mx = x1x - x0x;
        const float my = x1y - x0y;
        const float e0 = fabsf(x0x);
        const float e1 = fabsf(x0y);
        const float e2 = fabsf(x1x);
        const float e3 = fabsf(x1y);
        const float e01 = e0 + e1;
        const float e012 = e01 + e2;
        const float ext = e012 + e3;
        const float slack = kSweepSlack * ext;
        const float lim = s + slack;
        float cand[3] = {-1.0f, -1.0f, -1.0f};
        const float fx = x0x - ax;
        const float fy = x0y - ay;
        if (T.A > 0.0f) {
            const float L = sqrtf(T.A);
            const float sL = s * L;
            const float c0a = T.dx * fy;
            const float c0b = T.dy * fx;
            const float c0 = c0a - c0b;
            const float cma = T.dx * my;
            const float cmb = T.dy * mx;
            const float cm = cma - cmb;
            const float den = (c0 >= 0.0f) ? -cm : cm;
            if (den > 0.0f) {
                const float ac = fabsf(c0);
                const float over = ac - sL;
                const float num = (over > 0.0f) ? over : 0.0f;
                cand[0] = num / den;
            }
            const float gx = x0x - bx;
            const float gy = x0y - by;
            cand[2] = sweep_disc_root(gx, gy, mx, my, s);
        }
        cand[1] = sweep_disc_root(fx, fy, mx, my, s);
        bool have = false;
        for (int k = 0; k < 3; ++k) {
            const float tk = cand[k];
            if (!(tk >= 0.0f && tk <= 1.0f)) continue;
            if (have && !(tk < t)) continue;
            const float sx = tk * mx;
            const float sy = tk * my;
            const float xk = x0x + sx;
            const float yk = x0y + sy;
            ColliderTouch Tk;
            float sk;
            (void)sweep_measure(xk, yk, r, ax, ay, bx, by, R, &Tk, &sk);
            if (!(Tk.d <= lim)) continue;
            have = true;
            t = tk; X = xk; Y = yk; T = Tk;
        }
        if (!have) {
            if (!sweep_measure(x1x, x1y, r, ax, ay, bx, by, R, &T, &s)) return false;
            t = 1.0f; X = x1x; Y = x1y;
        }
    }
    float nx, ny;
    collider_normal(T, &nx, &ny);
    const float ex = X - x1x;
    const float ey = Y - x1y;
    const float px = nx * ex;
    const float py = ny * ey;
    const float along = px + py;
    const float depth = T.depth + along;
    if (!(depth > 0.0f)) return false;
    c->t = t; c->depth = depth;
    c->x = X; c->y = Y;
    c->nx = nx; c->ny = ny;
    c->gap = T.depth;
    c->s = s;
    return true;
}

// Does contact a of collider ja beat contact b of collider jb?  The least t, then the greatest depth, then the lowest
// index: a total order, so judging a collider twice changes nothing.
GPE_COLLIDER_FN bool sweep_better(const SweepContact &a, uint32_t ja, const SweepContact &b, uint32_t jb)
{
    if (a.t != b.t) return a.t < b.t;
    if (a.depth != b.depth) return a.depth > b.depth;
    return ja < jb;
}

// Step 5's question of one contact on prev -> q
GPE_COLLIDER_FN bool sweep_over_slop(const SweepContact &c)
{
    const float slop = kSweepSlop * c.s;
    return c.depth > slop;
}

// Step 4 without a surface: the plain pass's push and clamp, from the winner's normal and depth
GPE_COLLIDER_FN void sweep_push(float px, float py, float r, const SweepContact &c, float W, float H, float *ox, float *oy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float mx = c.nx * c.depth;
    const float my = c.ny * c.depth;
    const float qx = px + mx;
    const float qy = py + my;
    const float hix = W - r;
    const float hiy = H - r;
    *ox = surface_clamp(qx, r, hix);
    *oy = surface_clamp(qy, r, hiy);
}

// Step 5's fall-back: the first contact point, pushed out of what it touches there
GPE_COLLIDER_FN void sweep_stop(float r, const SweepContact &c, float W, float H, float *ox, float *oy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float g = (c.gap > 0.0f) ? c.gap : 0.0f;
    const float mx = c.nx * g;
    const float my = c.ny * g;
    const float qx = c.x + mx;
    const float qy = c.y + my;
    const float hix = W - r;
    const float hiy = H - r;
    *ox = surface_clamp(qx, r, hix);
    *oy = surface_clamp(qy, r, hiy);
}

// One axis of sweep_box: the cell of the coordinate t (in cells), or false.  A point up to half a cell outside the grid
// is filed under the border cell: a collider within s + slack of it lies within that plus half a cell of the border
// cell, inside the whole cell the lists are inflated by (a particle at the world's edge has its prev just outside).
GPE_COLLIDER_FN bool sweep_cell_axis(float t, float gf, uint32_t g, uint32_t *c)
{
    if (!(t >= -0.5f && t < gf + 0.5f)) return false;          // (a NaN: false)
    const float u = (t > 0.0f) ? t : 0.0f;
    const uint32_t i = (uint32_t)u;                            // in [0, 1025): the cast is an exact truncation
    *c = i < g ? i : g - 1;
    return true;
}

// The lookup box of a path: the cells of its two end points (collider_cell_of's products) and those between.  false: an
// end point has no cell (more than half a cell outside the grid, or a NaN), or the box spans more than kSweepBoxCells
// cells one way: the pass walks every collider.
GPE_COLLIDER_FN bool sweep_box(const ColliderGridView &g, float x0x, float x0y, float x1x, float x1y, uint32_t *cx0,
                               uint32_t *cx1, uint32_t *cy0, uint32_t *cy1)
{
    const float tx0 = x0x * g.inv_cell;
    const float ty0 = x0y * g.inv_cell;
    const float tx1 = x1x * g.inv_cell;
    const float ty1 = x1y * g.inv_cell;
    uint32_t ax, bx, ay, by;
    if (!sweep_cell_axis(tx0, g.gxf, g.gx, &ax) || !sweep_cell_axis(ty0, g.gyf, g.gy, &ay)) return false;
    if (!sweep_cell_axis(tx1, g.gxf, g.gx, &bx) || !sweep_cell_axis(ty1, g.gyf, g.gy, &by)) return false;
    *cx0 = ax < bx ? ax : bx;
    *cx1 = ax < bx ? bx : ax;
    *cy0 = ay < by ? ay : by;
    *cy1 = ay < by ? by : ay;
    return *cx1 - *cx0 < kSweepBoxCells && *cy1 - *cy0 < kSweepBoxCells;
}

}  // namespace gpe
