// k_collider.h -- the one definition of "this static capsule pushes this particle, how far and which way", and of the
// cell a particle looks its colliders up in: what the pass (k_colliders.hip), the host's grid builder
// (collider_grid.h) and the CPU test program (tests/cpp/collider_grid_tests.cpp) share.  No HIP header: plain g++
// compiles it (with -ffp-contract=off).
//
// A collider is a capsule: the segment a -> b thickened by R >= 0 (a == b: a disc; R == 0: a thin wall; a chain of
// them: a polyline).  One pass resolves, for every particle, ONLY the collider it penetrates deepest, every collider
// judged from the position the pass starts with.  The result is therefore a function of (p, r, colliders) alone:
// order-free across particles and exactly binnable; the overlapping capsules of a polyline do not push twice at their
// joints; a particle in a corner is resolved over two steps.  There is no swept test in this rule: a wall thinner than
// one step's displacement is tunnelled through -- hosts make walls thick, or switch on the swept form of the pass
// (k_sweep.h: the path prev -> pos against the static colliders; not the movers, not the collision solver's pushes).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPE_COLLIDER_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GPE_COLLIDER_FN inline
#endif

namespace gpe {

struct ColliderTouch {
    float depth;                 // s - d: how far the particle is pushed
    float qx, qy, d;             // the offset from the segment's nearest point to the centre, and its length
    float dx, dy, A;             // b - a and its squared length
    float u;                     // the clamped parameter of the nearest point on a -> b (k_surface.h: where a wall moves)
};

// The particle (centre p, stored radius r) against the capsule a -> b of radius R.  true: touched, *t filled.
// IEEE binary32, one rounding per operation, left to right, no FMA; `/` and sqrtf are correctly rounded; numpy float32
// reproduces it bit for bit (tests/_colliders_model.py).  The predicate is strict, the contact predicate's sense; a NaN
// anywhere makes a comparison false: u becomes 0, and h < s*s fails, which is "not touched".
GPE_COLLIDER_FN bool collider_touch(float px, float py, float r, float ax, float ay, float bx, float by, float R,
                                    ColliderTouch *t)
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
    if (!(h < ss)) return false;
    const float d = sqrtf(h);
    t->depth = s - d;
    t->qx = qx; t->qy = qy; t->d = d;
    t->dx = dx; t->dy = dy; t->A = A;
    t->u = u;
    return true;
}

// The direction a touched particle is pushed in: away from the segment's nearest point; a centre exactly on the axis
// goes to the left of a -> b; a centre exactly on a disc's centre goes along +x.
GPE_COLLIDER_FN void collider_normal(const ColliderTouch &t, float *nx, float *ny)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (t.d > 0.0f) {
        *nx = t.qx / t.d;
        *ny = t.qy / t.d;
    } else if (t.A > 0.0f) {
        const float L = sqrtf(t.A);
        *nx = (-t.dy) / L;
        *ny = t.dx / L;
    } else {
        *nx = 1.0f;
        *ny = 0.0f;
    }
}

// Among the touched colliders the largest key wins: the deepest penetration, the lowest collider index on a tie (the
// selection rule of the run monitor's fastest particle).  j < GPE_COLLIDERS_MAX, so a key is never 0.
GPE_COLLIDER_FN unsigned long long collider_key(float depth, uint32_t j)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &depth, sizeof(bits));
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - j);
}

// The lookup grid as the pass sees it: gx x gy cells of 1 / inv_cell world units from the origin.  rb: the radius
// bound the lists were built for.
struct ColliderGridView {
    float inv_cell = 0.0f;
    float gxf = 1.0f, gyf = 1.0f;        // (float)gx, (float)gy: exact, both <= kColliderGridMaxDim
    uint32_t gx = 1, gy = 1;
    float rb = 0.0f;
};
constexpr uint32_t kColliderGridMaxDim = 1024;

// The cell of p, or false when p has none (outside the grid, or a NaN coordinate): the pass then walks every collider.
// One binary32 product per axis.  Against the exact p / cell the product is off by less than 2^-22 * gx <= 2^-12 cells,
// so p lies within 2^-12 cells of the cell this returns; the lists are inflated by a whole cell (collider_grid.h).
GPE_COLLIDER_FN bool collider_cell_of(const ColliderGridView &g, float px, float py, uint32_t *cell)
{
    const float tx = px * g.inv_cell;
    const float ty = py * g.inv_cell;
    if (!(tx >= 0.0f && tx < g.gxf && ty >= 0.0f && ty < g.gyf)) return false;
    *cell = (uint32_t)ty * g.gx + (uint32_t)tx;                // both in [0, 1024): the casts are exact truncations
    return true;
}

}  // namespace gpe
