// k_surface.h -- the one definition of what an obstacle's surface does to the particle it pushes: bounce (restitution)
// and Coulomb friction, for the static colliders and the movers alike.  What the passes (k_colliders.hip, k_movers.hip),
// the host (gpe_surfaces.hip) and the CPU test program (tests/cpp/surface_tests.cpp) share.  No HIP header: plain g++
// compiles it (with -ffp-contract=off).
//
// The arithmetic rules are k_collider.h's: IEEE binary32, one rounding per operation, left to right, no FMA; `/` and
// sqrtf correctly rounded.  numpy float32 reproduces every function here bit for bit (tests/_surfaces_model.py).
//
// The acting obstacle is chosen exactly as without surfaces (collider_touch, collider_key, collider_normal: the deepest
// one, judged from the position the pass starts with).  The plain pass writes pos only: the Verlet velocity loses its
// component into the obstacle and keeps all of its tangential part.  A surface writes prev as well, so that the particle
// leaves with the velocity the material gives it.  What a surface is not: it does nothing between particles, knows no
// rolling or spin, and its friction sees the normal velocity change of this pass only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_collider.h"

namespace gpe {

constexpr uint32_t kSurfacePlain = 1u;                         // GPE_SURFACE_PLAIN
constexpr uint32_t kSurfaceKnownFlags = kSurfacePlain;

// A surface row as the device holds it (one float4): restitution e in [0, 1], friction mu >= 0, flags, reserved
struct SurfaceRow {
    float e, mu;
    uint32_t flags, reserved;
};

// why a row cannot be taken, or nullptr
inline const char *surface_refusal(float e, float mu, uint32_t flags, uint32_t reserved)
{
    if (!(e >= 0.0f && e <= 1.0f)) return "a restitution is NaN or outside [0, 1]";
    if (!(mu >= 0.0f) || !(mu <= 3.402823466e+38f)) return "a friction is NaN, infinite or negative";
    if (flags & ~kSurfaceKnownFlags) return "an unknown flag";
    if (reserved) return "reserved must be 0";
    return nullptr;
}

// K12's clamp (clamp_f of gpe_internal.h): a NaN x gives lo
GPE_COLLIDER_FN float surface_clamp(float x, float lo, float hi)
{
    const float m = (x > lo) ? x : lo;
    return (m < hi) ? m : hi;
}

// What the contact point of a mover moved in this step's advance: the posed capsule before it (a0, b0) = old[0..3],
// after it (a1, b1) = cap[0..3], the touch taken against (a1, b1) at the clamped parameter u.
GPE_COLLIDER_FN void surface_wall_move(const float *old, const float *cap, float u, float *wx, float *wy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float wax = cap[0] - old[0];
    const float way = cap[1] - old[1];
    const float wbx = cap[2] - old[2];
    const float wby = cap[3] - old[3];
    const float ex = wbx - wax;
    const float ey = wby - way;
    const float sx = u * ex;
    const float sy = u * ey;
    *wx = wax + sx;
    *wy = way + sy;
}

// Is p - prev finite in both components?  (false: the particle takes the plain rule, prev stays untouched)
GPE_COLLIDER_FN bool surface_velocity_finite(float px, float py, float prevx, float prevy)
{
    const float vx = px - prevx;
    const float vy = py - prevy;
    uint32_t bx, by;                                           // (the exponent field: no optimiser can fold this away)
    __builtin_memcpy(&bx, &vx, sizeof(bx));
    __builtin_memcpy(&by, &vy, sizeof(by));
    return (bx & 0x7F800000u) != 0x7F800000u && (by & 0x7F800000u) != 0x7F800000u;
}

// The particle at p (previous position prev, stored radius r), pushed along the normal n by depth, by a wall that moved
// w at the contact, on a surface (e, mu); the world is W x H.  out = (pos'x, pos'y, prev'x, prev'y).
//   q   = (px + nx*depth, py + ny*depth)                      the plain pass's push, the same bits
//   v   = p - prev;   rel = v - w
//   vn  = relx*nx + rely*ny
//   t   = (relx - vn*nx, rely - vn*ny)                        the tangential part, t0 = t
//   on  = (vn < 0) ? (-e)*vn : vn                             approaching: reflected and damped; separating: kept
//   jn  = on - vn                                             the normal velocity change, >= 0
//   tl  = sqrtf(tx*tx + ty*ty);   s = mu*jn
//   if s < tl:  k = (tl - s)/tl;  t = (tx*k, ty*k)            sliding: Coulomb, the change bounded by mu*jn
//   else:       t = (0, 0)                                    sticking
//   out = ((wx + on*nx) + tx, (wy + on*ny) + ty)              the velocity the particle leaves with
//   pos' = clamp(q - (t0 - t))                                K12's clamp as in the plain pass
//   prev' = pos' - out
// The tangential velocity friction removes is taken out of the position too: without that a particle that sticks on a
// slope creeps down by g*dt^2*sin every step.
GPE_COLLIDER_FN void surface_apply(float px, float py, float prevx, float prevy, float r, float nx, float ny, float depth,
                                   float wx, float wy, float e, float mu, float W, float H, float *out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float mx = nx * depth;
    const float my = ny * depth;
    const float qx = px + mx;
    const float qy = py + my;
    const float vx = px - prevx;
    const float vy = py - prevy;
    const float relx = vx - wx;
    const float rely = vy - wy;
    const float ax = relx * nx;
    const float ay = rely * ny;
    const float vn = ax + ay;
    const float cx = vn * nx;
    const float cy = vn * ny;
    const float t0x = relx - cx;
    const float t0y = rely - cy;
    const float me = -e;
    const float refl = me * vn;
    const float on = (vn < 0.0f) ? refl : vn;
    const float jn = on - vn;
    const float txx = t0x * t0x;
    const float tyy = t0y * t0y;
    const float hh = txx + tyy;
    const float tl = sqrtf(hh);
    const float s = mu * jn;
    float tx = 0.0f, ty = 0.0f;
    if (s < tl) {
        const float rest = tl - s;
        const float k = rest / tl;
        tx = t0x * k;
        ty = t0y * k;
    }
    const float bx = on * nx;
    const float by = on * ny;
    const float gx = wx + bx;
    const float gy = wy + by;
    const float outx = gx + tx;
    const float outy = gy + ty;
    const float lx = t0x - tx;
    const float ly = t0y - ty;
    const float ux = qx - lx;
    const float uy = qy - ly;
    const float hix = W - r;
    const float hiy = H - r;
    const float ox = surface_clamp(ux, r, hix);
    const float oy = surface_clamp(uy, r, hiy);
    out[0] = ox;
    out[1] = oy;
    out[2] = ox - outx;
    out[3] = oy - outy;
}

}  // namespace gpe
