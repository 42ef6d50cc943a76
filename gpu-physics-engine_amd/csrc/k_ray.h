// k_ray.h -- the one definition of "this segment touches this particle, and where": what gpe_cast_rays (k_raycast.hip)
// and gpe_query_segment (the segment kind of k_region.h) share, so that a ray's first hit is the member of the
// segment query's set with the least t.
#pragma once

#include "gpe_internal.h"

namespace gpe {

// The segment from o = (ox, oy) to e = (ex, ey) against the closed disc of radius |r| around c = (cx, cy).  true:
// touched, *t_out = the fraction of the way from o to e where the segment enters the disc (+0 when o lies inside it).
// IEEE binary32, one rounding per operation, left to right, no FMA (the build also compiles with -ffp-contract=off);
// `/` and sqrtf are correctly rounded; numpy float32 reproduces it bit for bit (tests/_ray_model.py).
// The closest-approach form: q = the offset of the line's point nearest to c, h = |q|^2, and the entry point lies
// w = sqrt((rr - h) / A) before it.  There is no B*B - A*C cancellation.  A radius of 0 or NaN is never hit; a NaN
// anywhere makes a comparison false, which is a miss.
__device__ __forceinline__ bool ray_touches(float ox, float oy, float ex, float ey, float cx, float cy, float r,
                                            float *t_out)
{
#pragma clang fp contract(off)
    const float a = fabsf(r);
    const float rr = a * a;
    if (!(a > 0.0f)) return false;
    const float dx = ex - ox;
    const float dy = ey - oy;
    const float fx = ox - cx;
    const float fy = oy - cy;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    const float A = dxx + dyy;
    const float fxx = fx * fx;
    const float fyy = fy * fy;
    const float C = fxx + fyy;
    if (C <= rr) {                                             // the origin lies in the closed disc
        *t_out = 0.0f;
        return true;
    }
    if (!(A > 0.0f)) return false;
    const float bx = fx * dx;
    const float by = fy * dy;
    const float B = bx + by;
    const float u = (-B) / A;
    const float ux = u * dx;
    const float uy = u * dy;
    const float qx = fx + ux;
    const float qy = fy + uy;
    const float qxx = qx * qx;
    const float qyy = qy * qy;
    const float h = qxx + qyy;
    if (!(h <= rr)) return false;
    const float g = rr - h;
    const float s = g / A;
    const float w = sqrtf(s);
    const float t = u - w;
    if (!(t >= 0.0f && t <= 1.0f)) return false;
    *t_out = t == 0.0f ? 0.0f : t;                            // -0 counts as, and is delivered as, +0
    return true;
}

}  // namespace gpe
