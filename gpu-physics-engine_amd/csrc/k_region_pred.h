// k_region_pred.h -- the disc and box predicates of the region queries, the kicks and the force fields on bare floats:
// the one definition behind k_region.h (dist2, in_region) and k_field.h (field_matches).  No HIP header: plain g++
// compiles it (with -ffp-contract=off).
#pragma once

#if defined(__HIPCC__)
#define GPE_REGION_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GPE_REGION_FN inline
#endif

namespace gpe {

// IEEE binary32, one rounding per operation, left to right, no FMA.
GPE_REGION_FN float region_dist2(float px, float py, float x, float y)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = px - x;
    const float dy = py - y;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    return dxx + dyy;
}

// the closed disc around (x0, y0) with rr = radius * radius
GPE_REGION_FN bool region_in_disc(float px, float py, float x0, float y0, float rr)
{
    return region_dist2(px, py, x0, y0) <= rr;
}

// the closed box [x0, x1] x [y0, y1]
GPE_REGION_FN bool region_in_box(float px, float py, float x0, float y0, float x1, float y1)
{
    return x0 <= px && px <= x1 && y0 <= py && py <= y1;
}

}  // namespace gpe
