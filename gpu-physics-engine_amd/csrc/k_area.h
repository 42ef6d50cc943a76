// k_area.h -- the one definition of "this loop moves its members by this much in one relaxation": what the pass
// (k_areas.hip) and the CPU test program (tests/cpp/area_table_tests.cpp) share.  No HIP header: plain g++ compiles it
// (with -ffp-contract=off).
//
// An area constraint ("loop") is `count` members named by uid, in order around a closed polygon, with a signed rest
// area (positive when the members turn from +x towards +y) and a stiffness.  One relaxation is the position-based-
// dynamics step on C = area - rest_area with equal masses: every member moves along the gradient of the area with
// respect to its own position, which is half the chord between its two neighbours turned by a quarter.  Every loop is
// judged from the positions the relaxation starts with (Jacobi); a particle's new position is the sum of its loops'
// corrections in ascending member index.  Both sums over a loop's members are the canonical sum S of k_body.h (its
// order depends on count alone), so no order of addition depends on the launch, on where the particles are stored or
// on the pipeline.  IEEE binary32, one rounding per operation, left to right, no FMA, no libm; `/` is correctly
// rounded; numpy float32 reproduces it bit for bit (tests/_areas_model.py).
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_body.h"
#include "k_bond.h"

#if defined(__HIPCC__)
#define GPE_AREA_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GPE_AREA_FN inline
#endif

namespace gpe {

// a loop's state byte: this relaxation's outcome (a loop never breaks)
enum AreaVerdict : uint32_t {
    kAreaActs = 0,               // member j receives corr_j
    kAreaInert = 2,              // this relaxation only: a member without a particle, NaN, coincident members, overflow
};

// q = p - p0, componentwise: member 0 is the origin (the area is translation invariant; the products stay small in a
// world that is thousands wide).
GPE_AREA_FN float area_rel(float p, float p0)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return p - p0;
}

// t_j = q_j x q_n: member j's term of twice the area (n: the next member around the ring).
GPE_AREA_FN float area_term(float qx, float qy, float nx, float ny)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = qx * ny;
    const float b = nx * qy;
    return a - b;
}

// g_j = d area / d p_j = (0.5 (q_n.y - q_m.y), 0.5 (q_m.x - q_n.x)) (m: the member before j); returns |g_j|^2.
GPE_AREA_FN float area_gradient(float nx, float ny, float mx, float my, float *gx, float *gy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dy = ny - my;
    const float dx = mx - nx;
    const float x = 0.5f * dy;
    const float y = 0.5f * dx;
    const float xx = x * x;
    const float yy = y * y;
    *gx = x;
    *gy = y;
    return xx + yy;
}

// The sums A2 = S(t) and D = S(|g|^2) of a loop whose members all have a particle -> area and lambda.  false: the loop
// is inert in this relaxation (NaN fails every comparison; coincident members give D == 0; overflow an infinity).
GPE_AREA_FN bool area_lambda(float A2, float D, float rest_area, float stiffness, float *area, float *lambda)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = 0.5f * A2;
    const float C = a - rest_area;
    if (!(D > 0.0f && D < INFINITY)) return false;
    if (!(C > -INFINITY && C < INFINITY)) return false;
    const float s = C * stiffness;
    const float q = s / D;
    *area = a;
    *lambda = -q;
    return true;
}

// corr_j = lambda * g_j, one product per component.
GPE_AREA_FN float area_scale(float lambda, float g)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return lambda * g;
}

// A particle with at least one acting loop: bond_move (k_bond.h): p + acc, then K12's clamp with its stored radius.

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the loop phase restated for the host, member by member and lane by lane (the CPU test program runs it) --------
// S(v) over all `count` members (body_sum with every member live).
inline float area_sum(const float *v, uint32_t count)
{
    const uint32_t G = body_width(count);
    float partial[kBodyMaxWidth];
    for (uint32_t l = 0; l < G; ++l) {
        float p = 0.0f;
        for (uint32_t j = l; j < count; j += G) p = body_add(p, v[j]);
        partial[l] = p;
    }
    for (uint32_t off = G / 2; off >= 1; off /= 2)
        for (uint32_t l = 0; l < off; ++l) partial[l] = body_add(partial[l], partial[l + off]);
    return partial[0];
}

// One loop over its members' positions (px, py) and live flags (a member whose uid names no particle is not live).
// corr: 2 * count floats (x, y per member), written when the loop acts; scratch: 2 * count floats.  value: (area,
// lambda), two NaNs unless the loop acts.
inline AreaVerdict area_pass_host(uint32_t count, const float *px, const float *py, const uint8_t *live, float rest_area,
                                  float stiffness, float *corr, float *scratch, float value[2])
{
    value[0] = value[1] = NAN;
    if (count < 3) return kAreaInert;
    for (uint32_t j = 0; j < count; ++j)
        if (!live[j]) return kAreaInert;
    float *t = scratch, *d = scratch + count;
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t n = (j + 1) % count, m = (j + count - 1) % count;
        const float qx = area_rel(px[j], px[0]), qy = area_rel(py[j], py[0]);
        const float nx = area_rel(px[n], px[0]), ny = area_rel(py[n], py[0]);
        const float mx = area_rel(px[m], px[0]), my = area_rel(py[m], py[0]);
        t[j] = area_term(qx, qy, nx, ny);
        d[j] = area_gradient(nx, ny, mx, my, &corr[2 * j], &corr[2 * j + 1]);
    }
    float area, lambda;
    if (!area_lambda(area_sum(t, count), area_sum(d, count), rest_area, stiffness, &area, &lambda)) return kAreaInert;
    for (uint32_t j = 0; j < count; ++j) {
        corr[2 * j] = area_scale(lambda, corr[2 * j]);
        corr[2 * j + 1] = area_scale(lambda, corr[2 * j + 1]);
    }
    value[0] = area;
    value[1] = lambda;
    return kAreaActs;
}
#endif

}  // namespace gpe
