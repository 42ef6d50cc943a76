// k_body.h -- the one definition of "this body's members move to here in one shape matching pass": what the pass
// (k_bodies.hip) and the CPU test program (tests/cpp/body_table_tests.cpp) share.  No HIP header: plain g++ compiles
// it (with -ffp-contract=off).
//
// A body is `count` members with rest positions.  One pass finds the translation and rotation of the rest shape that
// fits the live members best (in 2-D two sums give the angle: no polar decomposition) and moves every live member
// towards that pose by the body's stiffness.  Every sum over members is the canonical sum S below: its order of
// addition depends on count alone, never on the launch, on where the particles are stored or on the pipeline.
// IEEE binary32, one rounding per operation, left to right, no FMA; `/` and sqrtf are correctly rounded; numpy float32
// reproduces it bit for bit (tests/_bodies_model.py).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPE_BODY_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GPE_BODY_FN inline
#endif

namespace gpe {

constexpr uint32_t kBodyMaxWidth = 64;       // the widest sum: one wave

// a body's state byte: broken is sticky, the other two are this pass's outcome
enum BodyVerdict : uint32_t { kBodyActs = 0, kBodyBroken = 1, kBodyInert = 2 };

// G: the smallest power of two >= count, at most 64.  (count >= 2)
GPE_BODY_FN uint32_t body_width(uint32_t count)
{
    uint32_t g = 2;
    while (g < count && g < kBodyMaxWidth) g <<= 1;
    return g;
}

// One step of a lane's partial sum: partial starts at +0.0f, an absent member adds +0.0f.
GPE_BODY_FN float body_add(float partial, float v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return partial + v;
}

// (a, b) of one live member: q = r - rbar, d = p - c, a = q . d, b = q x d.
GPE_BODY_FN void body_moment(float rx, float ry, float rbx, float rby, float px, float py, float cx, float cy,
                             float *qx, float *qy, float *a, float *b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float x = rx - rbx;
    const float y = ry - rby;
    const float dx = px - cx;
    const float dy = py - cy;
    const float xx = x * dx;
    const float yy = y * dy;
    const float xy = x * dy;
    const float yx = y * dx;
    *qx = x;
    *qy = y;
    *a = xx + yy;
    *b = xy - yx;
}

// The rotation of the sums (A, B): false: the body is inert in this pass (NaN, overflow, coincident members,
// underflow).
GPE_BODY_FN bool body_rotation(float A, float B, float *co, float *si)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float aa = A * A;
    const float bb = B * B;
    const float h2 = aa + bb;
    const float h = sqrtf(h2);
    if (!(h > 0.0f && h < INFINITY)) return false;             // NaN fails both comparisons
    *co = A / h;
    *si = B / h;
    return true;
}

// The way (ex, ey) of one live member to its place in the matched pose, and its squared length.
GPE_BODY_FN float body_error(float qx, float qy, float px, float py, float cx, float cy, float co, float si, float *ex,
                             float *ey)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float cqx = co * qx;
    const float sqy = si * qy;
    const float sqx = si * qx;
    const float cqy = co * qy;
    const float tx = cqx - sqy;
    const float ty = sqx + cqy;
    const float gx = cx + tx;
    const float gy = cy + ty;
    const float x = gx - px;
    const float y = gy - py;
    const float xx = x * x;
    const float yy = y * y;
    *ex = x;
    *ey = y;
    return xx + yy;
}

// bd2: break_distance * break_distance, or kBodyNeverBreaks for a break_distance of 0.  Strict; a NaN e2 holds.
constexpr float kBodyNeverBreaks = -1.0f;
GPE_BODY_FN bool body_breaks(float e2, float bd2)
{
    return bd2 >= 0.0f && e2 > bd2;
}

// K12's clamp (gpe_internal.h clamp_f, restated for the host): a NaN x gives lo.
GPE_BODY_FN float body_clamp(float x, float lo, float hi)
{
    const float m = (x > lo) ? x : lo;
    return (m < hi) ? m : hi;
}

// A live member of a body that acts: p + stiffness * e, then K12's clamp with its stored radius r, as bond_move.
GPE_BODY_FN void body_move(float px, float py, float r, float stiffness, float ex, float ey, float W, float H, float *ox,
                           float *oy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float sx = stiffness * ex;
    const float sy = stiffness * ey;
    const float qx = px + sx;
    const float qy = py + sy;
    *ox = body_clamp(qx, r, W - r);
    *oy = body_clamp(qy, r, H - r);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the pass restated for the host, member by member and lane by lane (the CPU test program runs it) -------------
// S(v): v[j] of member j, live[j] == 0 adds +0.0f.
inline float body_sum(const float *v, const uint8_t *live, uint32_t count)
{
    const uint32_t G = body_width(count);
    float partial[kBodyMaxWidth];
    for (uint32_t l = 0; l < G; ++l) {
        float p = 0.0f;
        for (uint32_t j = l; j < count; j += G) p = body_add(p, live[j] ? v[j] : 0.0f);
        partial[l] = p;
    }
    for (uint32_t off = G / 2; off >= 1; off /= 2)
        for (uint32_t l = 0; l < off; ++l) partial[l] = body_add(partial[l], partial[l + off]);
    return partial[0];
}

// One body over its members' rest (rx, ry), positions (px, py) in place, radii and live flags; scratch: 4 * count
// floats.  pose: (cx, cy, co, si), four NaNs unless the body acts.
inline BodyVerdict body_pass_host(uint32_t count, const float *rx, const float *ry, float *px, float *py,
                                  const float *radius, const uint8_t *live, float stiffness, float bd2, float W, float H,
                                  float *scratch, float pose[4])
{
    pose[0] = pose[1] = pose[2] = pose[3] = NAN;
    uint32_t L = 0;
    for (uint32_t j = 0; j < count; ++j) L += live[j] ? 1u : 0u;
    if (L < 2) return kBodyInert;
    const float fL = (float)L;
    const float rbx = body_sum(rx, live, count) / fL, rby = body_sum(ry, live, count) / fL;
    const float cx = body_sum(px, live, count) / fL, cy = body_sum(py, live, count) / fL;
    float *qx = scratch, *qy = scratch + count, *a = scratch + 2 * count, *b = scratch + 3 * count;
    for (uint32_t j = 0; j < count; ++j) {
        qx[j] = qy[j] = a[j] = b[j] = 0.0f;
        if (live[j]) body_moment(rx[j], ry[j], rbx, rby, px[j], py[j], cx, cy, &qx[j], &qy[j], &a[j], &b[j]);
    }
    float co, si;
    if (!body_rotation(body_sum(a, live, count), body_sum(b, live, count), &co, &si)) return kBodyInert;
    float *ex = a, *ey = b;                                    // (the sums are taken: their storage is free)
    bool breaks = false;
    for (uint32_t j = 0; j < count; ++j) {
        if (!live[j]) continue;
        const float e2 = body_error(qx[j], qy[j], px[j], py[j], cx, cy, co, si, &ex[j], &ey[j]);
        breaks |= body_breaks(e2, bd2);
    }
    if (breaks) return kBodyBroken;
    for (uint32_t j = 0; j < count; ++j)
        if (live[j]) body_move(px[j], py[j], radius[j], stiffness, ex[j], ey[j], W, H, &px[j], &py[j]);
    pose[0] = cx; pose[1] = cy; pose[2] = co; pose[3] = si;
    return kBodyActs;
}
#endif

}  // namespace gpe
