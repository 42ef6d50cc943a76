// k_bond.h -- the one definition of "this distance bond moves its two ends by this much in one relaxation": what the
// pass (k_bonds.hip) and the CPU test program (tests/cpp/bond_graph_tests.cpp) share.  No HIP header: plain g++
// compiles it (with -ffp-contract=off).
//
// A bond ties particle a to particle b, or (an anchor) to a fixed point, at a rest length.  One relaxation judges every
// bond from the positions the relaxation starts with (Jacobi): the bond's correction is a function of those two
// positions and the bond alone, a particle's new position the sum of its bonds' corrections in ascending bond index.
// No order of addition depends on the launch, on where the particles are stored or on the pipeline.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPE_BOND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GPE_BOND_FN inline
#endif

namespace gpe {

enum BondVerdict : uint32_t {
    kBondActs = 0,               // (cx, cy) is its correction: a receives (+cx, +cy), b (-cx, -cy)
    kBondBroken = 1,             // longer than max_length: broken from now on (sticky; the caller keeps the flag)
    kBondInert = 2,              // this relaxation only: NaN, coincident centres or an overflowing distance
};

// The bond between a = (ax, ay) and b = (bx, by) (b: the other particle, or the anchor point).  w: 0.5f * stiffness
// for a pair, stiffness for an anchor, multiplied on the host.  IEEE binary32, one rounding per operation, left to
// right, no FMA; `/` and sqrtf are correctly rounded; numpy float32 reproduces it bit for bit (tests/_bonds_model.py).
// The break is strict: d == max_length holds.  max_length == 0: never breaks.
GPE_BOND_FN BondVerdict bond_correction(float ax, float ay, float bx, float by, float rest, float w, float max_length,
                                        float *cx, float *cy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = bx - ax;
    const float dy = by - ay;
    const float dxx = dx * dx;
    const float dyy = dy * dy;
    const float h = dxx + dyy;
    const float d = sqrtf(h);
    if (!(d > 0.0f && d < INFINITY)) return kBondInert;        // NaN fails both comparisons
    if (max_length > 0.0f && d > max_length) return kBondBroken;
    const float e = d - rest;
    const float f = e / d;
    const float g = f * w;
    *cx = g * dx;
    *cy = g * dy;
    return kBondActs;
}

// K12's clamp (gpe_internal.h clamp_f, restated for the host): a NaN x gives lo.
GPE_BOND_FN float bond_clamp(float x, float lo, float hi)
{
    const float m = (x > lo) ? x : lo;
    return (m < hi) ? m : hi;
}

// A particle with at least one acting bond: p + acc, then K12's clamp with its stored radius r, as collider_resolve.
GPE_BOND_FN void bond_move(float px, float py, float r, float accx, float accy, float W, float H, float *ox, float *oy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float qx = px + accx;
    const float qy = py + accy;
    *ox = bond_clamp(qx, r, W - r);
    *oy = bond_clamp(qy, r, H - r);
}

}  // namespace gpe
