// k_bend.h -- the one definition of "this bend moves its three particles by this much in one relaxation": what the pass
// (k_bends.hip) and the CPU test program (tests/cpp/bend_graph_tests.cpp) share.  No HIP header: plain g++ compiles it
// (with -ffp-contract=off).
//
// A bend names three particles: a, the hinge b and c, and holds the angle from u = a - b to v = c - b at a rest angle
// given as (rest_cos, rest_sin), so that nobody needs libm.  It is the position-based-dynamics step on C = sin(the
// deviation from the rest angle) with equal masses: the three corrections sum to zero.  One relaxation judges every bend
// from the positions the relaxation starts with (Jacobi): the bend's corrections are a function of those three
// positions and the bend alone, a particle's new position the sum of its bends' shares in ascending bend index.  No
// order of addition depends on the launch, on where the particles are stored or on the pipeline.  Under the coloured
// solver (gpe_set_bend_solver, bend_colours.h) the same bend_correction is judged from the positions as they are, colour
// after colour, and a bend moves its three particles itself (tests/cpp/bend_colours_tests.cpp replays that).
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_bond.h"

namespace gpe {

enum BendVerdict : uint32_t {
    kBendActs = 0,               // a receives (dax, day), c (dcx, dcy), the hinge (-(dax + dcx), -(day + dcy))
    kBendInert = 2,              // this relaxation only: NaN, a coincident centre, an arm that under- or overflows
};

// The bend over a = (ax, ay), the hinge b = (bx, by) and c = (cx, cy); (rc, rs) the rest angle's cosine and sine.  IEEE
// binary32, one rounding per operation, left to right, no FMA; `/` and sqrtf are correctly rounded; numpy float32
// reproduces it bit for bit (tests/_bends_model.py).  More than 90 degrees off the rest angle (dt < 0) the sine would
// shrink again: the bend then takes the largest correction, in the sense of cr; an exact fold-back (cr == 0) turns +1.
GPE_BOND_FN BendVerdict bend_correction(float ax, float ay, float bx, float by, float cx, float cy, float rc, float rs,
                                        float stiffness, float *dax, float *day, float *dcx, float *dcy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ux = ax - bx;
    const float uy = ay - by;
    const float vx = cx - bx;
    const float vy = cy - by;
    const float lu = ux * ux + uy * uy;
    const float lv = vx * vx + vy * vy;
    const float tx = rc * ux - rs * uy;                                // u turned by the rest angle
    const float ty = rs * ux + rc * uy;
    const float cr = tx * vy - ty * vx;
    const float dt = tx * vx + ty * vy;
    const float den = sqrtf(lu * lv);
    if (!(lu > 0.0f && lv > 0.0f && den > 0.0f && den < INFINITY)) return kBendInert;   // NaN fails every comparison
    float s = cr / den;
    if (dt < 0.0f) s = (cr < 0.0f) ? -1.0f : 1.0f;
    if (s != s) return kBendInert;
    const float gax = uy / lu;
    const float gay = -ux / lu;
    const float gcx = -vy / lv;
    const float gcy = vx / lv;
    const float gbx = -(gax + gcx);
    const float gby = -(gay + gcy);
    const float q = ((gax * gax + gay * gay) + (gcx * gcx + gcy * gcy)) + (gbx * gbx + gby * gby);
    if (!(q > 0.0f && q < INFINITY)) return kBendInert;
    const float m = s * stiffness;
    const float lam = -m / q;
    *dax = lam * gax;
    *day = lam * gay;
    *dcx = lam * gcx;
    *dcy = lam * gcy;
    return kBendActs;
}

// The hinge's share, formed where it is added: -(da + dc), one addition and an exact negation per component.
GPE_BOND_FN float bend_hinge_share(float da, float dc)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return -(da + dc);
}

// A particle with at least one acting bend: bond_move (k_bond.h): p + acc, then K12's clamp with its stored radius.

}  // namespace gpe
