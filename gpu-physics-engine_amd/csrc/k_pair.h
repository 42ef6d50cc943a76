// pair_response: one pair of the reference's collision response (collision_solver.wgsl:91-111) for a wave of 64
// lanes, and the small vector helpers it is written with.  Included by k_native.hip (every collide form) and by
// tests/hip/pair_probe.hip, which runs it over edge-case pairs against an IEEE binary32 restatement.
#pragma once

#include <type_traits>

#include "gpe_internal.h"

namespace gpe {

// One pair of the reference's response (collision_solver.wgsl:91-111), shared by the one-lane-per-cell and the
// lane-group resolution.  One wave-uniform early-out (no lane of the wave can collide), then straight-line code
// whose result a lane keeps or not by select.  Bit-exact shortcuts:
//  * r1 == r2 (and 1/r finite, non-zero): inv1 == inv2 and inv1 + inv1 == 2 inv1 exactly, so both weights
//    (:107-108) are exactly 0.5 -- the three divisions are skipped, not approximated.
//  * q = vx*vx + vy*vy > 1.000001 rs^2 implies rs^2 <= distance^2 (distance = sqrt(q) correctly rounded, so
//    distance^2 >= q (1 - 2^-22)): no collision (:95); q < 9.9e-9 implies distance < 0.0001 (:95; 0.0001f squared
//    is 9.99999995e-9): no collision either.  Neither needs the square root.
//  * the correctly rounded square root and quotients without the steps hipcc's sequences spend on scaling and
//    specials, IEEE division for the rare quotients below 2^-82 (below).
// Instruction budget (round 4; the tiles are bound by VALU issue at 100 M particles):
//  * x and y travel as one 64-bit register pair (f32x2): the subtraction, the squares, the two quotients' refinement
//    chains, the scalings and the final additions are the same operation on both components, and gfx950 issues
//    v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 -- IEEE binary32 per component, the same rounding as the scalar
//    forms -- in the slot of one scalar instruction.  Left to itself hipcc packed a quarter of them.
//  * the predicates are LANE MASKS (ballot64 / lanes_of, gpe_internal.h): every comparison is voted on its own and the masks are combined
//    by scalar ANDs.  A vote on `a && b` costs two VALU instructions (hipcc materialises the combined predicate as
//    0 / 1 and compares it again); the response votes three times per pair.
// `active`: the lanes that have a pair; `plain`: the lanes whose r1 is an ordinary number (1e-30 .. 1e30).  Returns the
// lanes that collided; (p1, p2) are updated in place for them.
#ifdef GPE_COUNT_PAIRS
// diagnostic builds only (scripts/soak_pairs.py): pairs the colour passes walk / resolve, over all tiles (the halo cells a
// tile recomputes for its neighbours included) -- what "ms per 10^9 pairs" in BASELINE.md is measured with
// (4096 counters each, by workgroup, 64 bytes apart: two counters for the whole device took 300 ms per step at 100 M; and
// only while g_pairs_on is set, so that a run reaches the step of interest at nearly the product's speed)
constexpr int kPairCounters = 4096;
__device__ unsigned long long g_pairs_walked[kPairCounters * 8], g_pairs_hit[kPairCounters * 8];
__device__ uint32_t g_pairs_on;
__device__ __forceinline__ void count_pairs(unsigned long long *ctr, const uint64_t m)
{
    if (m != 0 && g_pairs_on != 0u && lane_id() == (int)__builtin_ctzll(m))
        atomicAdd(&ctr[(blockIdx.x & (kPairCounters - 1)) * 8], (unsigned long long)__popcll(m));
}
#endif
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(const float v) { return (f32x2){v, v}; }
__device__ __forceinline__ f32x2 fma2(const f32x2 a, const f32x2 b, const f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 select2(const bool c, const f32x2 a, const f32x2 b) { return (f32x2){c ? a.x : b.x, c ? a.y : b.y}; }
__device__ __forceinline__ uint64_t plain_radius_lanes(const float r) { return ballot64(r >= 1e-30f) & ballot64(r <= 1e30f); }
// The lanes whose particle has a coordinate of -0 (a lane group's `careful` lanes, see pair_response).  A coordinate
// becomes -0 in a collision only if it was -0 before (p + c w == -0 needs p == -0), so one vote per particle covers
// all its pairs.
__device__ __forceinline__ uint64_t neg_zero_lanes(const f32x2 p)
{
    return ballot64(__builtin_amdgcn_classf(p.x, 0x20 /* -0 */)) | ballot64(__builtin_amdgcn_classf(p.y, 0x20));
}

// BOTH = false: only p1 is updated (the lane groups, where each lane of a pair computes its own half).  `lower`: the
// lanes whose particle is the pair's lower object index (the oracle's first particle; diagnostic builds count the pair
// on those lanes).  An upper lane computes p1 + c' w with c' from its own v' = p1 - p2, where the oracle computes
// p1 - c w with c from v = p2 - p1.  c' == -c exactly except when a component of v is 0: then the two zeros can have
// the same sign, and p1 - c w != p1 + c' w where that component of p1 is -0 (both particles at -0).  `careful`: lanes
// that may hold such a particle (neg_zero_lanes); their pairs take the IEEE path below in the oracle's orientation.
//
// The UNIFORM form: every particle has the one radius r, an ordinary number (plain_radius_lanes' range -- the host checks
// it once per configuration, NativeState::uniform).  Then the first shortcut above holds for every pair, and r1 + r2, its
// square and the prefilter's bound are the same three numbers for every pair: UniformRadii holds them, formed once per
// kernel by the very operations the general form performs per pair.  No r1 / r2, no `plain`, no general branch, weights
// of 0.5; every other line is shared with the general form, which every order-key kernel keeps.
struct UniformRadii { float r, sum, sum2, bound; };
__device__ __forceinline__ UniformRadii uniform_radii(const float r)
{
    UniformRadii U;
    U.r = r;
    U.sum = r + r;                                                    // :61
    U.sum2 = U.sum * U.sum;
    U.bound = U.sum2 * 1.000001f;
    return U;
}
template <bool BOTH, bool UNIFORM>
__device__ __forceinline__ uint64_t pair_response_core(const uint64_t active, f32x2 &p1, std::conditional_t<BOTH, f32x2 &, const f32x2 &> p2,
                                                       const float r1, const float r2, const uint64_t plain, const UniformRadii &U,
                                                       const float stiffness, const uint64_t lower, const uint64_t careful)
{
    (void)lower;
    (void)careful;
    (void)r1; (void)r2; (void)plain; (void)U;
#ifdef GPE_COUNT_PAIRS
    count_pairs(g_pairs_walked, active & lower);
#endif
    const f32x2 v = p1 - p2;                                          // :91 (live positions, :86)
    const f32x2 vv = v * v;
    const float q = vv.x + vv.y;
    float radius_sum, rs2, bound;
    if constexpr (UNIFORM) { radius_sum = U.sum; rs2 = U.sum2; bound = U.bound; }
    else {
        radius_sum = r1 + r2;                                         // :61
        rs2 = radius_sum * radius_sum;
        bound = rs2 * 1.000001f;
    }
    const uint64_t cand = active & ballot64(q <= bound) & ballot64(q >= 9.9e-9f);
    if (cand == 0) return 0;                                          // wave-uniform
    // The correctly rounded square root and quotients WITHOUT the steps hipcc's sequences spend on scaling and
    // specials.  A candidate has q in [9.9e-9, 1.000001 rs^2], so the square root's operand is a normal number and a
    // hit's distance lies in (1e-4, 2^64): its reciprocal is normal too.  The numerators are differences of positions,
    // which can be anything from 0 to subnormal when particles sit near x = 0 or y = 0.  The lanes that are not
    // candidates compute garbage that the selects below discard.
    //   sqrt: v_sqrt_f32 is within 1 ulp; try the neighbours with an exact residual (one fma each).
    //   x / d: r = 1/d refined once (shared by the two quotients); q0 = x r; q1 = q0 + (x - d q0) r; result =
    //   q1 + (x - d q1) r -- the core of v_div_scale / v_div_fmas / v_div_fixup.  The residuals x - d q are exact,
    //   and the result correctly rounded, while the quotient is at least 2^-82 in magnitude (then |x| > 2^-96 and the
    //   quotient is a normal number).  Below that the residual can round (numerators below ~2^-103), a subnormal
    //   quotient can land on a rounding midpoint, and RN(x r) can be 0 for x != 0: those lanes (a vote, then a
    //   wave-uniform branch) take IEEE x / d.
    float distance;
    {
        const float s0 = __builtin_amdgcn_sqrtf(q);
        const float s_dn = __int_as_float(__float_as_int(s0) - 1), s_up = __int_as_float(__float_as_int(s0) + 1);
        const float r_dn = __builtin_fmaf(-s_dn, s0, q);
        float sres = r_dn <= 0.0f ? s_dn : s0;
        const float r_up = __builtin_fmaf(-s_up, s0, q);
        sres = r_up > 0.0f ? s_up : sres;
        distance = sres;                                              // :93
    }
    const uint64_t hit = cand & ballot64(rs2 > distance * distance) & ballot64(distance > 0.0001f);   // :95
    const float depth = radius_sum - distance;                        // :97
    f32x2 u;
    {
        const float r0 = __builtin_amdgcn_rcpf(distance);
        const float e0 = __builtin_fmaf(-distance, r0, 1.0f);
        // the residuals as -(d q - x): the same value as x - d q, but -0 where x is -0 and q is -0 (x - d q is +0
        // there), so that a quotient of -0 stays -0; the negations are free operand modifiers
        const f32x2 rq = splat2(__builtin_fmaf(e0, r0, r0)), pd = splat2(distance);
        const f32x2 q0 = v * rq;
        const f32x2 q1 = fma2(-fma2(pd, q0, -v), rq, q0);
        u = fma2(-fma2(pd, q1, -v), rq, q1);
    }
    {
        // quotients below 2^-82 whose numerator is not 0 (the smaller quotient belongs to the smaller numerator; the
        // other one is >= 0.7).  The numerator, not the quotient, is tested against 0: RN(x r) can be 0 for x != 0.
        // Exact zeros -- axis-aligned pairs, common against the walls -- stay on the fast path, which is exact for them.
        const float umin = __builtin_fminf(__builtin_fabsf(u.x), __builtin_fabsf(u.y));
        const float vmin = __builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y));
        uint64_t slow = hit & ballot64(umin < 0x1p-82f) & ballot64(vmin != 0.0f);
        if constexpr (!BOTH) slow |= hit & careful;
        if (slow != 0) {                                              // wave-uniform
            if (lanes_of(slow)) {
                if constexpr (BOTH) {
                    u = (f32x2){v.x / distance, v.y / distance};
                } else {                                              // in the oracle's orientation: c = -(c of p2 - p1)
                    const bool up = !lanes_of(lower);
                    const f32x2 vo = select2(up, p2 - p1, v);
                    const f32x2 uo = {vo.x / distance, vo.y / distance};
                    u = select2(up, -uo, uo);
                }
            }
        }
    }
    const f32x2 c = (u * splat2(depth)) * splat2(stiffness);          // :98,101
    float w1 = 0.5f, w2 = 0.5f;                                       // == inv1 / (inv1 + inv1), exactly
    if constexpr (!UNIFORM) {
        const uint64_t general = hit & ~(ballot64(r1 == r2) & plain); // unequal (or odd) radii somewhere
        if (general != 0) {                                           // wave-uniform
            if (lanes_of(general)) {
                const float inv1 = 1.0f / r1, inv2 = 1.0f / r2;       // :103,104
                w1 = inv1 / (inv1 + inv2);                            // :107
                w2 = inv2 / (inv1 + inv2);                            // :108
            }
        }
    }
    const bool mine = lanes_of(hit);
    p1 = select2(mine, p1 + c * splat2(w1), p1);                      // :110
    if constexpr (BOTH) p2 = select2(mine, p2 - c * splat2(w2), p2);  // :111
#ifdef GPE_COUNT_PAIRS
    count_pairs(g_pairs_hit, hit & lower);
#endif
    return hit;
}
template <bool BOTH = true>
__device__ __forceinline__ uint64_t pair_response(const uint64_t active, f32x2 &p1, std::conditional_t<BOTH, f32x2 &, const f32x2 &> p2,
                                                  const float r1, const float r2, const uint64_t plain,
                                                  const float stiffness, const uint64_t lower = ~0ull,
                                                  const uint64_t careful = 0)
{
    return pair_response_core<BOTH, false>(active, p1, p2, r1, r2, plain, UniformRadii(), stiffness, lower, careful);
}
template <bool BOTH = true>
__device__ __forceinline__ uint64_t pair_response(const uint64_t active, f32x2 &p1, std::conditional_t<BOTH, f32x2 &, const f32x2 &> p2,
                                                  const UniformRadii &U, const float stiffness, const uint64_t lower = ~0ull,
                                                  const uint64_t careful = 0)
{
    return pair_response_core<BOTH, true>(active, p1, p2, 0.f, 0.f, 0ull, U, stiffness, lower, careful);
}

}  // namespace gpe
