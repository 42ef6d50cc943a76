// k_field.h -- the one definition of "this force field matches this particle, and what it contributes": what the pass
// (k_fields.hip), the host (gpe_fields.hip, field_grid.h) and the CPU test program (tests/cpp/field_grid_tests.cpp)
// share.  No HIP header: plain g++ compiles it (with -ffp-contract=off).
//
// A field is a region (everywhere, a closed disc, a closed box: the predicates of k_region_pred.h on the particle's
// centre c = pos alone; the particle's radius plays no part) and a kind.  One pass gathers, for one particle, the
// matching fields in ascending index into a sum of accelerations A and a product of drags s, then writes prev only:
// first the drag (the kick's GPE_VEL_SCALE), then the acceleration (the kick's GPE_VEL_ADD).  The result is a binary32
// function of (pos, prev, fields, dt) alone; ascending order is part of it, since the sums are ordered.
//
// IEEE binary32, one rounding per operation, left to right, no FMA; `/` and sqrtf are correctly rounded; numpy float32
// reproduces it bit for bit (tests/_fields_model.py).  The payload of a NaN that the arithmetic itself produces (a
// particle with a NaN coordinate under an EVERYWHERE field) is not specified.
#pragma once

#include <math.h>
#include <stdint.h>

#include "k_region_pred.h"

#define GPE_FIELD_FN GPE_REGION_FN

namespace gpe {

// include/gpe.h's enums, restated so that this header needs nothing else (gpe_fields.hip asserts they agree)
enum : uint32_t { kFieldEverywhere = 0, kFieldCircle = 1, kFieldBox = 2 };
enum : uint32_t { kFieldUniform = 0, kFieldRadial = 1, kFieldVortex = 2, kFieldDrag = 3 };
enum : uint32_t { kFalloffNone = 0, kFalloffLinear = 1 };

// A field as the pass reads it: 48 bytes, three float4 on the device.
struct FieldRecord {
    float x0, y0, x1, y1;        // the region, as gpe_field has it
    float px, py, fx, fy;        // the pole / the uniform acceleration
    float strength, reach;
    float rr;                    // CIRCLE: x1 * x1, rounded once
    uint32_t code;               // shape | kind << 8 | falloff << 16
};

GPE_FIELD_FN uint32_t field_code(uint32_t shape, uint32_t kind, uint32_t falloff) { return shape | (kind << 8) | (falloff << 16); }
GPE_FIELD_FN uint32_t field_shape(uint32_t code) { return code & 0xFFu; }
GPE_FIELD_FN uint32_t field_kind(uint32_t code) { return (code >> 8) & 0xFFu; }
GPE_FIELD_FN uint32_t field_falloff(uint32_t code) { return (code >> 16) & 0xFFu; }

GPE_FIELD_FN float field_rr(float radius)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return radius * radius;
}

// Does the region (x0, y0, x1, y1 | rr) of shape `shape` hold the centre (cx, cy)?  A NaN coordinate matches
// EVERYWHERE alone.
GPE_FIELD_FN bool field_matches(uint32_t shape, float x0, float y0, float x1, float y1, float rr, float cx, float cy)
{
    if (shape == kFieldCircle) return region_in_disc(cx, cy, x0, y0, rr);
    if (shape == kFieldBox) return region_in_box(cx, cy, x0, y0, x1, y1);
    return true;
}

// What the matching fields of one particle have added up to so far.
struct FieldSum {
    float ax = 0.0f, ay = 0.0f;  // A
    float s = 1.0f;
    bool accel = false, drag = false;
};

// The contribution of a matching field to the particle at (cx, cy).
GPE_FIELD_FN void field_contribute(const FieldRecord &f, float cx, float cy, FieldSum &sum)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t kind = field_kind(f.code);
    if (kind == kFieldDrag) {
        sum.s = sum.s * f.strength;
        sum.drag = true;
        return;
    }
    float gx = f.fx, gy = f.fy;
    if (kind != kFieldUniform) {
        const float dx = f.px - cx;
        const float dy = f.py - cy;
        const float dxx = dx * dx;
        const float dyy = dy * dy;
        const float h = dxx + dyy;
        const float len = sqrtf(h);
        float w = f.strength;
        if (field_falloff(f.code) == kFalloffLinear) {
            const float t = len / f.reach;
            float w1 = 1.0f - t;
            w1 = (w1 > 0.0f) ? w1 : 0.0f;                      // NaN -> 0
            w = f.strength * w1;
        }
        if (!(len > 0.0f)) {
            // on the pole (or a NaN): nothing.  The mouse attractor of verlet_one divides by its zero length there and
            // yields NaN; a field does not.
            gx = 0.0f;
            gy = 0.0f;
        } else if (kind == kFieldRadial) {
            const float ux = dx / len;
            const float uy = dy / len;
            gx = ux * w;
            gy = uy * w;
        } else {
            const float ux = (-dy) / len;
            const float uy = dx / len;
            gx = ux * w;
            gy = uy * w;
        }
    }
    sum.ax = sum.ax + gx;
    sum.ay = sum.ay + gy;
    sum.accel = true;
}

// The new prev of a particle at c with prev q under the sum: drags first, accelerations second.  false: no field
// matched, q is untouched and nothing is to be stored.
GPE_FIELD_FN bool field_finish(const FieldSum &sum, float dt2, float cx, float cy, float *qx, float *qy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!sum.accel && !sum.drag) return false;
    float x = *qx, y = *qy;
    if (sum.drag) {                                            // the kick's GPE_VEL_SCALE
        const float vx = cx - x;
        const float vy = cy - y;
        const float wx = vx * sum.s;
        const float wy = vy * sum.s;
        x = cx - wx;
        y = cy - wy;
    }
    if (sum.accel) {                                           // the kick's GPE_VEL_ADD
        const float ex = sum.ax * dt2;
        const float ey = sum.ay * dt2;
        x = x - ex;
        y = y - ey;
    }
    *qx = x;
    *qy = y;
    return true;
}

}  // namespace gpe
