// mover_grid.h -- the host's part of the movers' lookup grid: which view a world and a radius bound get (host
// arithmetic only; gpe_movers.hip chooses it before every build, so gpe_set_world costs nothing), and the masks as the
// device builds them, for tests/cpp/mover_grid_tests.cpp.  Pure C++ (no HIP), like collider_grid.h; the listing rule
// itself is in k_mover.h, shared with the device.  Also what gpe_set_movers and gpe_set_mover_poses refuse, and what the
// host derives from a mover at set time, so that the test program can drive both without a device.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gpe.h"
#include "k_mover.h"
#include "k_mover_sweep.h"
#include "lookup_grid.h"

namespace gpe {

// Why gpe_set_movers refuses this mover, or NULL when it takes it.
inline const char *mover_refusal(const gpe_mover &q)
{
    if (!isfinite(q.ax) || !isfinite(q.ay) || !isfinite(q.bx) || !isfinite(q.by)) return "a coordinate is not finite";
    if (!isfinite(q.radius) || !(q.radius >= 0.0f)) return "a radius is NaN, infinite or negative";   // (-0.0 >= 0: accepted)
    if (q.kind != GPE_MOVER_LINEAR && q.kind != GPE_MOVER_ROTATE) return "unknown kind";
    if (q.flags || q.reserved) return "flags and reserved must be 0";
    if (!isfinite(q.vx) || !isfinite(q.vy) || !isfinite(q.travel) || !isfinite(q.px) || !isfinite(q.py) || !isfinite(q.omega))
        return "a motion value is not finite";
    if (q.travel < 0.0f) return "travel must not be negative";
    if (q.kind == GPE_MOVER_LINEAR) {
        float speed, ux, uy;
        mover_direction(q.vx, q.vy, &speed, &ux, &uy);
        if (!isfinite(speed)) return "a velocity's speed is not finite";
    }
    return nullptr;
}

// Why gpe_set_mover_poses refuses the state (q0, q1) for this mover, or NULL.
inline const char *mover_state_refusal(const gpe_mover &q, float q0, float q1)
{
    if (!isfinite(q0) || !isfinite(q1)) return "a state is not finite";
    if (q.kind == GPE_MOVER_LINEAR) {
        if (q1 != 1.0f && q1 != -1.0f) return "a LINEAR mover's q1 must be +1 or -1";
        if (q.travel > 0.0f && !(q0 >= 0.0f && q0 <= q.travel)) return "a LINEAR mover's q0 must lie in [0, travel]";
    }
    return nullptr;
}

// What the device holds of a validated mover (a radius of -0.0 becomes +0).
inline MoverDef mover_define(const gpe_mover &q)
{
    MoverDef d;
    memset(&d, 0, sizeof(d));
    d.ax = q.ax; d.ay = q.ay; d.bx = q.bx; d.by = q.by;
    d.radius = q.radius == 0.0f ? 0.0f : q.radius;
    d.kind = q.kind;
    if (q.kind == GPE_MOVER_LINEAR) {
        d.travel = q.travel;
        mover_direction(q.vx, q.vy, &d.rate, &d.ux, &d.uy);
    } else {
        d.rate = q.omega;
        d.ux = q.px; d.uy = q.py;
    }
    d.pad0 = mover_arm(d);                                             // (k_mover_sweep.h: the swept pass's gate and listing)
    return d;
}

inline void mover_limits_add(MoverLimits &L, const MoverDef &d)
{
    if (d.kind == kMoverRotate) {
        L.max_omega = std::max(L.max_omega, fabsf(d.rate));
    } else if (d.travel > 0.0f) {
        L.max_speed = std::max(L.max_speed, d.rate);
        L.min_travel = L.bounded ? std::min(L.min_travel, d.travel) : d.travel;
        L.bounded = true;
    }
}

// Why a step of dt is refused for these limits, or NULL.
inline const char *mover_dt_refusal(const MoverLimits &L, float dt)
{
    if (!isfinite(dt)) return "dt is not finite (the context holds moving colliders)";
    if (!(fabsf(L.max_omega * dt) <= kMoverMaxTurn)) return "|omega * dt| must be at most 0.5 for every rotating mover";
    if (L.bounded && !(fabsf(L.max_speed * dt) <= L.min_travel))
        return "speed * |dt| must be at most travel for every mover that goes back and forth";
    return nullptr;
}

// The grid of one cell: every mover, whatever the world and rb are (lookup_grid.h).
inline MoverGridView mover_grid_one_cell(float rb, double extent)
{
    const LookupView v = lookup_grid_one_cell(rb, extent);
    MoverGridView g;
    g.view = v.view;
    g.cell = v.cell;
    return g;
}

// The view for the radius bound rb = |gpe_max_radius| and the world W x H, all as the context holds them (anything
// goes).  The chooser of lookup_grid.h with at most kMoverGridMaxDim cells per axis: cells of max(4 rb, max(W, H) / 128),
// doubled until both axes fit.  A mask has no capacity, so the first fit is taken.
inline MoverGridView mover_grid_choose(float rb_in, float W, float H)
{
    const LookupView v = lookup_grid_choose(fabsf(rb_in), W, H, kMoverGridMaxDim, 1e-20, [](const LookupView &) { return true; });
    MoverGridView g;
    g.view = v.view;
    g.cell = v.cell;
    return g;
}

inline uint32_t mover_mask_words(uint32_t k) { return (k + 63u) / 64u; }

// The masks of k posed capsules caps[4 j ..] with radii R[j], as k_movers_build sets them: masks[cell * words + w],
// summary[cell].  Returns the (cell, mover) bits set.
inline uint64_t mover_grid_fill(const MoverGridView &g, const float *caps, const float *R, uint32_t k, float rb,
                                std::vector<uint64_t> &masks, std::vector<uint32_t> &summary)
{
    const uint32_t gx = g.view.gx, gy = g.view.gy, words = mover_mask_words(k);
    masks.assign((size_t)gx * gy * words, 0);
    summary.assign((size_t)gx * gy, 0);
    uint64_t listed = 0;
    for (uint32_t j = 0; j < k; ++j) {
        uint32_t x0, y0, x1, y1;
        bool everywhere;
        if (!mover_cell_rect(g, caps + 4 * j, R[j], rb, &x0, &y0, &x1, &y1, &everywhere)) continue;
        for (uint32_t cy = y0; cy <= y1; ++cy)
            for (uint32_t cx = x0; cx <= x1; ++cx) {
                if (!everywhere && !mover_listed(g, caps + 4 * j, R[j], rb, cx, cy)) continue;
                const size_t cell = (size_t)cy * gx + cx;
                masks[cell * words + j / 64] |= 1ull << (j % 64);
                summary[cell] |= 1u << (j / 64);
                listed += 1;
            }
    }
    return listed;
}

}  // namespace gpe
