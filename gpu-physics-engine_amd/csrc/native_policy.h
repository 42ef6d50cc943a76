// native_policy.h -- the native step's launch heuristics (gpe_native.hip), apart from the launches they steer.
// Plain C++17, no HIP header: tests/cpp/native_policy_tests.cpp drives it step by step on the CPU.
//
// The tiles report statistics to pinned host words (gpe_internal.h kStat*), asynchronously: what the host reads lags
// by the steps still in flight (gpe_run bounds that).  Every call below takes one snapshot of them (NativeStats) and
// answers with a plain plan; the step functions do what the plan says.  Every form the heuristics choose is exact:
// they decide the speed of a step, never its result.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace gpe {

constexpr uint32_t kHintMax = 64;              // hinted tiles per dense launch (the front workgroups take two halves each)
constexpr uint64_t kArenaMaxSlots = 1ull << 30; // the arena's slot numbers are 32 bit; 40 GB of the 288 GB
// Windows beyond the 8x8 sub-tile's 1536 slots take their arrays from the spill arena; with the cells of up to
// 64 members resolved by whole waves that is faster than the compat kernels for the piles gravity builds (4 M
// particles, windows up to ~2900, cells up to ~53 members: 2.2 ms/step against 3.75).  Far denser blobs (mouse
// attraction: thousands per cell) are one-lane O(n^2) work that the overlapping windows would repeat: those leave
// the native path.
#ifndef GPE_WINDOW_HANDOVER
#define GPE_WINDOW_HANDOVER 16384
#endif
constexpr uint32_t kWindowHandover = GPE_WINDOW_HANDOVER;              // above it the context leaves the native path
constexpr uint32_t kWindowEligible = GPE_WINDOW_HANDOVER * 3 / 2;      // a scene whose windows exceed this never enters it
// A scene whose largest 24x24-cell window holds at most this many particles when it is configured starts without the
// precautionary launches (admit).  The population above which the tiles report a window (kWindowReport, k_native.hip):
// 2.3 x the mean of the benchmark density; a direct-slot tile runs over around 350 per window.
constexpr uint32_t kWindowQuietStart = 512;

// One reading of the pinned words (native_read_stats).
struct NativeStats {
    uint32_t window_max = 0;     // kStatWindowMax: largest 24x24-cell window population of the last native step
    uint32_t arena = 0;          // kStatArena: spill-arena slots it handed out
    uint32_t probe = 0;          // kStatProbe: window population the last asynchronous probe measured + 1 (0: none yet)
    uint32_t overflow = 0;       // kStatOverflow: 32x32 tiles over capacity, hinted ones included
    uint32_t sub_tiles = 0;      // kStatSubTiles (diagnostics)
    uint32_t spills = 0;         // kStatSpills (diagnostics)
    uint32_t sorts = 0;          // kStatSorts: running count of steps whose radix passes ran
    uint32_t overflow_new = 0;   // kStatOverflowNew: ... of `overflow`, the tiles the dense launch handed on itself
    uint32_t halves_over = 0;    // kStatHalvesOver: halves handed on to the over-capacity launch
};

// run(): take the native kernels this step?  The step function grows the arena and writes the handshake words.
struct RunPlan {
    bool run = false;
    uint64_t grow_arena = 0;     // reserve this many arena slots first; run() was told whether that worked
    bool arena_reset = false;    // kStatArena = 0 (after the growth)
    bool readmitted = false;     // a run that must stay native is back on it (reason NONE)
    bool hand_over = false;      // windows above kWindowHandover: to the compat kernels (reason DENSE_WINDOWS), kStatProbe = 0
    bool resume = false;         // the last probe found the windows thin again (reason NONE): kStatWindowMax = probe - 1, kStatProbe = 0
    bool probe = false;          // kStatProbe = 0 and enqueue a probe
};

// prepare(): the sort and histogram choices of native_prepare_step
struct PreparePlan {
    bool keep_table = false;     // the radix passes may keep the block table (the step function adds what it knows)
    bool fuse_hist = false;      // the hash kernel counts the radix digits, not the gated launch
};

// hints(): the dense launch's front workgroups
struct HintPlan {
    bool hints_on = false;       // tiles register hints (CollideArgs::hints_on)
    uint32_t front_wgs = 0;      // front workgroups of the dense launch (0 or 2 x kHintMax)
};

// overflow(): the launches behind the dense one
struct OverflowPlan {
    uint32_t halves_grid = 0;    // grid of the half-tile launch (0: it does not run)
    uint32_t overflow_grid = 0;  // grid of the over-capacity launch (128 or 1024)
};

struct NativePolicy {
    bool eligible = false;           // every particle inside the world box, grid small enough, windows not over-dense
    bool dense_hold = false;         // left the native path because windows were filling up
    uint32_t steps_since_check = 0;  // ... steps since the last probe
    uint32_t sort_hold = 0;          // steps left that sort unconditionally (the scene sorted on most steps anyway)
    uint32_t watch_steps = 0, watch_sorts = 0;   // the passes' counter over the current 64-step window
    bool watch_valid = false;
    bool hist_fused = false;         // the hash kernel counts the radix digits (most recent steps sorted), not the gated launch
    uint32_t hist_watch_steps = 0, hist_watch_sorts = 0;
    bool crowded = false;            // many tiles run over the direct-slot form: the dense launch uses the counting-sort form
    uint32_t calm_steps = 0;         // steps without an over-capacity tile or a crowded window while `crowded`
    uint32_t hint_quiet = 0xFFFFFFFFu; // native steps since a tile last ran over, hinted ones included (lagged): the dense launch's front workgroups
    uint32_t quiet_steps = 0;        // native steps since the dense launch last handed a tile on itself (lagged)
    bool handed_on_seen = false;     // ... and it has done so since the last configuration (or the scene was dense then)
    uint32_t new_streak = 0;         // consecutive native steps whose (lagged) list 1 was not empty
    uint32_t dense_quiet = 0xFFFFFFFFu; // native steps since list 1 or list 2 last had an entry (lagged): the over-capacity launch's grid

    // native_configure, before anything is measured.  sorts: the passes' counter as last published (the histogram
    // window counts from it).  (hint_quiet, new_streak, dense_quiet and calm_steps carry over.)
    void configure(uint32_t sorts)
    {
        eligible = false;
        dense_hold = false;
        steps_since_check = 0;
        quiet_steps = 0;
        handed_on_seen = false;
        crowded = false;
        hist_fused = false; hist_watch_steps = 0; hist_watch_sorts = sorts;
        sort_hold = 0; watch_steps = 0; watch_valid = false;
    }

    // native_configure, once the box check passed and the windows are measured (force: GPE_FLAG_NATIVE_FORCE).
    // The statistics lag: the host may be ~64 steps ahead of the first report.  A scene whose windows are thin now
    // (at most kWindowQuietStart) runs those steps without the precautionary launches -- no half-tile launch before a tile
    // has been handed on, the small over-capacity grid while the lists have never had an entry; a scene that is dense
    // from the start takes both from its first step.
    bool admit(uint32_t window_max, bool force)
    {
        if (window_max > kWindowQuietStart) { handed_on_seen = true; dense_quiet = 0; }
        eligible = window_max <= kWindowEligible || force;
        return eligible;
    }

    // native_should_run.  must_stay: the run needs the native kernels (forced, or order keys), density alone never
    // stops it.  reserve(slots) grows the spill arena (one synchronisation) and says whether it did; a run that may
    // leave does not take this step when it could not.  A held context probes the state every 256 steps and returns
    // when the windows have thinned out to 3/4 of the handover population.
    template <class Reserve>
    RunPlan run(const NativeStats &s, bool must_stay, bool in_box, uint64_t arena_cap, Reserve &&reserve)
    {
        RunPlan p;
        if (!eligible && must_stay && in_box) { eligible = true; dense_hold = false; p.readmitted = true; }
        if (eligible) {
            if ((uint64_t)s.arena * 2 > arena_cap && arena_cap < kArenaMaxSlots) {
                p.grow_arena = std::min<uint64_t>(arena_cap * 2, kArenaMaxSlots);
                if (!reserve(p.grow_arena) && !must_stay) return p;
                p.arena_reset = true;
            }
            if (!must_stay && s.window_max > kWindowHandover) {
                eligible = false;
                dense_hold = true;
                steps_since_check = 0;
                p.hand_over = true;
            }
            p.run = eligible;
            return p;
        }
        if (dense_hold) {
            if (s.probe != 0 && s.probe - 1u <= kWindowHandover * 3 / 4) {
                dense_hold = false;
                eligible = true;
                p.resume = p.run = true;
                return p;
            }
            if (++steps_since_check >= 256) {
                steps_since_check = 0;
                p.probe = true;
            }
        }
        return p;
    }

    // native_prepare_step.  always_sort: a configuration-time probe, which must not rely on the kept grouping (it skips
    // the sort-hold window but still advances the histogram window); sort_every_step: GPE_FLAG_SORT_EVERY_STEP;
    // fused_flag: GPE_FLAG_FUSED_HISTOGRAMS.
    // Sort hold: when three quarters of the last 64 steps sorted, the next 256 steps sort unconditionally.  While the
    // hold lasts every step sorts by decree, which says nothing about the scene: when it ends the count starts afresh
    // (one window for the lagged counter to settle, one to judge).
    // Fused histograms: while at least a quarter of the last 16 steps sorted.
    PreparePlan prepare(const NativeStats &s, bool always_sort, bool sort_every_step, bool fused_flag)
    {
        if (!always_sort) {
            if (sort_hold > 0) {
                if (--sort_hold == 0) { watch_steps = 0; watch_valid = false; }
            } else if (++watch_steps >= 64) {
                if (watch_valid && s.sorts - watch_sorts >= 48) sort_hold = 256;
                watch_sorts = s.sorts; watch_steps = 0; watch_valid = true;
            }
        }
        PreparePlan p;
        p.keep_table = !always_sort && !sort_every_step && sort_hold == 0;
        if (++hist_watch_steps >= 16) {
            hist_fused = (s.sorts - hist_watch_sorts) * 4u >= hist_watch_steps;
            hist_watch_sorts = s.sorts; hist_watch_steps = 0;
        }
        p.fuse_hist = hist_fused || fused_flag;
        return p;
    }

    // native_collide: does the dense launch take the counting-sort form?  Once more than 2 % (+4) of the `total` tiles
    // ran over; back to direct slots after 64 steps without a tile over capacity or a window above kWindowReport.
    // counting_flag: GPE_FLAG_COUNTING_SORT_TILES; ghosts_looked_up: order-key windows without ghost lists, which only
    // the counting-sort form serves.
    bool counting_sort(const NativeStats &s, uint32_t total, bool counting_flag, bool ghosts_looked_up)
    {
        if (!crowded) {
            if (s.overflow > total / 50u + 4u) { crowded = true; calm_steps = 0; }
        } else {
            calm_steps = (s.overflow == 0 && s.window_max == 0) ? calm_steps + 1 : 0;
            if (calm_steps >= 64) crowded = false;
        }
        return counting_flag || crowded || ghosts_looked_up;
    }

    // native_collide, direct-slot dense launches that do not split the tile grid only.  With rosters, up to 8 M
    // particles and without GPE_FLAG_NO_HALF_TILES; front workgroups while tiles ran over in the last 32 steps and the
    // front workgroups can take them.
    HintPlan hints(const NativeStats &s, bool rosters, bool no_half_tiles, uint64_t n)
    {
        HintPlan p;
        if (!rosters || no_half_tiles || n > (8ull << 20)) return p;
        p.hints_on = true;
        if (s.overflow != 0 && s.overflow <= 2u * kHintMax) hint_quiet = 0; else if (hint_quiet < 0xFFFFFFFFu) ++hint_quiet;
        if (hint_quiet < 32u && s.overflow <= 2u * kHintMax) p.front_wgs = 2u * kHintMax;
        return p;
    }

    // native_collide, after the dense launch.  front_wgs: what hints() chose (0 when it was not asked); direct_form:
    // the dense launch ran direct-slot tiles.  The half-tile launch runs behind direct-slot tiles only: with front
    // workgroups after 4 steps in a row that handed tiles on, without them while tiles were handed on in the last 32
    // steps (and, since the last configuration, only once a tile has been handed on or when the scene was dense then:
    // admit).  The over-capacity launch takes 128 workgroups up to 4 M particles while the lists have been empty for
    // 96 steps -- or have never had an entry -- or, with front workgroups, held at most 128 work items; else 1024.
    OverflowPlan overflow(const NativeStats &s, uint32_t front_wgs, bool direct_form, bool no_half_tiles, uint64_t n)
    {
        const uint32_t handed_on = front_wgs ? s.overflow_new : s.overflow;
        if (handed_on != 0) { quiet_steps = 0; handed_on_seen = true; }
        else if (quiet_steps < 0xFFFFFFFFu) ++quiet_steps;
        if (s.overflow_new != 0 || s.halves_over != 0 || (!front_wgs && s.overflow != 0)) dense_quiet = 0;
        else if (dense_quiet < 0xFFFFFFFFu) ++dense_quiet;
        if (s.overflow_new != 0) { if (new_streak < 0xFFFFFFFFu) ++new_streak; } else new_streak = 0;
        OverflowPlan p;
        const bool halves_wanted = front_wgs ? new_streak >= 4u : (handed_on_seen && quiet_steps < 32u);
        if (direct_form && halves_wanted && !no_half_tiles)
            p.halves_grid = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(64, 2ull * handed_on + 32));
        const uint64_t items = 4ull * s.overflow_new + 2ull * s.halves_over;
        const bool small_grid = n <= (4ull << 20) && (dense_quiet > 96 || (front_wgs != 0u && items <= 128u));
        p.overflow_grid = small_grid ? 128u : 1024u;
        return p;
    }
};

}  // namespace gpe
