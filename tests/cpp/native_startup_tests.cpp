// native_startup_tests.cpp -- the start of a freshly configured context in the native step's launch heuristics
// (gpu-physics-engine_amd/csrc/native_policy.h): no half-tile launch and the small over-capacity grid until a tile has
// been reported, unless the scene was dense when it was configured.  Driven step by step on the CPU with literal
// numbers, beside native_policy_tests.cpp (which pins the transitions that were there before).
//
// usage: native_startup_tests [--list]
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/native_policy.h"

using namespace gpe;

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { ++g_failures; std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

NativeStats quiet() { return NativeStats(); }

// a policy as native_configure leaves it: configure, then admit with the measured window population
NativePolicy configured(uint32_t window_max)
{
    NativePolicy p;
    p.configure(0);
    CHECK(p.admit(window_max, false));
    return p;
}

void test_quiet_context_from_step_one()
{
    NativePolicy p = configured(512);          // kWindowQuietStart itself is still thin
    CHECK(!p.handed_on_seen && p.quiet_steps == 0 && p.dense_quiet == 0xFFFFFFFFu);
    for (int i = 1; i <= 200; ++i) {
        const OverflowPlan o = p.overflow(quiet(), 0, true, false, 1u << 20);
        CHECK(o.halves_grid == 0);             // no half-tile launch, not even on step one
        CHECK(o.overflow_grid == 128);         // the 128-workgroup grid from step one
    }
    CHECK(p.quiet_steps == 200 && p.dense_quiet == 0xFFFFFFFFu && !p.handed_on_seen);
    // above 4 M particles the small grid is never taken, quiet or not
    CHECK(configured(0).overflow(quiet(), 0, true, false, (4ull << 20) + 1).overflow_grid == 1024);
    CHECK(configured(0).overflow(quiet(), 0, true, false, 4ull << 20).overflow_grid == 128);
}

void test_first_reported_tile_brings_both_back()
{
    NativePolicy p = configured(100);
    for (int i = 1; i <= 10; ++i) p.overflow(quiet(), 0, true, false, 1000);
    NativeStats s;
    s.overflow = 1;                            // one tile handed on (no front workgroups: any tile counts)
    OverflowPlan o = p.overflow(s, 0, true, false, 1000);
    CHECK(o.halves_grid == 64 && o.overflow_grid == 1024);
    CHECK(p.handed_on_seen && p.quiet_steps == 0 && p.dense_quiet == 0);
    for (int i = 1; i <= 31; ++i) {            // ... and from there on the counters are what they always were
        o = p.overflow(quiet(), 0, true, false, 1000);
        CHECK(o.halves_grid == 64 && o.overflow_grid == 1024);
    }
    o = p.overflow(quiet(), 0, true, false, 1000);                       // quiet_steps 32
    CHECK(o.halves_grid == 0 && o.overflow_grid == 1024);
    for (int i = 33; i <= 96; ++i) CHECK(p.overflow(quiet(), 0, true, false, 1000).overflow_grid == 1024);
    CHECK(p.overflow(quiet(), 0, true, false, 1000).overflow_grid == 128);   // dense_quiet 97
    CHECK(p.handed_on_seen);
}

void test_halves_over_alone_brings_the_grid_back()
{
    NativePolicy p = configured(0);
    NativeStats s;
    s.halves_over = 1;                         // list 2 had an entry: the full grid, but no tile was handed on
    const OverflowPlan o = p.overflow(s, 0, true, false, 1000);
    CHECK(o.overflow_grid == 1024 && o.halves_grid == 0 && !p.handed_on_seen && p.dense_quiet == 0);
}

void test_with_front_workgroups_hinted_tiles_do_not_count()
{
    NativePolicy p = configured(0);
    NativeStats s;
    s.overflow = 50;                           // all hinted: the dense launch handed nothing on itself
    for (int i = 1; i <= 5; ++i) p.overflow(s, 128, true, false, 1000);
    CHECK(!p.handed_on_seen && p.dense_quiet == 0xFFFFFFFFu);
    s.overflow_new = 2;
    p.overflow(s, 128, true, false, 1000);
    CHECK(p.handed_on_seen && p.dense_quiet == 0);
    // the front workgroups gone: the half-tile launch is wanted at once, as the counters say
    CHECK(p.overflow(quiet(), 0, true, false, 1000).halves_grid == 64);
}

void test_dense_configuration_starts_as_before()
{
    NativePolicy p = configured(513);          // kWindowQuietStart + 1
    CHECK(p.handed_on_seen && p.quiet_steps == 0 && p.dense_quiet == 0);
    for (int i = 1; i <= 32; ++i) {
        const OverflowPlan o = p.overflow(quiet(), 0, true, false, 1000);
        CHECK(o.halves_grid == (i < 32 ? 64u : 0u));                      // the half-tile launch for 31 steps: quiet_steps < 32
        CHECK(o.overflow_grid == 1024);
    }
    for (int i = 33; i <= 96; ++i) CHECK(p.overflow(quiet(), 0, true, false, 1000).overflow_grid == 1024);
    CHECK(p.overflow(quiet(), 0, true, false, 1000).overflow_grid == 128);   // dense_quiet 97
    // a scene too dense for the native path is not admitted, and is marked dense all the same
    NativePolicy q;
    q.configure(0);
    CHECK(!q.admit(24577, false) && q.handed_on_seen && q.dense_quiet == 0);
}

void test_configure_resets_the_member()
{
    NativePolicy p = configured(0);
    NativeStats s;
    s.overflow = 3;
    p.overflow(s, 0, true, false, 1000);
    CHECK(p.handed_on_seen && p.dense_quiet == 0);
    p.configure(5);
    CHECK(!p.handed_on_seen && p.quiet_steps == 0);
    CHECK(p.dense_quiet == 0);                 // carries over: the lists had an entry one step ago
    CHECK(p.admit(512, false) && !p.handed_on_seen);
    OverflowPlan o = p.overflow(quiet(), 0, true, false, 1000);
    CHECK(o.halves_grid == 0 && o.overflow_grid == 1024);                // no half-tile launch; the grid as the counter says
    p.configure(5);
    CHECK(p.admit(600, false) && p.handed_on_seen);                      // reconfigured on a dense scene
    o = p.overflow(quiet(), 0, true, false, 1000);
    CHECK(o.halves_grid == 64 && o.overflow_grid == 1024);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"quiet_context_from_step_one", test_quiet_context_from_step_one},
    {"first_reported_tile_brings_both_back", test_first_reported_tile_brings_both_back},
    {"halves_over_alone_brings_the_grid_back", test_halves_over_alone_brings_the_grid_back},
    {"with_front_workgroups_hinted_tiles_do_not_count", test_with_front_workgroups_hinted_tiles_do_not_count},
    {"dense_configuration_starts_as_before", test_dense_configuration_starts_as_before},
    {"configure_resets_the_member", test_configure_resets_the_member},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (const Test &t : kTests) std::printf("%s\n", t.name);
        return 0;
    }
    int failed = 0;
    for (const Test &t : kTests) {
        const int before = g_failures;
        t.fn();
        const bool ok = g_failures == before;
        failed += ok ? 0 : 1;
        std::printf("test %s ... %s\n", t.name, ok ? "ok" : "FAILED");
    }
    std::printf("%d of %zu failed\n", failed, kTests.size());
    return failed == 0 ? 0 : 1;
}
