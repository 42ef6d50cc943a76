// lookup_grid_tests.cpp -- what the lookup grids of the colliders, the fields and the movers share on the host
// (gpu-physics-engine_amd/csrc/lookup_grid.h), on the CPU: the resolution chooser at the three parameter sets against
// its closed form, the grid of one cell, and the CSR builder against a brute-force list per cell.  No HIP, no library:
// the header alone.
//
// usage: lookup_grid_tests [--list]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/lookup_grid.h"

using namespace gpe;

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { if (++g_failures < 20) std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

struct Params { const char *who; float rb; uint32_t dim; double min_world; };
const Params kParams[] = {
    {"colliders", 0.5f, 1024, 1e-20},      // cells of max(4 rb, world / 1024), at most 1024 per axis
    {"fields", 0.0f, 1024, 1e-6},          // cells of world / 1024
    {"movers", 0.5f, 128, 1e-20},          // cells of max(4 rb, world / 128), at most 128 per axis
};

bool same_bits(float a, float b) { return bits_of(a) == bits_of(b); }

// the one cell: no list but "every item"; a normal reciprocal of the extent, or 0
void check_one_cell(const LookupView &v, float rb, double extent)
{
    CHECK(v.view.gx == 1 && v.view.gy == 1 && v.view.gxf == 1.0f && v.view.gyf == 1.0f);
    CHECK(same_bits(v.view.rb, rb));
    const float inv = 1.0f / (float)extent;
    const bool usable = extent > 0.0 && std::isfinite((float)extent) && std::isfinite(inv) && inv >= 1e-30f;
    CHECK(same_bits(v.view.inv_cell, usable ? inv : 0.0f));
    CHECK(v.cell == (usable ? 1.0 / (double)inv : 1.0));
}

// The closed form.  A usable world gets cells of want0 * 2^m, want0 = max(4 rb, max(W, H) / dim), for the smallest m >= 0
// at which both axes have at most dim cells, skipping the first `refused` fits; the cell is the reciprocal of the
// binary32 reciprocal of that size and an axis has floor(extent / cell) + 1 cells.  One cell on both axes: the one cell.
void check_choice(const LookupView &v, const Params &p, float rb, float W, float H, int refused = 0)
{
    const double w = W, h = H, world = w < h ? h : w;                         // (a NaN width is the world: no usable one)
    const bool usable = w > 0.0 && h > 0.0 && std::isfinite(world) && std::isfinite(rb) && world >= p.min_world && world <= 1e20;
    if (!usable) {
        check_one_cell(v, rb, world > 0.0 && std::isfinite(world) ? 2.0 * world : 0.0);
        return;
    }
    const double want0 = std::fmax(4.0 * (double)rb, world / (double)p.dim);
    for (int m = 0; m < 200; ++m) {
        const float inv = 1.0f / (float)std::ldexp(want0, m);
        const double cell = 1.0 / (double)inv;
        const double nx = std::floor(w / cell) + 1.0, ny = std::floor(h / cell) + 1.0;
        if (nx <= 1.0 && ny <= 1.0) break;
        if (nx > (double)p.dim || ny > (double)p.dim) continue;
        if (refused-- > 0) continue;
        CHECK(same_bits(v.view.inv_cell, inv) && v.cell == cell);
        CHECK(v.view.gx == (uint32_t)nx && v.view.gy == (uint32_t)ny);
        CHECK(v.view.gxf == (float)v.view.gx && v.view.gyf == (float)v.view.gy);
        CHECK(same_bits(v.view.rb, rb));
        CHECK(w < (double)v.view.gx * cell && h < (double)v.view.gy * cell);     // the world lies strictly inside
        return;
    }
    check_one_cell(v, rb, 2.0 * world);
}

LookupView choose(const Params &p, float rb, float W, float H, int refuse = 0)
{
    return lookup_grid_choose(rb, W, H, p.dim, p.min_world, [&](const LookupView &) { return refuse-- <= 0; });
}

void test_chooser_worlds()
{
    const float worlds[][2] = {{200.0f, 200.0f}, {3048.0f, 1048.0f}, {1e6f, 10.0f}, {10.0f, 1e6f}, {200.0f, kInf},
                               {1e-3f, 1e-3f}, {1e-7f, 1e-7f}, {0.0f, 0.0f}, {200.0f, 0.0f}, {-5.0f, 200.0f},
                               {kNaN, 200.0f}, {200.0f, kNaN}, {1e21f, 1e21f}, {1e21f, 1.0f}, {1e20f, 1e20f},
                               {1e-25f, 1e-25f}, {0.37f, 977.3f}};
    for (const Params &p : kParams)
        for (const auto &wh : worlds) check_choice(choose(p, p.rb, wh[0], wh[1]), p, p.rb, wh[0], wh[1]);
    // what the three sets make of one world: 200 / 1024 is under 4 * 0.5, 200 / 128 is not
    CHECK(choose(kParams[0], 0.5f, 200.0f, 200.0f).view.gx == 101);             // cells of 2
    CHECK(choose(kParams[1], 0.0f, 200.0f, 200.0f).view.gx == 1024);            // cells of 200 / 1024, one doubling short
    CHECK(choose(kParams[2], 0.5f, 200.0f, 200.0f).view.gx == 101);
    CHECK(choose(kParams[2], 0.001f, 200.0f, 200.0f).view.gx <= 128);
    // a world under the fields' smallest, over the others': one cell there, a grid here
    CHECK(choose(kParams[1], 0.0f, 1e-7f, 1e-7f).view.gx == 1);
    CHECK(choose(kParams[0], 0.0f, 1e-7f, 1e-7f).view.gx > 1);
}

void test_chooser_radius_bounds()
{
    for (const Params &p : kParams)
        for (float rb : {0.0f, kInf, kNaN, 1e-4f, 3.0f, 1e6f})
            for (const auto &wh : {std::pair<float, float>(200.0f, 200.0f), std::pair<float, float>(3048.0f, 1048.0f)})
                check_choice(choose(p, rb, wh.first, wh.second), p, rb, wh.first, wh.second);
    // rb over the world: four radii span it, one cell
    CHECK(choose(kParams[0], 1e6f, 200.0f, 200.0f).view.gx == 1);
}

void test_chooser_retries()
{
    for (const Params &p : kParams)
        for (int refuse : {1, 2, 5, 100}) {
            check_choice(choose(p, p.rb, 3048.0f, 1048.0f, refuse), p, p.rb, 3048.0f, 1048.0f, refuse);
            check_choice(choose(p, 0.0f, 1e-3f, 1e-3f, refuse), p, 0.0f, 1e-3f, 1e-3f, refuse);
        }
    CHECK(choose(kParams[0], 0.5f, 200.0f, 200.0f, 100).view.gx == 1);          // every resolution refused: the one cell
    int asked = 0;
    (void)lookup_grid_choose(0.5f, kNaN, 200.0f, 1024, 1e-20, [&](const LookupView &) { ++asked; return true; });
    CHECK(asked == 0);                                                           // no usable world: nothing is tried
}

// membership[j][cell] -> the runs cells_of names, row by row; a full grid as one run
struct Membership {
    uint32_t gx, gy;
    std::vector<std::vector<uint8_t>> in;
    template <class Emit>
    void cells_of(uint32_t j, Emit emit) const
    {
        const std::vector<uint8_t> &m = in[j];
        const uint64_t cells = (uint64_t)gx * gy;
        bool full = true;
        for (uint8_t b : m) full = full && b;
        if (full) { emit(0, cells - 1); return; }
        for (uint32_t cy = 0; cy < gy; ++cy)
            for (uint32_t cx = 0; cx < gx; ++cx) {
                if (!m[(size_t)cy * gx + cx]) continue;
                uint32_t end = cx;
                while (end + 1 < gx && m[(size_t)cy * gx + end + 1]) ++end;
                if (!emit((uint64_t)cy * gx + cx, (uint64_t)cy * gx + end)) return;
                cx = end;
            }
    }
    uint64_t total() const
    {
        uint64_t t = 0;
        for (const auto &m : in) for (uint8_t b : m) t += b;
        return t;
    }
};

// the table against the list of every cell made the slow way
void check_fill(const Membership &M, uint64_t max_entries, bool fits)
{
    LookupGrid g;
    g.view.gx = M.gx; g.view.gy = M.gy;
    const uint32_t k = (uint32_t)M.in.size();
    const bool ok = lookup_grid_fill(g, k, max_entries, [&](uint32_t j, auto emit) { M.cells_of(j, emit); });
    CHECK(ok == fits);
    if (!ok || !fits) return;
    const size_t cells = (size_t)M.gx * M.gy;
    CHECK(g.cell_start.size() == cells + 1 && g.cell_start[0] == 0 && g.items.size() == M.total());
    if (g.cell_start.size() != cells + 1 || g.items.size() != M.total()) return;
    for (size_t c = 0; c < cells; ++c) {
        std::vector<uint32_t> want;
        for (uint32_t j = 0; j < k; ++j) if (M.in[j][c]) want.push_back(j);
        CHECK(g.cell_start[c] <= g.cell_start[c + 1] && g.cell_start[c + 1] <= g.items.size());
        if (!(g.cell_start[c] <= g.cell_start[c + 1] && g.cell_start[c + 1] <= g.items.size())) return;
        CHECK(std::vector<uint32_t>(g.items.begin() + g.cell_start[c], g.items.begin() + g.cell_start[c + 1]) == want);
    }
}

Membership membership(uint32_t gx, uint32_t gy, uint32_t k) { return {gx, gy, std::vector<std::vector<uint8_t>>(k, std::vector<uint8_t>((size_t)gx * gy, 0))}; }

void test_fill_small()
{
    check_fill(membership(5, 3, 0), 100, true);                                  // no items
    check_fill(membership(1, 1, 0), 0, true);
    Membership one = membership(5, 3, 1);                                        // one item in one cell
    one.in[0][7] = 1;
    check_fill(one, 100, true);
    check_fill(one, 1, true);
    check_fill(one, 0, false);
    Membership all = membership(7, 4, 3);                                        // an item in every cell, among others
    for (uint8_t &b : all.in[1]) b = 1;
    all.in[0][0] = all.in[0][27] = all.in[2][27] = all.in[2][13] = 1;
    check_fill(all, 100, true);
}

void test_fill_random_and_cut()
{
    std::mt19937 rng(20250712u);
    for (int round = 0; round < 40; ++round) {
        const uint32_t gx = 1 + rng() % 17, gy = 1 + rng() % 9, k = rng() % 24;
        Membership M = membership(gx, gy, k);
        for (auto &m : M.in) {
            const uint32_t density = rng() % 5;                                  // 0: empty ... 4: every cell
            for (uint8_t &b : m) b = density == 4 || (rng() % 4) < density;
        }
        const uint64_t total = M.total();
        check_fill(M, 1u << 20, true);
        check_fill(M, total, true);                                              // the cut exactly at the total
        if (total > 0) check_fill(M, total - 1, false);                          // the total one above the cut
        if (total > 3) check_fill(M, total / 2, false);
    }
}

// the build: the first resolution whose lists fit, else the one cell with every item
void test_build_retries_to_one_cell()
{
    const uint32_t k = 5;
    uint32_t gx = 0, gy = 0;
    int prepared = 0;
    auto prepare = [&](const LookupView &v) { gx = v.view.gx; gy = v.view.gy; ++prepared; };
    auto everywhere = [&](uint32_t, auto emit) { emit(0, (uint64_t)gx * gy - 1); };
    // every item in every cell: k * cells entries fit once the grid is small enough
    const LookupGrid g = lookup_grid_build(k, 0.5f, 200.0f, 100.0f, 1024, 1e-20, 400, prepare, everywhere);
    CHECK(prepared > 1 && (uint64_t)g.view.gx * g.view.gy * k <= 400 && g.view.gx > 1);
    CHECK(g.items.size() == (size_t)g.view.gx * g.view.gy * k && g.cell_start.size() == (size_t)g.view.gx * g.view.gy + 1);
    check_choice(g, kParams[0], 0.5f, 200.0f, 100.0f, prepared - 1);
    // nothing fits: the one cell
    const LookupGrid one = lookup_grid_build(k, 0.5f, 200.0f, 100.0f, 1024, 1e-20, 3, prepare, everywhere);
    check_one_cell(one, 0.5f, 400.0);
    CHECK(one.cell_start == std::vector<uint32_t>({0u, k}) && one.items == std::vector<uint32_t>({0u, 1u, 2u, 3u, 4u}));
    // no usable world: the one cell without a try
    prepared = 0;
    const LookupGrid none = lookup_grid_build(k, 0.5f, kNaN, 100.0f, 1024, 1e-20, 1u << 20, prepare, everywhere);
    check_one_cell(none, 0.5f, 0.0);
    CHECK(prepared == 0 && none.items.size() == k);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"chooser_worlds", test_chooser_worlds},
    {"chooser_radius_bounds", test_chooser_radius_bounds},
    {"chooser_retries", test_chooser_retries},
    {"fill_small", test_fill_small},
    {"fill_random_and_cut", test_fill_random_and_cut},
    {"build_retries_to_one_cell", test_build_retries_to_one_cell},
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
