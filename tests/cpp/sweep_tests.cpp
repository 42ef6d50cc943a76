// sweep_tests.cpp -- the swept colliders' rule as C++ states it (csrc/k_sweep.h over csrc/k_collider.h and
// csrc/k_surface.h), stand-alone: its own main, no HIP header, no GPU.  tests/test_sweep_cpu.py compiles it with
//   g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror
// once plain and once with -fsanitize=address,undefined, and runs it on the table the numpy model wrote
// (tests/golden/sweep_cases.txt: tests/_sweep_model.table_text()).  Every case is replayed bit for bit, by brute force
// over the table's colliders, without surfaces and with them.
//
// usage: sweep_tests [--list] [path of sweep_cases.txt]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/k_sweep.h"

using namespace gpe;

namespace {

int g_failures = 0;
const char *g_table = "tests/golden/sweep_cases.txt";

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { if (++g_failures < 20) std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

float from_bits(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

bool same(float got, uint32_t want)                            // the same bits, or both NaN
{
    return bits(got) == want || (std::isnan(got) && std::isnan(from_bits(want)));
}

const float kW = 200.0f, kH = 200.0f;

struct Capsule { float ax, ay, bx, by, R, e, mu; uint32_t flags; };

// the winner on x0 -> x1 (false: none) and whether any contact is deeper than the slop
bool search(const std::vector<Capsule> &cs, float x0x, float x0y, float x1x, float x1y, float r, SweepContact *best,
            uint32_t *who, bool *over)
{
    bool have = false;
    *over = false;
    for (uint32_t j = 0; j < cs.size(); ++j) {
        SweepContact c;
        if (!sweep_contact(x0x, x0y, x1x, x1y, r, cs[j].ax, cs[j].ay, cs[j].bx, cs[j].by, cs[j].R, &c)) continue;
        if (sweep_over_slop(c)) *over = true;
        if (!have || sweep_better(c, j, *best, *who)) { *best = c; *who = j; have = true; }
    }
    return have;
}

// the plain rule of k_collider.h / k_surface.h on p -> moved
bool plain_pass(const std::vector<Capsule> &cs, bool surfaces, const float *in, float *out)
{
    const float px = in[0], py = in[1], qx = in[2], qy = in[3], r = in[4];
    unsigned long long best = 0;
    for (uint32_t j = 0; j < cs.size(); ++j) {
        ColliderTouch t;
        if (!collider_touch(px, py, r, cs[j].ax, cs[j].ay, cs[j].bx, cs[j].by, cs[j].R, &t)) continue;
        const unsigned long long key = collider_key(t.depth, j);
        best = key > best ? key : best;
    }
    out[0] = px; out[1] = py; out[2] = qx; out[3] = qy;
    if (!best) return false;
    const Capsule &w = cs[0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull)];
    ColliderTouch t;
    float s;
    (void)sweep_measure(px, py, r, w.ax, w.ay, w.bx, w.by, w.R, &t, &s);   // the winner again: collider_touch's bits
    float nx, ny;
    collider_normal(t, &nx, &ny);
    if (surfaces && !(w.flags & kSurfacePlain) && surface_velocity_finite(px, py, qx, qy)) {
        surface_apply(px, py, qx, qy, r, nx, ny, t.depth, 0.0f, 0.0f, w.e, w.mu, kW, kH, out);
        return true;
    }
    const float mx = nx * t.depth;
    const float my = ny * t.depth;
    const float x = px + mx;
    const float y = py + my;
    out[0] = surface_clamp(x, r, kW - r);
    out[1] = surface_clamp(y, r, kH - r);
    return true;
}

// one particle through the swept pass -> flags (1 moved, 2 swept, 4 stopped), out = (pos', prev')
unsigned sweep_pass(const std::vector<Capsule> &cs, bool surfaces, const float *in, float *out)
{
    const float px = in[0], py = in[1], qx = in[2], qy = in[3], r = in[4];
    if (sweep_plain_particle(px, py, qx, qy)) return plain_pass(cs, surfaces, in, out) ? 1u : 0u;
    out[0] = px; out[1] = py; out[2] = qx; out[3] = qy;
    SweepContact win, other;
    uint32_t who = 0, who2 = 0;
    bool over = false;
    if (!search(cs, qx, qy, px, py, r, &win, &who, &over)) return 0;
    unsigned flags = 1u | ((win.t > 0.0f && win.t < 1.0f) ? 2u : 0u);
    float res[4] = {0, 0, qx, qy};
    if (surfaces && !(cs[who].flags & kSurfacePlain))
        surface_apply(px, py, qx, qy, r, win.nx, win.ny, win.depth, 0.0f, 0.0f, cs[who].e, cs[who].mu, kW, kH, res);
    else
        sweep_push(px, py, r, win, kW, kH, &res[0], &res[1]);
    (void)search(cs, qx, qy, res[0], res[1], r, &other, &who2, &over);
    if (over) {
        sweep_stop(r, win, kW, kH, &out[0], &out[1]);
        return flags | 4u;
    }
    for (int k = 0; k < 4; ++k) out[k] = res[k];
    return flags;
}

void test_table()
{
    std::FILE *f = std::fopen(g_table, "r");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<Capsule> cs;
    char line[1024];
    unsigned cases = 0, count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    while (std::fgets(line, sizeof(line), f)) {
        if (line[0] == 'k') {
            unsigned j, w[7], flags;
            const int got = std::sscanf(line, "k %u %x %x %x %x %x %x %x %u", &j, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &flags);
            CHECK(got == 9 && j == cs.size());
            if (got != 9) break;
            cs.push_back({from_bits(w[0]), from_bits(w[1]), from_bits(w[2]), from_bits(w[3]), from_bits(w[4]), from_bits(w[5]),
                          from_bits(w[6]), flags});
            continue;
        }
        if (line[0] != 'c') continue;
        unsigned i, w[5], fl[2], o[2][4];
        const int got = std::sscanf(line, "c %u %x %x %x %x %x %u %x %x %x %x %u %x %x %x %x", &i, &w[0], &w[1], &w[2], &w[3], &w[4],
                                    &fl[0], &o[0][0], &o[0][1], &o[0][2], &o[0][3], &fl[1], &o[1][0], &o[1][1], &o[1][2], &o[1][3]);
        CHECK(got == 16 && i == cases);
        if (got != 16) break;
        float in[5];
        for (int j = 0; j < 5; ++j) in[j] = from_bits(w[j]);
        for (int form = 0; form < 2; ++form) {
            float out[4] = {0, 0, 0, 0};
            const unsigned flags = sweep_pass(cs, form == 1, in, out);
            const bool ok = flags == fl[form] && same(out[0], o[form][0]) && same(out[1], o[form][1]) &&
                            same(out[2], o[form][2]) && same(out[3], o[form][3]);
            if (!ok && g_failures < 20)
                std::fprintf(stderr, "case %u form %d: got %u %08x %08x %08x %08x, the table has %u %08x %08x %08x %08x\n", i, form,
                             flags, bits(out[0]), bits(out[1]), bits(out[2]), bits(out[3]), fl[form], o[form][0], o[form][1],
                             o[form][2], o[form][3]);
            CHECK(ok);
            if (form == 0) count[flags & 7u] += 1;
        }
        ++cases;
    }
    std::fclose(f);
    // (the table must not pass vacuously: contacts at t = 0 or 1, swept ones, stopped ones)
    CHECK(cs.size() == 10 && cases == 600 && count[3] >= 100 && count[7] >= 50 && count[0] >= 50);
}

void test_properties()
{
    const float wall[5] = {0.0f, 10.0f, 100.0f, 10.0f, 0.0f};  // a thin wall along y = 10
    SweepContact c;
    // straight down through it from y = 5 to y = 25 with r = 0.5: met at y = 9.5, a quarter of the way
    CHECK(sweep_contact(50.0f, 5.0f, 50.0f, 25.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    CHECK(c.t == 0.225f && c.x == 50.0f && c.y == 9.5f && c.nx == 0.0f && c.ny == -1.0f && c.depth == 15.5f);
    float ox, oy;
    sweep_push(50.0f, 25.0f, 0.5f, c, kW, kH, &ox, &oy);
    CHECK(ox == 50.0f && oy == 9.5f);
    // the plain rule sees nothing there
    ColliderTouch t;
    CHECK(!collider_touch(50.0f, 25.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &t));
    // moving away from it, or past its end: no contact
    CHECK(!sweep_contact(50.0f, 5.0f, 50.0f, 1.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    CHECK(!sweep_contact(110.0f, 5.0f, 110.0f, 25.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    // resting at distance exactly s and kicked in: the entry is at t = 0
    CHECK(sweep_contact(50.0f, 9.5f, 50.0f, 30.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    CHECK(c.t == 0.0f && c.y == 9.5f && c.depth == 20.5f);
    // started inside and moving out: no contact; moving further in: t = 0 and the whole way back
    CHECK(!sweep_contact(50.0f, 9.75f, 50.0f, 8.0f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    CHECK(sweep_contact(50.0f, 9.75f, 50.0f, 9.875f, 0.5f, wall[0], wall[1], wall[2], wall[3], wall[4], &c));
    CHECK(c.t == 0.0f && c.depth == 0.375f);
    // through a disc peg of R = 3 along its diameter: met at its near side
    CHECK(sweep_contact(10.0f, 50.0f, 30.0f, 50.0f, 0.5f, 20.0f, 50.0f, 20.0f, 50.0f, 3.0f, &c));
    CHECK(std::fabs(c.x - 16.5f) < 1e-5f && c.nx == -1.0f && c.ny == 0.0f && std::fabs(c.depth - 13.5f) < 1e-5f);
    // the order: t, then depth, then the index
    SweepContact a = c, b = c;
    CHECK(sweep_better(a, 0, b, 1) && !sweep_better(a, 1, b, 0) && !sweep_better(a, 1, b, 1));
    b.depth = 14.0f;
    CHECK(sweep_better(b, 5, a, 0));
    b.t = a.t + 0.125f;
    CHECK(sweep_better(a, 5, b, 0));
    // the slop is a share of s
    a.s = 1.0f;
    a.depth = kSweepSlop;
    CHECK(!sweep_over_slop(a));
    a.depth = 2.0f * kSweepSlop;
    CHECK(sweep_over_slop(a));
    // who takes the plain rule
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(sweep_plain_particle(1.0f, 2.0f, 1.0f, 2.0f) && sweep_plain_particle(1.0f, 2.0f, nan, 2.0f));
    CHECK(sweep_plain_particle(1.0f, 2.0f, 1.0f, inf) && !sweep_plain_particle(1.0f, 2.0f, 1.0f, 2.5f));
    // the lookup box
    ColliderGridView g;
    g.inv_cell = 0.5f; g.gx = 40; g.gy = 10; g.gxf = 40.0f; g.gyf = 10.0f;
    uint32_t x0, x1, y0, y1;
    CHECK(sweep_box(g, 1.0f, 1.0f, 5.0f, 3.0f, &x0, &x1, &y0, &y1) && x0 == 0 && x1 == 2 && y0 == 0 && y1 == 1);
    CHECK(sweep_box(g, 5.0f, 3.0f, 1.0f, 1.0f, &x0, &x1, &y0, &y1) && x0 == 0 && x1 == 2 && y0 == 0 && y1 == 1);
    CHECK(sweep_box(g, 1.0f, 1.0f, 31.0f, 1.0f, &x0, &x1, &y0, &y1) && x0 == 0 && x1 == 15);   // kSweepBoxCells wide
    CHECK(!sweep_box(g, 1.0f, 1.0f, 33.0f, 1.0f, &x0, &x1, &y0, &y1));     // one more
    CHECK(!sweep_box(g, 1.0f, 1.0f, 85.0f, 1.0f, &x0, &x1, &y0, &y1) && !sweep_box(g, nan, 1.0f, 2.0f, 1.0f, &x0, &x1, &y0, &y1));
    // up to half a cell outside the grid: the border cell; further out: none
    CHECK(sweep_box(g, 1.0f, -0.75f, 2.0f, 1.0f, &x0, &x1, &y0, &y1) && y0 == 0 && y1 == 0 && x0 == 0 && x1 == 1);
    CHECK(sweep_box(g, 80.5f, 20.5f, 79.0f, 19.0f, &x0, &x1, &y0, &y1) && x0 == 39 && x1 == 39 && y0 == 9 && y1 == 9);
    CHECK(!sweep_box(g, 1.0f, -1.5f, 2.0f, 1.0f, &x0, &x1, &y0, &y1) && !sweep_box(g, 81.5f, 1.0f, 79.0f, 1.0f, &x0, &x1, &y0, &y1));
}

struct Test { const char *name; std::function<void()> run; };
const Test kTests[] = {{"table", test_table}, {"properties", test_properties}};

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (const Test &t : kTests) std::printf("%s\n", t.name);
        return 0;
    }
    if (argc > 1) g_table = argv[1];
    for (const Test &t : kTests) {
        const int before = g_failures;
        t.run();
        std::printf("test %s ... %s\n", t.name, g_failures == before ? "ok" : "FAILED");
    }
    if (g_failures) std::printf("%d checks failed\n", g_failures);
    return g_failures ? 1 : 0;
}
