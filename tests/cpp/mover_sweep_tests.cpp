// mover_sweep_tests.cpp -- the swept movers' rule as C++ states it (csrc/k_mover_sweep.h over csrc/k_mover.h,
// csrc/k_sweep.h and csrc/k_surface.h), stand-alone: its own main, no HIP header, no GPU.
// tests/test_mover_sweep_cpu.py compiles it with
//   g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror
// once plain and once with -fsanitize=address,undefined, and runs it on the table the numpy model wrote
// (tests/golden/mover_sweep_cases.txt: tests/_mover_sweep_model.table_text()).  Every case is replayed bit for bit by
// brute force over the table's movers, without surfaces and with them; then once more through the motion listing built
// on the CPU (the masks of the cells of the path's lookup box), which must give the same winner and the same bits.
//
// usage: mover_sweep_tests [--list] [path of mover_sweep_cases.txt]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/mover_grid.h"

using namespace gpe;

namespace {

int g_failures = 0;
const char *g_table = "tests/golden/mover_sweep_cases.txt";

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

const float kW = 200.0f, kH = 200.0f, kRb = 1.0f;
const float kDt = 1.0f / 60.0f;

struct Mover {
    MoverDef def;
    float c0[4], c1[4];
    MoverCarry carry;
    SurfaceRow surf;
};

// the movers a pass judges: all of them, or the candidates of a box
typedef std::vector<uint32_t> Cands;

bool search(const std::vector<Mover> &ms, const Cands &cands, float px, float py, float qx, float qy, float r,
            SweepContact *best, uint32_t *who, bool *over)
{
    bool have = false;
    *over = false;
    for (uint32_t j : cands) {
        SweepContact c;
        if (!mover_sweep_judge(ms[j].carry, ms[j].c1, ms[j].def.radius, px, py, qx, qy, r, &c)) continue;
        if (sweep_over_slop(c)) *over = true;
        if (!have || sweep_better(c, j, *best, *who)) { *best = c; *who = j; have = true; }
    }
    return have;
}

// the masks of the motion listing, as k_movers_sweep_build sets them
struct Listing {
    MoverGridView g;
    uint32_t words = 0;
    std::vector<uint64_t> masks;
};

Listing listing_of(const std::vector<Mover> &ms)
{
    Listing L;
    L.g = mover_grid_choose(kRb, kW, kH);
    L.words = mover_mask_words((uint32_t)ms.size());
    L.masks.assign((size_t)L.g.view.gx * L.g.view.gy * L.words, 0);
    for (uint32_t j = 0; j < ms.size(); ++j) {
        uint32_t x0, y0, x1, y1;
        bool everywhere;
        const Mover &m = ms[j];
        if (!mover_sweep_cell_rect(L.g, m.def, m.def.pad0, m.c0, m.c1, kRb, &x0, &y0, &x1, &y1, &everywhere)) continue;
        for (uint32_t cy = y0; cy <= y1; ++cy)
            for (uint32_t cx = x0; cx <= x1; ++cx)
                if (everywhere || mover_sweep_listed(L.g, m.def, m.def.pad0, m.c0, m.c1, kRb, cx, cy))
                    L.masks[((size_t)cy * L.g.view.gx + cx) * L.words + j / 64] |= 1ull << (j % 64);
    }
    return L;
}

// the candidates of the path x0 -> x1 as the pass finds them: every mover when the box fails or the radius is wide
Cands candidates(const Listing *L, size_t k, float x0x, float x0y, float x1x, float x1y, float r)
{
    Cands out;
    uint32_t cx0, cx1, cy0, cy1;
    if (!L || !(std::fabs(r) <= kRb) || !sweep_box(L->g.view, x0x, x0y, x1x, x1y, &cx0, &cx1, &cy0, &cy1)) {
        for (uint32_t j = 0; j < k; ++j) out.push_back(j);
        return out;
    }
    for (uint32_t w = 0; w < L->words; ++w) {
        uint64_t b = 0;
        for (uint32_t cy = cy0; cy <= cy1; ++cy)
            for (uint32_t cx = cx0; cx <= cx1; ++cx) b |= L->masks[((size_t)cy * L->g.view.gx + cx) * L->words + w];
        for (uint32_t i = 0; i < 64; ++i)
            if (b >> i & 1) out.push_back(w * 64 + i);
    }
    return out;
}

// one particle through the swept pass -> flags (1 moved, 2 swept, 4 stopped), out = (pos', prev'), *who the winner
unsigned sweep_pass(const std::vector<Mover> &ms, const Listing *L, bool surfaces, const float *in, float *out, uint32_t *who)
{
    const float px = in[0], py = in[1], qx = in[2], qy = in[3], r = in[4];
    out[0] = px; out[1] = py; out[2] = qx; out[3] = qy;
    *who = 0;
    SweepContact win, other;
    uint32_t who2 = 0;
    bool over = false;
    if (!search(ms, candidates(L, ms.size(), qx, qy, px, py, r), px, py, qx, qy, r, &win, who, &over)) return 0;
    const unsigned flags = 1u | ((win.t > 0.0f && win.t < 1.0f) ? 2u : 0u);
    const Mover &m = ms[*who];
    float res[4];
    mover_sweep_respond(win, m.c0, m.c1, m.def.radius, surfaces ? &m.surf : nullptr, px, py, qx, qy, r, kW, kH, res);
    (void)search(ms, candidates(L, ms.size(), qx, qy, res[0], res[1], r), res[0], res[1], qx, qy, r, &other, &who2, &over);
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
    std::vector<Mover> ms;
    Listing L;
    bool listed = false;
    char line[1024];
    unsigned cases = 0, count[8] = {0, 0, 0, 0, 0, 0, 0, 0}, through_grid = 0;
    while (std::fgets(line, sizeof(line), f)) {
        if (line[0] == 'm') {
            unsigned j, w[18], flags;
            int used = 0;
            if (std::sscanf(line, "m %u%n", &j, &used) != 1) { CHECK(false); break; }
            const char *p = line + used;
            bool ok = j == ms.size();
            for (int i = 0; i < 18 && ok; ++i) {
                int n = 0;
                ok = std::sscanf(p, "%x%n", &w[i], &n) == 1;
                p += n;
            }
            ok = ok && std::sscanf(p, "%u", &flags) == 1;
            CHECK(ok);
            if (!ok) break;
            gpe_mover q;
            static_assert(sizeof(q) == 14 * sizeof(uint32_t), "gpe_mover is 14 words");
            std::memcpy(&q, w, sizeof(q));
            CHECK(mover_refusal(q) == nullptr);
            Mover m;
            m.def = mover_define(q);
            CHECK(bits(m.def.pad0) == bits(mover_arm(m.def)) && m.def.pad1 == 0.0f);
            const float p0 = from_bits(w[14]), p1 = from_bits(w[15]);
            float q0 = p0, q1 = p1;
            mover_pose(m.def, q0, q1, m.c0);
            mover_advance(m.def, kDt, &q0, &q1);
            mover_pose(m.def, q0, q1, m.c1);
            mover_carry_of(m.def, kDt, p0, p1, q0, q1, m.c0, m.c1, m.def.pad0, &m.carry);
            m.surf = {from_bits(w[16]), from_bits(w[17]), flags, 0u};
            ms.push_back(m);
            continue;
        }
        if (line[0] != 'c') continue;
        if (!listed) {
            L = listing_of(ms);
            listed = true;
        }
        unsigned i, w[5], fl[2], wh[2], o[2][4];
        const int got = std::sscanf(line, "c %u %x %x %x %x %x %u %u %x %x %x %x %u %u %x %x %x %x", &i, &w[0], &w[1], &w[2], &w[3],
                                    &w[4], &fl[0], &wh[0], &o[0][0], &o[0][1], &o[0][2], &o[0][3], &fl[1], &wh[1], &o[1][0],
                                    &o[1][1], &o[1][2], &o[1][3]);
        CHECK(got == 18 && i == cases);
        if (got != 18) break;
        float in[5];
        for (int j = 0; j < 5; ++j) in[j] = from_bits(w[j]);
        for (int form = 0; form < 2; ++form) {
            for (int via = 0; via < 2; ++via) {                  // brute force, then through the motion listing
                float out[4] = {0, 0, 0, 0};
                uint32_t who = 0;
                const unsigned flags = sweep_pass(ms, via ? &L : nullptr, form == 1, in, out, &who);
                const bool ok = flags == fl[form] && who == wh[form] && same(out[0], o[form][0]) && same(out[1], o[form][1]) &&
                                same(out[2], o[form][2]) && same(out[3], o[form][3]);
                if (!ok && g_failures < 20)
                    std::fprintf(stderr, "case %u form %d via %d: got %u %u %08x %08x %08x %08x, the table has %u %u %08x %08x %08x %08x\n",
                                 i, form, via, flags, who, bits(out[0]), bits(out[1]), bits(out[2]), bits(out[3]), fl[form],
                                 wh[form], o[form][0], o[form][1], o[form][2], o[form][3]);
                CHECK(ok);
            }
            if (form == 0) count[fl[0] & 7u] += 1;
        }
        if (candidates(&L, ms.size(), in[2], in[3], in[0], in[1], in[4]).size() < ms.size()) through_grid += 1;
        ++cases;
    }
    std::fclose(f);
    // (the table must not pass vacuously: swept contacts, stopped ones, untouched ones, and most paths through the grid)
    CHECK(ms.size() == 9 && cases == 400 && count[3] >= 30 && count[7] >= 20 && count[0] >= 100 && through_grid >= 250);
    CHECK(L.g.view.gx > 16 && L.words == 1);
}

void test_properties()
{
    // a thin gate along x = 50 that moved 20 to the right in this step, a particle of radius 1 at rest in its way
    MoverCarry k;
    gpe_mover q;
    std::memset(&q, 0, sizeof(q));
    q.ax = 50.0f; q.ay = 10.0f; q.bx = 50.0f; q.by = 90.0f;
    q.kind = GPE_MOVER_LINEAR; q.vx = 1200.0f;
    const MoverDef d = mover_define(q);
    float p0 = 0.0f, p1 = 1.0f, c0[4], c1[4];
    float q0 = p0, q1 = p1;
    mover_pose(d, q0, q1, c0);
    mover_advance(d, kDt, &q0, &q1);
    mover_pose(d, q0, q1, c1);
    mover_carry_of(d, kDt, p0, p1, q0, q1, c0, c1, d.pad0, &k);
    CHECK(k.kind == kCarryShift && k.cx == c1[0] - c0[0] && k.cy == 0.0f && std::fabs(k.cx - 20.0f) < 1e-4f);
    SweepContact c;
    ColliderTouch t;
    CHECK(!collider_touch(60.0f, 50.0f, 1.0f, c1[0], c1[1], c1[2], c1[3], 0.0f, &t));   // the plain rule sees nothing
    CHECK(mover_sweep_judge(k, c1, 0.0f, 60.0f, 50.0f, 60.0f, 50.0f, 1.0f, &c));
    CHECK(c.t > 0.0f && c.t < 1.0f && c.nx == 1.0f && c.ny == 0.0f);
    float ox, oy;
    sweep_push(60.0f, 50.0f, 1.0f, c, kW, kH, &ox, &oy);
    CHECK(std::fabs(ox - (c1[0] + 1.0f)) < 1e-4f && oy == 50.0f);
    // a particle behind the old face stays behind: no contact
    CHECK(!mover_sweep_judge(k, c1, 0.0f, 45.0f, 50.0f, 45.0f, 50.0f, 1.0f, &c));
    // a mover that did not move: STILL, y0 = prev bit for bit, a resting particle gets the plain touch with t = 1
    mover_carry_of(d, 0.0f, q0, q1, q0, q1, c1, c1, d.pad0, &k);
    CHECK(k.kind == kCarryStill);
    float yx, yy;
    mover_carry(k, -0.0f, 3.0f, &yx, &yy);
    CHECK(bits(yx) == bits(-0.0f) && yy == 3.0f);
    CHECK(mover_sweep_judge(k, c1, 0.0f, c1[0] + 0.5f, 50.0f, c1[0] + 0.5f, 50.0f, 1.0f, &c));
    CHECK(collider_touch(c1[0] + 0.5f, 50.0f, 1.0f, c1[0], c1[1], c1[2], c1[3], 0.0f, &t));
    CHECK(c.t == 1.0f && bits(c.depth) == bits(t.depth) && c.depth == 0.5f && c.nx == 1.0f);
    // a rotor: the arm, the carry of a quarter of the polynomial's range, the gate
    std::memset(&q, 0, sizeof(q));
    q.ax = 100.0f; q.ay = 100.0f; q.bx = 130.0f; q.by = 100.0f;
    q.kind = GPE_MOVER_ROTATE; q.px = 100.0f; q.py = 100.0f; q.omega = 24.0f;
    const MoverDef r = mover_define(q);
    CHECK(r.pad0 == 30.0f && mover_arm(d) == 0.0f);
    p0 = 1.0f; p1 = 0.0f; q0 = p0; q1 = p1;
    mover_pose(r, q0, q1, c0);
    mover_advance(r, kDt, &q0, &q1);
    mover_pose(r, q0, q1, c1);
    mover_carry_of(r, kDt, p0, p1, q0, q1, c0, c1, r.pad0, &k);
    CHECK(k.kind == kCarryTurn && bits(k.cx) == bits(q0) && bits(k.cy) == bits(q1) && k.arm == 30.0f);
    mover_carry(k, 130.0f, 100.0f, &yx, &yy);                  // the tip's rest position is carried to the posed tip
    CHECK(bits(yx) == bits(c1[2]) && bits(yy) == bits(c1[3]));
    CHECK(mover_sweep_gate(k, 0.0f, 120.0f, 104.0f, 120.0f, 104.0f, 1.0f));
    CHECK(!mover_sweep_gate(k, 0.0f, 140.0f, 100.0f, 132.0f, 100.0f, 1.0f));
    CHECK(mover_sweep_gate(k, 0.0f, 60.0f, 101.0f, 140.0f, 101.0f, 1.0f));    // a path across the disc
    CHECK(mover_sweep_judge(k, c1, 0.0f, 120.0f, 104.0f, 120.0f, 104.0f, 1.0f, &c) && c.t > 0.0f && c.t < 1.0f);
    CHECK(!mover_sweep_judge(k, c1, 0.0f, 120.0f, 96.0f, 120.0f, 96.0f, 1.0f, &c));      // behind the old blade
    mover_carry_of(r, 0.0f, q0, q1, q0, q1, c1, c1, r.pad0, &k);
    CHECK(k.kind == kCarryStill);
    // the listing: the parallelogram's inside, and the disc
    const MoverGridView g = mover_grid_choose(1.0f, 200.0f, 200.0f);
    float far0[4] = {40.0f, 20.0f, 40.0f, 180.0f}, far1[4] = {160.0f, 20.0f, 160.0f, 180.0f};
    uint32_t x0, y0, x1, y1;
    bool everywhere;
    CHECK(mover_sweep_cell_rect(g, d, 0.0f, far0, far1, 1.0f, &x0, &y0, &x1, &y1, &everywhere) && !everywhere);
    const uint32_t mid = (uint32_t)(100.0 / g.cell);
    CHECK(mid >= x0 && mid <= x1 && mover_sweep_listed(g, d, 0.0f, far0, far1, 1.0f, mid, mid));   // far from every edge
    CHECK(!mover_listed(g, far1, 0.0f, 1.0f, mid, mid));
    CHECK(mover_sweep_cell_rect(g, r, r.pad0, c0, c1, 1.0f, &x0, &y0, &x1, &y1, &everywhere) && !everywhere);
    const uint32_t bx = (uint32_t)(100.0 / g.cell), by = (uint32_t)(75.0 / g.cell), ny = (uint32_t)(60.0 / g.cell);
    CHECK(mover_sweep_listed(g, r, r.pad0, c0, c1, 1.0f, bx, by) && !mover_sweep_listed(g, r, r.pad0, c0, c1, 1.0f, bx, ny));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float bad[4] = {nan, 20.0f, 40.0f, 180.0f};
    CHECK(mover_sweep_cell_rect(g, d, 0.0f, bad, far1, 1.0f, &x0, &y0, &x1, &y1, &everywhere) && everywhere);
    const MoverGridView one = mover_grid_one_cell(1.0f, 400.0);
    CHECK(mover_sweep_cell_rect(one, d, 0.0f, far0, far1, 1.0f, &x0, &y0, &x1, &y1, &everywhere) && everywhere);
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
