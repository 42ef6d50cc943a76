// mover_grid_tests.cpp -- the moving colliders on the CPU (gpu-physics-engine_amd/csrc/k_mover.h, mover_grid.h,
// k_collider.h): mover_advance and mover_pose replay a table of poses written by the numpy model
// (tests/golden/mover_poses.txt), and the lookup masks, built with the predicate the device uses, are checked for
// completeness against the pass's own touch predicate and cell function: for every point p whose cell lies in the
// grid, the cell's mask holds the bit of every mover collider_touch reports touched for a radius |r| <= rb.  Also what
// gpe_set_movers, gpe_set_mover_poses and the dt contract refuse.  No HIP, no library: the headers alone.  Compile with
// -ffp-contract=off.
//
// usage: mover_grid_tests [--list] [path of mover_poses.txt]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/mover_grid.h"

using namespace gpe;

namespace {

int g_failures = 0;
const char *g_table = "tests/golden/mover_poses.txt";
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

gpe_mover linear(float ax, float ay, float bx, float by, float R, float vx, float vy, float travel)
{
    gpe_mover m;
    std::memset(&m, 0, sizeof(m));
    m.ax = ax; m.ay = ay; m.bx = bx; m.by = by; m.radius = R;
    m.kind = GPE_MOVER_LINEAR;
    m.vx = vx; m.vy = vy; m.travel = travel;
    return m;
}

gpe_mover rotor(float ax, float ay, float bx, float by, float R, float px, float py, float omega)
{
    gpe_mover m;
    std::memset(&m, 0, sizeof(m));
    m.ax = ax; m.ay = ay; m.bx = bx; m.by = by; m.radius = R;
    m.kind = GPE_MOVER_ROTATE;
    m.px = px; m.py = py; m.omega = omega;
    return m;
}

// ---- the motion: the numpy model's table, bit for bit ---------------------------------------------------------------
void test_advance_table()
{
    std::FILE *f = std::fopen(g_table, "r");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<gpe_mover> set;
    std::vector<MoverDef> def;
    std::vector<float> q0, q1;
    char line[512];
    int steps = 0, rows = 0;
    while (std::fgets(line, sizeof(line), f)) {
        if (line[0] == 'm') {
            unsigned j, w[14];
            const int got = std::sscanf(line, "m %u %x %x %x %x %x %x %x %x %x %x %x %x %x %x", &j, &w[0], &w[1], &w[2], &w[3], &w[4],
                                        &w[5], &w[6], &w[7], &w[8], &w[9], &w[10], &w[11], &w[12], &w[13]);
            CHECK(got == 15 && j == set.size());
            if (got != 15) break;
            gpe_mover m;
            static_assert(sizeof(m) == 14 * sizeof(uint32_t), "gpe_mover is 14 words");
            uint32_t words[14];
            for (int i = 0; i < 14; ++i) words[i] = w[i];
            std::memcpy(&m, words, sizeof(m));
            CHECK(mover_refusal(m) == nullptr);
            set.push_back(m);
            def.push_back(mover_define(m));
            q0.push_back(m.kind == GPE_MOVER_LINEAR ? 0.0f : 1.0f);
            q1.push_back(m.kind == GPE_MOVER_LINEAR ? 1.0f : 0.0f);
        } else if (line[0] == 's') {
            unsigned s, j, w[7];
            const int got = std::sscanf(line, "s %u %u %x %x %x %x %x %x %x", &s, &j, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6]);
            CHECK(got == 9 && j < set.size());
            if (got != 9 || j >= set.size()) break;
            mover_advance(def[j], from_bits(w[0]), &q0[j], &q1[j]);
            float cap[4];
            mover_pose(def[j], q0[j], q1[j], cap);
            const bool same = bits(q0[j]) == w[1] && bits(q1[j]) == w[2] && bits(cap[0]) == w[3] && bits(cap[1]) == w[4] &&
                              bits(cap[2]) == w[5] && bits(cap[3]) == w[6];
            if (!same && g_failures < 5) std::fprintf(stderr, "step %u mover %u differs from the table\n", s, j);
            CHECK(same);
            steps = (int)s + 1;
            rows += 1;
        }
    }
    std::fclose(f);
    CHECK(set.size() == 8 && steps == 40 && rows == 320);
}

// ---- properties of the motion ---------------------------------------------------------------------------------------
void test_motion_properties()
{
    // a piston stays in [0, travel], turns at both ends, and landing exactly on an end turns one step later
    {
        const MoverDef d = mover_define(linear(0, 0, 1, 0, 0.5f, 0.25f, 0, 1.0f));   // speed 0.25, dt 1: 4 steps per leg
        float g = 0.0f, sgn = 1.0f;
        const float want_g[10] = {0.25f, 0.5f, 0.75f, 1.0f, 0.75f, 0.5f, 0.25f, 0.0f, 0.25f, 0.5f};
        const float want_s[10] = {1, 1, 1, 1, -1, -1, -1, -1, 1, 1};
        for (int s = 0; s < 10; ++s) {
            mover_advance(d, 1.0f, &g, &sgn);
            CHECK(g == want_g[s] && sgn == want_s[s]);
        }
    }
    {
        const MoverDef d = mover_define(linear(0, 0, 1, 0, 0.5f, 3.0f, 4.0f, 2.5f));
        float g = 0.0f, sgn = 1.0f;
        int turns = 0;
        for (int s = 0; s < 5000; ++s) {
            const float before = sgn;
            mover_advance(d, (s % 3) ? 1.0f / 60.0f : 0.37f, &g, &sgn);
            CHECK(g >= 0.0f && g <= 2.5f && (sgn == 1.0f || sgn == -1.0f));
            turns += sgn != before;
        }
        CHECK(turns > 100);
    }
    // speed 0 never moves; travel 0 goes on for ever
    {
        const MoverDef d = mover_define(linear(3, 4, 5, 6, 1, 0, 0, 2.0f));
        float g = 0.0f, sgn = 1.0f, cap[4];
        for (int s = 0; s < 100; ++s) mover_advance(d, 0.5f, &g, &sgn);
        mover_pose(d, g, sgn, cap);
        CHECK(bits(g) == 0 && sgn == 1.0f && cap[0] == 3 && cap[1] == 4 && cap[2] == 5 && cap[3] == 6);
        const MoverDef e = mover_define(linear(0, 0, 0, 0, 1, -2.0f, 0, 0.0f));
        g = 0.0f; sgn = 1.0f;
        for (int s = 0; s < 100; ++s) mover_advance(e, 0.5f, &g, &sgn);
        mover_pose(e, g, sgn, cap);
        CHECK(g == 100.0f && sgn == 1.0f && cap[0] == -100.0f && cap[1] == 0.0f);
    }
    // a rotor stays a unit vector and keeps its angle; omega * dt == 0 keeps every bit
    const double cases[4][2] = {{0.5, 1000}, {0.25, 5000}, {0.01, 20000}, {-0.5, 1000}};
    for (const auto &cs : cases) {
        const float x = (float)cs[0];
        const int steps = (int)cs[1];
        const MoverDef d = mover_define(rotor(0, 0, 1, 0, 0.5f, 0, 0, x));
        float c = 1.0f, s = 0.0f;
        double worst_len = 0.0, worst_angle = 0.0;
        for (int i = 1; i <= steps; ++i) {
            mover_advance(d, 1.0f, &c, &s);
            worst_len = std::fmax(worst_len, std::fabs(std::sqrt((double)c * c + (double)s * s) - 1.0));
            const double want = (double)x * i;
            const double off = std::remainder(std::atan2((double)s, (double)c) - want, 2.0 * M_PI);
            worst_angle = std::fmax(worst_angle, std::fabs(off) / i);
        }
        std::printf("  x %g steps %d: |len - 1| <= %.3g, angle error per step <= %.3g\n", cs[0], steps, worst_len, worst_angle);
        CHECK(worst_len <= std::ldexp(1.0, -21));
        CHECK(worst_angle <= std::ldexp(1.0, -22));
        const MoverDef still = mover_define(rotor(0, 0, 1, 0, 0.5f, 7, 9, 0.0f));
        const float c0 = c, s0 = s;
        mover_advance(still, 1.0f / 60.0f, &c, &s);
        CHECK(bits(c) == bits(c0) && bits(s) == bits(s0));
        mover_advance(d, 0.0f, &c, &s);
        CHECK(bits(c) == bits(c0) && bits(s) == bits(s0));
    }
}

// ---- what the host refuses ------------------------------------------------------------------------------------------
void test_refusals()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const gpe_mover ok_l = linear(1, 2, 3, 4, 0.5f, 1, 1, 2.0f), ok_r = rotor(1, 2, 3, 4, 0.5f, 5, 6, 2.0f);
    CHECK(!mover_refusal(ok_l) && !mover_refusal(ok_r));
    gpe_mover m = ok_l; m.radius = -0.0f;
    CHECK(!mover_refusal(m) && bits(mover_define(m).radius) == 0);
    m = ok_l; m.travel = 0.0f; CHECK(!mover_refusal(m));
    float *fields[] = {&m.ax, &m.ay, &m.bx, &m.by, &m.radius, &m.vx, &m.vy, &m.travel, &m.px, &m.py, &m.omega};
    for (float *field : fields)
        for (float bad : {nan, inf, -inf}) {
            m = ok_l; *field = bad; CHECK(mover_refusal(m) != nullptr);
            m = ok_r; *field = bad; CHECK(mover_refusal(m) != nullptr);
        }
    m = ok_l; m.radius = -0.25f; CHECK(mover_refusal(m) != nullptr);
    m = ok_l; m.kind = 2; CHECK(mover_refusal(m) != nullptr);
    m = ok_r; m.flags = 1; CHECK(mover_refusal(m) != nullptr);
    m = ok_r; m.reserved = 1; CHECK(mover_refusal(m) != nullptr);
    m = ok_l; m.travel = -1.0f; CHECK(mover_refusal(m) != nullptr);
    m = ok_l; m.vx = 3e38f; m.vy = 3e38f; CHECK(mover_refusal(m) != nullptr);          // the speed overflows
    // states
    CHECK(!mover_state_refusal(ok_l, 0.0f, 1.0f) && !mover_state_refusal(ok_l, 2.0f, -1.0f) && !mover_state_refusal(ok_r, 0.6f, 0.8f));
    CHECK(mover_state_refusal(ok_l, 1.0f, 0.5f) && mover_state_refusal(ok_l, 2.5f, 1.0f) && mover_state_refusal(ok_l, -0.5f, 1.0f));
    CHECK(mover_state_refusal(ok_l, nan, 1.0f) && mover_state_refusal(ok_r, 1.0f, inf) && mover_state_refusal(ok_r, nan, 0.0f));
    m = ok_l; m.travel = 0.0f;
    CHECK(!mover_state_refusal(m, 1e6f, 1.0f) && !mover_state_refusal(m, -5.0f, -1.0f));   // for ever: any finite progress
    // the dt contract
    MoverLimits L;
    CHECK(!mover_dt_refusal(L, 1e30f) && mover_dt_refusal(L, nan) && mover_dt_refusal(L, inf));
    mover_limits_add(L, mover_define(rotor(0, 0, 1, 0, 1, 0, 0, -3.0f)));
    mover_limits_add(L, mover_define(rotor(0, 0, 1, 0, 1, 0, 0, 2.0f)));
    CHECK(L.max_omega == 3.0f && !L.bounded);
    CHECK(!mover_dt_refusal(L, 0.125f) && !mover_dt_refusal(L, -0.125f) && !mover_dt_refusal(L, 0.0f));
    CHECK(mover_dt_refusal(L, 0.1875f) && mover_dt_refusal(L, -0.1875f));
    mover_limits_add(L, mover_define(linear(0, 0, 1, 0, 1, 100.0f, 0, 0.0f)));             // for ever: no bound on its speed
    CHECK(!L.bounded && !mover_dt_refusal(L, 0.125f));
    mover_limits_add(L, mover_define(linear(0, 0, 1, 0, 1, 3.0f, 4.0f, 2.0f)));
    mover_limits_add(L, mover_define(linear(0, 0, 1, 0, 1, 1.0f, 0, 0.5f)));
    CHECK(L.bounded && L.max_speed == 5.0f && L.min_travel == 0.5f);
    CHECK(!mover_dt_refusal(L, 0.1f) && !mover_dt_refusal(L, -0.1f) && mover_dt_refusal(L, 0.125f) && mover_dt_refusal(L, -0.125f));
}

// ---- the grid -------------------------------------------------------------------------------------------------------
struct Posed {
    std::vector<float> caps, R;          // 4 and 1 per mover
    uint32_t k() const { return (uint32_t)R.size(); }
    void add(const gpe_mover &m, int steps, float dt)
    {
        const MoverDef d = mover_define(m);
        float q0 = m.kind == GPE_MOVER_LINEAR ? 0.0f : 1.0f, q1 = m.kind == GPE_MOVER_LINEAR ? 1.0f : 0.0f, cap[4];
        for (int s = 0; s < steps; ++s) mover_advance(d, dt, &q0, &q1);
        mover_pose(d, q0, q1, cap);
        caps.insert(caps.end(), cap, cap + 4);
        R.push_back(d.radius);
    }
};

struct Built {
    MoverGridView g;
    std::vector<uint64_t> masks;
    std::vector<uint32_t> summary;
    uint64_t listed = 0;
    uint32_t words = 0;
};

Built build(const Posed &P, float rb, float W, float H)
{
    Built b;
    b.g = mover_grid_choose(rb, W, H);
    b.words = mover_mask_words(P.k());
    b.listed = mover_grid_fill(b.g, P.caps.data(), P.R.data(), P.k(), b.g.view.rb, b.masks, b.summary);
    return b;
}

void check_shape(const Built &b, uint32_t k)
{
    const ColliderGridView &v = b.g.view;
    const uint64_t cells = (uint64_t)v.gx * v.gy;
    CHECK(v.gx >= 1 && v.gy >= 1 && v.gx <= kMoverGridMaxDim && v.gy <= kMoverGridMaxDim);
    CHECK((float)v.gx == v.gxf && (float)v.gy == v.gyf);
    CHECK(b.words == (k + 63) / 64 && b.masks.size() == cells * b.words && b.summary.size() == cells);
    uint64_t set = 0;
    for (uint64_t c = 0; c < cells; ++c)
        for (uint32_t w = 0; w < b.words; ++w) {
            const uint64_t m = b.masks[c * b.words + w];
            set += (uint64_t)__builtin_popcountll(m);
            CHECK(((b.summary[c] >> w) & 1u) == (m != 0 ? 1u : 0u));
            if (w == b.words - 1 && (k % 64)) CHECK((m >> (k % 64)) == 0);         // no bit of a mover that does not exist
        }
    CHECK(set == b.listed);
    for (uint64_t c = 0; c < cells; ++c) CHECK((b.summary[c] >> b.words) == 0);
}

// every mover collider_touch reports for p and a radius within the bound is in the mask of p's cell
void check_point(const Built &b, const Posed &P, float px, float py, uint64_t *touches)
{
    uint32_t cell;
    if (!collider_cell_of(b.g.view, px, py, &cell)) return;
    const float rb = b.g.view.rb;
    const float radii[4] = {rb, -rb, rb * 0.5f, 0.0f};
    for (uint32_t j = 0; j < P.k(); ++j)
        for (float r : radii) {
            ColliderTouch t;
            if (!collider_touch(px, py, r, P.caps[4 * j], P.caps[4 * j + 1], P.caps[4 * j + 2], P.caps[4 * j + 3], P.R[j], &t)) continue;
            *touches += 1;
            const bool listed = (b.masks[(uint64_t)cell * b.words + j / 64] >> (j % 64)) & 1ull;
            if (!listed && g_failures < 5)
                std::fprintf(stderr, "mover %u touches (%g, %g) r %g but is not in cell %u\n", j, px, py, r, cell);
            CHECK(listed);
            break;
        }
}

uint64_t check_complete(const Built &b, const Posed &P, float W, float H, std::mt19937 &rng, int points)
{
    uint64_t touches = 0;
    std::uniform_real_distribution<float> ux(-0.05f * W, 1.05f * W), uy(-0.05f * H, 1.05f * H), un(-1.1f, 1.1f), u01(0.f, 1.f);
    const float cell = (float)b.g.cell, rb = b.g.view.rb;
    for (int i = 0; i < points; ++i) check_point(b, P, ux(rng), uy(rng), &touches);
    // around the posed surfaces, on both sides of "touched"
    for (uint32_t j = 0; j < P.k(); ++j)
        for (int i = 0; i < 6; ++i) {
            const float u = u01(rng), s = P.R[j] + rb;
            const float x = P.caps[4 * j] + u * (P.caps[4 * j + 2] - P.caps[4 * j]) + un(rng) * s;
            const float y = P.caps[4 * j + 1] + u * (P.caps[4 * j + 3] - P.caps[4 * j + 1]) + un(rng) * s;
            check_point(b, P, x, y, &touches);
        }
    // on cell borders, one ulp below and above them, and outside the grid
    for (uint32_t cx = 0; cx <= b.g.view.gx; cx += 1 + b.g.view.gx / 40)
        for (uint32_t cy = 0; cy <= b.g.view.gy; cy += 1 + b.g.view.gy / 40) {
            const float x = (float)cx * cell, y = (float)cy * cell;
            check_point(b, P, x, y, &touches);
            check_point(b, P, std::nextafterf(x, -1e30f), y, &touches);
            check_point(b, P, x, std::nextafterf(y, -1e30f), &touches);
            check_point(b, P, std::nextafterf(x, 1e30f), std::nextafterf(y, 1e30f), &touches);
            check_point(b, P, std::nextafterf(x, -1e30f), std::nextafterf(y, -1e30f), &touches);
        }
    check_point(b, P, -1.0f, 0.5f * H, &touches);
    check_point(b, P, 2.0f * W, 2.0f * H, &touches);
    check_point(b, P, std::numeric_limits<float>::quiet_NaN(), 1.0f, &touches);
    return touches;
}

Posed random_set(uint32_t k, float W, float H, std::mt19937 &rng)
{
    std::uniform_real_distribution<float> ux(0.f, W), uy(0.f, H), ud(-0.15f * W, 0.15f * W), ur(0.f, 3.f), u01(0.f, 1.f), uw(-3.f, 3.f);
    Posed P;
    for (uint32_t j = 0; j < k; ++j) {
        const float ax = ux(rng), ay = uy(rng);
        float bx = ax + ud(rng), by = ay + ud(rng), R = u01(rng) < 0.25f ? 0.0f : ur(rng);    // thin walls
        if (j % 7 == 0) { bx = ax; by = ay; }                                                   // discs
        const int steps = (int)(u01(rng) * 40.f);
        if (j % 2) P.add(rotor(ax, ay, bx, by, R, ax + ud(rng), ay + ud(rng), uw(rng)), steps, 1.0f / 8.0f);
        else P.add(linear(ax, ay, bx, by, R, uw(rng) * 4.f, uw(rng) * 4.f, (j % 4) ? 0.0f : 6.0f), steps, 1.0f / 8.0f);
    }
    return P;
}

void test_random_sets()
{
    std::mt19937 rng(1234);
    const uint32_t ks[4] = {1, 64, 65, 1024};
    for (uint32_t k : ks)
        for (int world = 0; world < 2; ++world) {
            const float W = world ? 200.0f : 3048.0f, H = world ? 200.0f : 1048.0f, rb = world ? 0.5f : 2.0f;
            Posed P = random_set(k, W, H, rng);
            if (k >= 64) {
                // one far outside the world, one slid far away, one beyond 2^17 cells, one whose |b - a|^2 overflows
                const size_t at = P.k() - 4;
                P.caps.resize(4 * at); P.R.resize(at);
                P.add(linear(-5.f * W, -3.f * H, -4.f * W, -3.f * H, 1.0f, 0, 0, 0), 0, 0.f);
                P.add(linear(10, 10, 20, 10, 1.0f, 1000.f, 0, 0), 40, 1.0f);
                P.add(linear(-3e9f, 0.4f * H, 3e9f, 0.4f * H + 1.f, 0.5f, 0, 0, 0), 0, 0.f);
                P.add(rotor(1e30f, 0.5f * H, -1e30f, 0.5f * H, 1.0f, 0, 0, 0.25f), 3, 1.0f);
            }
            CHECK(P.k() == k);
            const Built b = build(P, rb, W, H);
            check_shape(b, k);
            const uint64_t cells = (uint64_t)b.g.view.gx * b.g.view.gy;
            const uint64_t touches = check_complete(b, P, W, H, rng, k >= 1024 ? 3000 : 20000);
            std::printf("  k %u world %g x %g: grid %u x %u, %llu bits of %llu, %llu touches checked\n", k, W, H, b.g.view.gx,
                        b.g.view.gy, (unsigned long long)b.listed, (unsigned long long)(cells * k), (unsigned long long)touches);
            CHECK(touches > (k == 1 ? 0u : 100u));
            CHECK(b.listed > 0 && b.listed < cells * k);                               // culling happens
        }
}

void test_views()
{
    // cells of max(4 rb, max(W, H) / 128), W and H strictly inside the grid, at most 128 per axis
    MoverGridView g = mover_grid_choose(0.5f, 200.0f, 200.0f);
    CHECK(g.view.gx == 101 && g.view.gy == 101 && g.cell == 2.0 && g.view.rb == 0.5f);
    g = mover_grid_choose(-0.5f, 200.0f, 200.0f);
    CHECK(g.view.gx == 101 && g.view.rb == 0.5f);
    g = mover_grid_choose(0.5f, 3048.0f, 1048.0f);
    CHECK(g.view.gx <= 128 && g.view.gy <= 128 && g.view.gx >= 64 && (double)g.view.gx * g.cell > 3048.0 && (double)g.view.gy * g.cell > 1048.0);
    g = mover_grid_choose(0.001f, 1e6f, 10.0f);
    CHECK(g.view.gx <= 128 && g.view.gx >= 64 && g.view.gy == 1);
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> e(-12.f, 12.f);
    for (int i = 0; i < 20000; ++i) {
        const float W = std::pow(10.f, e(rng)), H = std::pow(10.f, e(rng)), rb = std::pow(10.f, e(rng));
        g = mover_grid_choose(rb, W, H);
        CHECK(g.view.gx >= 1 && g.view.gy >= 1 && g.view.gx <= kMoverGridMaxDim && g.view.gy <= kMoverGridMaxDim);
        if (g.view.gx * g.view.gy > 1) {
            CHECK(g.cell >= 4.0 * rb * 0.999999 && (double)g.view.gx * g.cell > W && (double)g.view.gy * g.cell > H);
            uint32_t cell;                                     // (W, H): the last cell, or rounded out of the grid
            CHECK(!collider_cell_of(g.view, W, H, &cell) || cell == g.view.gx * g.view.gy - 1);
        }
    }
    // worlds and bounds no grid can be cut for: one cell that lists everything
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float odd[][3] = {{0.5f, 200.f, inf}, {inf, 200.f, 200.f}, {nan, 200.f, 200.f}, {0.75f, 2.5f, 2.5f}, {0.5f, 1e-3f, 1e-3f},
                            {0.5f, 0.f, 10.f}, {0.5f, -1.f, 10.f}, {0.5f, nan, 10.f}, {0.5f, 1e25f, 1e25f}};
    Posed P;
    P.add(linear(1, 1, 2, 2, 0.5f, 0, 0, 0), 0, 0.f);
    P.add(rotor(100, 100, 150, 100, 1.0f, 100, 100, 1.0f), 5, 0.25f);
    for (const auto &o : odd) {
        const Built b = build(P, o[0], o[1], o[2]);
        CHECK(b.g.view.gx == 1 && b.g.view.gy == 1 && b.listed == 2 && b.masks.size() == 1 && b.masks[0] == 3 && b.summary[0] == 1);
    }
}

void test_everywhere_and_nowhere()
{
    // a capsule that is far, infinite or NaN is in every cell; one outside the world is in none
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const MoverGridView g = mover_grid_choose(0.5f, 200.0f, 200.0f);
    const float caps[][4] = {{-3e9f, 80.f, 3e9f, 81.f}, {inf, 0.f, 1.f, 1.f}, {1.f, nan, 1.f, 1.f}, {1e30f, 100.f, -1e30f, 100.f}};
    for (const auto &cap : caps) {
        uint32_t x0, y0, x1, y1;
        bool everywhere = false;
        CHECK(mover_cell_rect(g, cap, 0.5f, 0.5f, &x0, &y0, &x1, &y1, &everywhere) && everywhere);
        CHECK(x0 == 0 && y0 == 0 && x1 == g.view.gx - 1 && y1 == g.view.gy - 1);
    }
    const float out[][4] = {{-50.f, 100.f, -40.f, 100.f}, {100.f, 260.f, 120.f, 250.f}, {300.f, 300.f, 300.f, 300.f}};
    for (const auto &cap : out) {
        uint32_t x0, y0, x1, y1;
        bool everywhere = true;
        CHECK(!mover_cell_rect(g, cap, 0.5f, 0.5f, &x0, &y0, &x1, &y1, &everywhere) && !everywhere);
    }
    // a disc in the middle: a few cells around it, not the grid
    const float disc[4] = {100.f, 100.f, 100.f, 100.f};
    uint32_t x0, y0, x1, y1, n = 0;
    bool everywhere = true;
    CHECK(mover_cell_rect(g, disc, 1.0f, 0.5f, &x0, &y0, &x1, &y1, &everywhere) && !everywhere);
    for (uint32_t cy = y0; cy <= y1; ++cy)
        for (uint32_t cx = x0; cx <= x1; ++cx) n += mover_listed(g, disc, 1.0f, 0.5f, cx, cy);
    CHECK(n >= 9 && n <= 25 && x0 >= 46 && x1 <= 53);
}

struct Test { const char *name; std::function<void()> run; };
const Test kTests[] = {
    {"advance_table", test_advance_table}, {"motion_properties", test_motion_properties}, {"refusals", test_refusals},
    {"random_sets", test_random_sets},     {"views", test_views},                         {"everywhere_and_nowhere", test_everywhere_and_nowhere},
};

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
