// bond_colours_tests.cpp -- the colouring behind the bonds' coloured solver (gpu-physics-engine_amd/csrc/bond_colours.h)
// on the CPU: proper, the least-colour rule against a brute-force restatement, duplicates, anchors, the cap of 64
// colours, order / colour_start, dependence on the bond order alone -- and a coloured pass replayed from a table the
// numpy model wrote (tests/_bond_solver_model.table_text()) with the pass's own functions (csrc/k_bond.h), bit for bit.
// No HIP, no library: the three headers alone.  Compile with -ffp-contract=off.
//
// usage: bond_colours_tests [--list] [TABLE]          (without a table the replay reports itself skipped and fails)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/bond_colours.h"
#include "../../gpu-physics-engine_amd/csrc/bond_graph.h"
#include "../../gpu-physics-engine_amd/csrc/k_bond.h"

using namespace gpe;

namespace {

int g_failures = 0;
const char *g_table = nullptr;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { if (++g_failures < 20) std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

gpe_bond pair(uint32_t a, uint32_t b, float rest = 1.0f, float stiffness = 1.0f, float max_length = 0.0f)
{
    gpe_bond q;
    std::memset(&q, 0, sizeof(q));
    q.uid_a = a; q.uid_b = b; q.rest_length = rest; q.stiffness = stiffness; q.max_length = max_length;
    return q;
}

gpe_bond anchor(uint32_t a, float x, float y, float rest = 0.0f, float stiffness = 1.0f)
{
    gpe_bond q = pair(a, GPE_UID_ABSENT, rest, stiffness);
    q.flags = GPE_BOND_ANCHOR;
    q.anchor_x = x; q.anchor_y = y;
    return q;
}

// graph and colours of a set; *fits: what bond_colours_build said
BondColours coloured(const std::vector<gpe_bond> &set, bool *fits = nullptr)
{
    BondGraph g;
    CHECK(bond_set_problem(set.data(), set.size(), 1) == nullptr);
    CHECK(bond_graph_build(set.data(), set.size(), &g));
    BondColours col;
    const bool ok = bond_colours_build(g.rec.data(), g.rec.size(), g.nodes.size(), &col);
    if (fits) *fits = ok;
    return col;
}

// the rule restated by brute force over the uids: for bond j, every lower bond that shares an end
std::vector<uint32_t> brute_colours(const std::vector<gpe_bond> &set)
{
    const auto ends = [](const gpe_bond &q) {
        std::vector<uint32_t> e{q.uid_a};
        if (!(q.flags & GPE_BOND_ANCHOR)) e.push_back(q.uid_b);
        return e;
    };
    std::vector<uint32_t> colour(set.size());
    for (size_t j = 0; j < set.size(); ++j) {
        std::set<uint32_t> taken;
        for (size_t i = 0; i < j; ++i)
            for (uint32_t a : ends(set[i]))
                for (uint32_t b : ends(set[j]))
                    if (a == b) taken.insert(colour[i]);
        uint32_t c = 0;
        while (taken.count(c)) ++c;
        colour[j] = c;
    }
    return colour;
}

// what every colouring must satisfy, whatever the set
void check_colours(const std::vector<gpe_bond> &set, const BondColours &col)
{
    const size_t k = set.size();
    CHECK(col.colour.size() == k && col.order.size() == k && col.colour_start.size() == (size_t)col.colours + 1);
    if (col.colour.size() != k || col.order.size() != k || col.colour_start.size() != (size_t)col.colours + 1) return;
    CHECK(col.colour_start[0] == 0 && col.colour_start[col.colours] == k);
    std::map<std::pair<uint32_t, uint32_t>, int> at;                    // (uid, colour) -> bonds: proper means at most one
    uint32_t largest = 0;
    for (size_t j = 0; j < k; ++j) {
        CHECK(col.colour[j] < col.colours);
        CHECK(++at[std::make_pair(set[j].uid_a, col.colour[j])] == 1);
        if (!(set[j].flags & GPE_BOND_ANCHOR)) CHECK(++at[std::make_pair(set[j].uid_b, col.colour[j])] == 1);
    }
    std::vector<int> seen(k, 0);
    for (uint32_t c = 0; c < col.colours; ++c) {
        CHECK(col.colour_start[c] < col.colour_start[c + 1]);           // greedy leaves no colour empty
        largest = std::max(largest, col.colour_start[c + 1] - col.colour_start[c]);
        for (uint32_t e = col.colour_start[c]; e < col.colour_start[c + 1] && e < k; ++e) {
            const uint32_t j = col.order[e];
            CHECK(j < k);
            if (j >= k) continue;
            CHECK(col.colour[j] == c && seen[j]++ == 0);
            if (e > col.colour_start[c]) CHECK(col.order[e - 1] < j);   // ascending index within a colour
        }
    }
    CHECK(largest == col.largest);
    CHECK(col.colour == brute_colours(set));
}

void test_small_sets()
{
    bool fits = false;
    BondColours none = coloured({}, &fits);
    CHECK(fits && none.colours == 0 && none.largest == 0 && none.colour_start == std::vector<uint32_t>{0});
    // a chain 1-2-3-4-5 in order: the colours alternate
    const std::vector<gpe_bond> chain = {pair(1, 2), pair(2, 3), pair(3, 4), pair(4, 5)};
    BondColours c = coloured(chain, &fits);
    check_colours(chain, c);
    CHECK(fits && c.colour == (std::vector<uint32_t>{0, 1, 0, 1}) && c.order == (std::vector<uint32_t>{0, 2, 1, 3}));
    CHECK(c.colour_start == (std::vector<uint32_t>{0, 2, 4}) && c.colours == 2 && c.largest == 2);
    // listed from the middle outwards the same bonds get other colours: the order of the set is part of the result
    const std::vector<gpe_bond> other = {pair(2, 3), pair(1, 2), pair(4, 5), pair(3, 4)};
    BondColours d = coloured(other);
    check_colours(other, d);
    CHECK(d.colour == (std::vector<uint32_t>{0, 1, 0, 1}));               // (2,3) first: colour 0, where it had 1
    // ... and of nothing else: flags, lengths and which end is named first do not matter
    std::vector<gpe_bond> turned = chain;
    for (gpe_bond &q : turned) { std::swap(q.uid_a, q.uid_b); q.rest_length = 7.f; q.max_length = 9.f; q.flags |= GPE_BOND_BROKEN; }
    CHECK(coloured(turned).colour == c.colour);
}

void test_duplicates_and_anchors()
{
    // the twin of a duplicate shares both ends: another colour.  An anchor occupies its particle only: two anchors
    // on two particles share a colour whatever their points, two on one particle do not
    const std::vector<gpe_bond> set = {pair(1, 2), pair(1, 2), pair(2, 1), anchor(1, 5.f, 5.f), anchor(2, 5.f, 5.f),
                                       anchor(1, 5.f, 5.f), anchor(9, 5.f, 5.f), pair(9, 10)};
    BondColours c = coloured(set);
    check_colours(set, c);
    CHECK(c.colour == (std::vector<uint32_t>{0, 1, 2, 3, 3, 4, 0, 1}));
    CHECK(c.colours == 5 && c.largest == 2);
}

void test_stars_and_the_cap()
{
    for (uint32_t degree : {1u, 63u, 64u, 65u, 200u}) {
        std::vector<gpe_bond> star;
        for (uint32_t i = 0; i < degree; ++i) star.push_back(i % 2 ? pair(1000, i) : pair(i, 1000));
        bool fits = false;
        BondColours c = coloured(star, &fits);
        check_colours(star, c);
        CHECK(c.colours == degree && c.largest == 1);                  // every spoke its own colour
        CHECK(fits == (degree <= GPE_BOND_COLOURS_MAX));               // 64 accepted, 65 refused: the count is named
    }
    // a refused set past the first word of colours at some nodes only: a hub of 130 with a chain through its spokes
    std::vector<gpe_bond> set;
    for (uint32_t i = 0; i < 130; ++i) set.push_back(pair(5000, i));
    for (uint32_t i = 0; i + 1 < 130; ++i) set.push_back(pair(i, i + 1));
    bool fits = true;
    BondColours c = coloured(set, &fits);
    check_colours(set, c);
    CHECK(!fits && c.colours >= 130);
}

void test_random_sets()
{
    std::mt19937 rng(12);
    for (int round = 0; round < 60; ++round) {
        const uint32_t uids = 2 + rng() % 40, k = rng() % 200;
        std::vector<gpe_bond> set;
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t a = 100 + rng() % uids;
            uint32_t b = 100 + rng() % uids;
            if (rng() % 5 == 0) { set.push_back(anchor(a, 1.f, 2.f)); continue; }
            if (b == a) b = a + 1000;
            set.push_back(pair(a, b));
            if (rng() % 7 == 0) set.push_back(set.back());             // a duplicate right behind it
        }
        BondColours c = coloured(set);
        check_colours(set, c);
        // the uids' values do not matter, only which bonds share one: renamed monotonically or not, the same colours
        std::vector<gpe_bond> renamed = set;
        for (gpe_bond &q : renamed) {
            q.uid_a = 0xF0000000u - 7u * q.uid_a;
            if (!(q.flags & GPE_BOND_ANCHOR)) q.uid_b = 0xF0000000u - 7u * q.uid_b;
        }
        CHECK(coloured(renamed).colour == c.colour);
    }
}

// ---- the replay ------------------------------------------------------------------------------------------------------
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// A coloured pass over the table's particles as the device makes it: the graph and the colours from the two headers, a
// sweep in `order`, every bond judged by bond_correction and moved by bond_move in place, slots looked up per node.
void test_table()
{
    if (!g_table) { std::fprintf(stderr, "no table given\n"); CHECK(g_table != nullptr); return; }
    std::FILE *f = std::fopen(g_table, "r");
    CHECK(f != nullptr);
    if (!f) return;
    unsigned n = 0, k = 0, iterations = 0, w = 0, h = 0;
    CHECK(std::fscanf(f, "%u %u %u %x %x", &n, &k, &iterations, &w, &h) == 5);
    CHECK(n > 0 && n < 100000 && k > 0 && k < 100000 && iterations >= 1 && iterations <= GPE_BOND_ITER_MAX);
    if (g_failures) { std::fclose(f); return; }
    const float W = from_bits(w), H = from_bits(h);
    std::vector<uint32_t> uid(n);
    std::vector<float> rad(n), x(n), y(n);
    std::vector<uint32_t> wx(n), wy(n), px0(n), py0(n);                 // the bits wanted, the bits at the start
    for (unsigned i = 0; i < n; ++i) {
        unsigned u, r, px, py, ox, oy;
        CHECK(std::fscanf(f, "%u %x %x %x %x %x", &u, &r, &px, &py, &ox, &oy) == 6);
        uid[i] = u; rad[i] = from_bits(r); x[i] = from_bits(px); y[i] = from_bits(py); wx[i] = ox; wy[i] = oy;
        px0[i] = px; py0[i] = py;
    }
    std::vector<gpe_bond> set(k);
    std::vector<uint32_t> want_colour(k), want_broken(k);
    for (unsigned j = 0; j < k; ++j) {
        unsigned a, b, rest, st, ml, fl, ax, ay, col, br;
        CHECK(std::fscanf(f, "%u %u %x %x %x %u %x %x %u %u", &a, &b, &rest, &st, &ml, &fl, &ax, &ay, &col, &br) == 10);
        gpe_bond &q = set[j];
        q.uid_a = a; q.uid_b = b; q.rest_length = from_bits(rest); q.stiffness = from_bits(st);
        q.max_length = from_bits(ml); q.flags = fl; q.anchor_x = from_bits(ax); q.anchor_y = from_bits(ay);
        want_colour[j] = col; want_broken[j] = br;
    }
    std::fclose(f);
    if (g_failures) return;
    BondGraph g;
    BondColours col;
    CHECK(bond_set_problem(set.data(), k, iterations) == nullptr);
    CHECK(bond_graph_build(set.data(), k, &g));
    CHECK(bond_colours_build(g.rec.data(), k, g.nodes.size(), &col));
    CHECK(col.colour == want_colour);
    CHECK(col.colours > 8);                                            // (the hub's spokes)
    std::map<uint32_t, uint32_t> slot_of;
    for (unsigned i = 0; i < n; ++i) slot_of[uid[i]] = i;
    std::vector<uint32_t> node_slot(g.nodes.size());
    for (size_t v = 0; v < g.nodes.size(); ++v) {
        const auto it = slot_of.find(g.nodes[v]);
        node_slot[v] = it == slot_of.end() ? 0xffffffffu : it->second;
    }
    std::vector<uint8_t> state = g.state;
    unsigned broke = 0, inert = 0;
    for (unsigned it = 0; it < iterations; ++it) {
        for (uint32_t e = 0; e < k; ++e) {                              // (colour, index) order
            const uint32_t j = col.order[e];
            if (state[j] == kBondBroken) continue;
            const BondRecord &r = g.rec[j];
            const bool anch = (r.b & kBondAnchorBit) != 0;
            const uint32_t ia = r.b & ~kBondAnchorBit;
            const uint32_t sa = node_slot[r.a], sb = anch ? 0u : node_slot[r.b];
            uint32_t now = kBondInert;
            if (sa < n && sb < n) {
                const float bx = anch ? g.anchors[2 * ia] : x[sb], by = anch ? g.anchors[2 * ia + 1] : y[sb];
                float cx = 0.f, cy = 0.f;
                now = bond_correction(x[sa], y[sa], bx, by, r.rest, r.w, g.max_length.empty() ? 0.0f : g.max_length[j], &cx, &cy);
                if (now == kBondActs) {
                    bond_move(x[sa], y[sa], rad[sa], cx, cy, W, H, &x[sa], &y[sa]);
                    if (!anch) bond_move(x[sb], y[sb], rad[sb], -cx, -cy, W, H, &x[sb], &y[sb]);
                }
            }
            broke += now == kBondBroken;
            inert += now == kBondInert;
            state[j] = (uint8_t)now;
        }
    }
    unsigned bad = 0, moved = 0;
    for (unsigned i = 0; i < n; ++i) {
        bad += bits_of(x[i]) != wx[i] || bits_of(y[i]) != wy[i];
        moved += bits_of(x[i]) != px0[i] || bits_of(y[i]) != py0[i];
    }
    CHECK(bad == 0);
    for (unsigned j = 0; j < k; ++j) CHECK((state[j] == kBondBroken) == (want_broken[j] != 0));
    CHECK(broke > 10 && inert > 10 && moved > 1000 && moved < n);                      // both outcomes were on the table
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"small_sets", test_small_sets},
    {"duplicates_and_anchors", test_duplicates_and_anchors},
    {"stars_and_the_cap", test_stars_and_the_cap},
    {"random_sets", test_random_sets},
    {"table", test_table},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (const Test &t : kTests) std::printf("%s\n", t.name);
        return 0;
    }
    if (argc > 1) g_table = argv[1];
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
