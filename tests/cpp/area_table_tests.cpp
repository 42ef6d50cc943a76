// area_table_tests.cpp -- the host side of an area set (gpu-physics-engine_amd/csrc/area_table.h) built on the CPU: the
// width classes, the node list, the members' nodes, the CSR's order, every refusal of the validation, and one relaxation
// computed from the tables with the pass's own functions (csrc/k_area.h, area_pass_host), against a table the numpy
// model wrote (tests/_areas_model.py), bit for bit.  No HIP, no library: the headers alone.  Compile with
// -ffp-contract=off.
//
// usage: area_table_tests [--list] [--table FILE]
//
// The table is text, every float as the 8 hex digits of its bits:
//   n k members W H               particles (uid = index; a member's uid >= n names no particle), loops, members, world
//   n lines: x y radius
//   k lines: first count rest_area stiffness                       (first, count decimal)
//   members lines: uid
//   k lines: acts area lambda                                      (acts 0 / 1; the rest is not compared where 0)
//   members lines: cx cy                                           (not compared where the member's loop does not act)
//   n lines: x y                  after one relaxation
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/area_table.h"
#include "../../gpu-physics-engine_amd/csrc/k_area.h"

using namespace gpe;

namespace {

int g_failures = 0;
std::string g_table;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { if (++g_failures < 20) std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
float float_of(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

struct Set {
    std::vector<gpe_area> areas;
    std::vector<uint32_t> uid;
    void add(const std::vector<uint32_t> &members, float rest_area = 1.0f, float stiffness = 0.5f)
    {
        gpe_area q;
        std::memset(&q, 0, sizeof(q));
        q.first = (uint32_t)uid.size(); q.count = (uint32_t)members.size(); q.rest_area = rest_area; q.stiffness = stiffness;
        areas.push_back(q);
        uid.insert(uid.end(), members.begin(), members.end());
    }
    const char *problem(uint32_t iterations = 1) const
    {
        return area_set_problem(areas.data(), areas.size(), uid.data(), uid.size(), iterations);
    }
};

// what every table must satisfy, whatever the set
void check_table(const Set &s, const AreaTable &t)
{
    const size_t k = s.areas.size(), members = s.uid.size(), m = t.nodes.size();
    CHECK(t.rec.size() == k && t.order.size() == k && t.member_node.size() == members && t.inc.size() == members);
    CHECK(t.row_start.size() == m + 1 && t.row_start[0] == 0 && t.row_start[m] == members);
    CHECK(t.class_start[0] == 0 && t.class_start[kAreaClasses] == k);
    for (size_t v = 1; v < m; ++v) CHECK(t.nodes[v - 1] < t.nodes[v]);
    for (size_t i = 0; i < members; ++i) CHECK(t.member_node[i] < m && t.nodes[t.member_node[i]] == s.uid[i]);
    std::vector<int> seen(k, 0);
    for (uint32_t q = 0; q < kAreaClasses; ++q) {
        CHECK(t.class_start[q] <= t.class_start[q + 1]);
        for (uint32_t e = t.class_start[q]; e < t.class_start[q + 1] && e < k; ++e) {
            const uint32_t j = t.order[e];
            CHECK(j < k);
            if (j >= k) continue;
            CHECK(seen[j]++ == 0);
            CHECK(std::min(body_width(s.areas[j].count), 64u) == (4u << q));
            if (e > t.class_start[q]) CHECK(t.order[e - 1] < j);
        }
    }
    for (size_t j = 0; j < k; ++j) {
        CHECK(seen[j] == 1);
        CHECK(t.rec[j].first == s.areas[j].first && t.rec[j].count == s.areas[j].count);
        CHECK(t.rec[j].rest_area == s.areas[j].rest_area && t.rec[j].stiffness == s.areas[j].stiffness);
        CHECK(!(t.rec[j].rest_area == 0.0f && std::signbit(t.rec[j].rest_area)) && !std::signbit(t.rec[j].stiffness));
    }
    std::vector<int> listed(members, 0);
    uint32_t max_degree = 0;
    for (size_t v = 0; v < m; ++v) {
        CHECK(t.row_start[v] < t.row_start[v + 1]);            // a node is named by at least one member
        max_degree = std::max(max_degree, t.row_start[v + 1] - t.row_start[v]);
        for (uint32_t e = t.row_start[v]; e < t.row_start[v + 1]; ++e) {
            const AreaIncidence w = t.inc[e];
            CHECK(w.member < members && w.loop < k);
            if (w.member >= members || w.loop >= k) continue;
            if (e > t.row_start[v]) CHECK(t.inc[e - 1].member < w.member);     // ascending member index
            CHECK(t.member_node[w.member] == v && listed[w.member]++ == 0);
            CHECK(w.member >= s.areas[w.loop].first && w.member < s.areas[w.loop].first + s.areas[w.loop].count);
        }
    }
    CHECK(max_degree == t.max_degree);
}

// one relaxation of n particles whose uid is their index (a uid >= n names no particle) through the tables, as the two
// phases of the pass walk them
struct Relaxed {
    std::vector<uint32_t> verdict;
    std::vector<float> value;            // 2 per loop
    std::vector<float> corr;             // 2 per member
    std::vector<float> out;              // 2 per particle
};

Relaxed relax_by_table(const AreaTable &t, const std::vector<float> &pos, const std::vector<float> &radius, float W, float H)
{
    const size_t k = t.rec.size(), n = radius.size(), members = t.member_node.size();
    Relaxed R;
    R.verdict.assign(k, kAreaInert);
    R.value.assign(2 * k, NAN);
    R.corr.assign(2 * members, 0.0f);
    R.out = pos;
    std::vector<float> px, py, scratch;
    std::vector<uint8_t> live;
    for (uint32_t e = 0; e < k; ++e) {                           // class by class, as the launches go
        const uint32_t j = t.order[e];
        const AreaRecord &r = t.rec[j];
        px.assign(r.count, 0.0f); py.assign(r.count, 0.0f); live.assign(r.count, 0); scratch.assign(2 * (size_t)r.count, 0.0f);
        for (uint32_t i = 0; i < r.count; ++i) {
            const uint32_t p = t.nodes[t.member_node[r.first + i]];
            if (p >= n) continue;
            live[i] = 1; px[i] = pos[2 * (size_t)p]; py[i] = pos[2 * (size_t)p + 1];
        }
        R.verdict[j] = area_pass_host(r.count, px.data(), py.data(), live.data(), r.rest_area, r.stiffness,
                                      &R.corr[2 * (size_t)r.first], scratch.data(), &R.value[2 * (size_t)j]);
    }
    for (size_t v = 0; v < t.nodes.size(); ++v) {
        const uint32_t p = t.nodes[v];
        if (p >= n) continue;
        float accx = 0.0f, accy = 0.0f;
        bool any = false;
        for (uint32_t e = t.row_start[v]; e < t.row_start[v + 1]; ++e) {
            const AreaIncidence w = t.inc[e];
            if (R.verdict[w.loop] != kAreaActs) continue;
            accx = accx + R.corr[2 * (size_t)w.member];
            accy = accy + R.corr[2 * (size_t)w.member + 1];
            any = true;
        }
        if (any) bond_move(pos[2 * (size_t)p], pos[2 * (size_t)p + 1], radius[p], accx, accy, W, H, &R.out[2 * (size_t)p], &R.out[2 * (size_t)p + 1]);
    }
    return R;
}

void test_classes_and_order()
{
    Set s;
    const uint32_t counts[] = {3, 65, 4, 5, 8, 9, 64, 16, 17, 32, 33, 4096, 4};
    uint32_t next = 0;
    for (uint32_t c : counts) {
        std::vector<uint32_t> m(c);
        for (uint32_t i = 0; i < c; ++i) m[i] = next++;
        s.add(m);
    }
    CHECK(s.problem() == nullptr);
    AreaTable t;
    area_table_build(s.areas.data(), s.areas.size(), s.uid.data(), s.uid.size(), &t);
    check_table(s, t);
    const uint32_t want_start[] = {0, 3, 5, 7, 9, 13};
    for (uint32_t q = 0; q <= kAreaClasses; ++q) CHECK(t.class_start[q] == want_start[q]);
    const uint32_t want_order[] = {0, 2, 12, 3, 4, 5, 7, 8, 9, 1, 6, 10, 11};
    for (size_t e = 0; e < s.areas.size(); ++e) CHECK(t.order[e] == want_order[e]);
    CHECK(t.max_degree == 1 && t.nodes.size() == s.uid.size());
    CHECK(area_class(3) == 0 && area_class(4) == 0 && area_class(5) == 1 && area_class(64) == 4 && area_class(4096) == 4);
}

void test_shared_members_and_csr()
{
    // two squares sharing the edge 1 - 4, given second-first in member storage: the ranges tile in any order
    Set s;
    gpe_area a, b;
    std::memset(&a, 0, sizeof(a)); std::memset(&b, 0, sizeof(b));
    a.first = 4; a.count = 4; a.rest_area = 4.0f; a.stiffness = 1.0f;
    b.first = 0; b.count = 4; b.rest_area = -0.0f; b.stiffness = -0.0f;
    s.areas = {a, b};
    s.uid = {1, 2, 5, 4, /* loop 0: */ 0, 1, 4, 3};
    CHECK(s.problem() == nullptr);
    AreaTable t;
    area_table_build(s.areas.data(), 2, s.uid.data(), 8, &t);
    check_table(s, t);
    CHECK(t.nodes.size() == 6 && t.max_degree == 2);
    CHECK(bits_of(t.rec[1].rest_area) == 0 && bits_of(t.rec[1].stiffness) == 0);
    // node of uid 1: member 0 (loop 1), then member 5 (loop 0)
    CHECK(t.row_start[1] == 1 && t.row_start[2] == 3);
    CHECK(t.inc[1].member == 0 && t.inc[1].loop == 1 && t.inc[2].member == 5 && t.inc[2].loop == 0);
    // a hub in GPE_AREA_MAX_DEGREE triangles is accepted, one more is refused
    Set h;
    for (uint32_t j = 0; j < GPE_AREA_MAX_DEGREE; ++j) h.add({7, 100 + 2 * j, 101 + 2 * j});
    CHECK(h.problem() == nullptr);
    area_table_build(h.areas.data(), h.areas.size(), h.uid.data(), h.uid.size(), &t);
    check_table(h, t);
    CHECK(t.max_degree == GPE_AREA_MAX_DEGREE);
    h.add({7, 1000, 1001});
    CHECK(h.problem() != nullptr);
}

void test_k0()
{
    CHECK(area_set_problem(nullptr, 0, nullptr, 0, 1) == nullptr);
    CHECK(area_set_problem(nullptr, 0, nullptr, 0, 0) == nullptr);     // (k == 0 clears: nothing else is read)
    AreaTable t;
    area_table_build(nullptr, 0, nullptr, 0, &t);
    CHECK(t.rec.empty() && t.nodes.empty() && t.inc.empty() && t.row_start.size() == 1 && t.max_degree == 0);
}

void test_validation()
{
    auto base = [] { Set s; s.add({1, 2, 3}); s.add({3, 2, 4, 5}); return s; };
    auto bad = [&base](std::function<void(Set &)> change, uint32_t iterations = 1) {
        Set s = base();
        change(s);
        return s.problem(iterations) != nullptr;
    };
    CHECK(!bad([](Set &) {}));
    CHECK(!bad([](Set &s) { s.areas[1].rest_area = -0.0f; s.areas[1].stiffness = -0.0f; }));
    CHECK(!bad([](Set &s) { s.areas[1].rest_area = -3.0e38f; s.areas[1].stiffness = 1.0f; }, GPE_AREA_ITER_MAX));
    CHECK(bad([](Set &) {}, 0) && bad([](Set &) {}, GPE_AREA_ITER_MAX + 1));
    CHECK(bad([](Set &s) { s.areas[0].count = 2; }) && bad([](Set &s) { s.areas[1].count = GPE_AREA_MAX_MEMBERS + 1; }));
    CHECK(bad([](Set &s) { s.areas[1].first = 2; }));                   // overlap (and then a gap at the end)
    CHECK(bad([](Set &s) { s.areas[1].first = 4; s.uid.push_back(9); }));   // a gap
    CHECK(bad([](Set &s) { s.uid.push_back(9); }));                     // members left unused at the end
    CHECK(bad([](Set &s) { s.areas[1].count = 5; }));                   // runs past members
    CHECK(bad([](Set &s) { s.areas[1].first = 0xfffffffeu; }));         // first + count wraps in 32 bits: past members
    CHECK(bad([](Set &s) { s.uid[4] = GPE_UID_ABSENT; }));
    CHECK(bad([](Set &s) { s.uid[6] = 3; }));                           // a uid twice in one loop
    CHECK(bad([](Set &s) { s.areas[0].rest_area = NAN; }) && bad([](Set &s) { s.areas[0].rest_area = -INFINITY; }));
    CHECK(bad([](Set &s) { s.areas[0].stiffness = NAN; }) && bad([](Set &s) { s.areas[0].stiffness = 1.0000001f; }));
    CHECK(bad([](Set &s) { s.areas[0].stiffness = -0.25f; }));
    CHECK(bad([](Set &s) { s.areas[0].flags = 1; }) && bad([](Set &s) { s.areas[1].reserved = 1; }));
    const Set s = base();
    CHECK(area_set_problem(nullptr, 2, s.uid.data(), 7, 1) != nullptr && area_set_problem(s.areas.data(), 2, nullptr, 7, 1) != nullptr);
    CHECK(area_set_problem(s.areas.data(), (uint64_t)GPE_AREAS_MAX + 1, s.uid.data(), 7, 1) != nullptr);
    CHECK(area_set_problem(s.areas.data(), 2, s.uid.data(), (uint64_t)GPE_AREA_MEMBERS_MAX + 1, 1) != nullptr);
    // the targets of gpe_set_area_targets
    const float t[3] = {1.0f, -2.0f, 0.0f};
    CHECK(area_targets_problem(3, 0, 3, t) == nullptr && area_targets_problem(3, 3, 0, nullptr) == nullptr);
    CHECK(area_targets_problem(3, 1, 3, t) != nullptr && area_targets_problem(3, 4, 0, t) != nullptr);
    CHECK(area_targets_problem(3, 1, ~0ull, t) != nullptr && area_targets_problem(3, 0, 1, nullptr) != nullptr);
    const float n[1] = {NAN};
    CHECK(area_targets_problem(3, 2, 1, n) != nullptr);
}

void test_rule_by_hand()
{
    // the unit square, counter-clockwise, asked to double: area 1, C = -1, every |g|^2 = 0.5, D = 2, lambda = 0.5
    const float px[4] = {10.f, 11.f, 11.f, 10.f}, py[4] = {20.f, 20.f, 21.f, 21.f};
    const uint8_t live[4] = {1, 1, 1, 1};
    float corr[8], scratch[8], value[2];
    CHECK(area_pass_host(4, px, py, live, 2.0f, 1.0f, corr, scratch, value) == kAreaActs);
    CHECK(value[0] == 1.0f && value[1] == 0.5f);
    const float want[8] = {-0.25f, -0.25f, 0.25f, -0.25f, 0.25f, 0.25f, -0.25f, 0.25f};
    CHECK(std::memcmp(corr, want, sizeof(want)) == 0);
    // clockwise: the area is -1
    const float cx[4] = {10.f, 10.f, 11.f, 11.f}, cy[4] = {20.f, 21.f, 21.f, 20.f};
    CHECK(area_pass_host(4, cx, cy, live, -1.0f, 1.0f, corr, scratch, value) == kAreaActs && value[0] == -1.0f && value[1] == 0.0f);
    // a member without a particle, all members coincident, a NaN
    const uint8_t holed[4] = {1, 1, 0, 1};
    CHECK(area_pass_host(4, px, py, holed, 2.0f, 1.0f, corr, scratch, value) == kAreaInert && std::isnan(value[0]) && std::isnan(value[1]));
    const float zx[4] = {5.f, 5.f, 5.f, 5.f};
    CHECK(area_pass_host(4, zx, zx, live, 2.0f, 1.0f, corr, scratch, value) == kAreaInert);
    const float nx[4] = {10.f, NAN, 11.f, 10.f};
    CHECK(area_pass_host(4, nx, py, live, 2.0f, 1.0f, corr, scratch, value) == kAreaInert);
    const float hx[4] = {0.f, 3e19f, 3e19f, 0.f}, hy[4] = {0.f, 0.f, 3e19f, 3e19f};     // |g|^2 overflows
    CHECK(area_pass_host(4, hx, hy, live, 2.0f, 1.0f, corr, scratch, value) == kAreaInert);
}

bool read_hex(FILE *f, float *x)
{
    unsigned u = 0;
    if (std::fscanf(f, "%x", &u) != 1) return false;
    *x = float_of((uint32_t)u);
    return true;
}

// the model's table through the tables and the rule: the same verdicts, values, corrections and positions, bit for bit
void test_replay()
{
    if (g_table.empty()) { std::printf("replay: no --table given, nothing replayed\n"); return; }
    FILE *f = std::fopen(g_table.c_str(), "r");
    CHECK(f != nullptr);
    if (!f) return;
    unsigned n = 0, k = 0, members = 0;
    float W = 0.f, H = 0.f;
    bool ok = std::fscanf(f, "%u %u %u", &n, &k, &members) == 3 && read_hex(f, &W) && read_hex(f, &H) && n <= 1000000 &&
              k <= GPE_AREAS_MAX && members <= GPE_AREA_MEMBERS_MAX;
    if (!ok) { n = k = members = 0; }
    std::vector<float> pos(2 * (size_t)n), radius(n), want_value(2 * (size_t)k), want_corr(2 * (size_t)members), want_out(2 * (size_t)n);
    Set s;
    s.areas.resize(k);
    s.uid.resize(members);
    std::vector<unsigned> want_acts(k);
    for (unsigned i = 0; ok && i < n; ++i) ok = read_hex(f, &pos[2 * i]) && read_hex(f, &pos[2 * i + 1]) && read_hex(f, &radius[i]);
    for (unsigned j = 0; ok && j < k; ++j) {
        std::memset(&s.areas[j], 0, sizeof(gpe_area));
        ok = std::fscanf(f, "%u %u", &s.areas[j].first, &s.areas[j].count) == 2 && read_hex(f, &s.areas[j].rest_area) &&
             read_hex(f, &s.areas[j].stiffness);
    }
    for (unsigned i = 0; ok && i < members; ++i) ok = std::fscanf(f, "%u", &s.uid[i]) == 1;
    for (unsigned j = 0; ok && j < k; ++j)
        ok = std::fscanf(f, "%u", &want_acts[j]) == 1 && read_hex(f, &want_value[2 * j]) && read_hex(f, &want_value[2 * j + 1]);
    for (unsigned i = 0; ok && i < 2 * members; ++i) ok = read_hex(f, &want_corr[i]);
    for (unsigned i = 0; ok && i < 2 * n; ++i) ok = read_hex(f, &want_out[i]);
    std::fclose(f);
    CHECK(ok);
    if (!ok) return;
    CHECK(s.problem() == nullptr);
    if (s.problem() != nullptr) return;
    AreaTable t;
    area_table_build(s.areas.data(), k, s.uid.data(), members, &t);
    check_table(s, t);
    const Relaxed R = relax_by_table(t, pos, radius, W, H);
    unsigned acting = 0;
    for (unsigned j = 0; j < k; ++j) {
        CHECK((R.verdict[j] == kAreaActs) == (want_acts[j] == 1));
        if (R.verdict[j] != kAreaActs || want_acts[j] != 1) continue;
        ++acting;
        CHECK(std::memcmp(&R.value[2 * j], &want_value[2 * j], 8) == 0);
        CHECK(std::memcmp(&R.corr[2 * (size_t)s.areas[j].first], &want_corr[2 * (size_t)s.areas[j].first], 8 * (size_t)s.areas[j].count) == 0);
    }
    CHECK(acting > 0 || k == 0);
    CHECK(std::memcmp(R.out.data(), want_out.data(), want_out.size() * sizeof(float)) == 0);
    std::printf("replayed %u loops, %u acting, %u members, %u particles\n", k, acting, members, n);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"classes_and_order", test_classes_and_order},
    {"shared_members_and_csr", test_shared_members_and_csr},
    {"k0", test_k0},
    {"validation", test_validation},
    {"rule_by_hand", test_rule_by_hand},
    {"replay", test_replay},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (const Test &t : kTests) std::printf("%s\n", t.name);
        return 0;
    }
    if (argc > 2 && std::strcmp(argv[1], "--table") == 0) g_table = argv[2];
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
