// uid_nodes_tests.cpp -- the node list and the rows every uid-named step set builds on the host
// (gpu-physics-engine_amd/csrc/uid_nodes.h), on the CPU: nodes ascending and distinct, every incidence under its uid's
// node, the rows a CSR whose positions place every incidence exactly once and in incidence order, max_degree the
// longest row.  No HIP, no library: the header alone.
//
// usage: uid_nodes_tests [--list]
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/uid_nodes.h"

using namespace gpe;

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { if (++g_failures < 20) std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// what every result must satisfy, whatever the incidences; the counts come from a direct count per uid
void check_nodes(const std::vector<uint32_t> &uid, const UidNodes &u)
{
    const size_t count = uid.size(), m = u.nodes.size();
    std::map<uint32_t, uint32_t> direct;
    for (uint32_t x : uid) direct[x] += 1;
    CHECK(m == direct.size());
    CHECK(u.node_of.size() == count && u.at.size() == count && u.row_start.size() == m + 1);
    if (u.node_of.size() != count || u.at.size() != count || u.row_start.size() != m + 1 || m != direct.size()) return;
    CHECK(u.row_start[0] == 0 && u.row_start[m] == count);
    for (size_t v = 1; v < m; ++v) CHECK(u.nodes[v - 1] < u.nodes[v]);
    uint32_t longest = 0;
    for (size_t v = 0; v < m; ++v) {
        CHECK(u.row_start[v] <= u.row_start[v + 1]);
        CHECK(u.row_start[v + 1] - u.row_start[v] == direct[u.nodes[v]]);
        longest = std::max(longest, direct[u.nodes[v]]);
    }
    CHECK(u.max_degree == longest);
    std::vector<int> taken(count, 0);
    std::vector<int64_t> last(m, -1);                                   // per node: the position of its latest incidence
    for (size_t e = 0; e < count; ++e) {
        const uint32_t v = u.node_of[e], p = u.at[e];
        CHECK(v < m && p < count);
        if (!(v < m && p < count)) return;
        CHECK(u.nodes[v] == uid[e]);
        CHECK(p >= u.row_start[v] && p < u.row_start[v + 1]);
        CHECK((int64_t)p > last[v]);                                    // positions in a row ascend with incidence order
        last[v] = p;
        taken[p] += 1;
    }
    for (size_t p = 0; p < count; ++p) CHECK(taken[p] == 1);
}

UidNodes build(const std::vector<uint32_t> &uid)
{
    UidNodes u;
    uid_nodes_build(uid.data(), uid.size(), &u);
    check_nodes(uid, u);
    return u;
}

void test_no_incidences()
{
    UidNodes u;
    uid_nodes_build(nullptr, 0, &u);
    CHECK(u.nodes.empty() && u.node_of.empty() && u.at.empty() && u.max_degree == 0);
    CHECK(u.row_start.size() == 1 && u.row_start[0] == 0);
}

void test_one_uid()
{
    for (uint32_t times : {1u, 2u, 65u}) {
        const UidNodes u = build(std::vector<uint32_t>(times, 7u));
        CHECK(u.nodes.size() == 1 && u.nodes[0] == 7u && u.max_degree == times);
        for (uint32_t e = 0; e < times && e < u.at.size(); ++e) CHECK(u.at[e] == e && u.node_of[e] == 0);
    }
}

void test_descending_uids()
{
    const UidNodes u = build({900u, 40u, 40u, 3u, 0u});
    CHECK(u.nodes == std::vector<uint32_t>({0u, 3u, 40u, 900u}));
    CHECK(u.node_of == std::vector<uint32_t>({3u, 2u, 2u, 1u, 0u}));
    CHECK(u.row_start == std::vector<uint32_t>({0u, 1u, 2u, 4u, 5u}));
    CHECK(u.at == std::vector<uint32_t>({4u, 2u, 3u, 1u, 0u}));
    CHECK(u.max_degree == 2);
}

void test_random_incidences()
{
    std::mt19937 rng(20250611u);
    std::vector<uint32_t> pool(37);
    for (uint32_t &x : pool) x = rng();                                 // (equal draws only make the pool smaller)
    pool[0] = 0u;
    pool[1] = 0xfffffffeu;
    std::vector<uint32_t> uid(1000);
    for (uint32_t &x : uid) x = pool[rng() % pool.size()];
    const UidNodes u = build(uid);
    CHECK(u.nodes.size() <= 37 && u.nodes.size() > 1);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"no_incidences", test_no_incidences},
    {"one_uid", test_one_uid},
    {"descending_uids", test_descending_uids},
    {"random_incidences", test_random_incidences},
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
