// set_upload_tests.cpp -- the transaction that replaces a set's device tables (gpu-physics-engine_amd/csrc/set_upload.h)
// against a fake of the device calls that counts live blocks and fails its n-th call: after a failure anywhere nothing
// the transaction reserved is left, nothing is released twice, the caller's pointers are null, nothing but releases
// follows the failing call, and the first failure's status and text are what the caller gets.  No HIP, no library: the
// header alone.  The test that drives this builds it with -fsanitize=address,undefined.
//
// usage: set_upload_tests [--list]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/set_upload.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { ++g_failures; std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// The device calls, counted.  A block is real host memory (copies and fills write it, so the sanitizers see a write
// past a block or into a released one); call number fail_at (from 1, releases not counted) fails with status fail_at.
struct Fake {
    using Status = int;
    struct Shared {
        int calls = 0, fail_at = 0;
        int calls_after_failure = 0;         // reserve / copy / fill / wait issued behind the failing call
        bool failed = false;
        std::set<void *> live;
        int bad_releases = 0;                // of a block that is not live: released twice, or never reserved
        int releases = 0;
        std::string last_error, releases_said;
        std::vector<std::string> log;
    };
    Shared *s;
    std::string &last_error() { return s->last_error; }
    int begin(const std::string &what)
    {
        if (s->failed) ++s->calls_after_failure;
        s->log.push_back(what);
        if (++s->calls != s->fail_at) return 0;
        s->failed = true;
        s->last_error = what + " failed";
        return s->calls;
    }
    int reserve(const char *who, void **p, uint64_t bytes, const char *tag)
    {
        if (int st = begin(std::string(who) + ": reserve " + tag)) { *p = nullptr; return st; }
        *p = std::malloc(bytes);
        s->live.insert(*p);
        return 0;
    }
    void release(void *p)
    {
        ++s->releases;
        s->last_error = "a release reported damage";                   // (what a guarded release may do: the unwind must hide it)
        if (!s->live.erase(p)) { ++s->bad_releases; return; }
        std::free(p);
    }
    int copy(const char *who, const char *stage, void *dst, const void *src, uint64_t bytes)
    {
        if (int st = begin(std::string(who) + ": " + (stage ? stage : "-") + ": copy")) return st;
        std::memcpy(dst, src, bytes);
        return 0;
    }
    int fill(const char *who, const char *stage, void *dst, int byte, uint64_t bytes)
    {
        if (int st = begin(std::string(who) + ": " + (stage ? stage : "-") + ": fill")) return st;
        std::memset(dst, byte, bytes);
        return 0;
    }
    int wait(const char *who, const char *stage) { return begin(std::string(who) + ": " + (stage ? stage : "-") + ": wait"); }
    void free_all()
    {
        for (void *p : s->live) std::free(p);
        s->live.clear();
    }
};

using Upload = gpe::SetUpload<Fake>;

// what a gpe_set_* call does: five tables, three copies, two fills, the wait -- eleven backend calls
struct Tables {
    uint32_t *a = nullptr, *b = nullptr;
    float *c = nullptr;
    uint8_t *d = nullptr;
    unsigned long long *e = nullptr;
    bool all() const { return a && b && c && d && e; }
    bool none() const { return !a && !b && !c && !d && !e; }
};
const uint32_t kSrcA[4] = {1, 2, 3, 4};
const float kSrcC[3] = {1.f, 2.f, 3.f};
const unsigned long long kSrcE = 7;

void request_all(Upload &up, Tables &t)
{
    up.reserve(&t.a, 4, "t.a");
    up.reserve(&t.b, 6, "t.b");
    up.reserve(&t.c, 3, "t.c");
    up.reserve(&t.d, 5, "t.d");
    up.reserve(&t.e, 1, "t.e");
    up.copy(t.a, kSrcA, 4);
    up.copy(t.c, kSrcC, 3);
    up.copy(t.e, &kSrcE, 1);
    up.fill(t.b, 0xff, 6 * sizeof(uint32_t));
    up.fill(t.d, 0, 5);
}

void failing_call(int n)
{
    Fake::Shared sh;
    sh.fail_at = n;
    Tables t;
    Upload up(Fake{&sh}, "set");
    request_all(up, t);
    const int st = up.finish();
    CHECK(st == n);                                                    // the failing call's status ...
    CHECK(sh.last_error == sh.log[n - 1] + " failed");                 // ... and its text, not a release's
    CHECK(sh.live.empty());
    CHECK(sh.bad_releases == 0);
    CHECK(sh.releases == (n <= 5 ? n - 1 : 5));                        // what was reserved before it, each once
    CHECK(t.none());
    CHECK(sh.calls_after_failure == 0);
    CHECK(sh.calls == n);
    CHECK(up.finish() == n && sh.calls == n && sh.bad_releases == 0);  // (asked again: the same answer, no new call)
}

void no_failure()
{
    Fake::Shared sh;
    Tables t;
    {
        Upload up(Fake{&sh}, "set");
        request_all(up, t);
        CHECK(up.finish() == 0);
        CHECK(sh.calls == 11 && sh.log.back() == "set: upload: wait");
    }                                                                  // (destroyed after a success: the tables stay)
    CHECK(t.all() && sh.live.size() == 5 && sh.releases == 0 && sh.last_error.empty());
    CHECK(t.a[3] == 4 && t.c[2] == 3.f && *t.e == 7 && t.b[5] == 0xffffffffu && t.d[4] == 0);
    Fake{&sh}.free_all();
}

void an_optional_table_of_count_zero_is_skipped()
{
    Fake::Shared sh;
    uint32_t *need = nullptr, *optional = nullptr;
    Upload up(Fake{&sh}, "set", "grid upload");
    up.reserve(&need, 2, "t.need");
    up.reserve(&optional, 0, "t.optional");
    up.copy(optional, (const uint32_t *)nullptr, 0);                   // (and so are an empty copy and an empty fill)
    up.fill(optional, 0, 0);
    CHECK(up.finish() == 0);
    CHECK(need && !optional && sh.live.size() == 1);
    CHECK(sh.calls == 2 && sh.log[0] == "set: reserve t.need" && sh.log[1] == "set: grid upload: wait");
    Fake{&sh}.free_all();
}

void destroyed_without_finish()
{
    Fake::Shared sh;
    Tables t;
    {
        Upload up(Fake{&sh}, "set");
        request_all(up, t);
        CHECK(t.all() && sh.live.size() == 5);
        sh.last_error = "what the caller failed with";
    }
    CHECK(t.none() && sh.live.empty() && sh.releases == 5 && sh.bad_releases == 0);
    CHECK(sh.last_error == "what the caller failed with");
    CHECK(sh.calls == 10);                                             // (no wait)
}

void a_second_failure_does_not_replace_the_first()
{
    // every call from the third on would fail: only the third is ever issued
    Fake::Shared sh;
    sh.fail_at = 3;
    Tables t;
    Upload up(Fake{&sh}, "set", nullptr);
    request_all(up, t);
    sh.fail_at = 4;                                                    // (a later call would fail too, were it issued)
    CHECK(up.finish() == 3 && sh.calls == 3 && sh.last_error == "set: reserve t.c failed");
    CHECK(t.none() && sh.live.empty() && sh.releases == 2 && sh.bad_releases == 0);
}

struct Test { const char *name; std::function<void()> run; };

}  // namespace

int main(int argc, char **argv)
{
    std::vector<Test> tests;
    static const char *const kCalls[11] = {"reserve_1", "reserve_2", "reserve_3", "reserve_4", "reserve_5", "copy_1",
                                           "copy_2", "copy_3", "fill_1", "fill_2", "wait"};
    static std::string names[11];
    for (int n = 1; n <= 11; ++n) {
        names[n - 1] = std::string("failing_") + kCalls[n - 1];
        tests.push_back({names[n - 1].c_str(), [n] { failing_call(n); }});
    }
    tests.push_back({"no_failure", no_failure});
    tests.push_back({"an_optional_table_of_count_zero_is_skipped", an_optional_table_of_count_zero_is_skipped});
    tests.push_back({"destroyed_without_finish", destroyed_without_finish});
    tests.push_back({"a_second_failure_does_not_replace_the_first", a_second_failure_does_not_replace_the_first});
    if (argc > 1 && !std::strcmp(argv[1], "--list")) {
        for (const Test &t : tests) std::printf("%s\n", t.name);
        return 0;
    }
    for (const Test &t : tests) {
        const int before = g_failures;
        t.run();
        std::printf("test %s ... %s\n", t.name, g_failures == before ? "ok" : "FAILED");
    }
    return g_failures ? 1 : 0;
}
