// scope_events_tests.cpp -- the bookkeeping behind the profiling scopes (gpu-physics-engine_amd/csrc/scope_events.h)
// against a stub of the event calls: which scopes share an event, how many records a step costs, and that every event
// goes back to the pool -- and is destroyed -- exactly once.  No HIP, no library: the header alone.  The test that
// drives this builds it with -fsanitize=address,undefined.
//
// usage: scope_events_tests [--list]
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/scope_events.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { ++g_failures; std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// The event calls, counted.  An event is a number; record() stamps it with the position of the stream it marks: the
// number of enqueues so far.
struct Stub {
    using Event = int;
    struct Shared {
        int created = 0, destroyed = 0, records = 0, enqueues = 0, fail_creates_from = -1;
        std::map<int, int> stamp;        // event -> enqueues before its last record
        std::map<int, int> destroyed_of; // event -> times destroyed
    };
    Shared *s;
    bool create(int *e)
    {
        if (s->fail_creates_from >= 0 && s->created >= s->fail_creates_from) return false;
        *e = 100 + s->created++;
        return true;
    }
    void record(int e) { ++s->records; s->stamp[e] = s->enqueues; }
    void destroy(int e) { ++s->destroyed; ++s->destroyed_of[e]; }
};

using Events = gpe::ScopeEvents<Stub>;

// what the library's Scope does, and what its launch helpers do
struct Fixture {
    Stub::Shared sh;
    Stub be{&sh};
    Events ev;
    std::vector<std::string> names;
    struct Resolved { std::string name; int start, stop; };

    struct Scope {
        Fixture &f;
        int stat, start;
        bool shared;
        Scope(Fixture &fx, const char *name, bool sh_ = true) : f(fx), shared(sh_)
        {
            f.names.push_back(name);
            stat = (int)f.names.size() - 1;
            start = f.ev.open(f.be, shared);
        }
        ~Scope() { f.ev.close(f.be, start, stat, shared); }
    };
    void enqueue() { ++sh.enqueues; ev.note_enqueue(); }
    std::vector<Resolved> resolve()
    {
        std::vector<Resolved> out;
        ev.resolve([&](int stat, int a, int b) { out.push_back({names[stat], a, b}); });
        return out;
    }
    static const Resolved &find(const std::vector<Resolved> &v, const std::string &name, int nth = 0)
    {
        static const Resolved none{"", -1, -1};
        for (const Resolved &r : v)
            if (r.name == name && nth-- == 0) return r;
        ++g_failures;
        std::fprintf(stderr, "no resolved scope %s\n", name.c_str());
        return none;
    }
};

// the scopes and launches of a native step that keeps its table (gpe_native.hip, onesweep_sort with two passes)
void native_step(Fixture &f)
{
    f.ev.enter_region();
    {
        Fixture::Scope s(f, "native/hash");
        f.enqueue();
    }
    {
        Fixture::Scope s(f, "native/sort");
        f.enqueue();                                         // the gated histogram
        for (int p = 0; p < 2; ++p) {
            Fixture::Scope o(f, "sort/onesweep");
            f.enqueue();
        }
    }
    {
        Fixture::Scope s(f, "native/collide+verlet");
        f.enqueue();
    }
    {
        Fixture::Scope s(f, "native/collide-dense-regions");
        f.enqueue();
    }
    f.ev.leave_region();
}

void test_own_events_outside_a_region()
{
    Fixture f;
    {
        Fixture::Scope a(f, "a");
        f.enqueue();
    }
    {
        Fixture::Scope b(f, "b");                            // nothing enqueued since a's stop -- but nobody vouches for that here
        f.enqueue();
    }
    CHECK(f.sh.records == 4);
    const auto r = f.resolve();
    CHECK(r.size() == 2 && r[0].stop != r[1].start);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 4);
}

void test_native_step_records_seven_events()
{
    Fixture f;
    native_step(f);
    CHECK(f.sh.records == 7);
    CHECK(f.ev.pending() == 6);
    const auto r = f.resolve();
    CHECK(r.size() == 6);
    // closing order: nested scopes before their parent, as before
    const char *order[] = {"native/hash", "sort/onesweep", "sort/onesweep", "native/sort", "native/collide+verlet",
                           "native/collide-dense-regions"};
    for (size_t i = 0; i < r.size() && i < 6; ++i) CHECK(r[i].name == order[i]);
    const auto &hash = Fixture::find(r, "native/hash"), &sort = Fixture::find(r, "native/sort");
    const auto &p1 = Fixture::find(r, "sort/onesweep", 0), &p2 = Fixture::find(r, "sort/onesweep", 1);
    const auto &col = Fixture::find(r, "native/collide+verlet"), &dense = Fixture::find(r, "native/collide-dense-regions");
    CHECK(hash.stop == sort.start);                          // hash | sort
    CHECK(p1.start != sort.start);                           // the gated histogram lies between
    CHECK(p1.stop == p2.start);                              // pass 1 | pass 2
    CHECK(p2.stop == sort.stop && sort.stop == col.start);   // pass 2 | collide, which also closes native/sort
    CHECK(col.stop == dense.start);                          // collide | dense regions
    CHECK(hash.start != hash.stop && dense.start != dense.stop);
    // every scope brackets exactly its own launches: stamps are enqueue counts
    CHECK(f.sh.stamp[hash.start] == 0 && f.sh.stamp[hash.stop] == 1);
    CHECK(f.sh.stamp[sort.start] == 1 && f.sh.stamp[p1.start] == 2 && f.sh.stamp[p1.stop] == 3);
    CHECK(f.sh.stamp[p2.stop] == 4 && f.sh.stamp[col.stop] == 5 && f.sh.stamp[dense.stop] == 6);
    CHECK(f.ev.outstanding() == 0 && f.ev.created() == 7 && f.ev.pooled() == 7);
}

void test_events_are_reused_step_after_step()
{
    Fixture f;
    for (int step = 0; step < 5; ++step) native_step(f);
    CHECK(f.sh.records == 35 && f.ev.created() == 35);       // nothing resolved yet: every event still pending
    CHECK(f.resolve().size() == 30);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 35);
    for (int step = 0; step < 5; ++step) { native_step(f); f.resolve(); }
    CHECK(f.ev.created() == 35 && f.sh.created == 35);       // from the pool
    CHECK(f.ev.outstanding() == 0);
}

void test_enqueue_between_two_nested_scopes()
{
    Fixture f;
    f.ev.enter_region();
    {
        Fixture::Scope parent(f, "parent");
        {
            Fixture::Scope a(f, "a");
            f.enqueue();
        }
        f.enqueue();                                         // belongs to the parent alone
        {
            Fixture::Scope b(f, "b");
            f.enqueue();
        }
    }
    f.ev.leave_region();
    const auto r = f.resolve();
    const auto &a = Fixture::find(r, "a"), &b = Fixture::find(r, "b"), &p = Fixture::find(r, "parent");
    CHECK(p.start == a.start);                               // nothing between the parent's opening and a's
    CHECK(a.stop != b.start);
    CHECK(f.sh.stamp[a.stop] == 1 && f.sh.stamp[b.start] == 2);
    CHECK(p.stop == b.stop);
    CHECK(f.sh.records == 4);
    CHECK(f.ev.outstanding() == 0);
}

void test_enqueue_behind_the_last_nested_scope()
{
    Fixture f;
    f.ev.enter_region();
    {
        Fixture::Scope parent(f, "parent");
        {
            Fixture::Scope a(f, "a");
            f.enqueue();
        }
        f.enqueue();
    }
    f.ev.leave_region();
    const auto r = f.resolve();
    const auto &a = Fixture::find(r, "a"), &p = Fixture::find(r, "parent");
    CHECK(p.stop != a.stop && f.sh.stamp[p.stop] == 2 && f.sh.stamp[a.stop] == 1);
    CHECK(f.ev.outstanding() == 0);
}

void test_a_scope_nobody_vouches_for_keeps_its_pair()
{
    Fixture f;
    f.ev.enter_region();
    {
        Fixture::Scope a(f, "a");
        f.enqueue();
    }
    {
        Fixture::Scope own(f, "own", false);                 // e.g. a scope around launches that do not call note_enqueue
        ++f.sh.enqueues;                                     // ... such as this one
    }
    {
        Fixture::Scope b(f, "b");
        f.enqueue();
    }
    f.ev.leave_region();
    const auto r = f.resolve();
    const auto &a = Fixture::find(r, "a"), &own = Fixture::find(r, "own"), &b = Fixture::find(r, "b");
    CHECK(own.start != a.stop && own.stop != own.start);
    CHECK(b.start != own.stop && b.start != a.stop);
    CHECK(f.sh.stamp[b.start] == 2);
    CHECK(f.sh.records == 6);
    CHECK(f.ev.outstanding() == 0);
}

void test_boundaries_are_not_shared_across_a_region_s_ends()
{
    Fixture f;
    {
        Fixture::Scope before(f, "before");
        f.enqueue();
    }
    ++f.sh.enqueues;                                         // work outside the region, unannounced
    f.ev.enter_region();
    {
        Fixture::Scope in(f, "in");
        f.enqueue();
    }
    f.ev.leave_region();
    ++f.sh.enqueues;
    {
        Fixture::Scope after(f, "after");
        f.enqueue();
    }
    f.ev.enter_region();                                     // the next step's region: nothing of the last one's is left
    {
        Fixture::Scope next(f, "next");
        f.enqueue();
    }
    f.ev.leave_region();
    const auto r = f.resolve();
    CHECK(f.sh.records == 8);
    CHECK(Fixture::find(r, "in").start != Fixture::find(r, "before").stop);
    CHECK(Fixture::find(r, "after").start != Fixture::find(r, "in").stop);
    CHECK(Fixture::find(r, "next").start != Fixture::find(r, "in").stop);
    CHECK(f.sh.stamp[Fixture::find(r, "in").start] == 2 && f.sh.stamp[Fixture::find(r, "after").start] == 4);
    CHECK(f.ev.outstanding() == 0 && !f.ev.in_region());
}

void test_an_empty_scope_takes_one_event()
{
    Fixture f;
    f.ev.enter_region();
    {
        Fixture::Scope e(f, "empty");
    }
    f.ev.leave_region();
    const auto r = f.resolve();
    CHECK(r.size() == 1 && r[0].start == r[0].stop);
    CHECK(f.sh.records == 1);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 1);
}

void test_resolving_in_the_middle_keeps_the_boundary()
{
    // gpe_get_timings between two scopes of a region (no library path does that today; the bookkeeping must not care):
    // the boundary event is still held, so the pool cannot hand it out to be recorded again
    Fixture f;
    f.ev.enter_region();
    {
        Fixture::Scope a(f, "a");
        f.enqueue();
    }
    const auto r1 = f.resolve();
    CHECK(f.ev.outstanding() == 1);                          // the boundary
    {
        Fixture::Scope b(f, "b");
        f.enqueue();
        const auto r2 = f.resolve();                         // with b open
        CHECK(r2.empty() && f.ev.outstanding() == 1);        // b's start is the boundary
    }
    f.ev.leave_region();
    const auto r3 = f.resolve();
    CHECK(r1.size() == 1 && r3.size() == 1 && r3[0].start == r1[0].stop && r3[0].stop != r3[0].start);
    CHECK(f.sh.stamp[r3[0].start] == 1 && f.sh.stamp[r3[0].stop] == 2);
    CHECK(f.ev.outstanding() == 0 && f.ev.created() == 2);      // (b's stop is a's start, back from the pool)
}

void test_reset_and_profiling_off_and_on()
{
    // gpe_reset_timings = resolve and forget the results; gpe_set_profiling(0) = scopes stop opening; pending pairs stay
    // until somebody resolves them
    Fixture f;
    native_step(f);
    native_step(f);
    f.resolve();                                             // reset in the middle of a run
    CHECK(f.ev.outstanding() == 0);
    native_step(f);                                          // ... profiling goes off with these pending
    CHECK(f.ev.outstanding() == 7 && f.ev.pending() == 6);
    native_step(f);                                          // and on again
    CHECK(f.resolve().size() == 12);
    CHECK(f.ev.outstanding() == 0 && f.ev.created() == 14 && f.ev.pooled() == 14);
}

void test_destroy_with_scopes_pending()
{
    Fixture f;
    native_step(f);
    f.resolve();
    native_step(f);
    native_step(f);                                          // 12 pairs pending over 14 events
    CHECK(f.ev.pending() == 12 && f.ev.created() == 14);
    f.ev.destroy_all(f.be);
    CHECK(f.sh.destroyed == 14 && f.sh.created == 14);
    for (const auto &kv : f.sh.destroyed_of) CHECK(kv.second == 1);
    CHECK(f.ev.created() == 0 && f.ev.outstanding() == 0 && f.ev.pending() == 0);
    f.ev.destroy_all(f.be);                                  // again: nothing left to destroy
    CHECK(f.sh.destroyed == 14);
}

void test_event_creation_fails()
{
    Fixture f;
    f.sh.fail_creates_from = 1;                              // one event, then none
    f.ev.enter_region();
    {
        Fixture::Scope a(f, "a");
        f.enqueue();
    }                                                        // no stop event: the scope is dropped, its start goes back
    CHECK(f.ev.pending() == 0);
    f.sh.fail_creates_from = 0;
    {
        Fixture::Scope b(f, "b");                            // the one event is the boundary's, nothing can be created:
        f.enqueue();                                         // this scope records nothing at all
    }
    f.ev.leave_region();
    CHECK(f.ev.pending() == 0 && f.ev.outstanding() == 0 && f.ev.created() == 1);
    f.sh.fail_creates_from = -1;
    native_step(f);
    CHECK(f.resolve().size() == 6 && f.ev.outstanding() == 0);
    f.ev.destroy_all(f.be);
    CHECK(f.sh.destroyed == f.sh.created);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"own_events_outside_a_region", test_own_events_outside_a_region},
    {"native_step_records_seven_events", test_native_step_records_seven_events},
    {"events_are_reused_step_after_step", test_events_are_reused_step_after_step},
    {"enqueue_between_two_nested_scopes", test_enqueue_between_two_nested_scopes},
    {"enqueue_behind_the_last_nested_scope", test_enqueue_behind_the_last_nested_scope},
    {"a_scope_nobody_vouches_for_keeps_its_pair", test_a_scope_nobody_vouches_for_keeps_its_pair},
    {"boundaries_are_not_shared_across_a_region_s_ends", test_boundaries_are_not_shared_across_a_region_s_ends},
    {"an_empty_scope_takes_one_event", test_an_empty_scope_takes_one_event},
    {"resolving_in_the_middle_keeps_the_boundary", test_resolving_in_the_middle_keeps_the_boundary},
    {"reset_and_profiling_off_and_on", test_reset_and_profiling_off_and_on},
    {"destroy_with_scopes_pending", test_destroy_with_scopes_pending},
    {"event_creation_fails", test_event_creation_fails},
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
