// scope_stamps_tests.cpp -- the timestamp-slot backend of the profiling scopes (gpu-physics-engine_amd/csrc/
// scope_stamps.h) under ScopeEvents (scope_events.h), against a stub of the device: the sequences of
// scope_events_tests.cpp, and what is this backend's own -- who writes each stamp (a kernel of its own, or the launch
// that starts at the boundary), that every slot comes back to the pool exactly once, and that the buffer never grows
// while a slot is referenced.  No HIP, no library: the two headers alone.  The test that drives this builds it with
// -fsanitize=address,undefined.
//
// usage: scope_stamps_tests [--list]
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/csrc/scope_events.h"
#include "../../gpu-physics-engine_amd/csrc/scope_stamps.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { ++g_failures; std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// The device, counted.  The buffer is a vector; a stamp is the position of the stream it marks: the number of the
// library's own enqueues so far (the one-thread kernels are not counted: they are the clock, not the work).
struct Shared {
    std::vector<long> buf;               // -1: never stamped since the buffer was (re)allocated
    int enqueues = 0, stamp_kernels = 0, grows = 0, grows_with_slots_referenced = 0, fail_grows_from = -1;
    std::function<size_t()> outstanding; // of the ScopeEvents the backend serves
};
struct StubDev {
    Shared *s = nullptr;
    bool grow(uint32_t old_slots, uint32_t new_slots)
    {
        if (s->fail_grows_from >= 0 && s->grows >= s->fail_grows_from) return false;
        if (s->outstanding() != 0) ++s->grows_with_slots_referenced;
        std::vector<long> fresh(new_slots, -1);
        if (old_slots) fresh[0] = s->buf[0];                 // the origin's slot is kept
        s->buf.swap(fresh);
        ++s->grows;
        return true;
    }
    void stamp(uint32_t slot)
    {
        ++s->stamp_kernels;
        s->buf.at(slot) = s->enqueues;
    }
};

using Backend = gpe::StampBackend<StubDev>;
using Recorder = gpe::StampRecorder<StubDev>;
using Events = gpe::ScopeEvents<Recorder>;

// what the library's Scope, note_enqueue, ScopeRegion, launchers and stamps_make_room do
struct Fixture {
    Shared sh;
    Backend be;
    Recorder at_once{be, false};                             // a record with no hint
    Events ev;
    std::vector<std::string> names;
    std::multiset<uint32_t> resolved_slots;                  // every slot a resolved pair named
    int resolves = 0;
    struct Resolved { std::string name; uint32_t start, stop; };

    Fixture()
    {
        be.dev.s = &sh;
        sh.outstanding = [this] { return ev.outstanding(); };
    }
    enum : unsigned { kCarryStart = 1u, kCarryStop = 2u };   // Scope::Carry: the opening's / closing's stamp is owed to the next enqueue
    struct Scope {
        Fixture &f;
        int stat, start;
        bool shared;
        unsigned carry;
        Scope(Fixture &fx, const char *name, bool sh_ = true, unsigned carry_ = 0u) : f(fx), shared(sh_), carry(carry_)
        {
            f.names.push_back(name);
            stat = (int)f.names.size() - 1;
            if (!f.ev.in_region()) f.make_room(2);
            Recorder r{f.be, shared && (carry & kCarryStart) && f.ev.in_region()};
            start = f.ev.open(r, shared);
        }
        ~Scope()
        {
            if (start < 0) return;
            Recorder r{f.be, shared && (carry & kCarryStop) && f.ev.in_region()};
            f.ev.close(r, start, stat, shared);
        }
    };
    void enter() { ev.enter_region(); }
    void leave() { be.flush(); ev.leave_region(); }
    void enqueue() { ev.note_enqueue(); be.flush(); ++sh.enqueues; }
    void enqueue_gated()                                     // a launch whose first workgroup writes the owed stamp
    {
        const int64_t slot = be.take();
        ev.note_enqueue();
        be.flush();
        if (slot >= 0) sh.buf.at((size_t)slot) = sh.enqueues;
        ++sh.enqueues;
    }
    std::vector<Resolved> resolve()
    {
        std::vector<Resolved> out;
        ev.resolve([&](int stat, uint32_t a, uint32_t b) {
            out.push_back({names[stat], a, b});
            resolved_slots.insert(a);
            resolved_slots.insert(b);
        });
        return out;
    }
    void make_room(uint32_t need)
    {
        be.make_room(ev, need, [this] { ++resolves; resolve(); return true; });
    }
    long at(uint32_t slot) const { return sh.buf.at(slot); }
    static const Resolved &find(const std::vector<Resolved> &v, const std::string &name, int nth = 0)
    {
        static const Resolved none{"", 0, 0};
        for (const Resolved &r : v)
            if (r.name == name && nth-- == 0) return r;
        ++g_failures;
        std::fprintf(stderr, "no resolved scope %s\n", name.c_str());
        return none;
    }
};

// the scopes and launches of a native step that keeps its table (gpe_native.hip, onesweep_sort with two passes), behind
// the room do_step makes
void native_step(Fixture &f)
{
    f.make_room(64);
    f.enter();
    {
        Fixture::Scope s(f, "native/hash", true, Fixture::kCarryStop);   // (its launch comes at once: nothing to owe in front)
        f.enqueue();
    }
    {
        Fixture::Scope s(f, "native/sort");
        f.enqueue_gated();                                   // the gated histogram
        for (int p = 0; p < 2; ++p) {
            Fixture::Scope o(f, "sort/onesweep", true, Fixture::kCarryStart | Fixture::kCarryStop);
            f.enqueue_gated();
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
    f.leave();
}

void test_native_step_records_seven_stamps()
{
    Fixture f;
    native_step(f);
    CHECK(f.be.records == 7);
    CHECK(f.be.carried == 3 && f.be.kernels == 4 && f.sh.stamp_kernels == 4);   // the three gated sort launches carry theirs
    CHECK(f.be.owed < 0);
    CHECK(f.ev.pending() == 6);
    const auto r = f.resolve();
    CHECK(r.size() == 6);
    const char *order[] = {"native/hash", "sort/onesweep", "sort/onesweep", "native/sort", "native/collide+verlet",
                           "native/collide-dense-regions"};
    for (size_t i = 0; i < r.size() && i < 6; ++i) CHECK(r[i].name == order[i]);
    const auto &hash = Fixture::find(r, "native/hash"), &sort = Fixture::find(r, "native/sort");
    const auto &p1 = Fixture::find(r, "sort/onesweep", 0), &p2 = Fixture::find(r, "sort/onesweep", 1);
    const auto &col = Fixture::find(r, "native/collide+verlet"), &dense = Fixture::find(r, "native/collide-dense-regions");
    CHECK(hash.stop == sort.start && p1.start != sort.start && p1.stop == p2.start);
    CHECK(p2.stop == sort.stop && sort.stop == col.start && col.stop == dense.start);
    // every scope brackets exactly its own launches, whoever wrote the stamp
    CHECK(f.at(hash.start) == 0 && f.at(hash.stop) == 1 && f.at(p1.start) == 2 && f.at(p1.stop) == 3);
    CHECK(f.at(p2.stop) == 4 && f.at(col.stop) == 5 && f.at(dense.stop) == 6);
    CHECK(f.ev.outstanding() == 0 && f.ev.created() == 7 && f.ev.pooled() == 7);
    CHECK(hash.start != gpe::kStampOrigin && f.at(gpe::kStampOrigin) == -1);   // slot 0 is nobody's but the origin's
}

void test_scopes_outside_a_region_are_stamped_at_once()
{
    Fixture f;
    {
        Fixture::Scope a(f, "a");
        CHECK(f.be.owed < 0 && f.sh.stamp_kernels == 1);     // nobody announces the next enqueue here
        ++f.sh.enqueues;                                     // ... such as this one
    }
    {
        Fixture::Scope b(f, "b");
        f.enqueue();
    }
    CHECK(f.be.records == 4 && f.be.kernels == 4 && f.be.carried == 0);
    const auto r = f.resolve();
    CHECK(r.size() == 2 && r[0].stop != r[1].start);
    CHECK(f.at(r[0].start) == 0 && f.at(r[0].stop) == 1 && f.at(r[1].start) == 1 && f.at(r[1].stop) == 2);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 4);
}

void test_a_scope_nobody_vouches_for_is_stamped_at_once_inside_a_region()
{
    Fixture f;
    f.make_room(64);
    f.enter();
    {
        Fixture::Scope a(f, "a");
        f.enqueue();
    }
    {
        Fixture::Scope own(f, "own", false);                 // written at once, like a's stop before it
        CHECK(f.be.owed < 0 && f.sh.stamp_kernels == 3);
        ++f.sh.enqueues;                                     // a launch that does not call note_enqueue
    }
    {
        Fixture::Scope b(f, "b");
        f.enqueue();
    }
    f.leave();
    const auto r = f.resolve();
    const auto &a = Fixture::find(r, "a"), &own = Fixture::find(r, "own"), &b = Fixture::find(r, "b");
    CHECK(f.at(a.stop) == 1 && f.at(own.start) == 1 && f.at(own.stop) == 2 && f.at(b.start) == 2 && f.at(b.stop) == 3);
    CHECK(own.start != a.stop && b.start != own.stop);
    CHECK(f.be.records == 6 && f.be.carried == 0);
    CHECK(f.ev.outstanding() == 0);
}

void test_the_region_s_end_pays_what_is_owed()
{
    Fixture f;
    f.make_room(64);
    f.enter();
    {
        Fixture::Scope a(f, "a", true, Fixture::kCarryStart | Fixture::kCarryStop);
        CHECK(f.be.owed >= 0 && f.sh.stamp_kernels == 0);
        f.enqueue_gated();                                   // carries a's start
    }
    CHECK(f.be.owed >= 0);                                   // a's stop: the launch it was promised never comes
    f.leave();
    CHECK(f.be.owed < 0 && f.be.carried == 1 && f.be.kernels == 1);
    ++f.sh.enqueues;                                         // the next call's work: not inside a
    const auto r = f.resolve();
    CHECK(r.size() == 1 && f.at(r[0].start) == 0 && f.at(r[0].stop) == 1);
}

void test_an_enqueue_that_cannot_carry_pays_first()
{
    Fixture f;
    f.make_room(64);
    f.enter();
    {
        Fixture::Scope a(f, "a", true, Fixture::kCarryStart | Fixture::kCarryStop);
        f.enqueue();                                         // not a gated launch: a's start is written in front of it
        CHECK(f.be.owed < 0 && f.sh.stamp_kernels == 1 && f.be.carried == 0);
    }
    {
        Fixture::Scope b(f, "b");                            // shares a's stop, which is still owed
        CHECK(f.be.owed >= 0 && f.be.records == 2);
        f.enqueue();
    }
    CHECK(f.be.owed < 0);                                    // no hint: b's stop was written at once
    f.leave();
    const auto r = f.resolve();
    const auto &a = Fixture::find(r, "a"), &b = Fixture::find(r, "b");
    CHECK(a.stop == b.start && f.at(a.start) == 0 && f.at(a.stop) == 1 && f.at(b.stop) == 2);
    CHECK(f.be.records == 3 && f.be.kernels == 3 && f.be.carried == 0 && f.ev.outstanding() == 0);
}

void test_every_slot_comes_back_exactly_once()
{
    Fixture f;
    for (int step = 0; step < 5; ++step) native_step(f);
    CHECK(f.be.records == 35 && f.ev.created() == 35);       // nothing resolved yet: every slot still pending
    CHECK(f.resolve().size() == 30);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 35);
    // 60 references in all: a step's first and last boundary are named by one pair, its five inner ones by two ...
    CHECK(f.resolved_slots.size() == 60);
    std::set<uint32_t> distinct(f.resolved_slots.begin(), f.resolved_slots.end());
    CHECK(distinct.size() == 35 && *distinct.begin() == 1 && *distinct.rbegin() == 35);
    // ... and each came back once: five more steps take the same 35 from the pool, none twice at a time
    std::set<uint32_t> again;
    for (int step = 0; step < 5; ++step) native_step(f);
    CHECK(f.ev.created() == 35 && f.be.next == 36 && f.ev.pooled() == 0);
    for (const auto &r : f.resolve()) { again.insert(r.start); again.insert(r.stop); }
    CHECK(again == distinct);
    CHECK(f.ev.outstanding() == 0 && f.ev.pooled() == 35 && f.sh.grows == 1);
}

void test_reset_and_profiling_off_and_on()
{
    Fixture f;
    native_step(f);
    native_step(f);
    f.resolve();                                             // gpe_reset_timings in the middle of a run
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
    native_step(f);                                          // 12 pairs pending over 14 slots
    CHECK(f.ev.pending() == 12 && f.ev.created() == 14);
    f.ev.destroy_all(f.at_once);
    CHECK(f.ev.created() == 0 && f.ev.outstanding() == 0 && f.ev.pending() == 0);
    f.ev.destroy_all(f.at_once);                                  // again: nothing left
    CHECK(f.sh.grows == 1 && f.sh.grows_with_slots_referenced == 0);
}

void test_the_buffer_grows_only_with_no_slot_referenced()
{
    Fixture f;
    const uint32_t first = gpe::kStampSlotsFirst;
    f.make_room(1);
    f.be.dev.stamp(gpe::kStampOrigin);                       // gpe_set_profiling: the trace origin
    CHECK(f.be.capacity == first && f.sh.grows == 1);
    // profiling on every step and nobody reads the timings: 7 slots a step until fewer than 64 are left
    int steps = 0;
    while (f.resolves == 0 && steps < 100000) { native_step(f); ++steps; }
    CHECK(steps == (int)((first - 1 - 64) / 7) + 2);         // the step that found fewer than 64 resolved first
    CHECK(f.resolves == 1 && f.sh.grows == 2 && f.be.capacity == 2 * first);
    CHECK(f.sh.grows_with_slots_referenced == 0);
    CHECK(f.at(gpe::kStampOrigin) == 0);                     // the origin's stamp moved with the buffer
    CHECK(f.ev.pending() == 6);                              // that step's own pairs
    // a scope open around the caller holds a slot: nothing may move, however little room is left
    f.resolve();
    {
        Fixture::Scope outer(f, "outer", false);
        const uint32_t cap = f.be.capacity;
        f.be.next = cap;                                     // (as if every slot had been handed out)
        std::vector<int> taken;
        while (f.ev.pooled() > 0) taken.push_back(f.ev.open(f.at_once, false));
        f.make_room(64);
        CHECK(f.be.capacity == cap && f.sh.grows == 2 && f.sh.grows_with_slots_referenced == 0);
        {
            Fixture::Scope dropped(f, "dropped", false);     // no slot: the scope records nothing
            CHECK(dropped.start < 0);
        }
        for (int s : taken) f.ev.close(f.at_once, s, 0, false);
    }
    f.resolve();
    CHECK(f.ev.outstanding() == 0);
    f.be.next = f.be.capacity;
    const size_t pooled = f.ev.pooled();
    f.make_room((uint32_t)pooled + 1);                       // now it may
    CHECK(f.sh.grows == 3 && f.sh.grows_with_slots_referenced == 0 && f.be.capacity == 4 * first);
    native_step(f);
    CHECK(f.resolve().size() == 6 && f.ev.outstanding() == 0);
}

void test_no_buffer_no_scopes()
{
    Fixture f;
    f.sh.fail_grows_from = 0;                                // the allocation fails
    native_step(f);
    CHECK(f.be.records == 0 && f.ev.pending() == 0 && f.ev.outstanding() == 0 && f.sh.stamp_kernels == 0);
    f.sh.fail_grows_from = -1;
    native_step(f);
    CHECK(f.be.records == 7 && f.resolve().size() == 6);
}

struct Test { const char *name; std::function<void()> fn; };
const std::vector<Test> kTests = {
    {"native_step_records_seven_stamps", test_native_step_records_seven_stamps},
    {"scopes_outside_a_region_are_stamped_at_once", test_scopes_outside_a_region_are_stamped_at_once},
    {"a_scope_nobody_vouches_for_is_stamped_at_once_inside_a_region", test_a_scope_nobody_vouches_for_is_stamped_at_once_inside_a_region},
    {"the_region_s_end_pays_what_is_owed", test_the_region_s_end_pays_what_is_owed},
    {"an_enqueue_that_cannot_carry_pays_first", test_an_enqueue_that_cannot_carry_pays_first},
    {"every_slot_comes_back_exactly_once", test_every_slot_comes_back_exactly_once},
    {"reset_and_profiling_off_and_on", test_reset_and_profiling_off_and_on},
    {"destroy_with_scopes_pending", test_destroy_with_scopes_pending},
    {"the_buffer_grows_only_with_no_slot_referenced", test_the_buffer_grows_only_with_no_slot_referenced},
    {"no_buffer_no_scopes", test_no_buffer_no_scopes},
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
