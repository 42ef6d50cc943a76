// scope_stamps.h -- a backend of ScopeEvents (scope_events.h) whose "event" is a slot in a device buffer of 64-bit
// timestamps: a record is the GPU's constant-rate counter (wall_clock64(), the clock hipEventElapsedTime reports in)
// written into the slot in stream order, not an event packet.  No HIP header: what touches the device comes through
// Dev, so tests/cpp/scope_stamps_tests.cpp drives this with counters.
//
// Who writes the stamp.  Measured on an in-order stream that carries a 5 us kernel between boundaries
// (scripts/probes/stamp_boundary.hip, profiles/fixed_costs): an event record costs 2.9 us per boundary, a one-thread
// kernel that stores the counter 1.5 us, the same store by the first workgroup of the kernel that starts at the
// boundary nothing measurable.  So a record is written at once by the one-thread kernel, unless its scope says
// that the stamp is OWED to the enqueue that follows (Scope::kCarryStart / kCarryStop, handed to record() through the
// StampRecorder of that open or close; inside a tracked region of scope_events.h only: there every enqueue is
// announced).  The launchers of the hash and of the two gated sort kernels, which return at once on most steps, take an
// owed stamp -- take() -- and the kernel's first workgroup writes it; any other enqueue, and the region's end, pays it
// with the one-thread kernel first -- flush(), from note_enqueue().  The native step owes the boundaries around the hash
// (the one in front of it too: stamped at once, it counted the host's time to launch the hash as the hash's whenever the
// GPU was waiting for the host) and around the radix passes, and stamps at once those behind the two collide launches: owing a record stamps the scope that ends there only when the host has
// prepared the next launch, and on a small scene, where the GPU waits for the host, that time would count as the long
// kernel's.
//
// The buffer.  Slot 0 is the trace origin's; slots are handed out in order and pooled by ScopeEvents exactly as events
// are.  create() fails when the buffer is full -- the scope is then dropped, as when an event cannot be created --
// and the buffer grows, by doubling, only through make_room(): outside the step path and with no slot referenced,
// because growing moves the buffer.  make_room() first has the pending pairs resolved, which takes a synchronisation
// and brings their slots back to the pool, and then doubles the buffer, so that a long run with profiling on every
// step comes there ever more rarely.
//
// Dev: struct { bool grow(uint32_t old_slots, uint32_t new_slots);   // a buffer of new_slots that keeps slot 0; false: none
//               void stamp(uint32_t slot); }                         // enqueue the one-thread kernel
#pragma once

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

namespace gpe {

// 128 KiB .. 2 MiB of timestamps.  The first buffer holds 2300 sampled native steps: making room in the middle of a run
// costs a synchronisation and an allocation (about 10 ms measured, profiles/fixed_costs), so it should be rare.
constexpr uint32_t kStampSlotsFirst = 16384, kStampSlotsMax = 1u << 18;
constexpr uint32_t kStampOrigin = 0;

template <class Dev>
struct StampBackend {
    using Event = uint32_t;
    Dev dev;
    uint32_t capacity = 0;           // slots the buffer holds
    uint32_t next = 1;               // the first slot never handed out
    int64_t owed = -1;               // the slot whose stamp the next enqueue carries or pays
    uint64_t records = 0, kernels = 0, carried = 0;   // records in all; written by the one-thread kernel / by a launch

    bool create(Event *e)
    {
        if (next >= capacity) return false;
        *e = next++;
        return true;
    }
    // owe: the stamp is owed to the next enqueue, which carries or pays it; else it is written at once
    void record(Event e, bool owe)
    {
        flush();                     // (two records with nothing between them: a scope that does not share)
        ++records;
        if (owe) owed = (int64_t)e;
        else { dev.stamp(e); ++kernels; }
    }
    void destroy(Event) {}           // (the slots go with the buffer)

    // an enqueue that cannot carry the stamp, or the end of the region: the owed stamp is written now
    void flush()
    {
        if (owed < 0) return;
        dev.stamp((uint32_t)owed);
        ++kernels;
        owed = -1;
    }
    // a launch whose first workgroup writes the stamp: the slot, or -1 when none is owed
    int64_t take()
    {
        const int64_t s = owed;
        if (s >= 0) ++carried;
        owed = -1;
        return s;
    }

    // slots that can be handed out without growing, given the pool of the ScopeEvents this backend serves
    uint64_t room(size_t pooled) const { return (uint64_t)pooled + (capacity > next ? capacity - next : 0u); }
    // Outside the step path.  outstanding: the slots referenced (ScopeEvents::outstanding()); the buffer moves when it
    // grows, so it grows only when that is 0 -- the caller resolves what is pending first.  false: no room was made.
    bool grow(size_t outstanding)
    {
        if (outstanding != 0 || owed >= 0 || capacity >= kStampSlotsMax) return false;
        const uint32_t want = capacity ? 2 * capacity : kStampSlotsFirst;
        if (!dev.grow(capacity, want)) return false;
        capacity = want;
        return true;
    }
    // Outside the step path: afterwards at least `need` slots can be handed out, if that can be had.  ev: the
    // ScopeEvents this backend serves; resolve_all(): synchronise and resolve its pending pairs, false when that failed.
    // Where room cannot be had -- a scope is open around the caller and holds a slot, the buffer has reached its
    // largest size, the allocation fails -- the scopes that find no slot are dropped.
    template <class Events, class Resolve>
    void make_room(Events &ev, uint32_t need, Resolve &&resolve_all)
    {
        if (room(ev.pooled()) >= need) return;
        if (capacity) {
            flush();
            if (!resolve_all()) return;
        }
        do {
            if (!grow(ev.outstanding())) break;
        } while (room(ev.pooled()) < need);
    }
};

// The backend ScopeEvents is handed for one open or close of a scope: the slots, and whether the record that this open
// or close may make is owed to the next enqueue.
template <class Dev>
struct StampRecorder {
    using Event = uint32_t;
    StampBackend<Dev> &slots;
    bool owe = false;
    bool create(Event *e) { return slots.create(e); }
    void record(Event e) { slots.record(e, owe); }
    void destroy(Event e) { slots.destroy(e); }
};

}  // namespace gpe
