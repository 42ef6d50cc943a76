// scope_events.h -- which events the profiling scopes record, which they share, and when an event goes back to the pool.
// No HIP header: the event calls come through a backend, so tests/cpp/scope_events_tests.cpp drives this with counters.
//
// Every scope used to record an event pair of its own.  On the one in-order stream of a context the stop of a scope and
// the start of the next one mark the same point when nothing was enqueued between them, and each record is a barrier
// packet with a timestamp: a kept-table native step recorded 12 of them for 7 boundaries.  So, inside a TRACKED REGION
// -- a stretch of host code in which every enqueue onto the stream calls note_enqueue() (native_collide: DESIGN.md 5) --
//   * a scope that opens with nothing enqueued since the last recorded event takes that event as its start;
//   * a scope that closes with nothing enqueued since a nested scope's stop (or its own start) takes that event as its stop.
// Outside such a region nobody vouches for "nothing enqueued", and every scope keeps its own pair as before.
// Events are counted by reference: the scopes that use one (open or pending) and the boundary itself each hold one, and
// the event returns to the pool when the last of them lets go.
//
// Backend: struct { using Event = ...; bool create(Event *); void record(Event); void destroy(Event); }
#pragma once

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace gpe {

template <class Backend>
class ScopeEvents {
   public:
    using Event = typename Backend::Event;
    struct Pending {
        int stat;
        int start, stop;             // slots
    };

    // the library has enqueued onto the stream: the last recorded event no longer marks "now"
    void note_enqueue() { clean_ = false; }

    // A tracked region begins / ends: what was recorded before it is no boundary inside it, and the other way round.
    void enter_region() { forget_boundary(); ++region_; }
    void leave_region() { assert(region_ > 0); --region_; forget_boundary(); }
    void forget_boundary()
    {
        if (last_ >= 0) unref(last_);
        last_ = -1;
        clean_ = false;
    }

    // A scope opens: its start slot (one reference, the scope's), or -1 when no event could be created.
    // shared: the scope may share boundaries (it does so only inside a tracked region).
    int open(Backend &be, bool shared)
    {
        if (shared && region_ > 0 && clean_ && last_ >= 0) {
            ++slots_[last_].refs;
            return last_;
        }
        return record_new(be, shared && region_ > 0);
    }

    // ... and closes: the pair goes to the pending list (resolve() reads it once the stream has been synchronised).
    void close(Backend &be, int start, int stat, bool shared)
    {
        if (start < 0) return;
        int stop;
        if (shared && region_ > 0 && clean_ && last_ >= 0) {
            stop = last_;
            ++slots_[stop].refs;
        } else {
            stop = record_new(be, shared && region_ > 0);
        }
        if (stop < 0) { unref(start); return; }
        Pending p;
        p.stat = stat; p.start = start; p.stop = stop;
        pending_.push_back(p);
    }

    // f(stat, start event, stop event) for every pending pair, oldest first; the pairs let go of their events.
    template <class F>
    void resolve(F &&f)
    {
        for (const Pending &p : pending_) {
            f(p.stat, slots_[p.start].ev, slots_[p.stop].ev);
            unref(p.start);
            unref(p.stop);
        }
        pending_.clear();
    }

    // The context goes away: pending pairs are dropped unread, every event is destroyed (no scope may be open).
    void destroy_all(Backend &be)
    {
        for (const Pending &p : pending_) { unref(p.start); unref(p.stop); }
        pending_.clear();
        forget_boundary();
        assert(outstanding() == 0);
        for (Slot &s : slots_) be.destroy(s.ev);
        slots_.clear();
        free_.clear();
    }

    size_t created() const { return slots_.size(); }              // events that exist (in use + pooled)
    size_t pooled() const { return free_.size(); }
    size_t outstanding() const { return slots_.size() - free_.size(); }
    size_t pending() const { return pending_.size(); }
    bool in_region() const { return region_ > 0; }

   private:
    struct Slot {
        Event ev;
        uint32_t refs;
    };

    int record_new(Backend &be, bool boundary)
    {
        int slot;
        if (!free_.empty()) {
            slot = free_.back();
            free_.pop_back();
        } else {
            Slot s;
            s.refs = 0;
            if (!be.create(&s.ev)) return -1;
            slots_.push_back(s);
            slot = (int)slots_.size() - 1;
        }
        assert(slots_[slot].refs == 0);
        slots_[slot].refs = 1;
        be.record(slots_[slot].ev);
        if (boundary) {
            if (last_ >= 0) unref(last_);
            last_ = slot;
            ++slots_[slot].refs;
            clean_ = true;
        } else {
            clean_ = false;          // (a scope nobody vouches for: what it encloses may enqueue without saying so)
        }
        return slot;
    }

    void unref(int slot)
    {
        assert(slot >= 0 && (size_t)slot < slots_.size() && slots_[slot].refs > 0);
        if (--slots_[slot].refs == 0) free_.push_back(slot);
    }

    std::vector<Slot> slots_;
    std::vector<int> free_;
    std::vector<Pending> pending_;
    int last_ = -1;                  // the last event recorded inside the region (holds a reference), or -1
    bool clean_ = false;             // nothing enqueued since last_ was recorded
    int region_ = 0;
};

}  // namespace gpe
