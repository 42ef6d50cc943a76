// body_table.h -- the host side of a body set: its validation and the tables the pass reads.  Plain C++, no HIP header:
// gpe_bodies.hip includes it, and so does the CPU test program (tests/cpp/body_table_tests.cpp).
//
// body_table_build turns k bodies into
//   - one 16-byte record per body, in the order given: (first, count, stiffness, bd2), bd2 = break_distance *
//     break_distance rounded once, here (it may underflow to 0: every e2 > 0 then breaks), or kBodyNeverBreaks for a
//     break_distance of 0;
//   - the bodies' indices sorted by width class G = body_width(count) in {2, 4, 8, 16, 32, 64} (a body of more than 64
//     members joins the class of 64), ascending body index within a class, and where each class starts;
//   - a state byte per body: kBodyBroken for a body given with GPE_BODY_BROKEN, else kBodyInert (no pass yet).
// The pass serves 64 / G bodies of class G per wave, so which lanes add what is a function of the set alone.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gpe.h"
#include "k_body.h"

namespace gpe {

constexpr uint32_t kBodyClasses = 6;                   // G = 2 << class
constexpr uint32_t kBodyKnownFlags = GPE_BODY_BROKEN;

struct BodyRecord {              // 16 bytes: what the pass reads per body
    uint32_t first, count;
    float stiffness, bd2;
};

struct BodyTable {
    std::vector<BodyRecord> rec;         // k
    std::vector<uint32_t> order;         // k: body indices by class, ascending within a class
    uint32_t class_start[kBodyClasses + 1] = {0, 0, 0, 0, 0, 0, 0};   // order[class_start[q], class_start[q + 1]): class q
    std::vector<uint8_t> state;          // k
    uint64_t broken = 0;                 // bodies that start broken
};

inline uint32_t body_class(uint32_t count)             // log2(G) - 1
{
    uint32_t q = 0;
    while ((2u << q) < body_width(count)) ++q;
    return q;
}

// NULL: the set is valid.  Otherwise what is wrong with it (the caller names the call in front).
inline const char *body_set_problem(const gpe_body *bodies, uint64_t k, const uint32_t *member_uid,
                                    const float *member_rest_xy, uint64_t members)
{
    if (k == 0) return nullptr;                        // (clears the set: the arrays are not read)
    if (!bodies || !member_uid || !member_rest_xy) return "NULL bodies, member_uid or member_rest_xy";
    if (k > GPE_BODIES_MAX) return "k must be at most GPE_BODIES_MAX";
    if (members > GPE_BODY_MEMBERS_MAX) return "members must be at most GPE_BODY_MEMBERS_MAX";
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_body &q = bodies[j];
        if (q.count < 2 || q.count > GPE_BODY_MAX_MEMBERS) return "a count is outside 2 .. GPE_BODY_MAX_MEMBERS";
        if ((uint64_t)q.first + q.count > members) return "a body's members run past `members`";
        if (!(q.stiffness >= 0.0f && q.stiffness <= 1.0f)) return "a stiffness is NaN or outside [0, 1]";
        if (!isfinite(q.break_distance) || !(q.break_distance >= 0.0f))
            return "a break_distance is NaN, infinite or negative";
        if (q.flags & ~kBodyKnownFlags) return "unknown flag bits";
        if (q.reserved != 0) return "reserved must be 0";
    }
    // the ranges tile [0, members): sorted by first, each starts where the one before it ends
    std::vector<uint32_t> by_first(k);
    for (uint64_t j = 0; j < k; ++j) by_first[j] = (uint32_t)j;
    std::sort(by_first.begin(), by_first.end(),
              [bodies](uint32_t a, uint32_t b) { return bodies[a].first < bodies[b].first; });
    uint64_t at = 0;
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_body &q = bodies[by_first[j]];
        if (q.first < at) return "two bodies' member ranges overlap";
        if (q.first > at) return "members are left unused";
        at += q.count;
    }
    if (at != members) return "members are left unused";
    for (uint64_t i = 0; i < members; ++i) {
        if (member_uid[i] == GPE_UID_ABSENT) return "a member's uid is GPE_UID_ABSENT";
        if (!isfinite(member_rest_xy[2 * i]) || !isfinite(member_rest_xy[2 * i + 1]))
            return "a rest coordinate is not finite";
    }
    std::vector<uint32_t> sorted(member_uid, member_uid + members);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return "a uid is named twice";
    return nullptr;
}

// The tables of a set body_set_problem accepts.
inline void body_table_build(const gpe_body *bodies, uint64_t k, BodyTable *t)
{
    *t = BodyTable();
    t->rec.resize(k);
    t->state.assign(k, (uint8_t)kBodyInert);
    t->order.resize(k);
    uint32_t per_class[kBodyClasses] = {0, 0, 0, 0, 0, 0};
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_body &q = bodies[j];
        BodyRecord &r = t->rec[j];
        r.first = q.first;
        r.count = q.count;
        r.stiffness = q.stiffness;
        r.bd2 = q.break_distance > 0.0f ? q.break_distance * q.break_distance : kBodyNeverBreaks;   // one rounding
        if (q.flags & GPE_BODY_BROKEN) {
            t->state[j] = (uint8_t)kBodyBroken;
            t->broken += 1;
        }
        per_class[body_class(q.count)] += 1;
    }
    for (uint32_t q = 0; q < kBodyClasses; ++q) t->class_start[q + 1] = t->class_start[q] + per_class[q];
    uint32_t at[kBodyClasses];
    for (uint32_t q = 0; q < kBodyClasses; ++q) at[q] = t->class_start[q];
    for (uint64_t j = 0; j < k; ++j) t->order[at[body_class(bodies[j].count)]++] = (uint32_t)j;   // ascending j per class
}

}  // namespace gpe
