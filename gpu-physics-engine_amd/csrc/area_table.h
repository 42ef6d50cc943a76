// area_table.h -- the host side of an area set: its validation and the tables the pass reads.  Plain C++, no HIP header:
// gpe_areas.hip includes it, and so does the CPU test program (tests/cpp/area_table_tests.cpp).
//
// area_table_build turns k loops over `members` member uids into
//   - one 16-byte record per loop, in the order given: (first, count, rest_area, stiffness), -0.0 stored as +0;
//   - the loops' indices sorted by width class G = body_width(count) in {4, 8, 16, 32, 64} (a loop of more than 64
//     members joins the class of 64), ascending loop index within a class, and where each class starts;
//   - nodes: the distinct uids the members name, ascending (a uid may be a member of several loops);
//   - per member its node index;
//   - a CSR of incidences per node, in ascending member index: entry = (member index, loop index), so the node phase
//     finds the member's correction and its loop's state byte without a search.  The nodes and the rows are
//     uid_nodes.h's.
// The loop phase serves 64 / G loops of class G per wave, and a node adds its shares in the order of its row, so which
// lane adds what, and in which order, is a function of the set alone.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gpe.h"
#include "k_area.h"
#include "uid_nodes.h"

namespace gpe {

constexpr uint32_t kAreaClasses = 5;                   // G = 4 << class

struct AreaRecord {              // 16 bytes: what the loop phase reads per loop
    uint32_t first, count;
    float rest_area, stiffness;
};

struct AreaIncidence {           // 8 bytes: one membership of a node
    uint32_t member, loop;
};

struct AreaTable {
    std::vector<AreaRecord> rec;             // k
    std::vector<uint32_t> order;             // k: loop indices by class, ascending within a class
    uint32_t class_start[kAreaClasses + 1] = {0, 0, 0, 0, 0, 0};   // order[class_start[q], class_start[q + 1]): class q
    std::vector<uint32_t> nodes;             // m: the uids, ascending, distinct
    std::vector<uint32_t> member_node;       // members
    std::vector<uint32_t> row_start;         // m + 1
    std::vector<AreaIncidence> inc;          // row_start[m] = members entries
    uint32_t max_degree = 0;
};

inline uint32_t area_class(uint32_t count)             // log2(G) - 2  (count >= 3)
{
    uint32_t q = 0;
    while ((4u << q) < body_width(count)) ++q;
    return q;
}

// NULL: the set is valid.  Otherwise what is wrong with it (the caller names the call in front).
inline const char *area_set_problem(const gpe_area *areas, uint64_t k, const uint32_t *member_uid, uint64_t members,
                                    uint32_t iterations)
{
    if (k == 0) return nullptr;                        // (clears the set: nothing else is read)
    if (!areas || !member_uid) return "NULL areas or member_uid";
    if (k > GPE_AREAS_MAX) return "k must be at most GPE_AREAS_MAX";
    if (members > GPE_AREA_MEMBERS_MAX) return "members must be at most GPE_AREA_MEMBERS_MAX";
    if (iterations < 1 || iterations > GPE_AREA_ITER_MAX) return "iterations must be 1 .. GPE_AREA_ITER_MAX";
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_area &q = areas[j];
        if (q.count < 3 || q.count > GPE_AREA_MAX_MEMBERS) return "a count is outside 3 .. GPE_AREA_MAX_MEMBERS";
        if ((uint64_t)q.first + q.count > members) return "a loop's members run past `members`";
        if (!isfinite(q.rest_area)) return "a rest_area is not finite";
        if (!(q.stiffness >= 0.0f && q.stiffness <= 1.0f)) return "a stiffness is NaN or outside [0, 1]";
        if (q.flags != 0 || q.reserved != 0) return "flags and reserved must be 0";
    }
    // the ranges tile [0, members): sorted by first, each starts where the one before it ends
    std::vector<uint32_t> by_first(k);
    for (uint64_t j = 0; j < k; ++j) by_first[j] = (uint32_t)j;
    std::sort(by_first.begin(), by_first.end(),
              [areas](uint32_t a, uint32_t b) { return areas[a].first < areas[b].first; });
    uint64_t at = 0;
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_area &q = areas[by_first[j]];
        if (q.first < at) return "two loops' member ranges overlap";
        if (q.first > at) return "members are left unused";
        at += q.count;
    }
    if (at != members) return "members are left unused";
    for (uint64_t i = 0; i < members; ++i)
        if (member_uid[i] == GPE_UID_ABSENT) return "a member's uid is GPE_UID_ABSENT";
    std::vector<uint32_t> sorted;
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_area &q = areas[j];
        sorted.assign(member_uid + q.first, member_uid + q.first + q.count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return "a uid is named twice in one loop";
    }
    // (inside a loop a uid appears once, so a uid's appearances count its loops)
    sorted.assign(member_uid, member_uid + members);
    std::sort(sorted.begin(), sorted.end());
    uint64_t run = 0;
    for (uint64_t i = 0; i < members; ++i) {
        run = (i > 0 && sorted[i] == sorted[i - 1]) ? run + 1 : 1;
        if (run > GPE_AREA_MAX_DEGREE) return "a uid is a member of more than GPE_AREA_MAX_DEGREE loops";
    }
    return nullptr;
}

// What is wrong with new rest areas for loops first .. first + k - 1 of a set of `have` loops, or NULL.
inline const char *area_targets_problem(uint64_t have, uint64_t first, uint64_t k, const float *rest_area)
{
    if (first > have || k > have - first) return "the range runs past the set";
    if (k > 0 && !rest_area) return "NULL rest_area";
    for (uint64_t j = 0; j < k; ++j)
        if (!isfinite(rest_area[j])) return "a rest_area is not finite";
    return nullptr;
}

// The tables of a set area_set_problem accepts.
inline void area_table_build(const gpe_area *areas, uint64_t k, const uint32_t *member_uid, uint64_t members,
                             AreaTable *t)
{
    *t = AreaTable();
    t->rec.resize(k);
    t->order.resize(k);
    uint32_t per_class[kAreaClasses] = {0, 0, 0, 0, 0};
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_area &q = areas[j];
        AreaRecord &r = t->rec[j];
        r.first = q.first;
        r.count = q.count;
        r.rest_area = plus_zero(q.rest_area);
        r.stiffness = plus_zero(q.stiffness);
        per_class[area_class(q.count)] += 1;
    }
    for (uint32_t q = 0; q < kAreaClasses; ++q) t->class_start[q + 1] = t->class_start[q] + per_class[q];
    uint32_t at[kAreaClasses];
    for (uint32_t q = 0; q < kAreaClasses; ++q) at[q] = t->class_start[q];
    for (uint64_t j = 0; j < k; ++j) t->order[at[area_class(areas[j].count)]++] = (uint32_t)j;   // ascending j per class

    UidNodes u;                                                         // the member array as it stands
    uid_nodes_build(member_uid, members, &u);
    t->nodes = std::move(u.nodes);
    t->member_node = std::move(u.node_of);
    t->row_start = std::move(u.row_start);
    t->max_degree = u.max_degree;
    t->inc.resize(members);
    for (uint64_t j = 0; j < k; ++j)
        for (uint32_t i = 0; i < areas[j].count; ++i) {
            const uint32_t member = areas[j].first + i;
            t->inc[u.at[member]] = AreaIncidence{member, (uint32_t)j};
        }
}

}  // namespace gpe
