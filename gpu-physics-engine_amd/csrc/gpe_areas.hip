// gpe_areas.hip -- the area constraints of a context (gpe_set_areas and the rest): the set, its tables (area_table.h),
// the nodes' and members' storage slots (looked up again only when stale) and the pass behind every step
// (k_areas.hip).  What the entry points share with the other sets that name their particles by uid is uid_sets.h's;
// gpe_api.hip lists the set in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

#include "area_table.h"
#include "k_area.h"
#include "uid_sets.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static_assert(kAreaClasses + 1 == sizeof(AreaState().class_start) / sizeof(uint32_t), "AreaState keeps every class start");

void gpe::areas_release(gpe_ctx *c)
{
    AreaState &S = c->areas;
    dev_free(c, S.rec); dev_free(c, S.order); dev_free(c, S.member_node); dev_free(c, S.member_slot);
    node_table_free(c, S.nt); dev_free(c, S.inc);
    dev_free(c, S.corr); dev_free(c, S.state); dev_free(c, S.value);
    S = AreaState();
}

// (a stale set: the members take their nodes' slots behind the lookup)
gpe_status gpe::areas_pass(gpe_ctx *c)
{
    AreaState &S = c->areas;
    return uid_set_pass(c, S.set.empty(), S.nt.stale, "Areas", &S.passes,
                        [&] {
                            return uid_slots_resolve(c, "areas/resolve", S.nt,
                                                     [](gpe_ctx *x) { return launch_areas_expand(x, x->areas); });
                        },
                        [&] {
                            return launch_areas_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                     (uint32_t)S.nt.nodes, S.iterations);
                        });
}

gpe_status gpe_set_areas(gpe_ctx *c, const gpe_area *areas, uint64_t k, const uint32_t *member_uid, uint64_t members,
                         uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = area_set_problem(areas, k, member_uid, members, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_areas: ") + why);
    GPE_TRY(uid_set_open(c, "gpe_set_areas", k, areas_release));
    if (k == 0) return GPE_OK;
    AreaTable t;
    area_table_build(areas, k, member_uid, members, &t);
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    AreaState N;
    HipSetUpload up({c}, "gpe_set_areas");
    up.reserve(&N.rec, k, "uid.area_rec");
    up.reserve(&N.order, k, "uid.area_order");
    up.reserve(&N.member_node, members, "uid.area_member_node");
    up.reserve(&N.member_slot, members, "uid.area_member_slot");
    node_table_upload(up, &N.nt, t.nodes, t.row_start, "uid.area_node_uid", "uid.area_node_slot", "uid.area_row_start");
    up.reserve(&N.inc, members, "uid.area_inc");
    up.reserve(&N.corr, members, "uid.area_corr");
    up.reserve(&N.state, k, "uid.area_state");
    up.reserve(&N.value, k, "uid.area_value");
    up.copy(N.rec, t.rec.data(), k);
    up.copy(N.order, t.order.data(), k);
    up.copy(N.member_node, t.member_node.data(), members);
    up.copy(N.inc, t.inc.data(), members);
    up.fill(N.member_slot, 0xff, members * sizeof(uint32_t));
    up.fill(N.corr, 0, members * sizeof(float2));
    up.fill(N.state, (int)kAreaInert, k);
    up.fill(N.value, 0xff, k * sizeof(float2));                        // (all ones: a NaN)
    GPE_TRY(up.finish());
    areas_release(c);
    N.set.assign(areas, areas + k);
    for (gpe_area &q : N.set) {
        q.rest_area = plus_zero(q.rest_area);
        q.stiffness = plus_zero(q.stiffness);
    }
    N.member_uid_host.assign(member_uid, member_uid + members);
    N.iterations = iterations;
    N.members = members;
    memcpy(N.class_start, t.class_start, sizeof(N.class_start));
    c->areas = std::move(N);
    return GPE_OK;
}

gpe_status gpe_get_areas(const gpe_ctx *c, gpe_area *out, uint64_t capacity, uint64_t *k, uint32_t *member_uid_out,
                         uint64_t member_capacity, uint64_t *members)
{
    if (!c || !k || !members) return GPE_ERR_INVALID_ARG;
    if (capacity > 0 && !out) return GPE_ERR_INVALID_ARG;
    const AreaState &S = c->areas;
    *members = S.members;
    const uint64_t mm = std::min<uint64_t>(S.members, member_capacity);
    if (mm && member_uid_out) memcpy(member_uid_out, S.member_uid_host.data(), mm * sizeof(uint32_t));
    return rows_out(S.set, out, capacity, k);
}

gpe_status gpe_apply_areas(gpe_ctx *c)
{
    return uid_set_apply(c, has_areas, areas_pass);
}

gpe_status gpe_get_areas_info(gpe_ctx *c, gpe_areas_info *info)
{
    gpe_areas_info out;
    GPE_TRY(info_open(c, "gpe_get_areas_info", info, &out));
    const AreaState &S = c->areas;
    if (has_areas(c)) {
        out.iterations = S.iterations;
        out.k = S.set.size();
        out.members = S.members;
        out.nodes = S.nt.nodes;
        out.passes = S.passes;
        out.resolves = S.nt.resolves;
    }
    *info = out;
    return GPE_OK;
}

gpe_status gpe_get_area_values(gpe_ctx *c, float *area_lambda, uint64_t capacity, uint64_t *k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!k) return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_area_values: NULL k");
    const AreaState &S = c->areas;
    *k = S.set.size();
    const uint64_t m = std::min<uint64_t>(S.set.size(), capacity);
    if (m == 0 || !area_lambda) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return read_back(c, S.value, area_lambda, m * sizeof(float2));
}

// The pump: new rest areas for loops first .. first + k - 1, written into the records where they lie.
gpe_status gpe_set_area_targets(gpe_ctx *c, uint64_t first, uint64_t k, const float *rest_area)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    AreaState &S = c->areas;
    if (const char *why = area_targets_problem(S.set.size(), first, k, rest_area))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_area_targets: ") + why);
    if (k == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old targets)
    for (uint64_t j = 0; j < k; ++j) S.set[first + j].rest_area = plus_zero(rest_area[j]);
    // the records of the range again, as area_table_build wrote them: only their rest areas differ
    std::vector<AreaRecord> rows(k);
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_area &q = S.set[first + j];
        rows[j] = AreaRecord{q.first, q.count, q.rest_area, q.stiffness};
    }
    GPE_HIP(c, hipMemcpyAsync(S.rec + first, rows.data(), k * sizeof(AreaRecord), hipMemcpyHostToDevice, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (the rows go away with this call)
    return GPE_OK;
}
