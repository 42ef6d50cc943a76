// gpe_bodies.hip -- the rigid and soft bodies of a context (gpe_set_bodies and the rest): the set, its tables
// (body_table.h), the members' storage slots (looked up again only when stale) and the pass behind every step
// (k_bodies.hip).  What the entry points share with the other sets that name their particles by uid is uid_sets.h's;
// gpe_api.hip lists the set in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

#include "body_table.h"
#include "k_body.h"
#include "uid_sets.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

void gpe::bodies_release(gpe_ctx *c)
{
    BodyState &S = c->bodies;
    dev_free(c, S.rec); dev_free(c, S.order); dev_free(c, S.member_uid); dev_free(c, S.member_slot);
    dev_free(c, S.member_rest); dev_free(c, S.pose); dev_free(c, S.state); dev_free(c, S.broken);
    S = BodyState();
}

// (no node table: a uid is a member of one body, so the members are looked up directly)
gpe_status gpe::bodies_pass(gpe_ctx *c)
{
    BodyState &S = c->bodies;
    return uid_set_pass(c, S.set.empty(), S.stale, "Bodies", &S.passes,
                        [&] {
                            return uid_slots_resolve(c, "bodies/resolve", S.member_uid, S.members, S.member_slot,
                                                     &S.stale, &S.resolves);
                        },
                        [&] { return launch_bodies_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size()); });
}

gpe_status gpe_set_bodies(gpe_ctx *c, const gpe_body *bodies, uint64_t k, const uint32_t *member_uid,
                          const float *member_rest_xy, uint64_t members)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = body_set_problem(bodies, k, member_uid, member_rest_xy, members))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bodies: ") + why);
    GPE_TRY(uid_set_open(c, "gpe_set_bodies", k, bodies_release));
    if (k == 0) return GPE_OK;
    BodyTable t;
    body_table_build(bodies, k, &t);
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    const unsigned long long broken = t.broken;
    BodyState N;
    HipSetUpload up({c}, "gpe_set_bodies");
    up.reserve(&N.rec, k, "uid.body_rec");
    up.reserve(&N.order, k, "uid.body_order");
    up.reserve(&N.member_uid, members, "uid.body_member_uid");
    up.reserve(&N.member_slot, members, "uid.body_member_slot");
    up.reserve(&N.member_rest, members, "uid.body_member_rest");
    up.reserve(&N.pose, k, "uid.body_pose");
    up.reserve(&N.state, k, "uid.body_state");
    up.reserve(&N.broken, 1, "uid.body_broken");
    up.copy(N.rec, t.rec.data(), k);
    up.copy(N.order, t.order.data(), k);
    up.copy(N.member_uid, member_uid, members);
    up.copy(N.member_rest, member_rest_xy, 2 * members);
    up.copy(N.state, t.state.data(), k);
    up.fill(N.member_slot, 0xff, members * sizeof(uint32_t));
    up.fill(N.pose, 0xff, k * sizeof(float4));                         // (all ones: a NaN)
    up.copy(N.broken, &broken, 1);
    GPE_TRY(up.finish());
    bodies_release(c);
    N.set.assign(bodies, bodies + k);
    for (gpe_body &q : N.set) {
        q.flags &= ~(uint32_t)GPE_BODY_BROKEN;                         // (it set the state byte; the record does not keep it)
        q.break_distance = plus_zero(q.break_distance);
    }
    N.member_uid_host.assign(member_uid, member_uid + members);
    N.member_rest_host.assign(member_rest_xy, member_rest_xy + 2 * members);
    N.members = members;
    memcpy(N.class_start, t.class_start, sizeof(N.class_start));
    N.stale = true;
    c->bodies = std::move(N);
    return GPE_OK;
}

gpe_status gpe_get_bodies(gpe_ctx *c, gpe_body *out, uint8_t *broken_out, uint64_t capacity, uint64_t *k,
                          uint32_t *member_uid_out, float *member_rest_xy_out, uint64_t member_capacity,
                          uint64_t *members)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!k || !members) return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_bodies: NULL k or members");
    BodyState &S = c->bodies;
    *k = S.set.size();
    *members = S.members;
    const uint64_t m = std::min<uint64_t>(S.set.size(), capacity);
    const uint64_t mm = std::min<uint64_t>(S.members, member_capacity);
    if (mm && member_uid_out) memcpy(member_uid_out, S.member_uid_host.data(), mm * sizeof(uint32_t));
    if (mm && member_rest_xy_out) memcpy(member_rest_xy_out, S.member_rest_host.data(), 2 * mm * sizeof(float));
    if (m == 0) return GPE_OK;
    if (out) memcpy(out, S.set.data(), m * sizeof(gpe_body));
    return broken_out ? gpe::broken_out(c, S.state, m, kBodyBroken, broken_out) : GPE_OK;
}

gpe_status gpe_apply_bodies(gpe_ctx *c)
{
    return uid_set_apply(c, has_bodies, bodies_pass);
}

gpe_status gpe_get_body_poses(gpe_ctx *c, float *pose_xycs, uint64_t capacity, uint64_t *k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!k) return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_body_poses: NULL k");
    BodyState &S = c->bodies;
    *k = S.set.size();
    const uint64_t m = std::min<uint64_t>(S.set.size(), capacity);
    if (m == 0 || !pose_xycs) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return read_back(c, S.pose, pose_xycs, m * sizeof(float4));
}

gpe_status gpe_get_bodies_info(gpe_ctx *c, gpe_bodies_info *info)
{
    gpe_bodies_info out;
    GPE_TRY(info_open(c, "gpe_get_bodies_info", info, &out));
    const BodyState &S = c->bodies;
    if (has_bodies(c)) {
        out.k = S.set.size();
        out.members = S.members;
        out.passes = S.passes;
        out.resolves = S.resolves;
        GPE_TRY(info_broken(c, S.broken, &out));
    }
    *info = out;
    return GPE_OK;
}
