// gpe_bodies.hip -- the rigid and soft bodies of a context (gpe_set_bodies and the rest): the set, its tables
// (body_table.h), the members' storage slots (looked up again only when stale) and the pass behind every step
// (k_bodies.hip).  gpe_api.hip calls bodies_after_step from after_step and bodies_release from gpe_destroy.
#include <string.h>

#include "body_table.h"
#include "gpe_internal.h"
#include "k_body.h"
#include "k_uids.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static void bodies_free(gpe_ctx *c, BodyState &S)
{
    dev_free(c, S.rec); dev_free(c, S.order); dev_free(c, S.member_uid); dev_free(c, S.member_slot);
    dev_free(c, S.member_rest); dev_free(c, S.pose); dev_free(c, S.state); dev_free(c, S.broken);
}

void gpe::bodies_release(gpe_ctx *c)
{
    bodies_free(c, c->bodies);
    c->bodies = BodyState();
}

gpe_status gpe::refuse_bodies(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported while the context holds bodies "
                                                            "(gpe_set_bodies with k = 0 clears them)");
}

// One pass over the particles as they are now.  Enqueues only, unless the members' slots are stale: then the uid map
// is made ready first (its build synchronises) and one lookup per member is enqueued.
static gpe_status bodies_pass(gpe_ctx *c)
{
    BodyState &S = c->bodies;
    if (S.set.empty() || c->n == 0 || !c->pos || !c->uid.on || !c->uid.uids) return GPE_OK;
    if (S.stale) {
        GPE_TRY(uid_map_ready(c));
        Scope s(c, "bodies/resolve");
        GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, c->n, S.member_uid, S.members, S.member_slot,
                                nullptr, nullptr, nullptr));
        S.stale = false;
        S.resolves += 1;
    }
    Scope s(c, "Bodies");
    GPE_TRY(launch_bodies_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size()));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::bodies_after_step(gpe_ctx *c)
{
    return bodies_pass(c);                                            // (after_step has looked: the set is not empty)
}

gpe_status gpe_set_bodies(gpe_ctx *c, const gpe_body *bodies, uint64_t k, const uint32_t *member_uid,
                          const float *member_rest_xy, uint64_t members)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = body_set_problem(bodies, k, member_uid, member_rest_xy, members))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bodies: ") + why);
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_bodies");
    if (k > 0 && !c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_set_bodies: uids are off (gpe_enable_uids)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    if (k == 0) {
        bodies_release(c);
        return GPE_OK;
    }
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
    bodies_free(c, c->bodies);
    N.set.assign(bodies, bodies + k);
    for (gpe_body &q : N.set) {
        q.flags &= ~(uint32_t)GPE_BODY_BROKEN;                         // (it set the state byte; the record does not keep it)
        if (q.break_distance == 0.0f) q.break_distance = 0.0f;         // -0.0 -> +0
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
    if (broken_out) {
        GPE_HIP(c, hipSetDevice(c->device));
        std::vector<uint8_t> state(m);
        GPE_TRY(read_back(c, S.state, state.data(), m));
        for (uint64_t j = 0; j < m; ++j) broken_out[j] = state[j] == kBodyBroken ? 1 : 0;
    }
    return GPE_OK;
}

gpe_status gpe_apply_bodies(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has_bodies(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return bodies_pass(c);
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
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_bodies_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_bodies_info: NULL info or bad struct_size");
    BodyState &S = c->bodies;
    gpe_bodies_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    if (has_bodies(c)) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long broken = 0;
        GPE_TRY(read_back(c, S.broken, &broken, sizeof(broken)));
        out.k = S.set.size();
        out.members = S.members;
        out.passes = S.passes;
        out.broken = broken;
        out.live = out.k - broken;
        out.resolves = S.resolves;
    }
    *info = out;
    return GPE_OK;
}
