// gpe_bends.hip -- the bend constraints of a context (gpe_set_bends and the rest): the set, its graph (bend_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bends.hip).  gpe_api.hip
// calls bends_after_step from after_step and bends_release from gpe_destroy.
#include <string.h>

#include "bend_graph.h"
#include "gpe_internal.h"
#include "k_bend.h"
#include "k_uids.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static void bends_free(gpe_ctx *c, BendState &S)
{
    dev_free(c, S.rec);
    dev_free(c, S.node_uid); dev_free(c, S.node_slot); dev_free(c, S.row_start); dev_free(c, S.inc);
    dev_free(c, S.corr); dev_free(c, S.state);
}

void gpe::bends_release(gpe_ctx *c)
{
    bends_free(c, c->bends);
    c->bends = BendState();
}

gpe_status gpe::refuse_bends(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported while the context holds bends "
                                                            "(gpe_set_bends with k = 0 clears them)");
}

// One pass over the particles as they are now.  Enqueues only, unless the nodes' slots are stale: then the uid map is
// made ready first (its build synchronises) and one lookup per node is enqueued.
static gpe_status bends_pass(gpe_ctx *c)
{
    BendState &S = c->bends;
    if (S.set.empty() || c->n == 0 || !c->pos || !c->uid.on || !c->uid.uids) return GPE_OK;
    if (S.stale) {
        GPE_TRY(uid_map_ready(c));
        Scope s(c, "bends/resolve");
        GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, c->n, S.node_uid, S.nodes, S.node_slot, nullptr,
                                nullptr, nullptr));
        S.stale = false;
        S.resolves += 1;
    }
    Scope s(c, "Bends");
    GPE_TRY(launch_bends_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(), (uint32_t)S.nodes, S.iterations));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::bends_after_step(gpe_ctx *c)
{
    return bends_pass(c);                                             // (after_step has looked: the set is not empty)
}

gpe_status gpe_set_bends(gpe_ctx *c, const gpe_bend *bends, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bend_set_problem(bends, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bends: ") + why);
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_bends");
    if (k > 0 && !c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_set_bends: uids are off (gpe_enable_uids)");
    BendGraph g;
    if (k > 0 && !bend_graph_build(bends, k, &g))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_bends: a uid has more than GPE_BEND_MAX_DEGREE bends");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    if (k == 0) {
        bends_release(c);
        return GPE_OK;
    }
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    const uint64_t m = g.nodes.size();
    BendState N;
    HipSetUpload up({c}, "gpe_set_bends");
    up.reserve(&N.rec, 2 * k, "uid.bend_rec");
    up.reserve(&N.node_uid, m, "uid.bend_node_uid");
    up.reserve(&N.node_slot, m, "uid.bend_node_slot");
    up.reserve(&N.row_start, m + 1, "uid.bend_row_start");
    up.reserve(&N.inc, g.inc.size(), "uid.bend_inc");
    up.reserve(&N.corr, k, "uid.bend_corr");
    up.reserve(&N.state, k, "uid.bend_state");
    up.copy(N.rec, g.rec.data(), g.rec.size());
    up.copy(N.node_uid, g.nodes.data(), g.nodes.size());
    up.copy(N.row_start, g.row_start.data(), g.row_start.size());
    up.copy(N.inc, g.inc.data(), g.inc.size());
    up.fill(N.node_slot, 0xff, m * sizeof(uint32_t));
    up.fill(N.corr, 0, k * sizeof(float4));
    up.fill(N.state, (int)kBendInert, k);
    GPE_TRY(up.finish());
    bends_free(c, c->bends);
    N.set.assign(bends, bends + k);
    for (gpe_bend &q : N.set) {
        if (q.rest_cos == 0.0f) q.rest_cos = 0.0f;                     // -0.0 -> +0
        if (q.rest_sin == 0.0f) q.rest_sin = 0.0f;
        if (q.stiffness == 0.0f) q.stiffness = 0.0f;
    }
    N.iterations = iterations;
    N.nodes = m;
    N.stale = true;
    c->bends = std::move(N);
    return GPE_OK;
}

gpe_status gpe_get_bends(const gpe_ctx *c, gpe_bend *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k) return GPE_ERR_INVALID_ARG;
    if (capacity > 0 && !out) return GPE_ERR_INVALID_ARG;
    return rows_out(c->bends.set, out, capacity, k);
}

gpe_status gpe_apply_bends(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has_bends(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return bends_pass(c);
}

gpe_status gpe_get_bends_info(gpe_ctx *c, gpe_bends_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_bends_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_bends_info: NULL info or bad struct_size");
    const BendState &S = c->bends;
    gpe_bends_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    if (has_bends(c)) {
        out.iterations = S.iterations;
        out.k = S.set.size();
        out.nodes = S.nodes;
        out.passes = S.passes;
        out.resolves = S.resolves;
    }
    *info = out;
    return GPE_OK;
}
