// gpe_bends.hip -- the bend constraints of a context (gpe_set_bends and the rest): the set, its graph (bend_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bends.hip).  What the
// entry points share with the other sets that name their particles by uid is uid_sets.h's; gpe_api.hip lists the set
// in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

#include "bend_graph.h"
#include "k_bend.h"
#include "uid_sets.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

void gpe::bends_release(gpe_ctx *c)
{
    BendState &S = c->bends;
    dev_free(c, S.rec);
    node_table_free(c, S.nt); dev_free(c, S.inc);
    dev_free(c, S.corr); dev_free(c, S.state);
    S = BendState();
}

gpe_status gpe::bends_pass(gpe_ctx *c)
{
    BendState &S = c->bends;
    return uid_set_pass(c, S.set.empty(), S.nt.stale, "Bends", &S.passes,
                        [&] { return uid_slots_resolve(c, "bends/resolve", S.nt); },
                        [&] {
                            return launch_bends_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                     (uint32_t)S.nt.nodes, S.iterations);
                        });
}

gpe_status gpe_set_bends(gpe_ctx *c, const gpe_bend *bends, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bend_set_problem(bends, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bends: ") + why);
    BendGraph g;
    GPE_TRY(uid_set_open(c, "gpe_set_bends", k, bends_release, [&] {
        return bend_graph_build(bends, k, &g) ? nullptr : "a uid has more than GPE_BEND_MAX_DEGREE bends";
    }));
    if (k == 0) return GPE_OK;
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    BendState N;
    HipSetUpload up({c}, "gpe_set_bends");
    up.reserve(&N.rec, 2 * k, "uid.bend_rec");
    node_table_upload(up, &N.nt, g.nodes, g.row_start, "uid.bend_node_uid", "uid.bend_node_slot", "uid.bend_row_start");
    up.reserve(&N.inc, g.inc.size(), "uid.bend_inc");
    up.reserve(&N.corr, k, "uid.bend_corr");
    up.reserve(&N.state, k, "uid.bend_state");
    up.copy(N.rec, g.rec.data(), g.rec.size());
    up.copy(N.inc, g.inc.data(), g.inc.size());
    up.fill(N.corr, 0, k * sizeof(float4));
    up.fill(N.state, (int)kBendInert, k);
    GPE_TRY(up.finish());
    bends_release(c);
    N.set.assign(bends, bends + k);
    for (gpe_bend &q : N.set) {
        q.rest_cos = plus_zero(q.rest_cos);
        q.rest_sin = plus_zero(q.rest_sin);
        q.stiffness = plus_zero(q.stiffness);
    }
    N.iterations = iterations;
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
    return uid_set_apply(c, has_bends, bends_pass);
}

gpe_status gpe_get_bends_info(gpe_ctx *c, gpe_bends_info *info)
{
    gpe_bends_info out;
    GPE_TRY(info_open(c, "gpe_get_bends_info", info, &out));
    const BendState &S = c->bends;
    if (has_bends(c)) {
        out.iterations = S.iterations;
        out.k = S.set.size();
        out.nodes = S.nt.nodes;
        out.passes = S.passes;
        out.resolves = S.nt.resolves;
    }
    *info = out;
    return GPE_OK;
}
