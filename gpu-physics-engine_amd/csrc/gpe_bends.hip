// gpe_bends.hip -- the bend constraints of a context (gpe_set_bends and the rest): the set, its graph (bend_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bends.hip).  What the
// entry points share with the other sets that name their particles by uid is uid_sets.h's; gpe_api.hip lists the set
// in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

#include "bend_colours.h"
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
    dev_free(c, S.order); dev_free(c, S.colour_start);
    S = BendState();
}

gpe_status gpe::bends_pass(gpe_ctx *c)
{
    BendState &S = c->bends;
    return uid_set_pass(c, S.set.empty(), S.nt.stale, "Bends", &S.passes,
                        [&] { return uid_slots_resolve(c, "bends/resolve", S.nt); },
                        [&]() -> gpe_status {
                            if (c->bend_solver.mode == GPE_BEND_SOLVER_COLOURED) {
                                GPE_TRY(launch_bends_coloured(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                              (uint32_t)S.nt.nodes, S.iterations, &c->bend_solver.form));
                                c->bend_solver.passes += 1;
                                return GPE_OK;
                            }
                            return launch_bends_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                     (uint32_t)S.nt.nodes, S.iterations);
                        });
}

// The colours of g's bends (bend_colours.h).  NULL, or why the coloured solver cannot take the set (text kept in *why)
static const char *bend_colours_of(const BendGraph &g, BendColours *col, std::string *why)
{
    if (bend_colours_build(g.rec.data(), g.rec.size(), g.nodes.size(), col)) return nullptr;
    *why = "the coloured solver needs " + std::to_string(col->colours) +
           " colours for this set, more than GPE_BEND_COLOURS_MAX (gpe_set_bend_solver)";
    return why->c_str();
}

// The colour tables inside an upload transaction, into N.  Read by index below the count they are allocated with.  no slack
static void bend_colours_upload(HipSetUpload &up, BendState *N, const BendColours &col)
{
    up.reserve(&N->order, col.order.size(), "uid.bend_order");
    up.reserve(&N->colour_start, col.colour_start.size(), "uid.bend_colour_start");
    up.copy(N->order, col.order.data(), col.order.size());
    up.copy(N->colour_start, col.colour_start.data(), col.colour_start.size());
    N->colour_begin = col.colour_start;
    N->colours = col.colours;
    N->largest_colour = col.largest;
}

gpe_status gpe_set_bends(gpe_ctx *c, const gpe_bend *bends, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bend_set_problem(bends, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bends: ") + why);
    BendGraph g;
    BendColours col;
    std::string why;
    const bool coloured = c->bend_solver.mode == GPE_BEND_SOLVER_COLOURED;
    GPE_TRY(uid_set_open(c, "gpe_set_bends", k, bends_release, [&]() -> const char * {
        if (!bend_graph_build(bends, k, &g)) return "a uid has more than GPE_BEND_MAX_DEGREE bends";
        return coloured ? bend_colours_of(g, &col, &why) : nullptr;
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
    if (coloured) bend_colours_upload(up, &N, col);
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

// ---- the solver (gpe_set_bend_solver): a mode of the pass above, kept in c->bend_solver; the colour tables are the set's
gpe_status gpe_set_bend_solver(gpe_ctx *c, uint32_t mode)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (mode != GPE_BEND_SOLVER_JACOBI && mode != GPE_BEND_SOLVER_COLOURED)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_bend_solver: mode must be GPE_BEND_SOLVER_JACOBI or GPE_BEND_SOLVER_COLOURED");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_bend_solver");
    BendState &S = c->bends;
    BendColours col;
    const bool build = mode == GPE_BEND_SOLVER_COLOURED && !S.set.empty() && !S.order;
    if (build) {                                                       // from the kept set, before anything changes
        BendGraph g;
        std::string why;
        if (!bend_graph_build(S.set.data(), S.set.size(), &g))
            return fail(c, GPE_ERR_STATE, "gpe_set_bend_solver: the set held no longer builds");
        if (const char *no = bend_colours_of(g, &col, &why)) return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bend_solver: ") + no);
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old tables)
    if (build) {
        BendState N;                                                   // (only the colour fields are used)
        HipSetUpload up({c}, "gpe_set_bend_solver");
        bend_colours_upload(up, &N, col);
        GPE_TRY(up.finish());
        S.order = N.order; S.colour_start = N.colour_start;
        S.colour_begin = std::move(N.colour_begin);
        S.colours = N.colours; S.largest_colour = N.largest_colour;
    }
    if (mode == GPE_BEND_SOLVER_JACOBI) {
        dev_free(c, S.order); dev_free(c, S.colour_start);
        S.colour_begin.clear();
        S.colours = S.largest_colour = 0;
    }
    c->bend_solver = BendSolverState();
    c->bend_solver.mode = mode;
    return GPE_OK;
}

gpe_status gpe_get_bend_solver(gpe_ctx *c, uint32_t *mode)
{
    if (!c || !mode) return GPE_ERR_INVALID_ARG;
    *mode = c->bend_solver.mode;
    return GPE_OK;
}

gpe_status gpe_get_bend_solver_info(gpe_ctx *c, gpe_bend_solver_info *info)
{
    gpe_bend_solver_info out;
    GPE_TRY(info_open(c, "gpe_get_bend_solver_info", info, &out));
    out.mode = c->bend_solver.mode;
    out.colours = c->bends.colours;
    out.largest_colour = c->bends.largest_colour;
    out.form = c->bend_solver.form;
    out.lds_nodes_max = kBendLdsNodesMax;
    out.passes = c->bend_solver.passes;
    *info = out;
    return GPE_OK;
}
