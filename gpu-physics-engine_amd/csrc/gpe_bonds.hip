// gpe_bonds.hip -- the distance bonds of a context (gpe_set_bonds and the rest): the set, its graph (bond_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bonds.hip).  What the
// entry points share with the other sets that name their particles by uid is uid_sets.h's; gpe_api.hip lists the set
// in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

#include "bond_colours.h"
#include "bond_graph.h"
#include "k_bond.h"
#include "uid_sets.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

void gpe::bonds_release(gpe_ctx *c)
{
    BondState &S = c->bonds;
    dev_free(c, S.rec); dev_free(c, S.max_length); dev_free(c, S.anchors);
    node_table_free(c, S.nt); dev_free(c, S.inc);
    dev_free(c, S.corr); dev_free(c, S.state); dev_free(c, S.broken);
    dev_free(c, S.order); dev_free(c, S.colour_start);
    S = BondState();
}

gpe_status gpe::bonds_pass(gpe_ctx *c)
{
    BondState &S = c->bonds;
    return uid_set_pass(c, S.set.empty(), S.nt.stale, "Bonds", &S.passes,
                        [&] { return uid_slots_resolve(c, "bonds/resolve", S.nt); },
                        [&]() -> gpe_status {
                            if (c->bond_solver.mode == GPE_BOND_SOLVER_COLOURED) {
                                GPE_TRY(launch_bonds_coloured(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                              (uint32_t)S.nt.nodes, S.iterations, &c->bond_solver.form));
                                c->bond_solver.passes += 1;
                                return GPE_OK;
                            }
                            return launch_bonds_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                     (uint32_t)S.nt.nodes, S.iterations);
                        });
}

// The colours of g's bonds (bond_colours.h).  NULL, or why the coloured solver cannot take the set (text kept in *why)
static const char *bond_colours_of(const BondGraph &g, BondColours *col, std::string *why)
{
    if (bond_colours_build(g.rec.data(), g.rec.size(), g.nodes.size(), col)) return nullptr;
    *why = "the coloured solver needs " + std::to_string(col->colours) +
           " colours for this set, more than GPE_BOND_COLOURS_MAX (gpe_set_bond_solver)";
    return why->c_str();
}

// The colour tables inside an upload transaction, into N.  Read by index below the count they are allocated with.  no slack
static void bond_colours_upload(HipSetUpload &up, BondState *N, const BondColours &col)
{
    up.reserve(&N->order, col.order.size(), "uid.bond_order");
    up.reserve(&N->colour_start, col.colour_start.size(), "uid.bond_colour_start");
    up.copy(N->order, col.order.data(), col.order.size());
    up.copy(N->colour_start, col.colour_start.data(), col.colour_start.size());
    N->colour_begin = col.colour_start;
    N->colours = col.colours;
    N->largest_colour = col.largest;
}

gpe_status gpe_set_bonds(gpe_ctx *c, const gpe_bond *bonds, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bond_set_problem(bonds, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bonds: ") + why);
    BondGraph g;
    BondColours col;
    std::string why;
    const bool coloured = c->bond_solver.mode == GPE_BOND_SOLVER_COLOURED;
    GPE_TRY(uid_set_open(c, "gpe_set_bonds", k, bonds_release, [&]() -> const char * {
        if (!bond_graph_build(bonds, k, &g)) return "a uid has more than GPE_BOND_MAX_DEGREE bonds";
        return coloured ? bond_colours_of(g, &col, &why) : nullptr;
    }));
    if (k == 0) return GPE_OK;
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    const unsigned long long broken = g.broken;
    BondState N;
    N.n_anchors = (uint32_t)(g.anchors.size() / 2);
    HipSetUpload up({c}, "gpe_set_bonds");
    up.reserve(&N.rec, k, "uid.bond_rec");
    up.reserve(&N.max_length, g.max_length.empty() ? 0 : k, "uid.bond_max_length");
    up.reserve(&N.anchors, N.n_anchors, "uid.bond_anchors");
    node_table_upload(up, &N.nt, g.nodes, g.row_start, "uid.bond_node_uid", "uid.bond_node_slot", "uid.bond_row_start");
    up.reserve(&N.inc, g.inc.size(), "uid.bond_inc");
    up.reserve(&N.corr, k, "uid.bond_corr");
    up.reserve(&N.state, k, "uid.bond_state");
    up.reserve(&N.broken, 1, "uid.bond_broken");
    if (coloured) bond_colours_upload(up, &N, col);
    up.copy(N.rec, g.rec.data(), g.rec.size());
    up.copy(N.max_length, g.max_length.data(), g.max_length.size());
    up.copy(N.anchors, g.anchors.data(), g.anchors.size());
    up.copy(N.inc, g.inc.data(), g.inc.size());
    up.copy(N.state, g.state.data(), g.state.size());
    up.fill(N.corr, 0, k * sizeof(float2));
    up.copy(N.broken, &broken, 1);
    GPE_TRY(up.finish());
    bonds_release(c);
    N.set.assign(bonds, bonds + k);
    for (gpe_bond &q : N.set) {
        q.flags &= ~(uint32_t)GPE_BOND_BROKEN;                         // (it set the flag in state; the record does not keep it)
        q.rest_length = plus_zero(q.rest_length);
        q.max_length = plus_zero(q.max_length);
    }
    N.iterations = iterations;
    c->bonds = std::move(N);
    return GPE_OK;
}

gpe_status gpe_get_bonds(gpe_ctx *c, gpe_bond *out, uint8_t *broken_out, uint64_t capacity, uint64_t *k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!k) return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_bonds: NULL k");
    BondState &S = c->bonds;
    *k = S.set.size();
    const uint64_t m = std::min<uint64_t>(S.set.size(), capacity);
    if (m == 0) return GPE_OK;
    if (out) memcpy(out, S.set.data(), m * sizeof(gpe_bond));
    return broken_out ? gpe::broken_out(c, S.state, m, kBondBroken, broken_out) : GPE_OK;
}

gpe_status gpe_apply_bonds(gpe_ctx *c)
{
    return uid_set_apply(c, has_bonds, bonds_pass);
}

gpe_status gpe_get_bonds_info(gpe_ctx *c, gpe_bonds_info *info)
{
    gpe_bonds_info out;
    GPE_TRY(info_open(c, "gpe_get_bonds_info", info, &out));
    const BondState &S = c->bonds;
    if (has_bonds(c)) {
        out.iterations = S.iterations;
        out.k = S.set.size();
        out.nodes = S.nt.nodes;
        out.passes = S.passes;
        out.resolves = S.nt.resolves;
        GPE_TRY(info_broken(c, S.broken, &out));
    }
    *info = out;
    return GPE_OK;
}

// ---- the solver (gpe_set_bond_solver): a mode of the pass above, kept in c->bond_solver; the colour tables are the set's
gpe_status gpe_set_bond_solver(gpe_ctx *c, uint32_t mode)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (mode != GPE_BOND_SOLVER_JACOBI && mode != GPE_BOND_SOLVER_COLOURED)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_bond_solver: mode must be GPE_BOND_SOLVER_JACOBI or GPE_BOND_SOLVER_COLOURED");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_bond_solver");
    BondState &S = c->bonds;
    BondColours col;
    const bool build = mode == GPE_BOND_SOLVER_COLOURED && !S.set.empty() && !S.order;
    if (build) {                                                       // from the kept set, before anything changes
        BondGraph g;
        std::string why;
        if (!bond_graph_build(S.set.data(), S.set.size(), &g))
            return fail(c, GPE_ERR_STATE, "gpe_set_bond_solver: the set held no longer builds");
        if (const char *no = bond_colours_of(g, &col, &why)) return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bond_solver: ") + no);
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old tables)
    if (build) {
        BondState N;                                                   // (only the colour fields are used)
        HipSetUpload up({c}, "gpe_set_bond_solver");
        bond_colours_upload(up, &N, col);
        GPE_TRY(up.finish());
        S.order = N.order; S.colour_start = N.colour_start;
        S.colour_begin = std::move(N.colour_begin);
        S.colours = N.colours; S.largest_colour = N.largest_colour;
    }
    if (mode == GPE_BOND_SOLVER_JACOBI) {
        dev_free(c, S.order); dev_free(c, S.colour_start);
        S.colour_begin.clear();
        S.colours = S.largest_colour = 0;
    }
    c->bond_solver = BondSolverState();
    c->bond_solver.mode = mode;
    return GPE_OK;
}

gpe_status gpe_get_bond_solver(gpe_ctx *c, uint32_t *mode)
{
    if (!c || !mode) return GPE_ERR_INVALID_ARG;
    *mode = c->bond_solver.mode;
    return GPE_OK;
}

gpe_status gpe_get_bond_solver_info(gpe_ctx *c, gpe_bond_solver_info *info)
{
    gpe_bond_solver_info out;
    GPE_TRY(info_open(c, "gpe_get_bond_solver_info", info, &out));
    out.mode = c->bond_solver.mode;
    out.colours = c->bonds.colours;
    out.largest_colour = c->bonds.largest_colour;
    out.form = c->bond_solver.form;
    out.lds_nodes_max = kBondLdsNodesMax;
    out.passes = c->bond_solver.passes;
    *info = out;
    return GPE_OK;
}
