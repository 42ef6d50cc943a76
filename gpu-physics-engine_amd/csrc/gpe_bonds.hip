// gpe_bonds.hip -- the distance bonds of a context (gpe_set_bonds and the rest): the set, its graph (bond_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bonds.hip).  What the
// entry points share with the other sets that name their particles by uid is uid_sets.h's; gpe_api.hip lists the set
// in its table (after_step, gpe_destroy, the refusals).
#include <string.h>

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
    S = BondState();
}

gpe_status gpe::bonds_pass(gpe_ctx *c)
{
    BondState &S = c->bonds;
    return uid_set_pass(c, S.set.empty(), S.nt.stale, "Bonds", &S.passes,
                        [&] { return uid_slots_resolve(c, "bonds/resolve", S.nt); },
                        [&] {
                            return launch_bonds_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(),
                                                     (uint32_t)S.nt.nodes, S.iterations);
                        });
}

gpe_status gpe_set_bonds(gpe_ctx *c, const gpe_bond *bonds, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bond_set_problem(bonds, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bonds: ") + why);
    BondGraph g;
    GPE_TRY(uid_set_open(c, "gpe_set_bonds", k, bonds_release, [&] {
        return bond_graph_build(bonds, k, &g) ? nullptr : "a uid has more than GPE_BOND_MAX_DEGREE bonds";
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
