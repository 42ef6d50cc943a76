// gpe_bonds.hip -- the distance bonds of a context (gpe_set_bonds and the rest): the set, its graph (bond_graph.h), the
// nodes' storage slots (looked up again only when stale) and the pass behind every step (k_bonds.hip).  gpe_api.hip
// calls bonds_after_step from after_step and bonds_release from gpe_destroy.
#include <string.h>

#include "bond_graph.h"
#include "gpe_internal.h"
#include "k_bond.h"
#include "k_uids.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static void bonds_free(gpe_ctx *c, BondState &S)
{
    dev_free(c, S.rec); dev_free(c, S.max_length); dev_free(c, S.anchors);
    dev_free(c, S.node_uid); dev_free(c, S.node_slot); dev_free(c, S.row_start); dev_free(c, S.inc);
    dev_free(c, S.corr); dev_free(c, S.state); dev_free(c, S.broken);
}

void gpe::bonds_release(gpe_ctx *c)
{
    bonds_free(c, c->bonds);
    c->bonds = BondState();
}

gpe_status gpe::refuse_bonds(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported while the context holds bonds "
                                                            "(gpe_set_bonds with k = 0 clears them)");
}

// One pass over the particles as they are now.  Enqueues only, unless the nodes' slots are stale: then the uid map is
// made ready first (its build synchronises) and one lookup per node is enqueued.
static gpe_status bonds_pass(gpe_ctx *c)
{
    BondState &S = c->bonds;
    if (S.set.empty() || c->n == 0 || !c->pos || !c->uid.on || !c->uid.uids) return GPE_OK;
    if (S.stale) {
        GPE_TRY(uid_map_ready(c));
        Scope s(c, "bonds/resolve");
        GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, c->n, S.node_uid, S.nodes, S.node_slot, nullptr,
                                nullptr, nullptr));
        S.stale = false;
        S.resolves += 1;
    }
    Scope s(c, "Bonds");
    GPE_TRY(launch_bonds_pass(c, c->pos, c->radius, c->n, S, (uint32_t)S.set.size(), (uint32_t)S.nodes, S.iterations));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::bonds_after_step(gpe_ctx *c)
{
    return bonds_pass(c);                                             // (after_step has looked: the set is not empty)
}

gpe_status gpe_set_bonds(gpe_ctx *c, const gpe_bond *bonds, uint64_t k, uint32_t iterations)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (const char *why = bond_set_problem(bonds, k, iterations))
        return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_bonds: ") + why);
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_bonds");
    if (k > 0 && !c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_set_bonds: uids are off (gpe_enable_uids)");
    BondGraph g;
    if (k > 0 && !bond_graph_build(bonds, k, &g))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_bonds: a uid has more than GPE_BOND_MAX_DEGREE bonds");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    if (k == 0) {
        bonds_release(c);
        return GPE_OK;
    }
    // the new tables beside the old ones (set_upload.h).  Every array is read and written by index below the count it
    // is allocated with.  no slack
    const uint64_t m = g.nodes.size();
    const unsigned long long broken = g.broken;
    BondState N;
    N.n_anchors = (uint32_t)(g.anchors.size() / 2);
    HipSetUpload up({c}, "gpe_set_bonds");
    up.reserve(&N.rec, k, "uid.bond_rec");
    up.reserve(&N.max_length, g.max_length.empty() ? 0 : k, "uid.bond_max_length");
    up.reserve(&N.anchors, N.n_anchors, "uid.bond_anchors");
    up.reserve(&N.node_uid, m, "uid.bond_node_uid");
    up.reserve(&N.node_slot, m, "uid.bond_node_slot");
    up.reserve(&N.row_start, m + 1, "uid.bond_row_start");
    up.reserve(&N.inc, g.inc.size(), "uid.bond_inc");
    up.reserve(&N.corr, k, "uid.bond_corr");
    up.reserve(&N.state, k, "uid.bond_state");
    up.reserve(&N.broken, 1, "uid.bond_broken");
    up.copy(N.rec, g.rec.data(), g.rec.size());
    up.copy(N.max_length, g.max_length.data(), g.max_length.size());
    up.copy(N.anchors, g.anchors.data(), g.anchors.size());
    up.copy(N.node_uid, g.nodes.data(), g.nodes.size());
    up.copy(N.row_start, g.row_start.data(), g.row_start.size());
    up.copy(N.inc, g.inc.data(), g.inc.size());
    up.copy(N.state, g.state.data(), g.state.size());
    up.fill(N.node_slot, 0xff, m * sizeof(uint32_t));
    up.fill(N.corr, 0, k * sizeof(float2));
    up.copy(N.broken, &broken, 1);
    GPE_TRY(up.finish());
    bonds_free(c, c->bonds);
    N.set.assign(bonds, bonds + k);
    for (gpe_bond &q : N.set) {
        q.flags &= ~(uint32_t)GPE_BOND_BROKEN;                         // (it set the flag in state; the record does not keep it)
        if (q.rest_length == 0.0f) q.rest_length = 0.0f;               // -0.0 -> +0
        if (q.max_length == 0.0f) q.max_length = 0.0f;
    }
    N.iterations = iterations;
    N.nodes = m;
    N.stale = true;
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
    if (broken_out) {
        GPE_HIP(c, hipSetDevice(c->device));
        std::vector<uint8_t> state(m);
        GPE_TRY(read_back(c, S.state, state.data(), m));
        for (uint64_t j = 0; j < m; ++j) broken_out[j] = state[j] == kBondBroken ? 1 : 0;
    }
    return GPE_OK;
}

gpe_status gpe_apply_bonds(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has_bonds(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return bonds_pass(c);
}

gpe_status gpe_get_bonds_info(gpe_ctx *c, gpe_bonds_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_bonds_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_bonds_info: NULL info or bad struct_size");
    BondState &S = c->bonds;
    gpe_bonds_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    if (has_bonds(c)) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long broken = 0;
        GPE_TRY(read_back(c, S.broken, &broken, sizeof(broken)));
        out.iterations = S.iterations;
        out.k = S.set.size();
        out.nodes = S.nodes;
        out.passes = S.passes;
        out.broken = broken;
        out.live = out.k - broken;
        out.resolves = S.resolves;
    }
    *info = out;
    return GPE_OK;
}
