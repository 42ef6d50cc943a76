// uid_sets.h -- what the entry points of the step sets that name their particles by uid share (gpe_bonds.hip,
// gpe_bends.hip, gpe_areas.hip, gpe_bodies.hip): the slot lookup of a stale set, the skeleton of a pass, the opening of
// gpe_set_<sets>, gpe_apply_<sets>, the opening of gpe_get_<sets>_info and the two read-backs of broken flags.  Host
// code.  The sets' state is in gpe_internal.h (UidNodeTable and the four states), their table in gpe_api.hip.
#pragma once

#include <functional>

#include "gpe_internal.h"
#include "k_uids.h"
#include "uid_nodes.h"

namespace gpe {

// slots[i] = the storage index of uids[i] (0xffffffff for none), under the scope `scope_name`: the uid map is made ready
// first (its build synchronises), one lookup per uid is enqueued.  then: what else the set derives from the slots,
// enqueued under the same scope (the areas' member slots).  The set is no longer stale afterwards
inline gpe_status uid_slots_resolve(gpe_ctx *c, const char *scope_name, const uint32_t *uids, uint64_t count,
                                    uint32_t *slots, bool *stale, uint64_t *resolves,
                                    gpe_status (*then)(gpe_ctx *) = nullptr)
{
    GPE_TRY(uid_map_ready(c));
    Scope s(c, scope_name);
    GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, c->n, uids, count, slots, nullptr, nullptr, nullptr));
    if (then) GPE_TRY(then(c));
    *stale = false;
    *resolves += 1;
    return GPE_OK;
}

// ... of a node table
inline gpe_status uid_slots_resolve(gpe_ctx *c, const char *scope_name, UidNodeTable &T,
                                    gpe_status (*then)(gpe_ctx *) = nullptr)
{
    return uid_slots_resolve(c, scope_name, T.node_uid, T.nodes, T.node_slot, &T.stale, &T.resolves, then);
}

// One pass of a set over the particles as they are now, under the scope `scope`.  Enqueues only, unless the set's slots
// are stale: then resolve() looks them up first (uid_slots_resolve)
template <class Resolve, class Launch>
gpe_status uid_set_pass(gpe_ctx *c, bool empty, bool stale, const char *scope, uint64_t *passes, Resolve resolve,
                        Launch launch)
{
    if (empty || c->n == 0 || !c->pos || !c->uid.on || !c->uid.uids) return GPE_OK;
    if (stale) GPE_TRY(resolve());
    Scope s(c, scope);
    GPE_TRY(launch());
    *passes += 1;
    return GPE_OK;
}

// gpe_set_<sets> behind the set's own validation, in the one order its refusals have: a sharded context, uids off,
// what build() says of a set of k > 0 (NULL: nothing; the bonds' and bends' degree caps), then the device and the
// stream -- a pass in flight reads the old set -- and k == 0 releases the set: the caller returns
inline gpe_status uid_set_open(gpe_ctx *c, const char *who, uint64_t k, void (*release)(gpe_ctx *),
                               const std::function<const char *()> &build = nullptr)
{
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (k > 0 && !c->uid.on) return fail(c, GPE_ERR_STATE, std::string(who) + ": uids are off (gpe_enable_uids)");
    if (k > 0 && build)
        if (const char *why = build()) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": " + why);
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (k == 0) release(c);
    return GPE_OK;
}

// gpe_apply_<sets>
inline gpe_status uid_set_apply(gpe_ctx *c, bool (*has)(const gpe_ctx *), gpe_status (*pass)(gpe_ctx *))
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return pass(c);
}

// gpe_get_<sets>_info: the caller's struct is checked, *out zeroed but for its struct_size
template <class Info>
gpe_status info_open(gpe_ctx *c, const char *who, const Info *info, Info *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(Info))
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL info or bad struct_size");
    memset(out, 0, sizeof(*out));
    out->struct_size = info->struct_size;
    return GPE_OK;
}
// ... and out->broken, out->live from the set's device word and out->k (bonds, bodies)
template <class Info>
gpe_status info_broken(gpe_ctx *c, const unsigned long long *word, Info *out)
{
    GPE_HIP(c, hipSetDevice(c->device));
    unsigned long long broken = 0;
    GPE_TRY(read_back(c, word, &broken, sizeof(broken)));
    out->broken = broken;
    out->live = out->k - broken;
    return GPE_OK;
}

// out[j] = 1 where state[j] == broken_value, for the first m constraints (gpe_get_bonds, gpe_get_bodies)
inline gpe_status broken_out(gpe_ctx *c, const uint8_t *state, uint64_t m, uint8_t broken_value, uint8_t *out)
{
    GPE_HIP(c, hipSetDevice(c->device));
    std::vector<uint8_t> bytes(m);
    GPE_TRY(read_back(c, state, bytes.data(), m));
    for (uint64_t j = 0; j < m; ++j) out[j] = bytes[j] == broken_value ? 1 : 0;
    return GPE_OK;
}

}  // namespace gpe
