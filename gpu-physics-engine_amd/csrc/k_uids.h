// k_uids.h -- launchers of k_uids.hip: opt-in particle uids (gpe_enable_uids and friends, include/gpe.h).
#pragma once

#include "gpe_internal.h"

namespace gpe {

// uids[i] = first + (i - lo) for i in [lo, hi)
gpe_status launch_uid_iota(gpe_ctx *c, uint32_t *uids, uint64_t lo, uint64_t hi, uint32_t first);
// K4 with the uids carried through the same permutation (52 B per particle instead of 44)
gpe_status launch_rearrange_uids(gpe_ctx *c, const float2 *pos, const float2 *prev, const float *radius,
                                 const uint32_t *uids, const uint32_t *ids, uint64_t n, float2 *pos_out,
                                 float2 *prev_out, float *radius_out, uint32_t *uids_out);
// keys[i] = uids[i], vals[i] = i
gpe_status launch_uid_map_init(gpe_ctx *c, const uint32_t *uids, uint64_t n, uint32_t *keys, uint32_t *vals);
// *dup (zeroed by the caller) = 1 when two adjacent sorted keys are equal
gpe_status launch_uid_adjacent(gpe_ctx *c, const uint32_t *keys, uint64_t n, uint32_t *dup);
// For each of the k queries: the storage index of that uid (GPE_UID_ABSENT if none) and, where the output pointer is
// not NULL, its pos / prev / radius (quiet NaN if absent).  (keys, vals) is the sorted map of n >= 1 entries.
gpe_status launch_uid_find(gpe_ctx *c, const uint32_t *keys, const uint32_t *vals, uint64_t n, const uint32_t *query,
                           uint64_t k, uint32_t *index_out, float2 *pos_out, float2 *prev_out, float *radius_out);
// mask[index of uid] = 1 for every query found in the map (mask zeroed by the caller)
gpe_status launch_uid_mark(gpe_ctx *c, const uint32_t *keys, const uint32_t *vals, uint64_t n, const uint32_t *query,
                           uint64_t k, uint8_t *mask);

// The storage index of uid q in the sorted map (keys, vals) of n >= 1 entries, or GPE_UID_ABSENT.  lower_bound by
// halving: ceil(log2 n) steps, a select each.  (k_uid_find, k_uid_mark; k_edit_check of k_edit.hip)
__device__ __forceinline__ uint32_t uid_lookup(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                               uint32_t n, uint32_t q)
{
    uint32_t base = 0, len = n;
    while (len > 1) {                          // uniform: the same len sequence on every lane
        const uint32_t half = len >> 1;
        base = keys[base + half] < q ? base + half : base;
        len -= half;
    }
    const uint32_t at = base + (keys[base] < q ? 1u : 0u);
    const uint32_t hit = at < n ? keys[at] : ~q;
    return hit == q ? vals[at] : GPE_UID_ABSENT;
}

}  // namespace gpe
