// gpe_queries.hip -- the read-only queries of include/gpe.h: regions and picking, contacts, clusters, ray casts and
// nearest neighbours.  Each leaves the context as it was; their workspaces are freed with the particles (gpe_api.hip).
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <functional>
#include <limits>

#include "gpe_internal.h"
#include "k_uids.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

// ---- region queries and picking (k_query.hip) -------------------------------------------------------------
static gpe_status query_reserve(gpe_ctx *c, uint64_t stage_bytes)
{
    QueryWorkspace &ws = c->query_ws;
    const uint64_t tiles = query_tiles(c->n);
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_count);
        dev_free(c, ws.tile_key);
        ws.tiles_cap = 0;
        GPE_TRY(dev_alloc(c, &ws.tile_count, tiles, "query.tile_count"));
        GPE_TRY(dev_alloc(c, &ws.tile_key, tiles, "query.tile_key"));
        ws.tiles_cap = tiles;
    }
    if (!ws.pick) GPE_TRY(dev_alloc(c, &ws.pick, 1, "query.pick"));
    if (ws.stage_cap < stage_bytes) {
        dev_free(c, ws.stage);
        ws.stage_cap = 0;
        GPE_TRY(dev_alloc(c, &ws.stage, stage_bytes, "query.stage"));
        ws.stage_cap = stage_bytes;
    }
    return scan_reserve(c, tiles);
}

void gpe::query_release(gpe_ctx *c)
{
    QueryWorkspace &ws = c->query_ws;
    dev_free(c, ws.tile_count); dev_free(c, ws.tile_key); dev_free(c, ws.pick); dev_free(c, ws.stage);
    ws.tiles_cap = ws.stage_cap = 0;
}

static bool query_wants_rows(const gpe_query_result *out)
{
    return out->index || out->uid || out->pos_xy || out->prev_xy || out->radius;
}

// The checks every query shares, in this order: the result struct (nothing written when it is unusable), then
// out->count = 0, the sharded refusal and uids for a uid output.  *go = false: GPE_OK with count 0 (no particles).
static gpe_status query_begin(gpe_ctx *c, gpe_query_result *out, const char *who, bool *go)
{
    *go = false;
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL result");
    if (out->struct_size < sizeof(gpe_query_result))
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_query_result");
    out->count = 0;
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (out->uid && !c->uid.on) return refuse_uid_off(c, who);
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    *go = c->n > 0 && c->pos;
    return GPE_OK;
}

// The first min(total, capacity) rows of a selection into the requested arrays of `out`, and out->count = total.
// gather(m, index, uid, pos, prev, radius) launches the kernel that fills the staging parts (NULL: not requested).
using QueryGather = std::function<gpe_status(uint32_t, uint32_t *, uint32_t *, float2 *, float2 *, float *)>;
static gpe_status query_deliver(gpe_ctx *c, gpe_query_result *out, uint32_t total, const char *scope,
                                const QueryGather &gather)
{
    QueryWorkspace &ws = c->query_ws;
    const uint64_t m = std::min<uint64_t>(total, out->capacity);
    if (m > 0 && query_wants_rows(out)) {
        // staging, 256-byte aligned parts, only the requested fields: pos | prev | radius | index | uid
        StageLayout lay;
        const uint64_t o_pos = lay.part(out->pos_xy, m * 8), o_prev = lay.part(out->prev_xy, m * 8),
                       o_radius = lay.part(out->radius, m * 4), o_index = lay.part(out->index, m * 4),
                       o_uid = lay.part(out->uid, m * 4);
        GPE_TRY(query_reserve(c, lay.bytes));
        uint8_t *st = ws.stage;
        float2 *d_pos = out->pos_xy ? reinterpret_cast<float2 *>(st + o_pos) : nullptr;
        float2 *d_prev = out->prev_xy ? reinterpret_cast<float2 *>(st + o_prev) : nullptr;
        float *d_radius = out->radius ? reinterpret_cast<float *>(st + o_radius) : nullptr;
        uint32_t *d_index = out->index ? reinterpret_cast<uint32_t *>(st + o_index) : nullptr;
        uint32_t *d_uid = out->uid ? reinterpret_cast<uint32_t *>(st + o_uid) : nullptr;
        {
            Scope k(c, scope);
            GPE_TRY(gather((uint32_t)m, d_index, d_uid, d_pos, d_prev, d_radius));
        }
        if (d_index) GPE_HIP(c, hipMemcpyAsync(out->index, d_index, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_uid) GPE_HIP(c, hipMemcpyAsync(out->uid, d_uid, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_pos) GPE_HIP(c, hipMemcpyAsync(out->pos_xy, d_pos, m * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_prev) GPE_HIP(c, hipMemcpyAsync(out->prev_xy, d_prev, m * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_radius) GPE_HIP(c, hipMemcpyAsync(out->radius, d_radius, m * 4, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
    }
    out->count = total;
    return GPE_OK;
}

// Count (and, for requested rows, gather) the particles in the region; kind and region as launch_query_count takes them.
static gpe_status do_query(gpe_ctx *c, int kind, const float *region, gpe_query_result *out)
{
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(query_reserve(c, 0));
    QueryWorkspace &ws = c->query_ws;
    const uint64_t tiles = query_tiles(c->n);
    uint32_t total = 0;
    Scope s(c, "Query particles");
    {
        Scope k(c, "query/count");
        GPE_TRY(launch_query_count(c, kind, region, ws.tile_count));
    }
    {
        Scope k(c, "query/scan");
        GPE_TRY(inclusive_scan(c, ws.tile_count, tiles));
    }
    GPE_HIP(c, hipMemcpyAsync(&total, ws.tile_count + (tiles - 1), sizeof(total), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return query_deliver(c, out, total, "query/gather",
                         [&](uint32_t m, uint32_t *d_index, uint32_t *d_uid, float2 *d_pos, float2 *d_prev, float *d_radius) {
                             return launch_query_gather(c, kind, region, c->query_ws.tile_count, m, d_index, d_uid, d_pos,
                                                        d_prev, d_radius);
                         });
}

// The argument checks and the region words (as launch_query_count takes them) of the circle and box calls: the
// queries and the kicks (gpe_kick_*) share them, so that both select the same particles.
gpe_status gpe::circle_region(gpe_ctx *c, const char *who, float x, float y, float radius, float (&region)[5])
{
    if (!(radius >= 0.0f) || !isfinite(radius))
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": radius must be finite and >= 0");
    const float words[5] = {x, y, 0.f, 0.f, radius * radius};     // binary32, as gpe_remove_particles_in_circle
    std::copy(words, words + 5, region);
    return GPE_OK;
}

// *empty: x0 > x1 or y0 > y1, a box that holds nothing
gpe_status gpe::box_region(gpe_ctx *c, const char *who, float x0, float y0, float x1, float y1, float (&region)[5],
                           bool *empty)
{
    if (isnan(x0) || isnan(y0) || isnan(x1) || isnan(y1)) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NaN bound");
    const float words[5] = {x0, y0, x1, y1, 0.f};
    std::copy(words, words + 5, region);
    *empty = x0 > x1 || y0 > y1;
    return GPE_OK;
}

gpe_status gpe_query_circle(gpe_ctx *c, float x, float y, float radius, gpe_query_result *out)
{
    bool go = false;
    float region[5];
    GPE_TRY(query_begin(c, out, "gpe_query_circle", &go));
    GPE_TRY(circle_region(c, "gpe_query_circle", x, y, radius, region));
    if (!go) return GPE_OK;
    return do_query(c, 0, region, out);
}

gpe_status gpe_query_box(gpe_ctx *c, float x0, float y0, float x1, float y1, gpe_query_result *out)
{
    bool go = false;
    float region[5];
    bool empty = false;
    GPE_TRY(query_begin(c, out, "gpe_query_box", &go));
    GPE_TRY(box_region(c, "gpe_query_box", x0, y0, x1, y1, region, &empty));
    if (!go || empty) return GPE_OK;                              // an empty box holds nothing
    return do_query(c, 1, region, out);
}

gpe_status gpe_query_segment(gpe_ctx *c, float x0, float y0, float x1, float y1, gpe_query_result *out)
{
    bool go = false;
    GPE_TRY(query_begin(c, out, "gpe_query_segment", &go));
    if (!isfinite(x0) || !isfinite(y0) || !isfinite(x1) || !isfinite(y1))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_query_segment: an endpoint is not finite");
    if (!go) return GPE_OK;
    const float region[5] = {x0, y0, x1, y1, 0.f};
    return do_query(c, 2, region, out);
}

// Particle i alone, straight from the particle buffers: its row when there is room for one, and count = 1.
static gpe_status deliver_one_row(gpe_ctx *c, gpe_query_result *out, uint32_t i)
{
    if (out->capacity >= 1) {
        if (out->uid) GPE_HIP(c, hipMemcpyAsync(out->uid, c->uid.uids + i, 4, hipMemcpyDeviceToHost, c->stream));
        if (out->pos_xy) GPE_HIP(c, hipMemcpyAsync(out->pos_xy, c->pos + i, 8, hipMemcpyDeviceToHost, c->stream));
        if (out->prev_xy) GPE_HIP(c, hipMemcpyAsync(out->prev_xy, c->prev + i, 8, hipMemcpyDeviceToHost, c->stream));
        if (out->radius) GPE_HIP(c, hipMemcpyAsync(out->radius, c->radius + i, 4, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        if (out->index) out->index[0] = i;
    }
    out->count = 1;
    return GPE_OK;
}

gpe_status gpe_pick(gpe_ctx *c, float x, float y, gpe_query_result *out)
{
    bool go = false;
    GPE_TRY(query_begin(c, out, "gpe_pick", &go));
    if (!go) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(query_reserve(c, 0));
    QueryWorkspace &ws = c->query_ws;
    unsigned long long key = 0;
    {
        Scope s(c, "Query particles");
        Scope k(c, "query/pick");
        GPE_TRY(launch_pick(c, x, y, ws.tile_key, ws.pick));
    }
    GPE_HIP(c, hipMemcpyAsync(&key, ws.pick, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (key == ~0ull) return GPE_OK;                               // no disc contains the point
    const uint32_t i = (uint32_t)(key & 0xFFFFFFFFull);
    if (i >= c->n) return fail(c, GPE_ERR_STATE, "gpe_pick: bad index");
    return deliver_one_row(c, out, i);
}

// ---- contact queries (k_contacts.hip) ----------------------------------------------------------------------
static gpe_status contacts_reserve(gpe_ctx *c, uint64_t stage_bytes)
{
    ContactsWorkspace &ws = c->contacts_ws;
    const char *who = "gpe_query_contacts";
    const uint64_t n = c->n, tiles = contacts_tiles(n);
    if (ws.cap < n) {
        dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec); dev_free(c, ws.degree); dev_free(c, ws.upper);
        ws.cap = 0;
        // keys / vals: n words each.  slack: the 16 words sort_pairs' tile loads may read behind the n pairs
        GPE_TRY(ws_alloc(c, who, &ws.keys, n, 16 * sizeof(uint32_t), "contacts.keys"));
        GPE_TRY(ws_alloc(c, who, &ws.vals, n, 16 * sizeof(uint32_t), "contacts.vals"));
        // rec: n 16-byte records, read one at a time below n.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.rec, n, 0, "contacts.rec"));
        // degree: n words, written and read by index below n.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.degree, n, 0, "contacts.degree"));
        // upper: n words, scanned in place.  slack: the 16 words the scan's tile loads may read behind them
        GPE_TRY(ws_alloc(c, who, &ws.upper, n, 16 * sizeof(uint32_t), "contacts.upper"));
        ws.cap = n;
    }
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_sum);
        ws.tiles_cap = 0;
        // tile_sum: one 64-bit word per workgroup of the count.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.tile_sum, tiles, 0, "contacts.tile_sum"));
        ws.tiles_cap = tiles;
    }
    // total: one 64-bit word.  no slack
    if (!ws.total) GPE_TRY(ws_alloc(c, who, &ws.total, 1, 0, "contacts.total"));
    if (ws.stage_cap < stage_bytes) {
        dev_free(c, ws.stage);
        ws.stage_cap = 0;
        // stage: the 256-byte aligned parts of the requested per-pair arrays, written below capacity.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.stage, stage_bytes, 0, "contacts.stage"));
        ws.stage_cap = stage_bytes;
    }
    GPE_TRY(sort_reserve(c, n));
    return scan_reserve(c, n);
}

void gpe::contacts_release(gpe_ctx *c)
{
    ContactsWorkspace &ws = c->contacts_ws;
    dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec); dev_free(c, ws.degree); dev_free(c, ws.upper);
    dev_free(c, ws.tile_sum); dev_free(c, ws.total); dev_free(c, ws.stage);
    ws.cap = ws.tiles_cap = ws.stage_cap = 0;
}

// Stages (1) and (2) of the contact query, shared with the cluster query: the workspace, the cell keys under
// `cell_size`, the sort and the 16-byte records.  Leaves contacts_ws.keys / .rec sorted by cell.  Call inside the
// query's own scope, after the stream is idle.
static gpe_status contacts_bin(gpe_ctx *c, float cell_size)
{
    GPE_TRY(contacts_reserve(c, 0));
    ContactsWorkspace &ws = c->contacts_ws;
    {
        Scope k(c, "contacts/keys");
        GPE_TRY(launch_contacts_keys(c, cell_size, ws.keys, ws.vals));
    }
    {
        Scope k(c, "contacts/sort");
        GPE_TRY(sort_pairs(c, ws.keys, ws.vals, c->n));
        GPE_TRY(launch_contacts_records(c, ws.vals, ws.rec));
    }
    return GPE_OK;
}

gpe_status gpe_query_contacts(gpe_ctx *c, gpe_contact_result *out)
{
    const char *who = "gpe_query_contacts";
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL result");
    if (out->struct_size < sizeof(gpe_contact_result)) {
        if (out->struct_size >= offsetof(gpe_contact_result, count) + sizeof(out->count)) out->count = 0;   // it has one
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_contact_result");
    }
    out->count = 0;
    if (is_sharded(c)) return refuse_sharded(c, who);
    if ((out->uid_a || out->uid_b) && !c->uid.on) return refuse_uid_off(c, who);
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    const uint64_t n = c->n;
    if (n == 0 || !c->pos) return GPE_OK;
    // the query's own cell size: a contact implies a centre distance below 2 max|r|, less than one cell of 2.2 max|r|
    const float cell_size = gpe_compute_cell_size(fabsf(c->max_radius));
    if (n > 1 && !isfinite(cell_size)) return refuse_radius_not_finite(c, who);
    if (n == 1 || cell_size == 0.0f) {                             // one particle, or every radius 0: nothing touches
        if (out->degree) std::fill(out->degree, out->degree + n, 0u);
        return GPE_OK;
    }
    const bool want_pairs = out->index_a || out->index_b || out->uid_a || out->uid_b || out->overlap;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    ContactsWorkspace &ws = c->contacts_ws;
    unsigned long long total = 0;
    Scope s(c, "Query contacts");
    GPE_TRY(contacts_bin(c, cell_size));
    {
        Scope k(c, "contacts/count");
        GPE_TRY(launch_contacts_count(c, ws.keys, ws.rec, ws.degree, ws.upper, ws.tile_sum, ws.total));
    }
    GPE_HIP(c, hipMemcpyAsync(&total, ws.total, sizeof(total), hipMemcpyDeviceToHost, c->stream));
    if (out->degree) GPE_HIP(c, hipMemcpyAsync(out->degree, ws.degree, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (want_pairs && total > 0xFFFFFFFFull) {                    // the one error that leaves count (and degree) set
        out->count = total;
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 contacts cannot be listed");
    }
    const uint64_t m = std::min<uint64_t>(total, out->capacity);
    if (m > 0 && want_pairs) {
        // staging, 256-byte aligned parts, only the requested arrays: index_a | index_b | uid_a | uid_b | overlap
        StageLayout lay;
        const uint64_t o_a = lay.part(out->index_a, m * 4), o_b = lay.part(out->index_b, m * 4),
                       o_ua = lay.part(out->uid_a, m * 4), o_ub = lay.part(out->uid_b, m * 4),
                       o_ov = lay.part(out->overlap, m * 4);
        GPE_TRY(contacts_reserve(c, lay.bytes));
        uint8_t *st = ws.stage;
        uint32_t *d_a = out->index_a ? reinterpret_cast<uint32_t *>(st + o_a) : nullptr;
        uint32_t *d_b = out->index_b ? reinterpret_cast<uint32_t *>(st + o_b) : nullptr;
        uint32_t *d_ua = out->uid_a ? reinterpret_cast<uint32_t *>(st + o_ua) : nullptr;
        uint32_t *d_ub = out->uid_b ? reinterpret_cast<uint32_t *>(st + o_ub) : nullptr;
        float *d_ov = out->overlap ? reinterpret_cast<float *>(st + o_ov) : nullptr;
        {
            Scope k(c, "contacts/scan");
            GPE_TRY(inclusive_scan(c, ws.upper, n));
        }
        {
            Scope k(c, "contacts/gather");
            GPE_TRY(launch_contacts_gather(c, ws.keys, ws.rec, ws.upper, (uint32_t)m, d_a, d_b, d_ua, d_ub, d_ov));
        }
        if (d_a) GPE_HIP(c, hipMemcpyAsync(out->index_a, d_a, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_b) GPE_HIP(c, hipMemcpyAsync(out->index_b, d_b, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_ua) GPE_HIP(c, hipMemcpyAsync(out->uid_a, d_ua, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_ub) GPE_HIP(c, hipMemcpyAsync(out->uid_b, d_ub, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_ov) GPE_HIP(c, hipMemcpyAsync(out->overlap, d_ov, m * 4, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
    }
    out->count = total;
    return GPE_OK;
}

// ---- contact clusters (k_clusters.hip) ---------------------------------------------------------------------
static gpe_status clusters_reserve(gpe_ctx *c)
{
    ClustersWorkspace &ws = c->clusters_ws;
    const char *who = "gpe_query_clusters";
    const uint64_t n = c->n, tiles = contacts_tiles(n);
    if (ws.cap < n) {
        dev_free(c, ws.parent); dev_free(c, ws.label); dev_free(c, ws.root_size); dev_free(c, ws.size);
        ws.cap = 0;
        // parent: n words, read and written by index below n (the indices of the sorted records).  no slack
        GPE_TRY(ws_alloc(c, who, &ws.parent, n, 0, "clusters.parent"));
        // label: n words, written by index below n; the member kernels read it by index below n (guarded tile loads).  no slack
        GPE_TRY(ws_alloc(c, who, &ws.label, n, 0, "clusters.label"));
        // root_size: n words, indexed by a label, which is an index below n.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.root_size, n, 0, "clusters.root_size"));
        // size: n words, written by index below n.  no slack (nothing here is scanned; the members' scan runs on
        // query.tile_count)
        GPE_TRY(ws_alloc(c, who, &ws.size, n, 0, "clusters.size"));
        ws.cap = n;
    }
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_word);
        ws.tiles_cap = 0;
        // tile_word: one 64-bit word per workgroup of the flatten / sizes kernels.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.tile_word, tiles, 0, "clusters.tile_word"));
        ws.tiles_cap = tiles;
    }
    // words: two 64-bit words.  no slack
    if (!ws.words) GPE_TRY(ws_alloc(c, who, &ws.words, 2, 0, "clusters.words"));
    return GPE_OK;
}

void gpe::clusters_release(gpe_ctx *c)
{
    ClustersWorkspace &ws = c->clusters_ws;
    dev_free(c, ws.parent); dev_free(c, ws.label); dev_free(c, ws.root_size); dev_free(c, ws.size);
    dev_free(c, ws.tile_word); dev_free(c, ws.words);
    ws.cap = ws.tiles_cap = 0;
}

// The checks the two cluster queries share once the result struct is usable and its count is 0: the refusals of
// gpe_query_contacts.  *cell_size = the contact query's own cell size.
static gpe_status clusters_begin(gpe_ctx *c, const char *who, float *cell_size)
{
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    *cell_size = gpe_compute_cell_size(fabsf(c->max_radius));
    if (c->n > 1 && !isfinite(*cell_size)) return refuse_radius_not_finite(c, who);
    return GPE_OK;
}

// The labels of all particles into clusters_ws.label and the number of clusters into *count (read back; the stream is
// idle afterwards).  n > 1 and a finite non-zero cell size.  Call inside the "Query clusters" scope.
static gpe_status clusters_label(gpe_ctx *c, float cell_size, unsigned long long *count)
{
    GPE_TRY(clusters_reserve(c));
    GPE_TRY(contacts_bin(c, cell_size));
    ClustersWorkspace &ws = c->clusters_ws;
    {
        Scope k(c, "clusters/hook");
        GPE_TRY(launch_clusters_hook(c, c->contacts_ws.keys, c->contacts_ws.rec, ws.parent));
    }
    {
        Scope k(c, "clusters/flatten");
        GPE_TRY(launch_clusters_flatten(c, ws.parent, ws.label, ws.tile_word, ws.words));
    }
    GPE_HIP(c, hipMemcpyAsync(count, ws.words, sizeof(*count), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return GPE_OK;
}

gpe_status gpe_query_clusters(gpe_ctx *c, gpe_cluster_result *out)
{
    const char *who = "gpe_query_clusters";
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL result");
    if (out->struct_size < sizeof(gpe_cluster_result)) {
        if (out->struct_size >= offsetof(gpe_cluster_result, count) + sizeof(out->count)) out->count = 0;   // it has one
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_cluster_result");
    }
    out->count = 0;
    out->largest_size = out->largest_label = 0;
    float cell_size = 0.0f;
    GPE_TRY(clusters_begin(c, who, &cell_size));
    if (out->label_uid && !c->uid.on)
        return fail(c, GPE_ERR_STATE, std::string(who) + ": label_uid requested while uids are off");
    const uint64_t n = c->n;
    if (n == 0 || !c->pos) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (n == 1 || cell_size == 0.0f) {                             // one particle, or every radius 0: nothing touches
        if (out->label_uid) {                                      // label[i] = i: the particles' own uids
            GPE_HIP(c, hipMemcpyAsync(out->label_uid, c->uid.uids, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            GPE_HIP(c, hipStreamSynchronize(c->stream));
        }
        if (out->label) for (uint64_t i = 0; i < n; ++i) out->label[i] = (uint32_t)i;
        if (out->size) std::fill(out->size, out->size + n, 1u);
        out->count = n;
        out->largest_size = 1;
        out->largest_label = 0;
        return GPE_OK;
    }
    ClustersWorkspace &ws = c->clusters_ws;
    unsigned long long count = 0, largest = 0;
    Scope s(c, "Query clusters");
    GPE_TRY(clusters_label(c, cell_size, &count));
    {
        Scope k(c, "clusters/sizes");
        // parent is free after the flatten: it takes the uid of every particle's label
        GPE_TRY(launch_clusters_sizes(c, ws.label, ws.root_size, ws.size, out->label_uid ? ws.parent : nullptr, ws.tile_word,
                                      ws.words + 1));
    }
    GPE_HIP(c, hipMemcpyAsync(&largest, ws.words + 1, sizeof(largest), hipMemcpyDeviceToHost, c->stream));
    if (out->label) GPE_HIP(c, hipMemcpyAsync(out->label, ws.label, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (out->size) GPE_HIP(c, hipMemcpyAsync(out->size, ws.size, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (out->label_uid)
        GPE_HIP(c, hipMemcpyAsync(out->label_uid, ws.parent, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    out->count = count;
    out->largest_size = (uint32_t)(largest >> 32);
    out->largest_label = 0xFFFFFFFFu - (uint32_t)(largest & 0xFFFFFFFFull);
    return GPE_OK;
}

gpe_status gpe_query_cluster_of(gpe_ctx *c, uint32_t key_kind, uint32_t key, gpe_query_result *out)
{
    const char *who = "gpe_query_cluster_of";
    bool go = false;
    GPE_TRY(query_begin(c, out, who, &go));
    if (key_kind != GPE_CLUSTER_BY_INDEX && key_kind != GPE_CLUSTER_BY_UID)
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": unknown key_kind");
    if (key_kind == GPE_CLUSTER_BY_UID && !c->uid.on)
        return fail(c, GPE_ERR_STATE, std::string(who) + ": GPE_CLUSTER_BY_UID while uids are off");
    if (key_kind == GPE_CLUSTER_BY_INDEX && key >= c->n)
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": index >= gpe_len");
    float cell_size = 0.0f;
    GPE_TRY(clusters_begin(c, who, &cell_size));
    if (!go) return GPE_OK;                                        // no particles: every uid is absent
    const uint64_t n = c->n;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t seed = key;
    if (key_kind == GPE_CLUSTER_BY_UID) {                          // through the uid -> index map, as gpe_find_uids
        GPE_TRY(uid_map_ready(c));
        GPE_TRY(uid_query_reserve(c, 2 * sizeof(uint32_t)));
        uint32_t *d_index = reinterpret_cast<uint32_t *>(c->uid.query), *d_query = d_index + 1;
        GPE_HIP(c, hipMemcpyAsync(d_query, &key, sizeof(key), hipMemcpyHostToDevice, c->stream));
        {
            Scope k(c, "uids/find");
            GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, n, d_query, 1, d_index, nullptr, nullptr, nullptr));
        }
        GPE_HIP(c, hipMemcpyAsync(&seed, d_index, sizeof(seed), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        if (seed == GPE_UID_ABSENT) return GPE_OK;                 // an absent uid: count 0
        if (seed >= n) return fail(c, GPE_ERR_STATE, std::string(who) + ": bad index");
    }
    if (n == 1 || cell_size == 0.0f) return deliver_one_row(c, out, seed);   // nothing touches: the seed alone
    GPE_TRY(query_reserve(c, 0));
    ClustersWorkspace &ws = c->clusters_ws;
    const uint64_t tiles = query_tiles(n);
    unsigned long long count = 0;
    uint32_t want = 0, total = 0;
    Scope s(c, "Query clusters");
    GPE_TRY(clusters_label(c, cell_size, &count));
    GPE_HIP(c, hipMemcpyAsync(&want, ws.label + seed, sizeof(want), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    {
        Scope k(c, "clusters/gather");
        GPE_TRY(launch_clusters_member_count(c, ws.label, want, c->query_ws.tile_count));
        GPE_TRY(inclusive_scan(c, c->query_ws.tile_count, tiles));
    }
    GPE_HIP(c, hipMemcpyAsync(&total, c->query_ws.tile_count + (tiles - 1), sizeof(total), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return query_deliver(c, out, total, "clusters/gather",
                         [&](uint32_t m, uint32_t *d_index, uint32_t *d_uid, float2 *d_pos, float2 *d_prev, float *d_radius) {
                             return launch_clusters_member_gather(c, ws.label, want, c->query_ws.tile_count, m, d_index,
                                                                  d_uid, d_pos, d_prev, d_radius);
                         });
}

// ---- ray casts (k_raycast.hip) ------------------------------------------------------------------------------
// room for a batch of k rays; every array is read and written by index below k or kRayRowWords.  no slack
static gpe_status ray_reserve(gpe_ctx *c, uint64_t k)
{
    RayWorkspace &ws = c->ray_ws;
    const char *who = "gpe_cast_rays";
    if (!ws.row_start) GPE_TRY(ws_alloc(c, who, &ws.row_start, kRayRowWords, 0, "ray.row_start"));
    if (ws.cap < k) {
        dev_free(c, ws.from); dev_free(c, ws.to); dev_free(c, ws.index); dev_free(c, ws.uid); dev_free(c, ws.t);
        dev_free(c, ws.pos); dev_free(c, ws.radius);
        ws.cap = 0;
        GPE_TRY(ws_alloc(c, who, &ws.from, k, 0, "ray.from"));
        GPE_TRY(ws_alloc(c, who, &ws.to, k, 0, "ray.to"));
        GPE_TRY(ws_alloc(c, who, &ws.index, k, 0, "ray.index"));
        GPE_TRY(ws_alloc(c, who, &ws.uid, k, 0, "ray.uid"));
        GPE_TRY(ws_alloc(c, who, &ws.t, k, 0, "ray.t"));
        GPE_TRY(ws_alloc(c, who, &ws.pos, k, 0, "ray.pos"));
        GPE_TRY(ws_alloc(c, who, &ws.radius, k, 0, "ray.radius"));
        ws.cap = k;
    }
    return GPE_OK;
}

void gpe::ray_release(gpe_ctx *c)
{
    RayWorkspace &ws = c->ray_ws;
    dev_free(c, ws.row_start); dev_free(c, ws.from); dev_free(c, ws.to); dev_free(c, ws.index); dev_free(c, ws.uid);
    dev_free(c, ws.t); dev_free(c, ws.pos); dev_free(c, ws.radius);
    ws.cap = 0;
}

// every ray misses: the host fills the requested outputs
static void ray_fill_misses(gpe_ray_cast *r)
{
    const uint64_t k = r->k;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (r->index) std::fill(r->index, r->index + k, GPE_RAY_MISS);
    if (r->uid) std::fill(r->uid, r->uid + k, GPE_UID_ABSENT);
    if (r->t) std::fill(r->t, r->t + k, nan);
    if (r->pos_xy) std::fill(r->pos_xy, r->pos_xy + 2 * k, nan);
    if (r->radius) std::fill(r->radius, r->radius + k, nan);
}

gpe_status gpe_cast_rays(gpe_ctx *c, gpe_ray_cast *r)
{
    const char *who = "gpe_cast_rays";
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!r) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL cast");
    if (r->struct_size < sizeof(gpe_ray_cast))             // hits is the last field: a smaller struct has none
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_ray_cast");
    r->hits = 0;
    if (r->flags != 0) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": flags must be 0");
    const uint64_t k = r->k;
    if (k > 0 && (!r->from_xy || !r->to_xy)) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL endpoints");
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (r->uid && !c->uid.on) return refuse_uid_off(c, who);
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    if (k == 0) return GPE_OK;
    const bool any = c->n > 0 && c->pos;
    // the contact query's own cell size: a touched centre lies within max|r| = cell / 2.2 of its segment
    const float cell_size = any ? gpe_compute_cell_size(fabsf(c->max_radius)) : 0.0f;
    if (!isfinite(cell_size)) return refuse_radius_not_finite(c, who);
    const float bound = cell_size > 0.0f ? 131072.0f * cell_size : std::numeric_limits<float>::infinity();
    for (uint64_t i = 0; i < 2 * k; ++i) {
        const float a = r->from_xy[i], b = r->to_xy[i];
        if (!isfinite(a) || !isfinite(b) || !(fabsf(a) <= bound) || !(fabsf(b) <= bound))
            return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": an endpoint is not finite or lies more than 131072 "
                                                                   "cells from the origin");
    }
    if (!any || !(cell_size > 0.0f)) {                          // no particles, or every radius 0: nothing can be hit
        ray_fill_misses(r);
        return GPE_OK;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t batch = std::min<uint64_t>(k, kRayMaxBatch);
    GPE_TRY(ray_reserve(c, batch));
    RayWorkspace &ws = c->ray_ws;
    Scope s(c, "Cast rays");
    GPE_TRY(contacts_bin(c, cell_size));
    {
        Scope q(c, "rays/rows");
        GPE_TRY(launch_ray_row_start(c, c->contacts_ws.keys, ws.row_start));
    }
    std::vector<uint32_t> index(batch);
    uint64_t hits = 0;
    for (uint64_t base = 0; base < k; base += batch) {
        const uint64_t m = std::min<uint64_t>(batch, k - base);
        GPE_HIP(c, hipMemcpyAsync(ws.from, r->from_xy + 2 * base, m * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        GPE_HIP(c, hipMemcpyAsync(ws.to, r->to_xy + 2 * base, m * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        {
            Scope q(c, "rays/cast");
            GPE_TRY(launch_ray_cast(c, ws.from, ws.to, (uint32_t)m, cell_size, c->contacts_ws.keys, c->contacts_ws.rec,
                                    ws.row_start, ws.index, r->uid ? ws.uid : nullptr, r->t ? ws.t : nullptr,
                                    r->pos_xy ? ws.pos : nullptr, r->radius ? ws.radius : nullptr));
        }
        GPE_HIP(c, hipMemcpyAsync(index.data(), ws.index, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (r->uid) GPE_HIP(c, hipMemcpyAsync(r->uid + base, ws.uid, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (r->t) GPE_HIP(c, hipMemcpyAsync(r->t + base, ws.t, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (r->pos_xy) GPE_HIP(c, hipMemcpyAsync(r->pos_xy + 2 * base, ws.pos, m * 8, hipMemcpyDeviceToHost, c->stream));
        if (r->radius) GPE_HIP(c, hipMemcpyAsync(r->radius + base, ws.radius, m * 4, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < m; ++i) hits += index[i] != GPE_RAY_MISS;
        if (r->index) std::copy(index.begin(), index.begin() + m, r->index + base);
    }
    r->hits = hits;
    return GPE_OK;
}

// ---- nearest neighbours (k_nearest.hip) -------------------------------------------------------------------------
// room for a batch of k points of m slots each; every array is read and written by index below k, k * m or
// kRayRowWords.  no slack
static gpe_status nearest_reserve(gpe_ctx *c, uint64_t k, uint64_t m)
{
    NearestWorkspace &ws = c->nearest_ws;
    const char *who = "gpe_query_nearest";
    if (!ws.row_start) GPE_TRY(ws_alloc(c, who, &ws.row_start, kRayRowWords, 0, "nearest.row_start"));
    if (ws.cap < k) {
        dev_free(c, ws.points); dev_free(c, ws.count);
        ws.cap = 0;
        GPE_TRY(ws_alloc(c, who, &ws.points, k, 0, "nearest.points"));
        GPE_TRY(ws_alloc(c, who, &ws.count, k, 0, "nearest.count"));
        ws.cap = k;
    }
    const uint64_t slots = k * m;
    if (ws.slots_cap < slots) {
        dev_free(c, ws.index); dev_free(c, ws.uid); dev_free(c, ws.dist2); dev_free(c, ws.pos); dev_free(c, ws.radius);
        ws.slots_cap = 0;
        GPE_TRY(ws_alloc(c, who, &ws.index, slots, 0, "nearest.index"));
        GPE_TRY(ws_alloc(c, who, &ws.uid, slots, 0, "nearest.uid"));
        GPE_TRY(ws_alloc(c, who, &ws.dist2, slots, 0, "nearest.dist2"));
        GPE_TRY(ws_alloc(c, who, &ws.pos, slots, 0, "nearest.pos"));
        GPE_TRY(ws_alloc(c, who, &ws.radius, slots, 0, "nearest.radius"));
        ws.slots_cap = slots;
    }
    return GPE_OK;
}

void gpe::nearest_release(gpe_ctx *c)
{
    NearestWorkspace &ws = c->nearest_ws;
    dev_free(c, ws.row_start); dev_free(c, ws.points); dev_free(c, ws.count); dev_free(c, ws.index); dev_free(c, ws.uid);
    dev_free(c, ws.dist2); dev_free(c, ws.pos); dev_free(c, ws.radius);
    ws.cap = ws.slots_cap = 0;
}

// no point has a neighbour: the host fills the requested outputs
static void nearest_fill_none(gpe_nearest_query *q)
{
    const uint64_t k = q->k, slots = q->k * q->m;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (q->count) std::fill(q->count, q->count + k, 0u);
    if (q->index) std::fill(q->index, q->index + slots, GPE_NEAREST_NONE);
    if (q->uid) std::fill(q->uid, q->uid + slots, GPE_UID_ABSENT);
    if (q->dist2) std::fill(q->dist2, q->dist2 + slots, nan);
    if (q->pos_xy) std::fill(q->pos_xy, q->pos_xy + 2 * slots, nan);
    if (q->radius) std::fill(q->radius, q->radius + slots, nan);
}

gpe_status gpe_query_nearest(gpe_ctx *c, gpe_nearest_query *q)
{
    const char *who = "gpe_query_nearest";
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!q) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL query");
    if (q->struct_size < sizeof(gpe_nearest_query))        // found is the last field: a smaller struct has none
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_nearest_query");
    q->found = 0;
    if (q->flags != 0) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": flags must be 0");
    if (q->m == 0 || q->m > GPE_NEAREST_MAX_M) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": m must be 1 .. 64");
    const float md = q->max_distance;
    if (!(md >= 0.0f)) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": max_distance is NaN or negative");
    const uint64_t k = q->k, m = q->m;
    if (k > 0 && !q->point_xy) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL points");
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (q->uid && !c->uid.on) return refuse_uid_off(c, who);
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    if (k == 0) return GPE_OK;
    const bool any = c->n > 0 && c->pos;
    // the contact query's own cell while it is usable; the result never depends on it, only the points' bound does
    float cell_size = 0.0f;
    if (any) {
        cell_size = gpe_compute_cell_size(fabsf(c->max_radius));
        if (!(isfinite(cell_size) && cell_size > 0.0f)) cell_size = fmaxf(c->cfg.world_width, c->cfg.world_height) / 1024.0f;
        if (!(isfinite(cell_size) && cell_size > 0.0f))
            return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": neither the largest radius nor the world gives a "
                                                                   "finite positive cell size");
    }
    const float bound = any ? 131072.0f * cell_size : std::numeric_limits<float>::infinity();
    for (uint64_t i = 0; i < 2 * k; ++i) {
        const float a = q->point_xy[i];
        if (!isfinite(a) || !(fabsf(a) <= bound))
            return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": a point is not finite or lies more than 131072 "
                                                                   "cells from the origin");
    }
    if (!any) {                                                 // no particles: nothing to find
        nearest_fill_none(q);
        return GPE_OK;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t batch = std::min<uint64_t>(k, kNearestMaxSlots / m);
    GPE_TRY(nearest_reserve(c, batch, m));
    NearestWorkspace &ws = c->nearest_ws;
    Scope s(c, "Nearest");
    GPE_TRY(contacts_bin(c, cell_size));
    {
        Scope r(c, "nearest/rows");
        GPE_TRY(launch_ray_row_start(c, c->contacts_ws.keys, ws.row_start));
    }
    std::vector<uint32_t> count(batch);
    uint64_t found = 0;
    for (uint64_t base = 0; base < k; base += batch) {
        const uint64_t b = std::min<uint64_t>(batch, k - base), slots = b * m;
        GPE_HIP(c, hipMemcpyAsync(ws.points, q->point_xy + 2 * base, b * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        {
            Scope r(c, "nearest/search");
            GPE_TRY(launch_nearest(c, ws.points, (uint32_t)b, (uint32_t)m, md, cell_size, c->contacts_ws.keys,
                                   c->contacts_ws.rec, ws.row_start, ws.count, q->index ? ws.index : nullptr,
                                   q->uid ? ws.uid : nullptr, q->dist2 ? ws.dist2 : nullptr, q->pos_xy ? ws.pos : nullptr,
                                   q->radius ? ws.radius : nullptr));
        }
        const uint64_t at = base * m;
        GPE_HIP(c, hipMemcpyAsync(count.data(), ws.count, b * 4, hipMemcpyDeviceToHost, c->stream));
        if (q->index) GPE_HIP(c, hipMemcpyAsync(q->index + at, ws.index, slots * 4, hipMemcpyDeviceToHost, c->stream));
        if (q->uid) GPE_HIP(c, hipMemcpyAsync(q->uid + at, ws.uid, slots * 4, hipMemcpyDeviceToHost, c->stream));
        if (q->dist2) GPE_HIP(c, hipMemcpyAsync(q->dist2 + at, ws.dist2, slots * 4, hipMemcpyDeviceToHost, c->stream));
        if (q->pos_xy) GPE_HIP(c, hipMemcpyAsync(q->pos_xy + 2 * at, ws.pos, slots * 8, hipMemcpyDeviceToHost, c->stream));
        if (q->radius) GPE_HIP(c, hipMemcpyAsync(q->radius + at, ws.radius, slots * 4, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < b; ++i) found += count[i];
        if (q->count) std::copy(count.begin(), count.begin() + b, q->count + base);
    }
    q->found = found;
    return GPE_OK;
}
