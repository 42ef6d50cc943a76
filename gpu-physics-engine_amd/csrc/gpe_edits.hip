// gpe_edits.hip -- the entry points that change particles in place on the device: overlap-checked adds
// (gpe_add_particles_free), edits by index or uid (gpe_edit_particles) and velocity kicks (gpe_kick_*).
#include <math.h>

#include <algorithm>
#include <new>

#include "gpe_internal.h"
#include "k_uids.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

// ---- overlap-checked adds (k_spawn.hip) --------------------------------------------------------------------
// Scratch of the call's own: nothing of the contact or cluster workspaces is used, so a later query finds its buffers
// as it left them.
static gpe_status spawn_reserve(gpe_ctx *c, uint64_t k)
{
    SpawnWorkspace &ws = c->spawn_ws;
    const char *who = "gpe_add_particles_free";
    if (ws.cap < k) {
        dev_free(c, ws.pos); dev_free(c, ws.radius); dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec);
        dev_free(c, ws.blocked); dev_free(c, ws.state); dev_free(c, ws.rank); dev_free(c, ws.verdict);
        ws.cap = 0;
        // pos / radius: the k uploaded candidates, read by index below k.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.pos, k, 0, "spawn.pos"));
        GPE_TRY(ws_alloc(c, who, &ws.radius, k, 0, "spawn.radius"));
        // keys / vals: k words each.  slack: the 16 words sort_pairs' tile loads may read behind the k pairs
        GPE_TRY(ws_alloc(c, who, &ws.keys, k, 16 * sizeof(uint32_t), "spawn.keys"));
        GPE_TRY(ws_alloc(c, who, &ws.vals, k, 16 * sizeof(uint32_t), "spawn.vals"));
        // rec: k 16-byte records, read one at a time below k.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.rec, k, 0, "spawn.rec"));
        // blocked / state: k words each, written and read by index below k.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.blocked, k, 0, "spawn.blocked"));
        GPE_TRY(ws_alloc(c, who, &ws.state, k, 0, "spawn.state"));
        // rank: k words, scanned in place.  slack: the 16 words the scan's tile loads may read behind them
        GPE_TRY(ws_alloc(c, who, &ws.rank, k, 16 * sizeof(uint32_t), "spawn.rank"));
        // verdict: k bytes, written and copied out below k.  no slack
        GPE_TRY(ws_alloc(c, who, &ws.verdict, k, 0, "spawn.verdict"));
        ws.cap = k;
    }
    // ctl: kSpawnCtlWords words.  no slack
    if (!ws.ctl) GPE_TRY(ws_alloc(c, who, &ws.ctl, kSpawnCtlWords, 0, "spawn.ctl"));
    GPE_TRY(sort_reserve(c, k));
    return scan_reserve(c, k);
}

void gpe::spawn_release(gpe_ctx *c)
{
    SpawnWorkspace &ws = c->spawn_ws;
    dev_free(c, ws.pos); dev_free(c, ws.radius); dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec);
    dev_free(c, ws.blocked); dev_free(c, ws.state); dev_free(c, ws.rank); dev_free(c, ws.verdict); dev_free(c, ws.ctl);
    ws.cap = 0;
}

// The separation rounds: batches of kSpawnRoundsPerLook launches, then one look at the batch's undecided counters.
static gpe_status spawn_separate(gpe_ctx *c, uint32_t k, float cell_size)
{
    const SpawnWorkspace &ws = c->spawn_ws;
    uint32_t *left = ws.ctl + kSpawnCtlRounds, h_left[kSpawnRoundsPerLook];
    for (uint64_t rounds = 0;; rounds += kSpawnRoundsPerLook) {
        // (every round settles one more workgroup block at least, and the lowest undecided index: k rounds always suffice)
        if (rounds > (uint64_t)k + kSpawnRoundsPerLook) return fail(c, GPE_ERR_HIP, "gpe_add_particles_free: the separation did not settle");
        GPE_HIP(c, hipMemsetAsync(left, 0, sizeof(h_left), c->stream));
        for (int r = 0; r < kSpawnRoundsPerLook; ++r) {
            Scope s(c, "spawn/round");
            GPE_TRY(launch_spawn_round(c, ws, k, cell_size, left + r));
        }
        GPE_HIP(c, hipMemcpyAsync(h_left, left, sizeof(h_left), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        if (h_left[kSpawnRoundsPerLook - 1] == 0) return GPE_OK;
    }
}

gpe_status gpe_add_particles_free(gpe_ctx *c, gpe_particle_spawn *sp)
{
    const char *who = "gpe_add_particles_free";
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!sp) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL spawn");
    if (sp->struct_size < sizeof(gpe_particle_spawn))                  // (`added` is the last field: such a struct has none)
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": struct_size is smaller than gpe_particle_spawn");
    sp->added = 0;
    const uint32_t known = GPE_SPAWN_SEPARATE | GPE_SPAWN_INSIDE_WORLD | GPE_SPAWN_DRY_RUN;
    if (sp->flags & ~known) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": unknown flag bits");
    GPE_TRY(need_particles(c));
    if (is_sharded(c)) return refuse_sharded(c, who);
    const uint64_t k = sp->k;
    if (k == 0) return GPE_OK;
    if (!sp->pos_xy || !sp->radius) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL array");
    if (k > (1ull << 30) - 1 || c->n + k > (1ull << 30) - 1)
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": 4 (gpe_len + k) must fit in u32");
    // the search's own cell size: a contact implies a centre distance below 2 R, less than one cell of 2.2 R
    float big = fabsf(c->max_radius);
    bool finite = isfinite(big);
    for (uint64_t i = 0; i < k; ++i) {
        const float a = fabsf(sp->radius[i]);
        finite = finite && isfinite(a);
        big = a > big ? a : big;
    }
    const float cell_size = gpe_compute_cell_size(big);
    if (!finite || !isfinite(cell_size)) return refuse_radius_not_finite(c, who);
    const bool search = big > 0.0f;                                // every radius 0: nothing touches
    const bool separate = (sp->flags & GPE_SPAWN_SEPARATE) != 0 && search;
    const uint32_t k32 = (uint32_t)k;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> state;                                    // the verdicts: the user's array is written at the end only
    try {
        state.resize(k);
    } catch (const std::bad_alloc &) {
        return fail(c, GPE_ERR_OOM, std::string(who) + ": out of host memory for the verdicts");
    }
    {
        Scope s(c, "Spawn check");
        GPE_TRY(spawn_reserve(c, k));
        const SpawnWorkspace &ws = c->spawn_ws;
        GPE_HIP(c, hipMemcpyAsync(ws.pos, sp->pos_xy, k * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        GPE_HIP(c, hipMemcpyAsync(ws.radius, sp->radius, k * sizeof(float), hipMemcpyHostToDevice, c->stream));
        {
            Scope b(c, "spawn/bin");
            GPE_TRY(launch_spawn_keys(c, ws, k32, cell_size, (sp->flags & GPE_SPAWN_INSIDE_WORLD) != 0));
            if (search) {
                GPE_TRY(sort_pairs(c, ws.keys, ws.vals, k));
                GPE_TRY(launch_contacts_records_of(c, ws.pos, ws.radius, ws.vals, k, ws.rec));
            }
        }
        {
            Scope p(c, "spawn/pass");
            GPE_TRY(launch_spawn_pass(c, ws, k32, cell_size, search));
        }
        GPE_TRY(launch_spawn_resolve(c, ws, k32, separate));
        if (separate) {
            Scope r(c, "spawn/separate");
            GPE_TRY(spawn_separate(c, k32, cell_size));
        }
        GPE_TRY(launch_spawn_flags(c, ws, k32));
        GPE_HIP(c, hipMemcpyAsync(state.data(), ws.verdict, k, hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
    }
    uint64_t added = 0;
    for (uint64_t i = 0; i < k; ++i) added += state[i] == GPE_SPAWN_ADDED ? 1u : 0u;
    const bool append = added > 0 && !(sp->flags & GPE_SPAWN_DRY_RUN);
    if (append) {
        const uint64_t old_n = c->n, new_n = c->n + added;
        if (c->uid.on && c->uid.next + added > kUidLimit)
            return fail(c, GPE_ERR_STATE, std::string(who) + ": the new particles' uids would pass 2^32 - 1");
        if (new_n > c->cap) GPE_TRY(grow_particle_buffers(c, std::max<uint64_t>(new_n, c->cap * 2)));
        Scope s(c, "spawn/append");
        const SpawnWorkspace &ws = c->spawn_ws;
        GPE_TRY(inclusive_scan(c, ws.rank, k));                    // (the flags: launch_spawn_flags above)
        GPE_TRY(launch_spawn_scatter(c, ws, k32, old_n));
        c->n = new_n;
        c->n_owned = new_n;
        GPE_TRY(init_index_buffers(c, old_n, new_n));
        if (c->uid.on) {                                   // next .. next + added - 1, in input order
            GPE_TRY(launch_uid_iota(c, c->uid.uids, old_n, new_n, (uint32_t)c->uid.next));
            c->uid.next += added;
            c->uid.map_valid = false;
            uid_slots_stale(c);
        }
        // as gpe_add_particles of the added candidates: max_radius = max(max_radius, r), in input order
        for (uint64_t i = 0; i < k; ++i)
            if (state[i] == GPE_SPAWN_ADDED) c->max_radius = fmaxf(c->max_radius, sp->radius[i]);
        c->grid_max_radius = c->max_radius;
        refresh_cell_size(c);
        GPE_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (sp->verdict) std::copy(state.begin(), state.end(), sp->verdict);
    sp->added = added;
    return append ? reconfigure(c) : GPE_OK;
}

// ---- editing particles in place (k_edit.hip) ---------------------------------------------------------------
// One buffer of the edit workspace (tags "edit.*"): allocated at first use and, with a capacity word, regrown when
// `count` passes it (cap == NULL: a buffer of fixed size).  payload: count elements; slack_bytes: stated at the call
// with its reader.
template <typename T>
static gpe_status edit_buffer(gpe_ctx *c, T **p, uint64_t *cap, uint64_t count, uint64_t slack_bytes, const char *tag)
{
    if (*p && (!cap || *cap >= count)) return GPE_OK;
    dev_free(c, *p);
    if (cap) *cap = 0;
    // ("hipMalloc" is no caller's name: it keeps the text these failures always had, "hipMalloc: ...")
    GPE_TRY(ws_alloc(c, "hipMalloc", p, count, slack_bytes, tag));
    if (cap) *cap = count;
    return GPE_OK;
}

void gpe::edit_release(gpe_ctx *c)
{
    EditWorkspace &ws = c->edit_ws;
    dev_free(c, ws.keys); dev_free(c, ws.slots); dev_free(c, ws.fields); dev_free(c, ws.flag);
    dev_free(c, ws.tile_key); dev_free(c, ws.max_key); dev_free(c, ws.count);
    ws.keys_cap = ws.fields_cap = ws.tiles_cap = 0;
}

// staging rows, 256-byte aligned parts, only the requested fields: pos | prev | radius
struct EditRows {
    uint64_t o_prev = 0, o_radius = 0, bytes = 0;
};
static EditRows edit_rows(const gpe_particle_edit *e)
{
    StageLayout lay;
    EditRows r;
    lay.part(e->pos_xy, e->k * 8);                                 // (at offset 0)
    r.o_prev = lay.part(e->prev_xy, e->k * 8);
    r.o_radius = lay.part(e->radius, e->k * 4);
    r.bytes = lay.bytes;
    return r;
}

static gpe_status do_edit(gpe_ctx *c, gpe_particle_edit *e)
{
    EditWorkspace &ws = c->edit_ws;
    const uint64_t k = e->k, n = c->n;
    const bool by_uid = e->key_kind == GPE_EDIT_BY_UID;
    const EditRows rows = edit_rows(e);
    if (by_uid) GPE_TRY(uid_map_ready(c));
    // keys / slots (one capacity): sorted by sort_pairs, whose tile loads may read 16 words behind the k pairs
    uint64_t cap_keys = ws.keys ? ws.keys_cap : 0, cap_slots = ws.slots ? ws.keys_cap : 0;
    ws.keys_cap = 0;
    GPE_TRY(edit_buffer(c, &ws.keys, &cap_keys, k, 16 * sizeof(uint32_t), "edit.keys"));
    GPE_TRY(edit_buffer(c, &ws.slots, &cap_slots, k, 16 * sizeof(uint32_t), "edit.slots"));
    ws.keys_cap = std::min(cap_keys, cap_slots);
    GPE_TRY(edit_buffer(c, &ws.fields, &ws.fields_cap, rows.bytes, 0, "edit.fields"));
    GPE_TRY(edit_buffer(c, &ws.flag, nullptr, 2, 0, "edit.flag"));
    if (k > 1) GPE_TRY(sort_reserve(c, k));
    Scope s(c, "Edit particles");
    uint32_t flag[2] = {0, 0};
    {
        Scope sk(c, "edit/check");
        GPE_HIP(c, hipMemcpyAsync(ws.keys, e->keys, k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        GPE_HIP(c, hipMemsetAsync(ws.flag, 0, sizeof(flag), c->stream));
        GPE_TRY(launch_edit_check(c, by_uid, ws.keys, ws.slots, k, ws.flag));
        if (k > 1) {                                             // two keys naming one particle become neighbours
            GPE_TRY(sort_pairs(c, ws.keys, ws.slots, k));
            GPE_TRY(launch_edit_adjacent(c, ws.keys, k, ws.flag));
        }
    }
    GPE_HIP(c, hipMemcpyAsync(flag, ws.flag, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (flag[0] & kEditBadIndex) return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: an index is not below gpe_len");
    if (flag[0] & kEditDuplicate) return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: two keys name the same particle");
    if (flag[1] == 0) return GPE_OK;                             // every uid absent: nothing to write
    // from here on the particles change
    uint8_t *st = ws.fields;
    const float2 *d_pos = e->pos_xy ? reinterpret_cast<const float2 *>(st) : nullptr;
    const float2 *d_prev = e->prev_xy ? reinterpret_cast<const float2 *>(st + rows.o_prev) : nullptr;
    const float *d_radius = e->radius ? reinterpret_cast<const float *>(st + rows.o_radius) : nullptr;
    {
        Scope sk(c, "edit/apply");
        if (d_pos) GPE_HIP(c, hipMemcpyAsync(st, e->pos_xy, k * 8, hipMemcpyHostToDevice, c->stream));
        if (d_prev) GPE_HIP(c, hipMemcpyAsync(st + rows.o_prev, e->prev_xy, k * 8, hipMemcpyHostToDevice, c->stream));
        if (d_radius) GPE_HIP(c, hipMemcpyAsync(st + rows.o_radius, e->radius, k * 4, hipMemcpyHostToDevice, c->stream));
        GPE_TRY(launch_edit_apply(c, ws.keys, ws.slots, k, d_pos, d_prev, d_radius));
    }
    if (d_radius) {
        const uint64_t tiles = query_tiles(n);
        GPE_TRY(edit_buffer(c, &ws.tile_key, &ws.tiles_cap, tiles, 0, "edit.tile_key"));
        GPE_TRY(edit_buffer(c, &ws.max_key, nullptr, 1, 0, "edit.max_key"));
        unsigned long long key = 0;
        {
            Scope sk(c, "edit/max radius");
            GPE_TRY(launch_edit_max_radius(c, ws.tile_key, ws.max_key));
        }
        GPE_HIP(c, hipMemcpyAsync(&key, ws.max_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        const uint32_t winner = (uint32_t)(key & 0xFFFFFFFFull);   // index of the max |radius|, the last on ties
        if (winner >= n) return fail(c, GPE_ERR_STATE, "gpe_edit_particles: bad max-radius index");
        float max_r = 0.f;
        GPE_HIP(c, hipMemcpyAsync(&max_r, c->radius + winner, sizeof(max_r), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        c->max_radius = max_r;                                   // sign kept
        c->grid_max_radius = c->max_radius;
        refresh_cell_size(c);
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));                 // the host arrays may be released on return
    if (d_pos || d_radius) GPE_TRY(reconfigure_native(c));       // (prev alone is part of no kept structure)
    e->edited = flag[1];
    return GPE_OK;
}

gpe_status gpe_edit_particles(gpe_ctx *c, gpe_particle_edit *e)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!e) return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: NULL edit");
    if (e->struct_size < sizeof(gpe_particle_edit))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: struct_size is smaller than gpe_particle_edit");
    e->edited = 0;
    if (!e->keys) return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: NULL keys");
    if (e->key_kind != GPE_EDIT_BY_INDEX && e->key_kind != GPE_EDIT_BY_UID)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: unknown key_kind");
    if (!e->pos_xy && !e->prev_xy && !e->radius)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: every field array is NULL");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_edit_particles");
    if (e->key_kind == GPE_EDIT_BY_UID && !c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_edit_particles: uids are off");
    if (e->k == 0) return GPE_OK;
    GPE_TRY(need_particles(c));
    // (more indices than particles repeat one; a list of uids may be padded with absent ones)
    if (e->key_kind == GPE_EDIT_BY_INDEX && e->k > c->n)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: two keys name the same particle");
    if (e->k > (1ull << 30) - 1) return fail(c, GPE_ERR_INVALID_ARG, "gpe_edit_particles: k too large");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return do_edit(c, e);
}

// The checks the two kicks share, in this order: *n_kicked = 0, the sharded refusal, op and a.
static gpe_status kick_begin(gpe_ctx *c, const char *who, uint32_t op, float ax, float ay, uint64_t *n_kicked)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (n_kicked) *n_kicked = 0;
    if (is_sharded(c)) return refuse_sharded(c, who);
    if (op != GPE_VEL_ADD && op != GPE_VEL_SET && op != GPE_VEL_SCALE)
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": unknown operation");
    if (!isfinite(ax) || !isfinite(ay)) return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": ax and ay must be finite");
    return GPE_OK;
}

static gpe_status do_kick(gpe_ctx *c, bool box, const float *region, uint32_t op, float ax, float ay, uint64_t *n_kicked)
{
    if (c->n == 0 || !c->pos) return GPE_OK;                      // nothing to kick
    GPE_HIP(c, hipSetDevice(c->device));
    unsigned long long *d_count = nullptr;
    if (n_kicked) {
        GPE_TRY(edit_buffer(c, &c->edit_ws.count, nullptr, 1, 0, "edit.count"));
        d_count = c->edit_ws.count;
    }
    {
        Scope s(c, "Kick particles");
        GPE_TRY(launch_kick(c, box, region, op, ax, ay, d_count));
    }
    if (!n_kicked) return GPE_OK;                                 // stream-ordered, like gpe_step
    unsigned long long kicked = 0;
    GPE_HIP(c, hipMemcpyAsync(&kicked, d_count, sizeof(kicked), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    *n_kicked = kicked;
    return GPE_OK;
}

gpe_status gpe_kick_circle(gpe_ctx *c, float x, float y, float radius, uint32_t op, float ax, float ay, uint64_t *n_kicked)
{
    float region[5];
    GPE_TRY(kick_begin(c, "gpe_kick_circle", op, ax, ay, n_kicked));
    GPE_TRY(circle_region(c, "gpe_kick_circle", x, y, radius, region));
    return do_kick(c, false, region, op, ax, ay, n_kicked);
}

gpe_status gpe_kick_box(gpe_ctx *c, float x0, float y0, float x1, float y1, uint32_t op, float ax, float ay,
                        uint64_t *n_kicked)
{
    float region[5];
    bool empty = false;
    GPE_TRY(kick_begin(c, "gpe_kick_box", op, ax, ay, n_kicked));
    GPE_TRY(box_region(c, "gpe_kick_box", x0, y0, x1, y1, region, &empty));
    if (empty) return GPE_OK;                                     // an empty box holds nothing
    return do_kick(c, true, region, op, ax, ay, n_kicked);
}
