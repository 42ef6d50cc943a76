// gpe_api.hip -- the extern "C" boundary of include/gpe.h: context, device memory, particle buffers, set / add / remove,
// uids, step ordering, downloads, profiling.  The queries are in gpe_queries.hip, the checked add, edits and kicks in
// gpe_edits.hip, the tracers and the monitor in gpe_observe.hip, the static colliders in gpe_colliders.hip, the force fields in gpe_fields.hip, the moving colliders in gpe_movers.hip.
// The sets that name their particles by uid -- the distance bonds in gpe_bonds.hip, the bend constraints in
// gpe_bends.hip, the area constraints in gpe_areas.hip, the rigid and soft bodies in gpe_bodies.hip -- share their
// node table (gpe_internal.h UidNodeTable; uid_nodes.h builds it, k_uid_nodes.h walks it) and the edges of their entry
// points (uid_sets.h); this file lists them once (kUidSets).  All device work goes to one in-order hipStream per context.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>

#include "gpe_internal.h"
#include "k_uids.h"

namespace gpe {

static std::mutex g_err_mu;
static std::string g_last_error;

gpe_status fail(gpe_ctx *ctx, gpe_status code, const std::string &msg)
{
    if (ctx) ctx->last_error = msg;
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_last_error = msg;
    return code;
}

// ---- profiling scopes ---------------------------------------------------------------------------
static int stat_index(gpe_ctx *c, const char *name)
{
    for (size_t i = 0; i < c->stats.size(); ++i)
        if (c->stats[i].name == name) return (int)i;
    ScopeStat s;
    s.name = name;
    c->stats.push_back(s);
    return (int)c->stats.size() - 1;
}

static void stamps_make_room(gpe_ctx *c, uint32_t need);

Scope::Scope(gpe_ctx *ctx, const char *name, Boundaries b, unsigned carry)
    : ctx_(ctx), shared_(b == kSharedBoundaries), carry_(carry)
{
    if (!ctx_ || !ctx_->profiling) return;
    stat_ = stat_index(ctx_, name);
    stamps_ = scope_uses_stamps(ctx_);
    if (stamps_) {
        if (!ctx_->scope_stamps.in_region()) stamps_make_room(ctx_, 2);      // (the step makes its own room: do_step)
        StampRecorder<HipStampDev> be{ctx_->stamp_be, shared_ && (carry_ & kCarryStart) && ctx_->scope_stamps.in_region()};
        start_ = ctx_->scope_stamps.open(be, shared_);
        return;
    }
    HipScopeBackend be{ctx_->stream};
    start_ = ctx_->scope_events.open(be, shared_);
}

Scope::~Scope()
{
    if (!ctx_ || start_ < 0) return;
    if (stamps_) {
        StampRecorder<HipStampDev> be{ctx_->stamp_be, shared_ && (carry_ & kCarryStop) && ctx_->scope_stamps.in_region()};
        ctx_->scope_stamps.close(be, start_, stat_, shared_);
        return;
    }
    HipScopeBackend be{ctx_->stream};
    ctx_->scope_events.close(be, start_, stat_, shared_);
}

constexpr size_t kTraceCap = 1u << 16;

static void resolved(gpe_ctx *c, int stat, float ms, bool has_origin, float t0)
{
    c->stats[stat].total_ms += ms;
    c->stats[stat].calls += 1;
    if (!has_origin) return;
    if (c->trace.size() >= kTraceCap) c->trace.erase(c->trace.begin(), c->trace.begin() + kTraceCap / 2);
    TraceEvent e;
    e.stat = stat; e.start_ms = t0; e.dur_ms = ms;
    c->trace.push_back(e);
}

// (after a stream synchronisation) reads the pending pairs into the statistics and the trace; their events or slots go
// back to the pool, a shared one when the last pair that uses it has been read.  The slots are read with one copy.
static void resolve_pending(gpe_ctx *c)
{
    c->scope_events.resolve([c](int stat, hipEvent_t start, hipEvent_t stop) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, start, stop) != hipSuccess) return;
        float t0 = 0.f;
        const bool has_origin = c->trace_origin && hipEventElapsedTime(&t0, c->trace_origin, start) == hipSuccess;
        resolved(c, stat, ms, has_origin, t0);
    });
    if (c->scope_stamps.pending() == 0) return;
    auto &be = c->stamp_be;
    std::vector<unsigned long long> ticks(be.next);
    const bool read = be.dev.buf && c->stamp_khz > 0.0 &&
                      hipMemcpy(ticks.data(), be.dev.buf, ticks.size() * sizeof(ticks[0]), hipMemcpyDeviceToHost) == hipSuccess;
    if (!read) (void)hipGetLastError();
    c->scope_stamps.resolve([&](int stat, uint32_t start, uint32_t stop) {
        if (!read) return;
        // milliseconds as binary32, as hipEventElapsedTime hands them out
        const float ms = (float)((double)(long long)(ticks[stop] - ticks[start]) / c->stamp_khz);
        const float t0 = (float)((double)(long long)(ticks[start] - ticks[kStampOrigin]) / c->stamp_khz);
        resolved(c, stat, ms, c->stamp_origin, t0);
    });
}

// ---- the timestamp slots behind the scopes (scope_stamps.h) ---------------------------------------------------------
__global__ void k_scope_stamp(unsigned long long *slot) { *slot = wall_clock64(); }

void HipStampDev::stamp(uint32_t slot)
{
    hipLaunchKernelGGL(k_scope_stamp, dim3(1), dim3(1), 0, c->stream, buf + slot);
    (void)hipGetLastError();
}

// Nothing references a slot (StampBackend::grow) and the stream has been synchronised: only the origin's is kept.
bool HipStampDev::grow(uint32_t old_slots, uint32_t new_slots)
{
    unsigned long long *fresh = nullptr;
    if (dev_reserve(c, &fresh, (uint64_t)new_slots * sizeof(*fresh), 0, "native.scope_stamps") != hipSuccess) return false;
    if (old_slots && hipMemcpy(fresh, buf, sizeof(*fresh), hipMemcpyDeviceToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)dev_release(c, fresh);
        return false;
    }
    (void)dev_release(c, buf);
    buf = fresh;
    return true;
}

// Outside the step path: at least `need` slots can be handed out afterwards, if that can be had (StampBackend::make_room).
static void stamps_make_room(gpe_ctx *c, uint32_t need)
{
    auto &be = c->stamp_be;
    if (be.room(c->scope_stamps.pooled()) >= need) return;
    if (c->stamp_khz <= 0.0) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
        c->stamp_khz = (double)khz;
    }
    be.dev.c = c;
    be.make_room(c->scope_stamps, need, [c] {
        if (hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
        resolve_pending(c);
        return true;
    });
}

// ---- device memory: payload, slack, red zones ------------------------------------------
// The only place that calls the runtime's allocator.  Every allocation of a context is in c->guard.live.
constexpr uint32_t kGuardCanary = 0x3C3u, kGuardPoison = 0x2A5u;       // the defaults of gpe_config.guard_canary / guard_poison

struct GuardZoneDesc { uint64_t start, bytes; };                       // a red zone: device address, length
struct GuardZoneHit { unsigned long long first, last; };               // damaged bytes, relative to start (first = ~0: none)

// base[0, words): the canary, except the bytes [pay_lo, pay_hi) which get the poison (bytewise at the edges)
__global__ void k_guard_fill(uint32_t *base, uint64_t words, uint64_t pay_lo, uint64_t pay_hi, uint32_t canary,
                             uint32_t poison)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t b = 4 * w + k;
            v |= ((b >= pay_lo && b < pay_hi) ? poison : canary) & (0xFFu << (8 * k));
        }
        base[w] = v;
    }
}

// One workgroup per zone.  Reads the aligned words that cover the zone (all inside the allocation: its base is
// 256-byte aligned and its size a multiple of 16) and compares the zone's own bytes only.
__global__ void k_guard_check(const GuardZoneDesc *zones, GuardZoneHit *hits, uint32_t canary)
{
    const GuardZoneDesc z = zones[blockIdx.x];
    const uint64_t lo = z.start, hi = z.start + z.bytes;
    for (uint64_t a = (lo & ~3ull) + 4ull * threadIdx.x; a < hi; a += 4ull * blockDim.x) {
        uint32_t v = *(const uint32_t *)a ^ canary;
        for (uint32_t k = 0; k < 4; ++k)
            if (a + k < lo || a + k >= hi) v &= ~(0xFFu << (8 * k));   // the unaligned head / tail of a zone
        if (v == 0) continue;
        const uint64_t fb = (uint64_t)(__builtin_ctz(v) >> 3), lb = (uint64_t)((31 - __builtin_clz(v)) >> 3);
        atomicMin(&hits[blockIdx.x].first, (unsigned long long)(a + fb - lo));
        atomicMax(&hits[blockIdx.x].last, (unsigned long long)(a + lb - lo));
    }
}

static void guard_sync(gpe_ctx *c)
{
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->shard.xstream) (void)hipStreamSynchronize(c->shard.xstream);
}

// Compare the zones of list[0, count) with the canary; damaged ones are appended to out (up to GPE_GUARD_MAX_ZONES
// entries in all) and counted in *damaged.  Synchronises.
static hipError_t guard_scan(gpe_ctx *c, const DevAlloc *list, size_t count, std::vector<gpe_guard_zone> &out,
                             uint32_t *damaged)
{
    if (count == 0) return hipSuccess;
    std::vector<GuardZoneDesc> desc(2 * count);
    std::vector<GuardZoneHit> hit(2 * count);
    for (size_t i = 0; i < count; ++i) {
        const DevAlloc &a = list[i];
        const uint64_t base = (uint64_t)a.base, ptr = (uint64_t)a.ptr;
        desc[2 * i] = {base, ptr - base};
        desc[2 * i + 1] = {ptr + a.payload, base + a.total - (ptr + a.payload)};
        hit[2 * i] = hit[2 * i + 1] = {~0ull, 0ull};
    }
    const size_t desc_bytes = desc.size() * sizeof(GuardZoneDesc), hit_bytes = hit.size() * sizeof(GuardZoneHit);
    uint8_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, desc_bytes + hit_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    guard_sync(c);
    e = hipMemcpy(d, desc.data(), desc_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + desc_bytes, hit.data(), hit_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_guard_check, dim3((uint32_t)desc.size()), dim3(kStreamBlock), 0, c->stream,
                           (const GuardZoneDesc *)d, (GuardZoneHit *)(d + desc_bytes), c->guard.canary);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(hit.data(), d + desc_bytes, hit_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    for (size_t z = 0; z < hit.size(); ++z) {
        if (hit[z].first == ~0ull) continue;
        *damaged += 1;
        if (out.size() >= GPE_GUARD_MAX_ZONES) continue;
        const DevAlloc &a = list[z / 2];
        gpe_guard_zone g;
        memset(&g, 0, sizeof(g));
        strncpy(g.tag, a.tag, sizeof(g.tag) - 1);
        g.side = (z & 1) ? GPE_GUARD_REAR : GPE_GUARD_FRONT;
        const int64_t origin = (z & 1) ? 0 : -(int64_t)desc[z].bytes;  // front zone: relative to the payload's first byte
        g.first_offset = origin + (int64_t)hit[z].first;
        g.last_offset = origin + (int64_t)hit[z].last;
        g.payload_bytes = a.payload;
        (void)hipMemcpy(&g.first_word, (const void *)((desc[z].start + hit[z].first) & ~3ull), 4, hipMemcpyDeviceToHost);
        out.push_back(g);
    }
    return hipSuccess;
}

static std::string guard_zone_text(const gpe_guard_zone &g)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "guard: %s zone of \"%s\" (payload %llu B) damaged at bytes %lld..%lld, first word 0x%08x",
             g.side == GPE_GUARD_REAR ? "rear" : "front", g.tag, (unsigned long long)g.payload_bytes,
             (long long)g.first_offset, (long long)g.last_offset, g.first_word);
    return buf;
}

hipError_t gpe_dev_reserve(gpe_ctx *c, void **ptr, uint64_t payload_bytes, uint64_t slack_bytes, const char *tag)
{
    *ptr = nullptr;
    GuardState &G = c->guard;
    DevAlloc a;
    a.payload = payload_bytes; a.slack = slack_bytes; a.tag = tag;
    uint64_t front = 0;
    a.total = payload_bytes + slack_bytes;
    if (G.on) {
        front = kGuardZone;                                            // (a multiple of 256: the payload stays aligned)
        a.total = (front + payload_bytes + slack_bytes + kGuardZone + 15) & ~15ull;
    }
    hipError_t e = hipMalloc(&a.base, a.total);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }        // reported by the caller: not left for the next launch check
    a.ptr = (uint8_t *)a.base + front;
    if (G.on) {
        hipLaunchKernelGGL(k_guard_fill, dim3(stream_grid(a.total / 4)), dim3(kStreamBlock), 0, c->stream,
                           (uint32_t *)a.base, a.total / 4, front, front + payload_bytes, G.canary, G.poison);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the buffer may be used on another stream next)
        if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(a.base); return e; }
    }
    G.live.push_back(a);
    *ptr = a.ptr;
    return hipSuccess;
}

hipError_t gpe_dev_release(gpe_ctx *c, void **ptr)
{
    void *p = *ptr;
    *ptr = nullptr;
    if (!p) return hipSuccess;
    GuardState &G = c->guard;
    size_t i = G.live.size();
    while (i > 0 && G.live[i - 1].ptr != p) --i;                       // (the newest first: buffers are mostly replaced)
    if (i == 0) return G.on ? hipErrorInvalidValue : hipFree(p);       // not this context's: the caller's to free
    const DevAlloc a = G.live[i - 1];
    G.live.erase(G.live.begin() + (i - 1));
    if (G.on) {
        size_t k = 0;
        while (k < G.released.size() && strcmp(G.released[k].tag, a.tag) != 0) ++k;
        if (k == G.released.size()) G.released.push_back(a);
        G.released[k] = a;
        G.released[k].ptr = G.released[k].base = nullptr;
        // the zones go with the buffer: look at them now, and keep what they show for the next gpe_guard_check -- or
        // that they could not be looked at
        const hipError_t e = guard_scan(c, &a, 1, G.kept, &G.kept_count);
        if (e != hipSuccess && G.scan_failed == hipSuccess) G.scan_failed = e;
    }
    return hipFree(a.base);
}

// ---- the refusals several entry points word alike (gpe_internal.h) -----------------------------------------------
gpe_status refuse_sharded(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, order keys "
                                                            "or an active cell box)");
}

gpe_status refuse_holds(gpe_ctx *c, const char *who, const char *sets, const char *setter)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported while the context holds " + sets + " (" +
                                            setter + " with k = 0 clears them)");
}

// The sets that name their particles by uid, in the order of their passes behind a step (after_step).  refusal: the
// set's rank when a context that holds several is refused -- bonds, bodies, bends, areas: which text the caller sees
struct UidSet {
    const char *name, *setter;
    int refusal;
    bool (*has)(const gpe_ctx *);
    void (*release)(gpe_ctx *);
    gpe_status (*pass)(gpe_ctx *);
};
static const UidSet kUidSets[] = {
    {"bends", "gpe_set_bends", 2, has_bends, bends_release, bends_pass},
    {"areas", "gpe_set_areas", 3, has_areas, areas_release, areas_pass},
    {"bonds", "gpe_set_bonds", 0, has_bonds, bonds_release, bonds_pass},
    {"bodies", "gpe_set_bodies", 1, has_bodies, bodies_release, bodies_pass},
};

// GPE_ERR_UNSUPPORTED when the context holds one of them (taking the uids away, sharding)
static gpe_status refuse_uid_sets(gpe_ctx *c, const char *who)
{
    const UidSet *first = nullptr;
    for (const UidSet &s : kUidSets)
        if (s.has(c) && (!first || s.refusal < first->refusal)) first = &s;
    return first ? refuse_holds(c, who, first->name, first->setter) : GPE_OK;
}

gpe_status refuse_step_sets(gpe_ctx *c, const char *who, const char *uid_refusal)
{
    GPE_TRY(refuse_uid_sets(c, who));
    if (c->uid.on) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": " + uid_refusal);
    if (has_colliders(c)) return refuse_colliders(c, who);
    if (has_fields(c)) return refuse_fields(c, who);
    if (has_movers(c)) return refuse_movers(c, who);
    return GPE_OK;
}

gpe_status refuse_too_many(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
}

gpe_status refuse_uid_off(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_STATE, std::string(who) + ": uid requested while uids are off");
}

gpe_status refuse_radius_not_finite(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": the largest radius is not finite");
}

// ---- particle buffers --------------------------------------------------------------------------------------------
static void remove_release(gpe_ctx *c);            // below, each with its reserve functions
static void uid_release(gpe_ctx *c);

static void free_particle_buffers(gpe_ctx *c)
{
    dev_free(c, c->pos); dev_free(c, c->prev); dev_free(c, c->radius);
    dev_free(c, c->pos_copy); dev_free(c, c->prev_copy); dev_free(c, c->radius_copy);
    dev_free(c, c->home_cell_ids); dev_free(c, c->particle_ids);
    dev_free(c, c->cell_ids); dev_free(c, c->object_ids);
    dev_free(c, c->chunk_obj_count); dev_free(c, c->collision_cells); dev_free(c, c->indirect_args);
    dev_free(c, c->order_keys);
    remove_release(c); query_release(c); contacts_release(c); ray_release(c); nearest_release(c);
    clusters_release(c); edit_release(c); spawn_release(c);
    uid_release(c);
    c->cap = 0;
}

__global__ void k_fill_u32(uint32_t *p, uint64_t n, uint32_t v)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
__global__ void k_iota_u32(uint32_t *p, uint64_t lo, uint64_t hi)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride)
        p[i] = (uint32_t)i;
}

static gpe_status fill_u32(gpe_ctx *c, uint32_t *p, uint64_t n, uint32_t v)
{
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(k_fill_u32, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, p, n, v);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

static uint64_t total_cell_ids(const gpe_ctx *c) { return c->n * GPE_MAX_CELLS_PER_OBJECT; }
static uint64_t num_chunks(const gpe_ctx *c)
{
    return (total_cell_ids(c) + GPE_COUNTING_CHUNK_SIZE - 1) / GPE_COUNTING_CHUNK_SIZE;
}

// The reference's grid / collision-cell buffers (4 entries per particle: 52 B per particle) and the sort
// partners for 4N pairs (32 B per particle) are touched by the compat kernels only.  A COMPAT context allocates
// them with the particles; a NATIVE context when something first asks for them: a per-module entry point
// (gpe_grid_*, gpe_build_collision_cells, gpe_solve_collisions), array access, gpe_set_mode(COMPAT), or a step
// the native kernels hand over (particles outside the box, over-dense windows) -- the one place where that costs
// an allocation on the step path, once.  At 100 M particles that is 8.4 GB of 15 that stay unallocated.
static gpe_status alloc_grid_buffers(gpe_ctx *c, uint64_t cap)
{
    gpe_status st = dev_alloc(c, &c->cell_ids, cap * 4, "grid.cell_ids");
    if (st == GPE_OK) st = dev_alloc(c, &c->object_ids, cap * 4, "grid.object_ids");
    if (st == GPE_OK) st = dev_alloc(c, &c->chunk_obj_count, cap, "grid.chunk_obj_count");
    if (st == GPE_OK) st = dev_alloc(c, &c->collision_cells, cap * 4, "grid.collision_cells");
    if (st == GPE_OK) st = dev_alloc(c, &c->indirect_args, 4, "grid.indirect_args");
    if (st == GPE_OK) st = sort_reserve(c, cap * 4);
    if (st != GPE_OK) {
        dev_free(c, c->cell_ids); dev_free(c, c->object_ids); dev_free(c, c->chunk_obj_count);
        dev_free(c, c->collision_cells); dev_free(c, c->indirect_args);
    }
    return st;
}

// Allocate every particle-count-dependent buffer for `cap` particles (State::new, state.rs:34-70).
static gpe_status alloc_particle_buffers(gpe_ctx *c, uint64_t cap, bool with_grid)
{
    GPE_TRY(dev_alloc(c, &c->pos, cap, "particles.pos"));
    GPE_TRY(dev_alloc(c, &c->prev, cap, "particles.prev"));
    GPE_TRY(dev_alloc(c, &c->radius, cap, "particles.radius"));
    GPE_TRY(dev_alloc(c, &c->pos_copy, cap, "particles.pos_copy"));
    GPE_TRY(dev_alloc(c, &c->prev_copy, cap, "particles.prev_copy"));
    GPE_TRY(dev_alloc(c, &c->radius_copy, cap, "particles.radius_copy"));
    GPE_TRY(dev_alloc(c, &c->home_cell_ids, cap, "particles.home_cell_ids"));
    GPE_TRY(dev_alloc(c, &c->particle_ids, cap, "particles.particle_ids"));
    GPE_TRY(dev_alloc(c, &c->order_keys, cap, "particles.order_keys"));
    if (c->uid.on) {
        GPE_TRY(dev_alloc(c, &c->uid.uids, cap, "uid.uids"));
        GPE_TRY(dev_alloc(c, &c->uid.uids_copy, cap, "uid.uids_copy"));
    }
    c->cap = cap;
    if (with_grid) GPE_TRY(alloc_grid_buffers(c, cap));
    else GPE_TRY(sort_reserve(c, cap));                                // the Morton re-sort's N pairs
    GPE_TRY(scan_reserve(c, cap));
    return GPE_OK;
}

// Initial values of the index buffers for particles [lo, hi).
gpe_status init_index_buffers(gpe_ctx *c, uint64_t lo, uint64_t hi)
{
    if (hi <= lo) return GPE_OK;
    const uint64_t cnt = hi - lo;
    GPE_TRY(fill_u32(c, c->home_cell_ids + lo, cnt, kUnused));              // particle_system.rs:130-133
    hipLaunchKernelGGL(k_iota_u32, dim3(stream_grid(cnt)), dim3(kStreamBlock), 0, c->stream,
                       c->particle_ids, lo, hi);                            // particle_sort.rs:30
    GPE_HIP(c, hipGetLastError());
    if (!c->cell_ids) return GPE_OK;                                        // not allocated yet: need_grid_buffers
    GPE_TRY(fill_u32(c, c->cell_ids + 4 * lo, 4 * cnt, kUnused));           // grid.rs:80-83
    GPE_TRY(fill_u32(c, c->object_ids + 4 * lo, 4 * cnt, 0u));              // grid.rs:85-89
    GPE_TRY(fill_u32(c, c->collision_cells + 4 * lo, 4 * cnt, kUnused));    // collision_cell_buffers.rs:23-27
    GPE_TRY(fill_u32(c, c->chunk_obj_count + lo, cnt, 0u));                 // collision_cell_buffers.rs:17-21
    return GPE_OK;
}

// Every user of the grid / collision-cell buffers calls this first (see alloc_grid_buffers).
static gpe_status need_grid_buffers(gpe_ctx *c)
{
    if (c->cell_ids || c->cap == 0) return GPE_OK;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(alloc_grid_buffers(c, c->cap));
    const uint64_t cnt = c->n;
    GPE_TRY(fill_u32(c, c->cell_ids, 4 * cnt, kUnused));
    GPE_TRY(fill_u32(c, c->object_ids, 4 * cnt, 0u));
    GPE_TRY(fill_u32(c, c->collision_cells, 4 * cnt, kUnused));
    GPE_TRY(fill_u32(c, c->chunk_obj_count, cnt, 0u));
    return GPE_OK;
}

// Reallocate every particle-count-dependent buffer for `cap` particles, keeping the contents of the
// first c->n (GpuBuffer::push grows x2 with a device copy, utils/gpu_buffer.rs:49-87).  Synchronises.
// Transactional: the new set is allocated beside the old one and takes its place only when every allocation and
// copy has succeeded; on failure the new set is freed and the context is exactly as before.
struct ParticleBufferSet {
    float2 *pos = nullptr, *prev = nullptr, *pos_copy = nullptr, *prev_copy = nullptr;
    float *radius = nullptr, *radius_copy = nullptr;
    uint32_t *home_cell_ids = nullptr, *particle_ids = nullptr, *cell_ids = nullptr, *object_ids = nullptr,
             *chunk_obj_count = nullptr, *collision_cells = nullptr, *indirect_args = nullptr, *order_keys = nullptr;
    uint32_t *uids = nullptr, *uids_copy = nullptr;
    uint64_t cap = 0;
};
static ParticleBufferSet take_buffers(gpe_ctx *c)
{
    ParticleBufferSet b;
    b.pos = c->pos; b.prev = c->prev; b.pos_copy = c->pos_copy; b.prev_copy = c->prev_copy;
    b.radius = c->radius; b.radius_copy = c->radius_copy;
    b.home_cell_ids = c->home_cell_ids; b.particle_ids = c->particle_ids; b.cell_ids = c->cell_ids;
    b.object_ids = c->object_ids; b.chunk_obj_count = c->chunk_obj_count; b.collision_cells = c->collision_cells;
    b.indirect_args = c->indirect_args; b.order_keys = c->order_keys;
    b.uids = c->uid.uids; b.uids_copy = c->uid.uids_copy;
    b.cap = c->cap;
    c->pos = c->prev = c->pos_copy = c->prev_copy = nullptr;
    c->radius = c->radius_copy = nullptr;
    c->home_cell_ids = c->particle_ids = c->cell_ids = c->object_ids = nullptr;
    c->chunk_obj_count = c->collision_cells = c->indirect_args = c->order_keys = nullptr;
    c->uid.uids = c->uid.uids_copy = nullptr;
    c->cap = 0;
    return b;
}
static void put_buffers(gpe_ctx *c, const ParticleBufferSet &b)
{
    c->pos = b.pos; c->prev = b.prev; c->pos_copy = b.pos_copy; c->prev_copy = b.prev_copy;
    c->radius = b.radius; c->radius_copy = b.radius_copy;
    c->home_cell_ids = b.home_cell_ids; c->particle_ids = b.particle_ids; c->cell_ids = b.cell_ids;
    c->object_ids = b.object_ids; c->chunk_obj_count = b.chunk_obj_count; c->collision_cells = b.collision_cells;
    c->indirect_args = b.indirect_args; c->order_keys = b.order_keys;
    c->uid.uids = b.uids; c->uid.uids_copy = b.uids_copy;
    c->cap = b.cap;
}

static gpe_status copy_into_new_buffers(gpe_ctx *c, const ParticleBufferSet &old, uint64_t old_n)
{
    if (!old.pos || old_n == 0) return GPE_OK;
#define GPE_COPY_OLD(field, count)                                                                     \
    GPE_HIP(c, hipMemcpyAsync(c->field, old.field, (count) * sizeof(*c->field), hipMemcpyDeviceToDevice, c->stream))
    GPE_COPY_OLD(pos, old_n); GPE_COPY_OLD(prev, old_n); GPE_COPY_OLD(radius, old_n);
    GPE_COPY_OLD(home_cell_ids, old_n); GPE_COPY_OLD(particle_ids, old_n);
    if (old.cell_ids) {
        GPE_COPY_OLD(cell_ids, 4 * old_n); GPE_COPY_OLD(object_ids, 4 * old_n);
        GPE_COPY_OLD(chunk_obj_count, old_n); GPE_COPY_OLD(collision_cells, 4 * old_n);
        GPE_COPY_OLD(indirect_args, 3);
    }
    if (old.order_keys) GPE_COPY_OLD(order_keys, old_n);
#undef GPE_COPY_OLD
    if (old.uids && c->uid.uids)
        GPE_HIP(c, hipMemcpyAsync(c->uid.uids, old.uids, old_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return GPE_OK;
}

gpe_status grow_particle_buffers(gpe_ctx *c, uint64_t cap)
{
    const uint64_t old_n = c->n;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    const ParticleBufferSet old = take_buffers(c);                     // the context now holds no particle buffer
    gpe_status st = alloc_particle_buffers(c, cap, old.cell_ids != nullptr || c->cfg.mode != GPE_MODE_NATIVE);
    if (st == GPE_OK) st = copy_into_new_buffers(c, old, old_n);
    if (st != GPE_OK) {
        const std::string why = c->last_error;
        free_particle_buffers(c);                                      // whatever part of the new set exists
        put_buffers(c, old);                                           // the context is as it was
        c->last_error = why;
        return st;
    }
    float2 *f2[] = {old.pos, old.prev, old.pos_copy, old.prev_copy};
    for (float2 *p : f2) dev_free(c, p);
    float *f1[] = {old.radius, old.radius_copy};
    for (float *p : f1) dev_free(c, p);
    uint32_t *u[] = {old.home_cell_ids, old.particle_ids, old.cell_ids, old.object_ids, old.chunk_obj_count,
                     old.collision_cells, old.indirect_args, old.order_keys, old.uids, old.uids_copy};
    for (uint32_t *p : u) dev_free(c, p);
    return GPE_OK;
}

static float max_abs_radius(const float *radius, uint64_t n, float start)
{
    // particle_system.rs:51: the radius of largest magnitude (the element itself, sign kept; of several elements
    // of that magnitude the last one -- Rust's max_by -- which decides the sign of cell_size for radii like [2, -2])
    float best = start;
    for (uint64_t i = 0; i < n; ++i)
        if (!(fabsf(radius[i]) < fabsf(best))) best = radius[i];      // ties: the LAST element, as Iterator::max_by returns
    return best;
}

void refresh_cell_size(gpe_ctx *c)
{
    c->cell_size = c->grid_max_radius * c->cfg.cell_size_multiplier;        // grid.rs:159-161
}

gpe_status need_particles(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (c->n == 0 || !c->pos) return fail(c, GPE_ERR_STATE, "no particles: call gpe_set_particles first");
    return GPE_OK;
}

// ---- removal (k_remove.hip) ---------------------------------------------------------------------------
static gpe_status check_removable(gpe_ctx *c, const char *who)
{
    GPE_TRY(need_particles(c));
    if (is_sharded(c)) return refuse_sharded(c, who);
    return GPE_OK;
}

static gpe_status remove_reserve(gpe_ctx *c, uint64_t mask_bytes)
{
    RemoveWorkspace &ws = c->remove_ws;
    const uint64_t tiles = remove_tiles(c->n);
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_count);
        dev_free(c, ws.tile_key);
        ws.tiles_cap = 0;
        GPE_TRY(dev_alloc(c, &ws.tile_count, tiles, "remove.tile_count"));
        GPE_TRY(dev_alloc(c, &ws.tile_key, tiles, "remove.tile_key"));
        ws.tiles_cap = tiles;
    }
    if (!ws.max_key) GPE_TRY(dev_alloc(c, &ws.max_key, 1, "remove.max_key"));
    if (ws.mask_cap < mask_bytes) {
        const uint64_t want = std::max(c->cap, mask_bytes);             // (a later call on fewer particles fits)
        dev_free(c, ws.mask);
        ws.mask_cap = 0;
        GPE_TRY(dev_alloc(c, &ws.mask, want, "remove.mask"));
        ws.mask_cap = want;
    }
    return scan_reserve(c, tiles);
}

static void remove_release(gpe_ctx *c)
{
    RemoveWorkspace &ws = c->remove_ws;
    dev_free(c, ws.tile_count); dev_free(c, ws.tile_key); dev_free(c, ws.max_key); dev_free(c, ws.mask);
    ws.tiles_cap = ws.mask_cap = 0;
}

// Stable compaction of the particles that survive `mask` (device bytes, != 0: removed) or, mask == NULL, the disc
// around (x, y) with rr = radius^2.  Counts first: removing nothing or everything leaves the context untouched.
// Afterwards the context is what gpe_set_particles(survivors) leaves on it.
static gpe_status do_remove(gpe_ctx *c, const uint8_t *mask, float x, float y, float rr, uint64_t *n_removed)
{
    RemoveWorkspace &ws = c->remove_ws;
    const uint64_t n = c->n, tiles = remove_tiles(n);
    uint32_t survivors = 0;
    unsigned long long key = 0;
    Scope s(c, "Remove particles");
    {
        Scope k(c, "remove/count");
        GPE_TRY(launch_remove_count(c, mask, x, y, rr, ws.tile_count, ws.tile_key, ws.max_key));
    }
    {
        Scope k(c, "remove/scan");
        GPE_TRY(inclusive_scan(c, ws.tile_count, tiles));
    }
    GPE_HIP(c, hipMemcpyAsync(&survivors, ws.tile_count + (tiles - 1), sizeof(survivors), hipMemcpyDeviceToHost,
                              c->stream));
    GPE_HIP(c, hipMemcpyAsync(&key, ws.max_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (survivors == n) return GPE_OK;                                   // nothing removed: the context is untouched
    if (survivors == 0)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles: the call would remove every particle");
    const uint32_t winner = (uint32_t)(key & 0xFFFFFFFFull);           // old index of the survivors' max |radius|
    if (winner >= n) return fail(c, GPE_ERR_STATE, "gpe_remove_particles: bad max-radius index");
    float max_r = 0.f;
    GPE_HIP(c, hipMemcpyAsync(&max_r, c->radius + winner, sizeof(max_r), hipMemcpyDeviceToHost, c->stream));
    {
        Scope k(c, "remove/scatter");
        GPE_TRY(launch_remove_scatter(c, mask, x, y, rr, ws.tile_count, c->uid.uids, c->uid.uids_copy));
    }
    std::swap(c->pos, c->pos_copy);                                     // as do_resort
    std::swap(c->prev, c->prev_copy);
    std::swap(c->radius, c->radius_copy);
    if (c->uid.on) {
        std::swap(c->uid.uids, c->uid.uids_copy);
        c->uid.map_valid = false;
        uid_slots_stale(c);
    }
    c->n = survivors;
    c->n_owned = survivors;
    {
        Scope k(c, "remove/index reset");
        GPE_TRY(init_index_buffers(c, 0, survivors));
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    c->max_radius = max_r;                    // max_abs_radius over the survivors: largest |r|, last on ties, sign kept
    c->grid_max_radius = c->max_radius;
    refresh_cell_size(c);
    if (n_removed) *n_removed = n - survivors;
    return reconfigure_native(c);
}

// ---- uids (k_uids.hip) ----------------------------------------------------------------------------------
// Off -> on: the uid buffers for the current capacity (none yet without particles).
static gpe_status uids_switch_on(gpe_ctx *c)
{
    UidState &u = c->uid;
    if (c->cap > 0) {
        gpe_status st = dev_alloc(c, &u.uids, c->cap, "uid.uids");
        if (st == GPE_OK) st = dev_alloc(c, &u.uids_copy, c->cap, "uid.uids_copy");
        if (st != GPE_OK) {
            uid_release(c);
            return st;
        }
    }
    u.on = true;
    u.map_valid = false;
    uid_slots_stale(c);
    return GPE_OK;
}

// The map of the c->n >= 1 uids at src (the live ones, or those gpe_set_uids staged): (uid, index) pairs sorted by
// uid, *dup = some uid occurs twice, map_max = the last key.  Synchronises.  Leaves map_valid to the caller.
static gpe_status uid_map_build(gpe_ctx *c, const uint32_t *src, bool *dup)
{
    UidState &u = c->uid;
    const uint64_t n = c->n;
    u.map_valid = false;
    if (u.map_cap < n) {
        dev_free(c, u.map_keys);
        dev_free(c, u.map_vals);
        u.map_cap = 0;
        const uint64_t want = std::max(c->cap, n);
        GPE_TRY(dev_alloc(c, &u.map_keys, want, "uid.map_keys"));
        GPE_TRY(dev_alloc(c, &u.map_vals, want, "uid.map_vals"));
        u.map_cap = want;
    }
    if (!u.dup) GPE_TRY(dev_alloc(c, &u.dup, 1, "uid.dup"));
    GPE_TRY(sort_reserve(c, n));
    {
        Scope s(c, "uids/map");
        GPE_TRY(launch_uid_map_init(c, src, n, u.map_keys, u.map_vals));
        GPE_TRY(sort_pairs(c, u.map_keys, u.map_vals, n));
        GPE_HIP(c, hipMemsetAsync(u.dup, 0, sizeof(uint32_t), c->stream));
        GPE_TRY(launch_uid_adjacent(c, u.map_keys, n, u.dup));
    }
    uint32_t words[2] = {0, 0};
    GPE_HIP(c, hipMemcpyAsync(&words[0], u.dup, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipMemcpyAsync(&words[1], u.map_keys + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    *dup = words[0] != 0;
    u.map_max = words[1];
    return GPE_OK;
}

// The live uids' map, rebuilt only when something has made it stale.  Needs c->n >= 1.
gpe_status uid_map_ready(gpe_ctx *c)
{
    if (c->uid.map_valid) return GPE_OK;
    bool dup = false;
    GPE_TRY(uid_map_build(c, c->uid.uids, &dup));
    if (dup) return fail(c, GPE_ERR_STATE, "uids: two particles share a uid");
    c->uid.map_valid = true;
    return GPE_OK;
}

gpe_status uid_query_reserve(gpe_ctx *c, uint64_t bytes)
{
    UidState &u = c->uid;
    if (u.query_cap >= bytes) return GPE_OK;
    dev_free(c, u.query);
    u.query_cap = 0;
    GPE_TRY(dev_alloc(c, &u.query, bytes, "uid.query"));
    u.query_cap = bytes;
    return GPE_OK;
}

// The uid buffers, the uid -> index map and the lookup staging (the uid switch itself stays as it is).
static void uid_release(gpe_ctx *c)
{
    UidState &u = c->uid;
    dev_free(c, u.uids); dev_free(c, u.uids_copy);
    dev_free(c, u.map_keys); dev_free(c, u.map_vals); dev_free(c, u.dup); dev_free(c, u.query);
    u.map_cap = u.query_cap = 0;
    u.map_valid = false;
    uid_slots_stale(c);
}

// ---- step pieces ------------------------------------------------------------------------------------
static gpe_status do_resort(gpe_ctx *c)
{
    // particle_sort.rs:58-69
    GPE_TRY(launch_home_cell_ids(c, c->pos, c->n, c->cell_size, c->home_cell_ids, c->particle_ids));
    {
        Scope s(c, "Particle sort");   // particle_sort.rs:64
        GPE_TRY(sort_pairs(c, c->home_cell_ids, c->particle_ids, c->n));
    }
    if (c->uid.on) {                   // the uids follow the same permutation (k_uids.hip)
        GPE_TRY(launch_rearrange_uids(c, c->pos, c->prev, c->radius, c->uid.uids, c->particle_ids, c->n, c->pos_copy,
                                      c->prev_copy, c->radius_copy, c->uid.uids_copy));
        std::swap(c->uid.uids, c->uid.uids_copy);
        c->uid.map_valid = false;
        uid_slots_stale(c);
    } else {
        GPE_TRY(launch_rearrange(c, c->pos, c->prev, c->radius, c->particle_ids, c->n, c->pos_copy,
                                 c->prev_copy, c->radius_copy));
    }
    // particle_rearrange.rs:205-238 copies the copy set back; swapping the two sets is equivalent
    std::swap(c->pos, c->pos_copy);
    std::swap(c->prev, c->prev_copy);
    std::swap(c->radius, c->radius_copy);
    return GPE_OK;
}

static gpe_status do_grid_sort(gpe_ctx *c)
{
    GPE_TRY(need_grid_buffers(c));
    Scope s(c, "Sort map");   // grid.rs:329
    return sort_pairs(c, c->cell_ids, c->object_ids, total_cell_ids(c));
}

static gpe_status do_build_collision_cells(gpe_ctx *c)
{
    // collision_cell_builder.rs:211-236
    GPE_TRY(need_grid_buffers(c));
    GPE_TRY(launch_count_chunks(c, c->cell_ids, total_cell_ids(c), c->chunk_obj_count));
    {
        Scope s(c, "Collision cell prefix sum");   // collision_cell_builder.rs:227
        GPE_TRY(inclusive_scan(c, c->chunk_obj_count, num_chunks(c)));
    }
    GPE_TRY(launch_build_collision_cells(c, c->cell_ids, total_cell_ids(c), c->chunk_obj_count,
                                         num_chunks(c), c->collision_cells, c->indirect_args));
    return GPE_OK;
}

static gpe_status do_solve_colors(gpe_ctx *c)
{
    GPE_TRY(need_grid_buffers(c));
    for (uint32_t color = 1; color <= 4; ++color)   // collision_solver.rs:224
        GPE_TRY(launch_solve_color(c, c->collision_cells, c->chunk_obj_count, num_chunks(c), c->cell_ids,
                                   c->object_ids, total_cell_ids(c), c->pos, c->radius, c->cfg.stiffness,
                                   color));
    return GPE_OK;
}

static gpe_status do_step_scoped(gpe_ctx *c, float dt, uint32_t flags)
{
    // state.rs:115-131
    if (flags & GPE_STEP_RESORT) GPE_TRY(do_resort(c));                          // :122-125
    const bool native = native_should_run(c);
    if (c->use_order_keys && !native)
        return fail(c, GPE_ERR_UNSUPPORTED,
                    "order keys (sharded run) need the native pipeline: mode NATIVE, particles inside the world "
                    "box, bounded density");
    (native ? c->native.native_steps : c->native.compat_steps) += 1;
    if (native) {
        // grid update + collision solve as N-key sort + LDS cell windows (gpe_native.hip, k_native.hip); the resolved
        // positions land in the scratch set, which then becomes the live one.  The integration (:130) is
        // applied as the tiles write their particles back -- same arithmetic, one pass over memory less.
        const VerletParams vp = verlet_params(c, dt);
        GPE_TRY(native_collide(c, c->pos, c->pos_copy, &vp));
        std::swap(c->pos, c->pos_copy);
        return GPE_OK;
    }
    GPE_TRY(need_grid_buffers(c));
    GPE_TRY(launch_build_cell_ids(c, c->pos, c->radius, c->n, c->cell_size, c->cell_ids,
                                  c->object_ids));                               // :126 Grid::update
    GPE_TRY(do_grid_sort(c));
    GPE_TRY(do_build_collision_cells(c));                                        // :127
    GPE_TRY(do_solve_colors(c));
    GPE_TRY(launch_verlet(c, c->pos, c->prev, c->radius, c->n_owned, dt));       // :130
    return GPE_OK;
}

// Sampled profiling (gpe_set_profiling(ctx, k > 1)): only every k-th step records its scopes -- an event pair
// per kernel costs more than some of the kernels at small particle counts.
static gpe_status do_step(gpe_ctx *c, float dt, uint32_t flags)
{
    if (c->profile_every > 1) c->profiling = (c->profile_step++ % c->profile_every) == 0;
    if (c->profiling && scope_uses_stamps(c)) stamps_make_room(c, 64);      // (more slots than a step's scopes take)
    const gpe_status st = do_step_scoped(c, dt, flags);
    if (c->profile_every > 1) c->profiling = true;
    return st;
}

// Device-side error words (sticky): reported at the synchronising entry points.  The three copies go to pinned words
// and are enqueued behind the context's work, so the one wait for the stream is also the wait for them.
// wait_exchange (gpe_sync alone, as before): the exchange stream of a sharded run is waited for first -- whatever it was
// given has then run, whatever of the context's stream it waited for included, and the copies behind the context's
// stream see what either of them wrote.  Where that wait fails, the context's own stream is asked first, as it used to
// be, so that a failure of both is reported as the same call's.
gpe_status check_device_errors(gpe_ctx *c, bool wait_exchange)
{
    GPE_TRY(error_words_reserve(c));
    uint32_t *words = c->err_words;
    words[0] = words[1] = words[2] = 0u;
    if (wait_exchange && c->shard.xstream && hipStreamSynchronize(c->shard.xstream) != hipSuccess) {
        (void)hipGetLastError();
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->shard.xstream));
    }
    if (c->shard.counts)
        GPE_HIP(c, hipMemcpyAsync(&words[2], c->shard.counts + kShardError, 4, hipMemcpyDeviceToHost, c->stream));
    if (c->native.tile_ctl)
        GPE_HIP(c, hipMemcpyAsync(&words[0], c->native.tile_ctl + 8, 4, hipMemcpyDeviceToHost, c->stream));
    if (c->os_ws.ctl)
        GPE_HIP(c, hipMemcpyAsync(&words[1], c->os_ws.ctl + 4, 4, hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (words[1]) return fail(c, GPE_ERR_HIP, "radix sort: decoupled look-back timed out");
    if (words[0] & 2u)
        return fail(c, GPE_ERR_UNSUPPORTED,
                    "native collide: a region of 24x24 cells holds more particles than the LDS cell window "
                    "takes; results of that step are unresolved there -- use GPE_MODE_COMPAT for this scene");
    if (words[0] & 5u)
        return fail(c, GPE_ERR_STATE, "native collide: a particle left the world box between steps");
    if (words[0] & 16u)
        return fail(c, GPE_ERR_STATE, "sharded run: the device-side particle count passed the host's bound");
    if (words[2])
        return fail(c, GPE_ERR_UNSUPPORTED, shard_error_text(words[2]));
    return GPE_OK;
}

// (Re)derive the native pipeline's cell box after anything it depends on changed.
gpe_status reconfigure(gpe_ctx *c)
{
    if (c->cfg.mode == GPE_MODE_NATIVE && c->n > 0) return native_configure(c);
    c->native.policy.eligible = false;
    return GPE_OK;
}

gpe_status reconfigure_native(gpe_ctx *c) { return reconfigure(c); }

gpe_status step_for_shard(gpe_ctx *c, float dt) { return do_step(c, dt, 0u); }
gpe_status resort_for_shard(gpe_ctx *c) { return do_resort(c); }
gpe_status grow_for_shard(gpe_ctx *c, uint64_t capacity) { return grow_particle_buffers(c, capacity); }

}  // namespace gpe

using namespace gpe;

// =====================================================================================================
// extern "C"
// =====================================================================================================
extern "C" {

uint32_t gpe_abi_version(void) { return GPE_ABI_VERSION; }

gpe_status gpe_config_default(gpe_config *cfg)
{
    if (!cfg) return GPE_ERR_INVALID_ARG;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(gpe_config);
    cfg->device = -1;
    cfg->world_width = 3048.0f;          // state.rs:35
    cfg->world_height = 1048.0f;
    cfg->gravity_x = 0.0f;               // particle_integration.wgsl:21
    cfg->gravity_y = 0.0f;
    cfg->cell_size_multiplier = 2.2f;    // grid.rs:20
    cfg->stiffness = 0.6f;               // collision_solver.wgsl:2
    cfg->mouse_strength = 150.0f;        // particle_integration.wgsl:22
    cfg->mode = GPE_MODE_NATIVE;         // (falls back to the COMPAT kernels by itself: gpe_get_pipeline_info)
    cfg->profiling = 0;
    cfg->flags = 0;
    return GPE_OK;
}

const char *gpe_last_error(const gpe_ctx *ctx)
{
    if (ctx) return ctx->last_error.c_str();
    std::lock_guard<std::mutex> lk(g_err_mu);
    static thread_local std::string copy;
    copy = g_last_error;
    return copy.c_str();
}

gpe_status gpe_create(const gpe_config *cfg, gpe_ctx **out)
{
    if (!out) return fail(nullptr, GPE_ERR_INVALID_ARG, "gpe_create: out is NULL");
    *out = nullptr;
    gpe_config local;
    gpe_config_default(&local);
    if (cfg) {
        if (cfg->struct_size == 0 || cfg->struct_size > sizeof(gpe_config))
            return fail(nullptr, GPE_ERR_INVALID_ARG, "gpe_create: bad gpe_config.struct_size");
        memcpy(&local, cfg, cfg->struct_size);
        local.struct_size = (uint32_t)sizeof(gpe_config);
    }
    if (local.mode != GPE_MODE_COMPAT && local.mode != GPE_MODE_NATIVE)
        return fail(nullptr, GPE_ERR_INVALID_ARG, "gpe_create: unknown mode");
    if (local.flags & GPE_FLAG_GUARD_ALLOCS) {
        // (without the flag the two words are not looked at, as when they were reserved)
        // nonzero, a nonzero finite f32 (a denormal), and as an index of 16-byte elements inside a 16 KiB zone
        const uint32_t ca = local.guard_canary ? local.guard_canary : kGuardCanary;
        const uint32_t po = local.guard_poison ? local.guard_poison : kGuardPoison;
        if (ca >= kGuardZone / 16 || po >= kGuardZone / 16 || ca == po)
            return fail(nullptr, GPE_ERR_INVALID_ARG, "gpe_create: guard_canary / guard_poison must be in [1, 1023] and differ");
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, GPE_ERR_NO_DEVICE,
                    "gpe_create: no HIP device visible (this library has no CPU fallback)");
    int dev = local.device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= count) return fail(nullptr, GPE_ERR_INVALID_ARG, "gpe_create: device ordinal out of range");
    gpe_ctx *c = new (std::nothrow) gpe_ctx();
    if (!c) return fail(nullptr, GPE_ERR_OOM, "gpe_create: host allocation failed");
    c->cfg = local;
    c->device = dev;
    c->profiling = local.profiling != 0;
    c->profile_every = local.profiling;
    c->use_onesweep = (local.flags & GPE_FLAG_SAFE_SORT) == 0;
    c->guard.on = (local.flags & GPE_FLAG_GUARD_ALLOCS) != 0;
    c->guard.canary = local.guard_canary ? local.guard_canary : kGuardCanary;
    c->guard.poison = local.guard_poison ? local.guard_poison : kGuardPoison;
    if ((e = hipSetDevice(dev)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        std::string m = std::string("gpe_create: ") + hipGetErrorName(e);
        delete c;
        return fail(nullptr, GPE_ERR_HIP, m);
    }
    c->stream = c->own_stream;
    *out = c;
    return GPE_OK;
}

gpe_status gpe_destroy(gpe_ctx *c)
{
    if (!c) return GPE_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    resolve_pending(c);
    {
        HipScopeBackend be{c->stream};
        c->scope_events.destroy_all(be);
    }
    {
        StampRecorder<HipStampDev> be{c->stamp_be};
        c->scope_stamps.destroy_all(be);
    }
    (void)dev_release(c, c->stamp_be.dev.buf);
    if (c->trace_origin) (void)hipEventDestroy(c->trace_origin);
    error_words_release(c);
    free_particle_buffers(c);
    observers_release(c);
    colliders_release(c);
    sweep_release(c);
    for (const UidSet &s : kUidSets) s.release(c);
    fields_release(c);
    movers_release(c);
    mover_sweep_release(c);
    sort_release(c);
    scan_release(c);
    onesweep_release(c);
    native_release(c);
    group_leave(c);
    ctl_release(c);
    comm_release(c);
    shard_release(c);
    // a stream lent by gpe_set_stream belongs to the caller (a host framework may still hold buffers and
    // events that name it): only the library's own stream is destroyed
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return GPE_OK;
}

gpe_status gpe_sync(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    return check_device_errors(c, true);               // (one wait per stream, the error words' copies behind the work)
}

gpe_status gpe_get_pipeline_info(gpe_ctx *c, gpe_pipeline_info *info)
{
    if (!c || !info) return GPE_ERR_INVALID_ARG;
    if (info->struct_size == 0 || info->struct_size > sizeof(gpe_pipeline_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_pipeline_info: bad struct_size");
    gpe_pipeline_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    const NativeState &N = c->native;
    if (c->cfg.mode != GPE_MODE_NATIVE) { out.pipeline = GPE_PIPELINE_COMPAT; out.reason = GPE_REASON_MODE_COMPAT; }
    else if (c->n == 0) { out.pipeline = GPE_PIPELINE_COMPAT; out.reason = GPE_REASON_NO_PARTICLES; }
    else if (N.policy.eligible || ((N.force || c->use_order_keys) && N.in_box)) { out.pipeline = GPE_PIPELINE_NATIVE; out.reason = GPE_REASON_NONE; }
    else { out.pipeline = GPE_PIPELINE_COMPAT; out.reason = N.reason; }
    out.sort_passes = (uint32_t)N.passes;
    out.native_steps = N.native_steps;
    out.compat_steps = N.compat_steps;
    if (N.host_stat) {
        const NativeStats s = native_read_stats(N);
        out.window_max = s.window_max;
        out.arena_slots = s.arena; out.overflow_tiles = s.overflow;
        out.overflow_subtiles = s.sub_tiles; out.overflow_spills = s.spills;
    }
    out.uniform_radius = (out.pipeline == GPE_PIPELINE_NATIVE && N.uniform) ? 1u : 0u;
    if (N.tile_ctl) {
        uint32_t sorts = 0, seen = 0;
        GPE_HIP(c, hipMemcpyAsync(&sorts, N.tile_ctl + kNativeCtlSorts, sizeof(sorts), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipMemcpyAsync(&seen, N.tile_ctl + kNativeCtlSortsSeen, sizeof(seen), hipMemcpyDeviceToHost, c->stream));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        out.native_sorts = sorts;
        out.roster_stamp = seen;
    }
    memcpy(info, &out, info->struct_size);
    return GPE_OK;
}

gpe_status gpe_set_mode(gpe_ctx *c, uint32_t mode)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (mode != GPE_MODE_COMPAT && mode != GPE_MODE_NATIVE) return fail(c, GPE_ERR_INVALID_ARG, "unknown mode");
    c->cfg.mode = mode;
    if (mode == GPE_MODE_COMPAT) GPE_TRY(need_grid_buffers(c));
    return reconfigure(c);
}

// ---- particles -----------------------------------------------------------------------------------------
gpe_status gpe_set_particles(gpe_ctx *c, const float *pos_xy, const float *prev_xy, const float *radius,
                             uint64_t n)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!pos_xy || !radius || n == 0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_particles: NULL array or n == 0");
    if (n > (1ull << 30) - 1) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_particles: 4n must fit in u32");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (n > c->cap) {
        free_particle_buffers(c);
        gpe_status s = alloc_particle_buffers(c, n, c->cfg.mode != GPE_MODE_NATIVE);
        if (s != GPE_OK) { free_particle_buffers(c); c->n = 0; return s; }
    }
    c->n = n;
    c->n_owned = n;
    GPE_HIP(c, hipMemcpyAsync(c->pos, pos_xy, n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    GPE_HIP(c, hipMemcpyAsync(c->prev, prev_xy ? prev_xy : pos_xy, n * sizeof(float2), hipMemcpyHostToDevice,
                              c->stream));
    GPE_HIP(c, hipMemcpyAsync(c->radius, radius, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    GPE_TRY(init_index_buffers(c, 0, n));
    if (c->uid.on) {                                   // as gpe_enable_uids: uid = storage index
        GPE_TRY(launch_uid_iota(c, c->uid.uids, 0, n, 0u));
        c->uid.next = n;
        c->uid.map_valid = false;
        uid_slots_stale(c);
    }
    c->max_radius = max_abs_radius(radius, n, radius[0]);
    c->grid_max_radius = c->max_radius;       // Grid::new (grid.rs:66-71)
    refresh_cell_size(c);
    GPE_HIP(c, hipStreamSynchronize(c->stream));   // the host arrays may be released on return
    return reconfigure(c);
}

gpe_status gpe_add_particles(gpe_ctx *c, const float *pos_xy, const float *radius, uint64_t n_add)
{
    GPE_TRY(need_particles(c));
    if (!pos_xy || !radius) return fail(c, GPE_ERR_INVALID_ARG, "gpe_add_particles: NULL array");
    if (n_add == 0) return GPE_OK;
    const uint64_t old_n = c->n, new_n = c->n + n_add;
    if (new_n > (1ull << 30) - 1) return fail(c, GPE_ERR_INVALID_ARG, "gpe_add_particles: 4n must fit in u32");
    if (c->uid.on && c->uid.next + n_add > kUidLimit)
        return fail(c, GPE_ERR_STATE, "gpe_add_particles: the new particles' uids would pass 2^32 - 1");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (new_n > c->cap) GPE_TRY(grow_particle_buffers(c, std::max<uint64_t>(new_n, c->cap * 2)));
    GPE_HIP(c, hipMemcpyAsync(c->pos + old_n, pos_xy, n_add * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    GPE_HIP(c, hipMemcpyAsync(c->prev + old_n, pos_xy, n_add * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    GPE_HIP(c, hipMemcpyAsync(c->radius + old_n, radius, n_add * sizeof(float), hipMemcpyHostToDevice, c->stream));
    c->n = new_n;
    c->n_owned = new_n;
    GPE_TRY(init_index_buffers(c, old_n, new_n));
    if (c->uid.on) {                                   // next .. next + n_add - 1, in input order
        GPE_TRY(launch_uid_iota(c, c->uid.uids, old_n, new_n, (uint32_t)c->uid.next));
        c->uid.next += n_add;
        c->uid.map_valid = false;
        uid_slots_stale(c);
    }
    // particle_system.rs:198: max_radius = max(max_radius, r)
    for (uint64_t i = 0; i < n_add; ++i) c->max_radius = fmaxf(c->max_radius, radius[i]);
    c->grid_max_radius = c->max_radius;   // Grid::refresh_grid (grid.rs:266)
    refresh_cell_size(c);
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return reconfigure(c);
}

gpe_status gpe_remove_particles(gpe_ctx *c, const uint8_t *remove, uint64_t n, uint64_t *n_removed)
{
    if (n_removed) *n_removed = 0;
    GPE_TRY(check_removable(c, "gpe_remove_particles"));
    if (!remove) return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles: NULL mask");
    if (n != c->n) return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles: n must equal gpe_len");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(remove_reserve(c, n));
    GPE_HIP(c, hipMemcpyAsync(c->remove_ws.mask, remove, n, hipMemcpyHostToDevice, c->stream));
    return do_remove(c, c->remove_ws.mask, 0.f, 0.f, 0.f, n_removed);
}

gpe_status gpe_remove_particles_in_circle(gpe_ctx *c, float x, float y, float radius, uint64_t *n_removed)
{
    if (n_removed) *n_removed = 0;
    GPE_TRY(check_removable(c, "gpe_remove_particles_in_circle"));
    if (!(radius >= 0.0f) || !isfinite(radius))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles_in_circle: radius must be finite and >= 0");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(remove_reserve(c, 0));
    const float rr = radius * radius;        // binary32, as the device's side of the test
    return do_remove(c, nullptr, x, y, rr, n_removed);
}

// ---- uids ------------------------------------------------------------------------------------------------
gpe_status gpe_enable_uids(gpe_ctx *c, int32_t enable)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    UidState &u = c->uid;
    if (!enable) {
        if (!u.on) return GPE_OK;
        GPE_TRY(refuse_uid_sets(c, "gpe_enable_uids"));         // (they name their particles by uid)
        GPE_HIP(c, hipSetDevice(c->device));
        GPE_HIP(c, hipStreamSynchronize(c->stream));           // (a re-sort in flight may still read them)
        uid_release(c);
        u.on = false;
        u.next = 0;
        return GPE_OK;
    }
    if (u.on) return GPE_OK;                                   // keeps the current uids
    if (is_sharded(c)) return refuse_sharded(c, "gpe_enable_uids");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(uids_switch_on(c));
    const gpe_status st = launch_uid_iota(c, u.uids, 0, c->n, 0u);
    if (st != GPE_OK) {
        uid_release(c);
        u.on = false;
        return st;
    }
    u.next = c->n;
    return GPE_OK;
}

gpe_status gpe_set_uids(gpe_ctx *c, const uint32_t *uids, uint64_t n)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_uids");
    if (!uids) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_uids: NULL uids");
    if (n != c->n) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_uids: n must equal gpe_len");
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    UidState &u = c->uid;
    const bool was_on = u.on;
    if (!was_on) GPE_TRY(uids_switch_on(c));
    // staged in the copy partner and checked there: the live uids change only when the new ones pass
    bool dup = false;
    gpe_status st = GPE_OK;
    const hipError_t e = hipMemcpyAsync(u.uids_copy, uids, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        st = fail(c, GPE_ERR_HIP, std::string("gpe_set_uids: upload: ") + hipGetErrorName(e));
    }
    if (st == GPE_OK) st = uid_map_build(c, u.uids_copy, &dup);
    if (st == GPE_OK && dup) st = fail(c, GPE_ERR_INVALID_ARG, "gpe_set_uids: two particles would share a uid");
    if (st != GPE_OK) {
        if (!was_on) {                                         // off as before
            uid_release(c);
            u.on = false;
        }
        return st;
    }
    std::swap(u.uids, u.uids_copy);
    u.next = (uint64_t)u.map_max + 1;
    u.map_valid = true;                                        // the map just built is the new uids'
    uid_slots_stale(c);                                        // (uid_map_build cleared map_valid on the way)
    return GPE_OK;
}

gpe_status gpe_next_uid(const gpe_ctx *c, uint64_t *next)
{
    if (!c || !next) return GPE_ERR_INVALID_ARG;
    if (!c->uid.on) return fail(const_cast<gpe_ctx *>(c), GPE_ERR_STATE, "gpe_next_uid: uids are off");
    *next = c->uid.next;
    return GPE_OK;
}

gpe_status gpe_set_next_uid(gpe_ctx *c, uint64_t next)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_set_next_uid: uids are off");
    if (next > kUidLimit) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_next_uid: next must be at most 2^32");
    if (c->n > 0) {
        GPE_HIP(c, hipSetDevice(c->device));
        GPE_HIP(c, hipStreamSynchronize(c->stream));
        GPE_TRY(uid_map_ready(c));
        if (next <= c->uid.map_max)
            return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_next_uid: next must be above every current uid");
    }
    c->uid.next = next;
    return GPE_OK;
}

gpe_status gpe_find_uids(gpe_ctx *c, const uint32_t *uids, uint64_t k, uint32_t *index_out, float *pos_xy_out,
                         float *prev_xy_out, float *radius_out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_find_uids: uids are off");
    if (!uids) return fail(c, GPE_ERR_INVALID_ARG, "gpe_find_uids: NULL uids");
    if (k > (1ull << 40)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_find_uids: k too large");
    if (k == 0) return GPE_OK;
    if (c->n == 0) {                                           // no particles: every uid is absent
        const float nan = nanf("");
        for (uint64_t i = 0; i < k; ++i) {
            if (index_out) index_out[i] = GPE_UID_ABSENT;
            if (pos_xy_out) pos_xy_out[2 * i] = pos_xy_out[2 * i + 1] = nan;
            if (prev_xy_out) prev_xy_out[2 * i] = prev_xy_out[2 * i + 1] = nan;
            if (radius_out) radius_out[i] = nan;
        }
        return GPE_OK;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(uid_map_ready(c));
    // staging: pos f32[2k] | prev f32[2k] | radius f32[k] | index u32[k] | query u32[k]
    GPE_TRY(uid_query_reserve(c, 28 * k));
    float2 *d_pos = reinterpret_cast<float2 *>(c->uid.query);
    float2 *d_prev = d_pos + k;
    float *d_radius = reinterpret_cast<float *>(d_prev + k);
    uint32_t *d_index = reinterpret_cast<uint32_t *>(d_radius + k);
    uint32_t *d_query = d_index + k;
    GPE_HIP(c, hipMemcpyAsync(d_query, uids, k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, "uids/find");
        GPE_TRY(launch_uid_find(c, c->uid.map_keys, c->uid.map_vals, c->n, d_query, k, d_index,
                                pos_xy_out ? d_pos : nullptr, prev_xy_out ? d_prev : nullptr,
                                radius_out ? d_radius : nullptr));
    }
    if (index_out)
        GPE_HIP(c, hipMemcpyAsync(index_out, d_index, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (pos_xy_out)
        GPE_HIP(c, hipMemcpyAsync(pos_xy_out, d_pos, k * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    if (prev_xy_out)
        GPE_HIP(c, hipMemcpyAsync(prev_xy_out, d_prev, k * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    if (radius_out)
        GPE_HIP(c, hipMemcpyAsync(radius_out, d_radius, k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return check_device_errors(c);
}

gpe_status gpe_remove_particles_by_uid(gpe_ctx *c, const uint32_t *uids, uint64_t k, uint64_t *n_removed)
{
    if (n_removed) *n_removed = 0;
    GPE_TRY(check_removable(c, "gpe_remove_particles_by_uid"));
    if (!c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_remove_particles_by_uid: uids are off");
    if (!uids) return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles_by_uid: NULL uids");
    if (k > (1ull << 40)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_remove_particles_by_uid: k too large");
    if (k == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(uid_map_ready(c));
    GPE_TRY(remove_reserve(c, c->n));
    GPE_TRY(uid_query_reserve(c, 4 * k));
    uint32_t *d_query = reinterpret_cast<uint32_t *>(c->uid.query);
    GPE_HIP(c, hipMemcpyAsync(d_query, uids, k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, "uids/mark");
        GPE_HIP(c, hipMemsetAsync(c->remove_ws.mask, 0, c->n, c->stream));
        GPE_TRY(launch_uid_mark(c, c->uid.map_keys, c->uid.map_vals, c->n, d_query, k, c->remove_ws.mask));
    }
    return do_remove(c, c->remove_ws.mask, 0.f, 0.f, 0.f, n_removed);
}

gpe_status gpe_len(const gpe_ctx *c, uint64_t *n)
{
    if (!c || !n) return GPE_ERR_INVALID_ARG;
    *n = c->n;
    return GPE_OK;
}

gpe_status gpe_max_radius(const gpe_ctx *c, float *r)
{
    if (!c || !r) return GPE_ERR_INVALID_ARG;
    *r = c->max_radius;
    return GPE_OK;
}

gpe_status gpe_set_mouse(gpe_ctx *c, int32_t pressed, float x, float y)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    c->mouse_pressed = pressed ? 1 : 0;
    c->mouse_x = x;
    c->mouse_y = y;
    return GPE_OK;
}

gpe_status gpe_set_world(gpe_ctx *c, float w, float h)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    c->cfg.world_width = w;
    c->cfg.world_height = h;
    fields_world_changed(c);
    return reconfigure(c);
}

gpe_status gpe_set_gravity(gpe_ctx *c, float gx, float gy)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    c->cfg.gravity_x = gx;
    c->cfg.gravity_y = gy;
    return GPE_OK;
}

gpe_status gpe_world(const gpe_ctx *c, float *w, float *h)
{
    if (!c || !w || !h) return GPE_ERR_INVALID_ARG;
    *w = c->cfg.world_width;
    *h = c->cfg.world_height;
    return GPE_OK;
}

gpe_status gpe_gravity(const gpe_ctx *c, float *gx, float *gy)
{
    if (!c || !gx || !gy) return GPE_ERR_INVALID_ARG;
    *gx = c->cfg.gravity_x;
    *gy = c->cfg.gravity_y;
    return GPE_OK;
}

gpe_status gpe_mouse(const gpe_ctx *c, int32_t *pressed, float *x, float *y)
{
    if (!c || !pressed || !x || !y) return GPE_ERR_INVALID_ARG;
    *pressed = (int32_t)c->mouse_pressed;
    *x = c->mouse_x;
    *y = c->mouse_y;
    return GPE_OK;
}

gpe_status gpe_morton_resort(gpe_ctx *c)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    return do_resort(c);
}

gpe_status gpe_integrate(gpe_ctx *c, float dt)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    return launch_verlet(c, c->pos, c->prev, c->radius, c->n_owned, dt);
}

// ---- grid ---------------------------------------------------------------------------------------------
float gpe_compute_cell_size(float max_obj_radius) { return max_obj_radius * 2.2f; }

gpe_status gpe_grid_set_max_radius(gpe_ctx *c, float r)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    c->grid_max_radius = r;
    refresh_cell_size(c);
    return reconfigure(c);
}

gpe_status gpe_cell_size(const gpe_ctx *c, float *cs)
{
    if (!c || !cs) return GPE_ERR_INVALID_ARG;
    *cs = c->cell_size;
    return GPE_OK;
}

gpe_status gpe_grid_max_radius(const gpe_ctx *c, float *r)
{
    if (!c || !r) return GPE_ERR_INVALID_ARG;
    *r = c->grid_max_radius;
    return GPE_OK;
}

gpe_status gpe_grid_build(gpe_ctx *c)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(need_grid_buffers(c));
    return launch_build_cell_ids(c, c->pos, c->radius, c->n, c->cell_size, c->cell_ids, c->object_ids);
}

gpe_status gpe_grid_sort(gpe_ctx *c)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    return do_grid_sort(c);
}

gpe_status gpe_grid_update(gpe_ctx *c)
{
    GPE_TRY(gpe_grid_build(c));
    return do_grid_sort(c);
}

// ---- physics ---------------------------------------------------------------------------------------------
gpe_status gpe_build_collision_cells(gpe_ctx *c)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    return do_build_collision_cells(c);
}

gpe_status gpe_solve_collisions(gpe_ctx *c)
{
    GPE_TRY(gpe_build_collision_cells(c));
    return do_solve_colors(c);
}

// ---- step ------------------------------------------------------------------------------------------------
// The passes behind every step of gpe_step / gpe_run, in the one order they have (a test arms them all):
// bends, then areas, then bonds (lengths keep the last word over angles and areas), then bodies (a bond can hang a body from an anchor), then
// the obstacles, which keep the last word over all three --
// the movers first, the static walls behind them (a piston squeezes particles against a wall, the wall wins) -- then
// the fields, which write prev only and so are judged where the step and the obstacles left the particle, then the
// observers, whose frames see the result.  A context without a set pays that set's flag test and no call.
static inline gpe_status after_step(gpe_ctx *c, float dt)
{
    for (const UidSet &s : kUidSets)
        if (s.has(c)) GPE_TRY(s.pass(c));
    if (has_movers(c)) GPE_TRY(movers_after_step(c, dt));
    if (has_colliders(c)) GPE_TRY(colliders_after_step(c));
    if (has_fields(c)) GPE_TRY(fields_after_step(c, dt));
    return observers_after_step(c);
}

gpe_status gpe_step(gpe_ctx *c, float dt, uint32_t flags)
{
    GPE_TRY(need_particles(c));
    GPE_TRY(movers_check_dt(c, dt, "gpe_step"));
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(do_step(c, dt, flags));
    return after_step(c, dt);
}

gpe_status gpe_run(gpe_ctx *c, float dt, uint64_t steps, uint64_t resort_every, int32_t resort_first)
{
    GPE_TRY(need_particles(c));
    GPE_TRY(movers_check_dt(c, dt, "gpe_run"));
    GPE_HIP(c, hipSetDevice(c->device));
    // The host may run at most ~64 steps ahead of the device: bounds the queue and the lag of the
    // device-side statistics the step policy reads (native_should_run).
    hipEvent_t fence[2] = {nullptr, nullptr};
    bool armed[2] = {false, false};
    gpe_status rc = GPE_OK;
    for (uint64_t s = 0; s < steps && rc == GPE_OK; ++s) {
        if ((s & 31u) == 0 && steps > 64) {
            const int slot = (int)((s >> 5) & 1u);
            if (armed[slot]) (void)hipEventSynchronize(fence[slot]);
            if (!fence[slot] && hipEventCreateWithFlags(&fence[slot], hipEventDisableTiming) != hipSuccess)
                fence[slot] = nullptr;
            if (fence[slot]) armed[slot] = hipEventRecord(fence[slot], c->stream) == hipSuccess;
        }
        const bool resort = (s == 0 && resort_first) || (resort_every && s > 0 && (s % resort_every) == 0);
        rc = do_step(c, dt, resort ? GPE_STEP_RESORT : 0u);
        if (rc == GPE_OK) rc = after_step(c, dt);
    }
    for (hipEvent_t e : fence) if (e) (void)hipEventDestroy(e);
    return rc;
}

// ---- downloads ---------------------------------------------------------------------------------------------
static gpe_status locate(gpe_ctx *c, gpe_array what, const void **ptr, uint64_t *bytes, bool sizes_only = false)
{
    const uint64_t n = c->n;
    if (sizes_only) {}
    else if (what == GPE_CELL_IDS || what == GPE_OBJECT_IDS || what == GPE_COLLISION_CELLS ||
        what == GPE_NUM_COLLISION_CELLS || what == GPE_CHUNK_OBJ_COUNT || what == GPE_INDIRECT_ARGS)
        GPE_TRY(need_grid_buffers(c));
    switch (what) {
        case GPE_POS: *ptr = c->pos; *bytes = n * 8; break;
        case GPE_PREV: *ptr = c->prev; *bytes = n * 8; break;
        case GPE_RADIUS: *ptr = c->radius; *bytes = n * 4; break;
        case GPE_HOME_CELL_IDS: *ptr = c->home_cell_ids; *bytes = n * 4; break;
        case GPE_PARTICLE_IDS: *ptr = c->particle_ids; *bytes = n * 4; break;
        case GPE_CELL_IDS: *ptr = c->cell_ids; *bytes = n * 16; break;
        case GPE_OBJECT_IDS: *ptr = c->object_ids; *bytes = n * 16; break;
        case GPE_COLLISION_CELLS: *ptr = c->collision_cells; *bytes = n * 16; break;
        case GPE_NUM_COLLISION_CELLS:
            *ptr = c->chunk_obj_count ? c->chunk_obj_count + (num_chunks(c) - 1) : nullptr;
            *bytes = 4;
            break;
        case GPE_CHUNK_OBJ_COUNT: *ptr = c->chunk_obj_count; *bytes = num_chunks(c) * 4; break;
        case GPE_INDIRECT_ARGS: *ptr = c->indirect_args; *bytes = 12; break;
        case GPE_ORDER_KEYS: *ptr = c->order_keys; *bytes = n * 4; break;
        case GPE_UIDS:
            if (!c->uid.on) return fail(c, GPE_ERR_STATE, "GPE_UIDS: uids are off (gpe_enable_uids)");
            *ptr = c->uid.uids;
            *bytes = n * 4;
            break;
        default: return fail(c, GPE_ERR_INVALID_ARG, "unknown gpe_array");
    }
    return GPE_OK;
}

gpe_status gpe_array_bytes(const gpe_ctx *c, gpe_array what, uint64_t *bytes)
{
    if (!c || !bytes) return GPE_ERR_INVALID_ARG;
    const void *p;
    return locate(const_cast<gpe_ctx *>(c), what, &p, bytes, true);
}

gpe_status gpe_device_ptr(gpe_ctx *c, gpe_array what, void **device_ptr, uint64_t *bytes)
{
    GPE_TRY(need_particles(c));
    if (!device_ptr) return fail(c, GPE_ERR_INVALID_ARG, "device_ptr is NULL");
    const void *p;
    uint64_t b;
    GPE_TRY(locate(c, what, &p, &b));
    // (the caller may write radii through it: the step reads every particle's radius again until the next configuration)
    if (what == GPE_RADIUS) c->native.uniform = false;
    *device_ptr = const_cast<void *>(p);
    if (bytes) *bytes = b;
    return GPE_OK;
}

gpe_status gpe_download(gpe_ctx *c, gpe_array what, void *dst, uint64_t bytes)
{
    GPE_TRY(need_particles(c));
    if (!dst) return fail(c, GPE_ERR_INVALID_ARG, "gpe_download: dst is NULL");
    const void *p;
    uint64_t b;
    GPE_TRY(locate(c, what, &p, &b));
    if (bytes != b) return fail(c, GPE_ERR_INVALID_ARG, "gpe_download: byte count does not match the array");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipMemcpyAsync(dst, p, b, hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return check_device_errors(c);
}

// ---- guarded allocations ---------------------------------------------------------------------------------------
gpe_status gpe_guard_check(gpe_ctx *c, gpe_guard_report *out)
{
    if (!c || !out || out->struct_size != sizeof(gpe_guard_report)) return GPE_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(*out);
    GuardState &G = c->guard;
    if (!G.on) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    std::vector<gpe_guard_zone> found = G.kept;
    uint32_t damaged = G.kept_count;
    GPE_HIP(c, guard_scan(c, G.live.data(), G.live.size(), found, &damaged));
    if (G.scan_failed != hipSuccess)
        return fail(c, GPE_ERR_HIP, std::string("gpe_guard_check: the zones of a released buffer could not be checked: ") +
                                        hipGetErrorName(G.scan_failed));
    out->damaged = damaged;
    out->listed = (uint32_t)found.size();
    out->allocations = (uint32_t)G.live.size();
    for (size_t i = 0; i < found.size(); ++i) out->zones[i] = found[i];
    if (damaged) return fail(c, GPE_OK, guard_zone_text(found[0]));    // a finding, not an error: the text all the same
    return GPE_OK;
}

gpe_status gpe_guard_registry(gpe_ctx *c, char *text, uint64_t capacity, uint64_t *needed)
{
    if (!c || (!text && capacity)) return GPE_ERR_INVALID_ARG;
    std::string all;
    for (const std::vector<DevAlloc> *list : {&c->guard.live, &c->guard.released})
        for (const DevAlloc &a : *list)
            all += std::string(a.tag) + " " + std::to_string(a.payload) + " " + std::to_string(a.slack) +
                   (list == &c->guard.live ? " live\n" : " released\n");
    for (const DevAlloc &a : c->guard.pinned)                          // (host blocks: one line per block that exists)
        all += std::string(a.tag) + " " + std::to_string(a.payload) + " 0 pinned\n";
    if (needed) *needed = all.size() + 1;
    if (capacity) {
        const size_t k = std::min<size_t>(all.size(), capacity - 1);
        memcpy(text, all.data(), k);
        text[k] = 0;
    }
    return GPE_OK;
}

// ---- primitives ---------------------------------------------------------------------------------------------
gpe_status gpe_buffer_alloc(gpe_ctx *c, uint64_t bytes, void **device_ptr)
{
    if (!c || !device_ptr) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipSetDevice(c->device));
    *device_ptr = nullptr;
    // payload: the bytes asked for.  slack: the round-up to 16 bytes and 64 more, which the primitives may read past a
    // caller's n elements (the 4-keys-per-lane loads of the sort and scan tiles) but never write
    hipError_t e = gpe_dev_reserve(c, device_ptr, bytes, std::max<uint64_t>(bytes, 16) + 64 - bytes, "user.buffer");
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_buffer_alloc: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_buffer_alloc: ") + hipGetErrorName(e));
    return GPE_OK;
}

gpe_status gpe_buffer_free(gpe_ctx *c, void *device_ptr)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!device_ptr) return GPE_OK;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_HIP(c, gpe_dev_release(c, &device_ptr));
    return GPE_OK;
}

gpe_status gpe_buffer_upload(gpe_ctx *c, void *device_ptr, const void *src, uint64_t bytes)
{
    if (!c || (!device_ptr && bytes) || (!src && bytes)) return GPE_ERR_INVALID_ARG;
    if (bytes == 0) return GPE_OK;
    GPE_HIP(c, hipMemcpyAsync(device_ptr, src, bytes, hipMemcpyHostToDevice, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return GPE_OK;
}

gpe_status gpe_buffer_download(gpe_ctx *c, const void *device_ptr, void *dst, uint64_t bytes)
{
    if (!c || (!device_ptr && bytes) || (!dst && bytes)) return GPE_ERR_INVALID_ARG;
    if (bytes == 0) return GPE_OK;
    GPE_HIP(c, hipMemcpyAsync(dst, device_ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    return GPE_OK;
}

gpe_status gpe_sort_pairs_u32(gpe_ctx *c, uint32_t *d_keys, uint32_t *d_payload, uint64_t n)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (n == 0) return GPE_OK;
    if (!d_keys || !d_payload) return fail(c, GPE_ERR_INVALID_ARG, "gpe_sort_pairs_u32: NULL buffer");
    if (n > 0xffffffffull) return fail(c, GPE_ERR_INVALID_ARG, "gpe_sort_pairs_u32: n must be < 2^32");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(sort_reserve(c, n));
    return sort_pairs(c, d_keys, d_payload, n);
}

gpe_status gpe_sort_histogram_u32(gpe_ctx *c, const uint32_t *d_keys, uint64_t n, uint32_t shift,
                                  uint32_t *d_hist256)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!d_hist256 || (!d_keys && n) || shift > 24) return fail(c, GPE_ERR_INVALID_ARG, "gpe_sort_histogram_u32: bad argument");
    GPE_HIP(c, hipSetDevice(c->device));
    return sort_histogram(c, d_keys, n, shift, d_hist256);
}

gpe_status gpe_sort_scatter_pass_u32(gpe_ctx *c, const uint32_t *ka, const uint32_t *va, uint32_t *kb,
                                     uint32_t *vb, uint64_t n, uint32_t shift)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (n == 0) return GPE_OK;
    if (!ka || !va || !kb || !vb || shift > 24) return fail(c, GPE_ERR_INVALID_ARG, "gpe_sort_scatter_pass_u32: bad argument");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(sort_reserve(c, n));
    return sort_scatter_pass(c, ka, va, kb, vb, n, shift);
}

gpe_status gpe_inclusive_scan_u32(gpe_ctx *c, uint32_t *d_data, uint64_t n)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (n == 0) return GPE_OK;
    if (!d_data) return fail(c, GPE_ERR_INVALID_ARG, "gpe_inclusive_scan_u32: NULL buffer");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(scan_reserve(c, n));
    return inclusive_scan(c, d_data, n);
}

// ---- sharding support -------------------------------------------------------------------------------------
gpe_status gpe_reserve(gpe_ctx *c, uint64_t capacity)
{
    GPE_TRY(need_particles(c));
    if (capacity > (1ull << 30) - 1) return fail(c, GPE_ERR_INVALID_ARG, "gpe_reserve: 4n must fit in u32");
    GPE_HIP(c, hipSetDevice(c->device));
    if (capacity > c->cap) {
        GPE_TRY(grow_particle_buffers(c, capacity));
        GPE_TRY(reconfigure(c));
    }
    return GPE_OK;
}

gpe_status gpe_capacity(const gpe_ctx *c, uint64_t *capacity)
{
    if (!c || !capacity) return GPE_ERR_INVALID_ARG;
    *capacity = c->cap;
    return GPE_OK;
}

gpe_status gpe_set_counts(gpe_ctx *c, uint64_t n_total, uint64_t n_owned)
{
    GPE_TRY(need_particles(c));
    if (n_total == 0 || n_total > c->cap || n_owned > n_total)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_counts: need 0 < n_owned <= n_total <= capacity");
    GPE_TRY(refuse_step_sets(c, "gpe_set_counts", "not supported while uids are on"));
    c->n = n_total;
    c->n_owned = n_owned;
    c->native.uniform = false;                 // (slots the configuration has not looked at: NativeState::uniform)
    return GPE_OK;
}

gpe_status gpe_use_order_keys(gpe_ctx *c, int32_t enable)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (enable) GPE_TRY(refuse_step_sets(c, "gpe_use_order_keys", "sharded runs carry order keys, not uids (uids are on)"));
    c->use_order_keys = enable != 0;
    if (enable) c->native.uniform = false;     // (order-key tiles keep the general path: NativeState::uniform)
    return GPE_OK;
}

gpe_status gpe_set_active_cells(gpe_ctx *c, int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (cx1 < cx0 || cy1 < cy0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_active_cells: empty box");
    c->active_box[0] = cx0; c->active_box[1] = cy0; c->active_box[2] = cx1; c->active_box[3] = cy1;
    c->has_active_box = true;
    if (c->n == 0 || !c->pos) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return reconfigure(c);                     // the block box (sort keys, block table) follows the active box
}

gpe_status gpe_stream_handle(gpe_ctx *c, void **hip_stream)
{
    if (!c || !hip_stream) return GPE_ERR_INVALID_ARG;
    *hip_stream = (void *)c->stream;
    return GPE_OK;
}

static gpe_status mark_trace_origin(gpe_ctx *c);        // below, with the profiling entry points

gpe_status gpe_set_stream(gpe_ctx *c, void *hip_stream)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    resolve_pending(c);                                   // event pairs recorded on the stream being left
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (c->trace_origin || c->stamp_origin) (void)mark_trace_origin(c);    // (in the form the scopes on this stream take)
    for (int i = 0; i < 2; ++i) c->shard.armed[i] = false;
    return GPE_OK;
}

gpe_status gpe_refresh(gpe_ctx *c)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    return reconfigure(c);
}

gpe_status gpe_shard_classify(gpe_ctx *c, const uint8_t *d_owner_of_block, const uint32_t *d_dest_mask_of_block,
                              int32_t blocks_x, int32_t blocks_y, uint32_t my_rank, uint32_t *d_out_index,
                              uint32_t *d_out_info, uint32_t *d_out_count, uint64_t out_capacity)
{
    GPE_TRY(need_particles(c));
    if (!d_owner_of_block || !d_dest_mask_of_block || !d_out_index || !d_out_info || !d_out_count || blocks_x <= 0 ||
        blocks_y <= 0)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_shard_classify: bad argument");
    GPE_HIP(c, hipSetDevice(c->device));
    return launch_shard_classify(c, d_owner_of_block, d_dest_mask_of_block, blocks_x, blocks_y, my_rank, d_out_index,
                                 d_out_info, d_out_count, out_capacity);
}

// ---- profiling ---------------------------------------------------------------------------------------------
static gpe_status mark_trace_origin(gpe_ctx *c)
{
    if (scope_uses_stamps(c)) {
        stamps_make_room(c, 1);                                            // (the buffer, at the first call)
        c->stamp_origin = c->stamp_be.capacity != 0;
        if (c->stamp_origin) c->stamp_be.dev.stamp(kStampOrigin);
        return GPE_OK;
    }
    if (!c->trace_origin) GPE_HIP(c, hipEventCreate(&c->trace_origin));
    GPE_HIP(c, hipEventRecord(c->trace_origin, c->stream));
    return GPE_OK;
}

gpe_status gpe_set_profiling(gpe_ctx *c, uint32_t on)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    c->profiling = on != 0;
    c->profile_every = on;
    c->profile_step = 0;
    if (on && !(scope_uses_stamps(c) ? c->stamp_origin : c->trace_origin != nullptr)) GPE_TRY(mark_trace_origin(c));
    return GPE_OK;
}

gpe_status gpe_reset_timings(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    resolve_pending(c);
    c->stats.clear();
    c->trace.clear();
    return mark_trace_origin(c);
}

gpe_status gpe_get_trace(gpe_ctx *c, gpe_trace_event *out, uint32_t *count)
{
    if (!c || !count) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    resolve_pending(c);
    const uint32_t avail = (uint32_t)c->trace.size();
    if (out) {
        const uint32_t m = std::min(avail, *count);
        for (uint32_t i = 0; i < m; ++i) {
            const TraceEvent &e = c->trace[avail - m + i];               // the newest m, oldest first
            memset(&out[i], 0, sizeof(gpe_trace_event));
            strncpy(out[i].name, c->stats[e.stat].name.c_str(), sizeof(out[i].name) - 1);
            out[i].start_ms = e.start_ms;
            out[i].duration_ms = e.dur_ms;
        }
    }
    *count = avail;
    return GPE_OK;
}

gpe_status gpe_get_timings(gpe_ctx *c, gpe_timing *out, uint32_t *count)
{
    if (!c || !count) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    resolve_pending(c);
    const uint32_t avail = (uint32_t)c->stats.size();
    if (out) {
        const uint32_t m = std::min(avail, *count);
        for (uint32_t i = 0; i < m; ++i) {
            memset(&out[i], 0, sizeof(gpe_timing));
            strncpy(out[i].name, c->stats[i].name.c_str(), sizeof(out[i].name) - 1);
            out[i].total_ms = c->stats[i].total_ms;
            out[i].calls = c->stats[i].calls;
        }
    }
    *count = avail;
    return GPE_OK;
}

}  // extern "C"
