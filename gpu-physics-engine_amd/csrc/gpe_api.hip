// gpe_api.hip -- the extern "C" boundary of include/gpe.h: context, buffers, step ordering,
// downloads, profiling.  All device work goes to one in-order hipStream per context.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <limits>
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

Scope::Scope(gpe_ctx *ctx, const char *name, Boundaries b) : ctx_(ctx), shared_(b == kSharedBoundaries)
{
    if (!ctx_ || !ctx_->profiling) return;
    stat_ = stat_index(ctx_, name);
    HipScopeBackend be{ctx_->stream};
    start_ = ctx_->scope_events.open(be, shared_);
}

Scope::~Scope()
{
    if (!ctx_ || start_ < 0) return;
    HipScopeBackend be{ctx_->stream};
    ctx_->scope_events.close(be, start_, stat_, shared_);
}

constexpr size_t kTraceCap = 1u << 16;

// (after a stream synchronisation) reads the pending pairs into the statistics and the trace; their events go back to
// the pool, a shared one when the last pair that uses it has been read
static void resolve_pending(gpe_ctx *c)
{
    c->scope_events.resolve([c](int stat, hipEvent_t start, hipEvent_t stop) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, start, stop) != hipSuccess) return;
        c->stats[stat].total_ms += ms;
        c->stats[stat].calls += 1;
        float t0 = 0.f;
        if (c->trace_origin && hipEventElapsedTime(&t0, c->trace_origin, start) == hipSuccess) {
            if (c->trace.size() >= kTraceCap) c->trace.erase(c->trace.begin(), c->trace.begin() + kTraceCap / 2);
            TraceEvent e;
            e.stat = stat; e.start_ms = t0; e.dur_ms = ms;
            c->trace.push_back(e);
        }
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

template <typename T>
static gpe_status dev_alloc(gpe_ctx *c, T **p, uint64_t count, const char *tag)
{
    // payload: count elements.  slack: the round-up to 4 elements and 64 bytes -- no kernel is known to read them; they
    // keep the unguarded allocation at the size it always had (max(count, 4) * sizeof(T) + 64)
    const uint64_t payload = count * sizeof(T);
    hipError_t e = dev_reserve(c, p, payload, std::max<uint64_t>(count, 4) * sizeof(T) + 64 - payload, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "hipMalloc: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorName(e));
    return GPE_OK;
}

template <typename T>
static void dev_free(gpe_ctx *c, T *&p)
{
    (void)dev_release(c, p);
}

// The uid buffers, the uid -> index map and the lookup staging (the uid switch itself stays as it is).
static void free_uid_buffers(gpe_ctx *c)
{
    UidState &u = c->uid;
    dev_free(c, u.uids); dev_free(c, u.uids_copy);
    dev_free(c, u.map_keys); dev_free(c, u.map_vals); dev_free(c, u.dup); dev_free(c, u.query);
    u.map_cap = u.query_cap = 0;
    u.map_valid = false;
    c->tracers.stale = true;
}

static void free_particle_buffers(gpe_ctx *c)
{
    dev_free(c, c->pos); dev_free(c, c->prev); dev_free(c, c->radius);
    dev_free(c, c->pos_copy); dev_free(c, c->prev_copy); dev_free(c, c->radius_copy);
    dev_free(c, c->home_cell_ids); dev_free(c, c->particle_ids);
    dev_free(c, c->cell_ids); dev_free(c, c->object_ids);
    dev_free(c, c->chunk_obj_count); dev_free(c, c->collision_cells); dev_free(c, c->indirect_args);
    dev_free(c, c->order_keys);
    dev_free(c, c->remove_ws.tile_count); dev_free(c, c->remove_ws.tile_key); dev_free(c, c->remove_ws.max_key);
    dev_free(c, c->remove_ws.mask);
    c->remove_ws.tiles_cap = c->remove_ws.mask_cap = 0;
    dev_free(c, c->query_ws.tile_count); dev_free(c, c->query_ws.tile_key); dev_free(c, c->query_ws.pick);
    dev_free(c, c->query_ws.stage);
    c->query_ws.tiles_cap = c->query_ws.stage_cap = 0;
    ContactsWorkspace &k = c->contacts_ws;
    dev_free(c, k.keys); dev_free(c, k.vals); dev_free(c, k.rec); dev_free(c, k.degree); dev_free(c, k.upper);
    dev_free(c, k.tile_sum); dev_free(c, k.total); dev_free(c, k.stage);
    k.cap = k.tiles_cap = k.stage_cap = 0;
    RayWorkspace &y = c->ray_ws;
    dev_free(c, y.row_start); dev_free(c, y.from); dev_free(c, y.to); dev_free(c, y.index); dev_free(c, y.uid);
    dev_free(c, y.t); dev_free(c, y.pos); dev_free(c, y.radius);
    y.cap = 0;
    NearestWorkspace &nn = c->nearest_ws;
    dev_free(c, nn.row_start); dev_free(c, nn.points); dev_free(c, nn.count); dev_free(c, nn.index); dev_free(c, nn.uid);
    dev_free(c, nn.dist2); dev_free(c, nn.pos); dev_free(c, nn.radius);
    nn.cap = nn.slots_cap = 0;
    ClustersWorkspace &u = c->clusters_ws;
    dev_free(c, u.parent); dev_free(c, u.label); dev_free(c, u.root_size); dev_free(c, u.size);
    dev_free(c, u.tile_word); dev_free(c, u.words);
    u.cap = u.tiles_cap = 0;
    EditWorkspace &e = c->edit_ws;
    dev_free(c, e.keys); dev_free(c, e.slots); dev_free(c, e.fields); dev_free(c, e.flag);
    dev_free(c, e.tile_key); dev_free(c, e.max_key); dev_free(c, e.count);
    e.keys_cap = e.fields_cap = e.tiles_cap = 0;
    SpawnWorkspace &w = c->spawn_ws;
    dev_free(c, w.pos); dev_free(c, w.radius); dev_free(c, w.keys); dev_free(c, w.vals); dev_free(c, w.rec);
    dev_free(c, w.blocked); dev_free(c, w.state); dev_free(c, w.rank); dev_free(c, w.verdict); dev_free(c, w.ctl);
    w.cap = 0;
    free_uid_buffers(c);
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
static gpe_status init_index_buffers(gpe_ctx *c, uint64_t lo, uint64_t hi)
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

static gpe_status grow_particle_buffers(gpe_ctx *c, uint64_t cap)
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

static void refresh_cell_size(gpe_ctx *c)
{
    c->cell_size = c->grid_max_radius * c->cfg.cell_size_multiplier;        // grid.rs:159-161
}

static gpe_status need_particles(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (c->n == 0 || !c->pos) return fail(c, GPE_ERR_STATE, "no particles: call gpe_set_particles first");
    return GPE_OK;
}

// ---- removal (k_remove.hip) ---------------------------------------------------------------------------
static gpe_status check_removable(gpe_ctx *c, const char *who)
{
    GPE_TRY(need_particles(c));
    if (c->shard.on || c->use_order_keys || c->has_active_box)
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
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
        c->tracers.stale = true;
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
constexpr uint64_t kUidLimit = 1ull << 32;                     // next_uid may reach 2^32: then no particle can be added

static bool is_sharded(const gpe_ctx *c) { return c->shard.on || c->use_order_keys || c->has_active_box; }

// Off -> on: the uid buffers for the current capacity (none yet without particles).
static gpe_status uids_switch_on(gpe_ctx *c)
{
    UidState &u = c->uid;
    if (c->cap > 0) {
        gpe_status st = dev_alloc(c, &u.uids, c->cap, "uid.uids");
        if (st == GPE_OK) st = dev_alloc(c, &u.uids_copy, c->cap, "uid.uids_copy");
        if (st != GPE_OK) {
            free_uid_buffers(c);
            return st;
        }
    }
    u.on = true;
    u.map_valid = false;
    c->tracers.stale = true;
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
static gpe_status uid_map_ready(gpe_ctx *c)
{
    if (c->uid.map_valid) return GPE_OK;
    bool dup = false;
    GPE_TRY(uid_map_build(c, c->uid.uids, &dup));
    if (dup) return fail(c, GPE_ERR_STATE, "uids: two particles share a uid");
    c->uid.map_valid = true;
    return GPE_OK;
}

static gpe_status uid_query_reserve(gpe_ctx *c, uint64_t bytes)
{
    UidState &u = c->uid;
    if (u.query_cap >= bytes) return GPE_OK;
    dev_free(c, u.query);
    u.query_cap = 0;
    GPE_TRY(dev_alloc(c, &u.query, bytes, "uid.query"));
    u.query_cap = bytes;
    return GPE_OK;
}

// ---- tracers (k_tracers.hip) ---------------------------------------------------------------------------------
static gpe_status tracers_alloc(gpe_ctx *c, void **p, uint64_t payload, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, 0, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_tracers_begin: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_tracers_begin: ") + hipGetErrorName(e));
    return GPE_OK;
}

static void tracers_release(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    dev_free(c, t.keys); dev_free(c, t.perm); dev_free(c, t.slot_index);
    dev_free(c, t.ring_pos); dev_free(c, t.ring_prev); dev_free(c, t.ring_index);
    t = TracerState();
}

// One frame at the current steps_seen into ring slot recorded % frames.  Enqueues only: a memset and the resolve pass
// when the slot table is stale, then the sample.  The step numbers stay on the host, which issues every frame.
static gpe_status tracers_take_frame(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    const uint32_t k = (uint32_t)t.k;
    if (t.stale) {
        Scope s(c, "tracers/resolve");
        GPE_HIP(c, hipMemsetAsync(t.slot_index, 0xff, k * sizeof(uint32_t), c->stream));
        if (c->uid.on && c->uid.uids)                                  // uids off: nothing to read, every tracer is absent
            GPE_TRY(launch_tracers_resolve(c, c->uid.uids, c->n, t.keys, t.perm, k, t.lo, t.hi, t.slot_index));
        t.stale = false;
    }
    const uint64_t slot = t.recorded % t.frames, row = slot * t.k;
    {
        Scope s(c, "tracers/sample");
        GPE_TRY(launch_tracers_sample(c, t.slot_index, k, c->pos, c->prev, c->n, t.ring_pos ? t.ring_pos + row : nullptr,
                                      t.ring_prev ? t.ring_prev + row : nullptr,
                                      t.ring_index ? t.ring_index + row : nullptr));
    }
    t.step_of[slot] = t.steps_seen;
    t.recorded += 1;
    t.held = std::min(t.held + 1, t.frames);
    return GPE_OK;
}

// After every step of gpe_step / gpe_run on an armed context.
static gpe_status tracers_after_step(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    t.steps_seen += 1;
    return t.steps_seen % t.every == 0 ? tracers_take_frame(c) : GPE_OK;
}

// ---- run monitor (k_monitor.hip) -------------------------------------------------------------------------------
static void monitor_release(gpe_ctx *c)
{
    dev_free(c, c->monitor.ring); dev_free(c, c->monitor.partials);
    c->monitor = MonitorState();
}

static gpe_status monitor_alloc(gpe_ctx *c, const char *who, void **p, uint64_t payload, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, 0, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, std::string(who) + ": does not fit in device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string(who) + ": " + hipGetErrorName(e));
    return GPE_OK;
}

// The scratch of every record: the partial records, then the device record of gpe_measure.  Written by index below
// monitor_grid(n) <= kMonitorMaxBlocks and whole records.  no slack
static gpe_status monitor_reserve(gpe_ctx *c, const char *who)
{
    if (c->monitor.partials) return GPE_OK;
    return monitor_alloc(c, who, (void **)&c->monitor.partials,
                         kMonitorMaxBlocks * kMonitorPartialBytes + sizeof(gpe_measures), "monitor.partials");
}

// One record of the particles as they are now into *out (device memory).  Enqueues only.  Reads whichever pos / prev /
// uids are live (the native step swaps pos with its copy partner), gpe_len and the world at this moment.
static gpe_status monitor_record(gpe_ctx *c, const char *who, float rest_speed, uint64_t step, gpe_measures *out)
{
    if (c->n > 0xFFFFFFFFull)
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
    const float rs2 = rest_speed * rest_speed;                         // binary32 (-0.0 -> +0, +inf -> +inf)
    if (c->n) {
        Scope s(c, "monitor/partial");
        GPE_TRY(launch_monitor_partial(c, c->pos, c->prev, c->n, rs2, c->cfg.world_width, c->cfg.world_height,
                                       c->monitor.partials));
    }
    Scope s(c, "monitor/final");
    return launch_monitor_final(c, c->monitor.partials, c->n, step, c->uid.on ? c->uid.uids : nullptr, out);
}

// One frame at the current steps_seen into ring slot recorded % frames.
static gpe_status monitor_take_frame(gpe_ctx *c)
{
    MonitorState &m = c->monitor;
    GPE_TRY(monitor_record(c, "gpe_monitor", m.rest_speed, m.steps_seen, m.ring + m.recorded % m.frames));
    m.recorded += 1;
    m.held = std::min(m.held + 1, m.frames);
    return GPE_OK;
}

// After every step of gpe_step / gpe_run on an armed context.
static gpe_status monitor_after_step(gpe_ctx *c)
{
    MonitorState &m = c->monitor;
    m.steps_seen += 1;
    return m.steps_seen % m.every == 0 ? monitor_take_frame(c) : GPE_OK;
}

// ---- in-place edits (k_edit.hip) ---------------------------------------------------------------------------
// One buffer of the edit workspace (tags "edit.*"): allocated at first use and, with a capacity word, regrown when
// `count` passes it (cap == NULL: a buffer of fixed size).  payload: count elements; slack_bytes: stated at the call
// with its reader.
template <typename T>
static gpe_status edit_buffer(gpe_ctx *c, T **p, uint64_t *cap, uint64_t count, uint64_t slack_bytes, const char *tag)
{
    if (*p && (!cap || *cap >= count)) return GPE_OK;
    dev_free(c, *p);
    if (cap) *cap = 0;
    const hipError_t e = dev_reserve(c, p, count * sizeof(T), slack_bytes, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "hipMalloc: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorName(e));
    if (cap) *cap = count;
    return GPE_OK;
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
        c->tracers.stale = true;
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
    const gpe_status st = do_step_scoped(c, dt, flags);
    if (c->profile_every > 1) c->profiling = true;
    return st;
}

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
    if (c->trace_origin) (void)hipEventDestroy(c->trace_origin);
    free_particle_buffers(c);
    tracers_release(c);
    monitor_release(c);
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

// Device-side error words (sticky): reported at the synchronising entry points.
static gpe_status check_device_errors(gpe_ctx *c)
{
    uint32_t words[3] = {0, 0, 0};
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
static gpe_status reconfigure(gpe_ctx *c)
{
    if (c->cfg.mode == GPE_MODE_NATIVE && c->n > 0) return native_configure(c);
    c->native.policy.eligible = false;
    return GPE_OK;
}

extern "C++" {
namespace gpe {
gpe_status reconfigure_native(gpe_ctx *c) { return reconfigure(c); }
}
}

gpe_status gpe_sync(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (c->shard.xstream) GPE_HIP(c, hipStreamSynchronize(c->shard.xstream));   // (a sharded run's exchange stream)
    return check_device_errors(c);
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
        c->tracers.stale = true;
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
        c->tracers.stale = true;
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
        GPE_HIP(c, hipSetDevice(c->device));
        GPE_HIP(c, hipStreamSynchronize(c->stream));           // (a re-sort in flight may still read them)
        free_uid_buffers(c);
        u.on = false;
        u.next = 0;
        return GPE_OK;
    }
    if (u.on) return GPE_OK;                                   // keeps the current uids
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_enable_uids: not supported on a sharded context (gpe_shard_*, order "
                                            "keys or an active cell box)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_TRY(uids_switch_on(c));
    const gpe_status st = launch_uid_iota(c, u.uids, 0, c->n, 0u);
    if (st != GPE_OK) {
        free_uid_buffers(c);
        u.on = false;
        return st;
    }
    u.next = c->n;
    return GPE_OK;
}

gpe_status gpe_set_uids(gpe_ctx *c, const uint32_t *uids, uint64_t n)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_set_uids: not supported on a sharded context (gpe_shard_*, order "
                                            "keys or an active cell box)");
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
            free_uid_buffers(c);
            u.on = false;
        }
        return st;
    }
    std::swap(u.uids, u.uids_copy);
    u.next = (uint64_t)u.map_max + 1;
    u.map_valid = true;                                        // the map just built is the new uids'
    c->tracers.stale = true;                                   // (uid_map_build cleared map_valid on the way)
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

// ---- tracers (k_tracers.hip) ---------------------------------------------------------------------------------
gpe_status gpe_tracers_begin(gpe_ctx *c, const gpe_tracer_config *cfg)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!cfg || cfg->struct_size < sizeof(gpe_tracer_config))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: NULL cfg or bad struct_size");
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_tracers_begin: not supported on a sharded context (gpe_shard_*, order "
                                            "keys or an active cell box)");
    constexpr uint32_t kFields = GPE_TRACER_POS | GPE_TRACER_PREV | GPE_TRACER_INDEX;
    if (!cfg->uids) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: NULL uids");
    if (cfg->k == 0 || cfg->k > GPE_TRACERS_MAX)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: k must be 1 .. GPE_TRACERS_MAX");
    if (cfg->every == 0 || cfg->frames == 0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: every and frames must be >= 1");
    if (cfg->fields == 0 || (cfg->fields & ~kFields))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: fields must be GPE_TRACER_* bits, at least one");
    const uint32_t k = (uint32_t)cfg->k;
    // the tracked uids ascending with the tracer each one is: what the resolve pass searches
    std::vector<uint32_t> perm(k), keys(k);
    for (uint32_t j = 0; j < k; ++j) perm[j] = j;
    std::sort(perm.begin(), perm.end(), [cfg](uint32_t a, uint32_t b) { return cfg->uids[a] < cfg->uids[b]; });
    for (uint32_t j = 0; j < k; ++j) keys[j] = cfg->uids[perm[j]];
    for (uint32_t j = 1; j < k; ++j)
        if (keys[j] == keys[j - 1]) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: two tracers share a uid");
    if (c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_begin: already armed (gpe_tracers_end first)");
    if (!c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_tracers_begin: uids are off (gpe_enable_uids)");
    GPE_TRY(need_particles(c));
    if (cfg->frames > (1ull << 40) / k)                                // (frames * k * 8 bytes is far past any device)
        return fail(c, GPE_ERR_OOM, "gpe_tracers_begin: the ring does not fit in device memory");
    GPE_HIP(c, hipSetDevice(c->device));
    TracerState &t = c->tracers;
    const uint64_t rows = cfg->frames * cfg->k;
    // every array is read and written by index below k or frames * k (the resolve pass reads keys by single words
    // below k, the uids by 16-byte groups below n / 4 and single words below n).  no slack
    gpe_status st = tracers_alloc(c, (void **)&t.keys, k * sizeof(uint32_t), "tracers.keys");
    if (st == GPE_OK) st = tracers_alloc(c, (void **)&t.perm, k * sizeof(uint32_t), "tracers.perm");
    if (st == GPE_OK) st = tracers_alloc(c, (void **)&t.slot_index, k * sizeof(uint32_t), "tracers.slot_index");
    if (st == GPE_OK && (cfg->fields & GPE_TRACER_POS))
        st = tracers_alloc(c, (void **)&t.ring_pos, rows * sizeof(float2), "tracers.ring_pos");
    if (st == GPE_OK && (cfg->fields & GPE_TRACER_PREV))
        st = tracers_alloc(c, (void **)&t.ring_prev, rows * sizeof(float2), "tracers.ring_prev");
    if (st == GPE_OK && (cfg->fields & GPE_TRACER_INDEX))
        st = tracers_alloc(c, (void **)&t.ring_index, rows * sizeof(uint32_t), "tracers.ring_index");
    if (st == GPE_OK) {
        hipError_t e = hipMemcpyAsync(t.keys, keys.data(), k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(t.perm, perm.data(), k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // the host vectors go away on return
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st = fail(c, GPE_ERR_HIP, std::string("gpe_tracers_begin: upload: ") + hipGetErrorName(e));
        }
    }
    if (st != GPE_OK) {
        const std::string why = c->last_error;
        tracers_release(c);                                            // unarmed, as before
        c->last_error = why;
        return st;
    }
    t.armed = true;
    t.stale = true;
    t.fields = cfg->fields;
    t.k = cfg->k; t.every = cfg->every; t.frames = cfg->frames;
    t.steps_seen = t.recorded = t.held = 0;
    t.lo = keys.front(); t.hi = keys.back();
    t.step_of.assign((size_t)cfg->frames, 0);
    return GPE_OK;
}

gpe_status gpe_tracers_sample(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_sample: not armed (gpe_tracers_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    return tracers_take_frame(c);
}

gpe_status gpe_tracers_read(gpe_ctx *c, gpe_tracer_frames *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out || out->struct_size < sizeof(gpe_tracer_frames))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: NULL out or bad struct_size");
    out->count = out->recorded = 0;
    TracerState &t = c->tracers;
    if (!t.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_read: not armed (gpe_tracers_begin)");
    if (out->flags & ~(uint32_t)GPE_TRACERS_CONSUME) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: unknown flag");
    if ((out->pos_xy && !t.ring_pos) || (out->prev_xy && !t.ring_prev) || (out->index && !t.ring_index))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: an array for a field the recorder was not configured with");
    GPE_HIP(c, hipSetDevice(c->device));
    const uint64_t m = std::min(t.held, out->capacity), first = t.recorded - m;   // frames first .. recorded - 1
    // the frames lie in at most two runs of ring slots
    for (uint64_t done = 0; done < m;) {
        const uint64_t slot = (first + done) % t.frames, run = std::min(m - done, t.frames - slot);
        const uint64_t src = slot * t.k, dst = done * t.k, rows = run * t.k;
        if (out->pos_xy)
            GPE_HIP(c, hipMemcpyAsync(out->pos_xy + 2 * dst, t.ring_pos + src, rows * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        if (out->prev_xy)
            GPE_HIP(c, hipMemcpyAsync(out->prev_xy + 2 * dst, t.ring_prev + src, rows * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        if (out->index)
            GPE_HIP(c, hipMemcpyAsync(out->index + dst, t.ring_index + src, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->step)
            for (uint64_t f = 0; f < run; ++f) out->step[done + f] = t.step_of[slot + f];
        done += run;
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    out->count = t.held;
    out->recorded = t.recorded;
    if (out->flags & GPE_TRACERS_CONSUME) t.held = 0;
    return check_device_errors(c);
}

gpe_status gpe_tracers_end(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_end: not armed (gpe_tracers_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (frames in flight still write the ring)
    tracers_release(c);
    return GPE_OK;
}

// ---- run monitor (k_monitor.hip) -------------------------------------------------------------------------------
static bool monitor_rest_speed_ok(float r) { return r >= 0.0f; }      // NaN and negatives fail; -0.0 and +inf pass

gpe_status gpe_measure(gpe_ctx *c, float rest_speed, gpe_measures *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out) return fail(c, GPE_ERR_INVALID_ARG, "gpe_measure: NULL out");
    if (!monitor_rest_speed_ok(rest_speed)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_measure: rest_speed is NaN or negative");
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_measure: not supported on a sharded context (gpe_shard_*, order keys or "
                                            "an active cell box)");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, "gpe_measure: more than 2^32 - 1 particles");
    gpe_measures r;
    if (c->n == 0) {                                                   // nothing to read: the "none" values
        memset(&r, 0, sizeof(r));
        r.min_x = r.min_y = INFINITY;
        r.max_x = r.max_y = -INFINITY;
        r.max_v2_index = r.first_irregular = 0xFFFFFFFFu;
        r.max_v2_uid = r.first_irregular_uid = GPE_UID_ABSENT;
        *out = r;
        return GPE_OK;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(monitor_reserve(c, "gpe_measure"));
    gpe_measures *dev = (gpe_measures *)(c->monitor.partials + kMonitorMaxBlocks * kMonitorPartialBytes);
    GPE_TRY(monitor_record(c, "gpe_measure", rest_speed, 0, dev));
    GPE_HIP(c, hipMemcpyAsync(&r, dev, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    GPE_TRY(check_device_errors(c));                                   // (synchronises the stream)
    *out = r;
    return GPE_OK;
}

gpe_status gpe_monitor_begin(gpe_ctx *c, const gpe_monitor_config *cfg)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!cfg || cfg->struct_size < sizeof(gpe_monitor_config))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: NULL cfg or bad struct_size");
    if (cfg->flags) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: flags must be 0");
    if (cfg->every == 0 || cfg->frames == 0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: every and frames must be >= 1");
    if (!monitor_rest_speed_ok(cfg->rest_speed))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: rest_speed is NaN or negative");
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_monitor_begin: not supported on a sharded context (gpe_shard_*, order "
                                            "keys or an active cell box)");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, "gpe_monitor_begin: more than 2^32 - 1 particles");
    MonitorState &m = c->monitor;
    if (m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_begin: already armed (gpe_monitor_end first)");
    GPE_TRY(need_particles(c));
    if (cfg->frames > (1ull << 40) / sizeof(gpe_measures))             // (far past any device)
        return fail(c, GPE_ERR_OOM, "gpe_monitor_begin: the ring does not fit in device memory");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(monitor_reserve(c, "gpe_monitor_begin"));
    // written one whole record at a time, at slot recorded % frames.  no slack
    GPE_TRY(monitor_alloc(c, "gpe_monitor_begin: the ring", (void **)&m.ring, cfg->frames * sizeof(gpe_measures), "monitor.ring"));
    m.armed = true;
    m.every = cfg->every; m.frames = cfg->frames; m.rest_speed = cfg->rest_speed;
    m.steps_seen = m.recorded = m.held = 0;
    return GPE_OK;
}

gpe_status gpe_monitor_sample(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->monitor.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_sample: not armed (gpe_monitor_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    return monitor_take_frame(c);
}

gpe_status gpe_monitor_read(gpe_ctx *c, gpe_monitor_frames *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out || out->struct_size < sizeof(gpe_monitor_frames))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_read: NULL out or bad struct_size");
    MonitorState &m = c->monitor;
    if (!m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_read: not armed (gpe_monitor_begin)");
    if (out->flags & ~(uint32_t)GPE_MONITOR_CONSUME) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_read: unknown flag");
    GPE_HIP(c, hipSetDevice(c->device));
    const uint64_t want = out->frames ? std::min(m.held, out->capacity) : 0, first = m.recorded - want;
    // records first .. recorded - 1 lie in at most two runs of ring slots
    for (uint64_t done = 0; done < want;) {
        const uint64_t slot = (first + done) % m.frames, run = std::min(want - done, m.frames - slot);
        GPE_HIP(c, hipMemcpyAsync(out->frames + done, m.ring + slot, run * sizeof(gpe_measures), hipMemcpyDeviceToHost, c->stream));
        done += run;
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    out->count = m.held;
    out->recorded = m.recorded;
    if (out->flags & GPE_MONITOR_CONSUME) m.held = 0;
    return check_device_errors(c);
}

gpe_status gpe_monitor_end(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    MonitorState &m = c->monitor;
    if (!m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_end: not armed (gpe_monitor_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (frames in flight still write the ring)
    dev_free(c, m.ring);
    uint8_t *keep = m.partials;                                        // gpe_measure goes on using the scratch
    m = MonitorState();
    m.partials = keep;
    return GPE_OK;
}

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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
    if (out->uid && !c->uid.on) return fail(c, GPE_ERR_STATE, std::string(who) + ": uid requested while uids are off");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
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
        auto part = [m](bool on, uint64_t width) { return on ? (m * width + 255) / 256 * 256 : 0; };
        const uint64_t o_prev = part(out->pos_xy, 8), o_radius = o_prev + part(out->prev_xy, 8),
                       o_index = o_radius + part(out->radius, 4), o_uid = o_index + part(out->index, 4),
                       bytes = o_uid + part(out->uid, 4);
        GPE_TRY(query_reserve(c, bytes));
        uint8_t *st = ws.stage;
        float2 *d_pos = out->pos_xy ? reinterpret_cast<float2 *>(st) : nullptr;
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
static gpe_status circle_region(gpe_ctx *c, const char *who, float x, float y, float radius, float (&region)[5])
{
    if (!(radius >= 0.0f) || !isfinite(radius))
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": radius must be finite and >= 0");
    const float words[5] = {x, y, 0.f, 0.f, radius * radius};     // binary32, as gpe_remove_particles_in_circle
    std::copy(words, words + 5, region);
    return GPE_OK;
}

// *empty: x0 > x1 or y0 > y1, a box that holds nothing
static gpe_status box_region(gpe_ctx *c, const char *who, float x0, float y0, float x1, float y1, float (&region)[5],
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
    if (out->capacity >= 1) {                                     // one row: straight from the particle buffers
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

// ---- contact queries (k_contacts.hip) ----------------------------------------------------------------------
static gpe_status contacts_alloc(gpe_ctx *c, void **p, uint64_t payload, uint64_t slack, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, slack, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_query_contacts: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_query_contacts: ") + hipGetErrorName(e));
    return GPE_OK;
}

static gpe_status contacts_reserve(gpe_ctx *c, uint64_t stage_bytes)
{
    ContactsWorkspace &ws = c->contacts_ws;
    const uint64_t n = c->n, tiles = contacts_tiles(n);
    if (ws.cap < n) {
        dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec); dev_free(c, ws.degree); dev_free(c, ws.upper);
        ws.cap = 0;
        // keys / vals: n words each.  slack: the 16 words sort_pairs' tile loads may read behind the n pairs
        GPE_TRY(contacts_alloc(c, (void **)&ws.keys, n * sizeof(uint32_t), 16 * sizeof(uint32_t), "contacts.keys"));
        GPE_TRY(contacts_alloc(c, (void **)&ws.vals, n * sizeof(uint32_t), 16 * sizeof(uint32_t), "contacts.vals"));
        // rec: n 16-byte records, read one at a time below n.  no slack
        GPE_TRY(contacts_alloc(c, (void **)&ws.rec, n * sizeof(uint4), 0, "contacts.rec"));
        // degree: n words, written and read by index below n.  no slack
        GPE_TRY(contacts_alloc(c, (void **)&ws.degree, n * sizeof(uint32_t), 0, "contacts.degree"));
        // upper: n words, scanned in place.  slack: the 16 words the scan's tile loads may read behind them
        GPE_TRY(contacts_alloc(c, (void **)&ws.upper, n * sizeof(uint32_t), 16 * sizeof(uint32_t), "contacts.upper"));
        ws.cap = n;
    }
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_sum);
        ws.tiles_cap = 0;
        // tile_sum: one 64-bit word per workgroup of the count.  no slack
        GPE_TRY(contacts_alloc(c, (void **)&ws.tile_sum, tiles * sizeof(unsigned long long), 0, "contacts.tile_sum"));
        ws.tiles_cap = tiles;
    }
    // total: one 64-bit word.  no slack
    if (!ws.total) GPE_TRY(contacts_alloc(c, (void **)&ws.total, sizeof(unsigned long long), 0, "contacts.total"));
    if (ws.stage_cap < stage_bytes) {
        dev_free(c, ws.stage);
        ws.stage_cap = 0;
        // stage: the 256-byte aligned parts of the requested per-pair arrays, written below capacity.  no slack
        GPE_TRY(contacts_alloc(c, (void **)&ws.stage, stage_bytes, 0, "contacts.stage"));
        ws.stage_cap = stage_bytes;
    }
    GPE_TRY(sort_reserve(c, n));
    return scan_reserve(c, n);
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
    if ((out->uid_a || out->uid_b) && !c->uid.on)
        return fail(c, GPE_ERR_STATE, std::string(who) + ": uid requested while uids are off");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
    const uint64_t n = c->n;
    if (n == 0 || !c->pos) return GPE_OK;
    // the query's own cell size: a contact implies a centre distance below 2 max|r|, less than one cell of 2.2 max|r|
    const float cell_size = gpe_compute_cell_size(fabsf(c->max_radius));
    if (n > 1 && !isfinite(cell_size))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": the largest radius is not finite");
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
        auto part = [m](bool on) { return on ? (m * 4 + 255) / 256 * 256 : 0; };
        const uint64_t o_b = part(out->index_a), o_ua = o_b + part(out->index_b), o_ub = o_ua + part(out->uid_a),
                       o_ov = o_ub + part(out->uid_b), bytes = o_ov + part(out->overlap);
        GPE_TRY(contacts_reserve(c, bytes));
        uint8_t *st = ws.stage;
        uint32_t *d_a = out->index_a ? reinterpret_cast<uint32_t *>(st) : nullptr;
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
static gpe_status clusters_alloc(gpe_ctx *c, void **p, uint64_t payload, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, 0, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_query_clusters: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_query_clusters: ") + hipGetErrorName(e));
    return GPE_OK;
}

static gpe_status clusters_reserve(gpe_ctx *c)
{
    ClustersWorkspace &ws = c->clusters_ws;
    const uint64_t n = c->n, tiles = contacts_tiles(n);
    if (ws.cap < n) {
        dev_free(c, ws.parent); dev_free(c, ws.label); dev_free(c, ws.root_size); dev_free(c, ws.size);
        ws.cap = 0;
        // parent: n words, read and written by index below n (the indices of the sorted records).  no slack
        GPE_TRY(clusters_alloc(c, (void **)&ws.parent, n * sizeof(uint32_t), "clusters.parent"));
        // label: n words, written by index below n; the member kernels read it by index below n (guarded tile loads).  no slack
        GPE_TRY(clusters_alloc(c, (void **)&ws.label, n * sizeof(uint32_t), "clusters.label"));
        // root_size: n words, indexed by a label, which is an index below n.  no slack
        GPE_TRY(clusters_alloc(c, (void **)&ws.root_size, n * sizeof(uint32_t), "clusters.root_size"));
        // size: n words, written by index below n.  no slack (nothing here is scanned; the members' scan runs on
        // query.tile_count)
        GPE_TRY(clusters_alloc(c, (void **)&ws.size, n * sizeof(uint32_t), "clusters.size"));
        ws.cap = n;
    }
    if (ws.tiles_cap < tiles) {
        dev_free(c, ws.tile_word);
        ws.tiles_cap = 0;
        // tile_word: one 64-bit word per workgroup of the flatten / sizes kernels.  no slack
        GPE_TRY(clusters_alloc(c, (void **)&ws.tile_word, tiles * sizeof(unsigned long long), "clusters.tile_word"));
        ws.tiles_cap = tiles;
    }
    // words: two 64-bit words.  no slack
    if (!ws.words) GPE_TRY(clusters_alloc(c, (void **)&ws.words, 2 * sizeof(unsigned long long), "clusters.words"));
    return GPE_OK;
}

// The checks the two cluster queries share once the result struct is usable and its count is 0: the refusals of
// gpe_query_contacts.  *cell_size = the contact query's own cell size.
static gpe_status clusters_begin(gpe_ctx *c, const char *who, float *cell_size)
{
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
    *cell_size = gpe_compute_cell_size(fabsf(c->max_radius));
    if (c->n > 1 && !isfinite(*cell_size))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": the largest radius is not finite");
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
    if (n == 1 || cell_size == 0.0f) {                             // nothing touches: the seed alone, from the particle buffers
        const uint32_t i = seed;
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
static gpe_status ray_alloc(gpe_ctx *c, void **p, uint64_t payload, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, 0, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_cast_rays: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_cast_rays: ") + hipGetErrorName(e));
    return GPE_OK;
}

// room for a batch of k rays; every array is read and written by index below k or kRayRowWords.  no slack
static gpe_status ray_reserve(gpe_ctx *c, uint64_t k)
{
    RayWorkspace &ws = c->ray_ws;
    if (!ws.row_start) GPE_TRY(ray_alloc(c, (void **)&ws.row_start, kRayRowWords * sizeof(uint32_t), "ray.row_start"));
    if (ws.cap < k) {
        dev_free(c, ws.from); dev_free(c, ws.to); dev_free(c, ws.index); dev_free(c, ws.uid); dev_free(c, ws.t);
        dev_free(c, ws.pos); dev_free(c, ws.radius);
        ws.cap = 0;
        GPE_TRY(ray_alloc(c, (void **)&ws.from, k * sizeof(float2), "ray.from"));
        GPE_TRY(ray_alloc(c, (void **)&ws.to, k * sizeof(float2), "ray.to"));
        GPE_TRY(ray_alloc(c, (void **)&ws.index, k * sizeof(uint32_t), "ray.index"));
        GPE_TRY(ray_alloc(c, (void **)&ws.uid, k * sizeof(uint32_t), "ray.uid"));
        GPE_TRY(ray_alloc(c, (void **)&ws.t, k * sizeof(float), "ray.t"));
        GPE_TRY(ray_alloc(c, (void **)&ws.pos, k * sizeof(float2), "ray.pos"));
        GPE_TRY(ray_alloc(c, (void **)&ws.radius, k * sizeof(float), "ray.radius"));
        ws.cap = k;
    }
    return GPE_OK;
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
    if (r->uid && !c->uid.on) return fail(c, GPE_ERR_STATE, std::string(who) + ": uid requested while uids are off");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
    if (k == 0) return GPE_OK;
    const bool any = c->n > 0 && c->pos;
    // the contact query's own cell size: a touched centre lies within max|r| = cell / 2.2 of its segment
    const float cell_size = any ? gpe_compute_cell_size(fabsf(c->max_radius)) : 0.0f;
    if (!isfinite(cell_size)) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": the largest radius is not finite");
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
static gpe_status nearest_alloc(gpe_ctx *c, void **p, uint64_t payload, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, 0, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_query_nearest: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_query_nearest: ") + hipGetErrorName(e));
    return GPE_OK;
}

// room for a batch of k points of m slots each; every array is read and written by index below k, k * m or
// kRayRowWords.  no slack
static gpe_status nearest_reserve(gpe_ctx *c, uint64_t k, uint64_t m)
{
    NearestWorkspace &ws = c->nearest_ws;
    if (!ws.row_start)
        GPE_TRY(nearest_alloc(c, (void **)&ws.row_start, kRayRowWords * sizeof(uint32_t), "nearest.row_start"));
    if (ws.cap < k) {
        dev_free(c, ws.points); dev_free(c, ws.count);
        ws.cap = 0;
        GPE_TRY(nearest_alloc(c, (void **)&ws.points, k * sizeof(float2), "nearest.points"));
        GPE_TRY(nearest_alloc(c, (void **)&ws.count, k * sizeof(uint32_t), "nearest.count"));
        ws.cap = k;
    }
    const uint64_t slots = k * m;
    if (ws.slots_cap < slots) {
        dev_free(c, ws.index); dev_free(c, ws.uid); dev_free(c, ws.dist2); dev_free(c, ws.pos); dev_free(c, ws.radius);
        ws.slots_cap = 0;
        GPE_TRY(nearest_alloc(c, (void **)&ws.index, slots * sizeof(uint32_t), "nearest.index"));
        GPE_TRY(nearest_alloc(c, (void **)&ws.uid, slots * sizeof(uint32_t), "nearest.uid"));
        GPE_TRY(nearest_alloc(c, (void **)&ws.dist2, slots * sizeof(float), "nearest.dist2"));
        GPE_TRY(nearest_alloc(c, (void **)&ws.pos, slots * sizeof(float2), "nearest.pos"));
        GPE_TRY(nearest_alloc(c, (void **)&ws.radius, slots * sizeof(float), "nearest.radius"));
        ws.slots_cap = slots;
    }
    return GPE_OK;
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
    if (q->uid && !c->uid.on) return fail(c, GPE_ERR_STATE, std::string(who) + ": uid requested while uids are off");
    if (c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 particles");
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

// ---- overlap-checked adds (k_spawn.hip) --------------------------------------------------------------------
static gpe_status spawn_alloc(gpe_ctx *c, void **p, uint64_t payload, uint64_t slack, const char *tag)
{
    const hipError_t e = gpe_dev_reserve(c, p, payload, slack, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "gpe_add_particles_free: out of device memory");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("gpe_add_particles_free: ") + hipGetErrorName(e));
    return GPE_OK;
}

// Scratch of the call's own: nothing of the contact or cluster workspaces is used, so a later query finds its buffers
// as it left them.
static gpe_status spawn_reserve(gpe_ctx *c, uint64_t k)
{
    SpawnWorkspace &ws = c->spawn_ws;
    if (ws.cap < k) {
        dev_free(c, ws.pos); dev_free(c, ws.radius); dev_free(c, ws.keys); dev_free(c, ws.vals); dev_free(c, ws.rec);
        dev_free(c, ws.blocked); dev_free(c, ws.state); dev_free(c, ws.rank); dev_free(c, ws.verdict);
        ws.cap = 0;
        // pos / radius: the k uploaded candidates, read by index below k.  no slack
        GPE_TRY(spawn_alloc(c, (void **)&ws.pos, k * sizeof(float2), 0, "spawn.pos"));
        GPE_TRY(spawn_alloc(c, (void **)&ws.radius, k * sizeof(float), 0, "spawn.radius"));
        // keys / vals: k words each.  slack: the 16 words sort_pairs' tile loads may read behind the k pairs
        GPE_TRY(spawn_alloc(c, (void **)&ws.keys, k * sizeof(uint32_t), 16 * sizeof(uint32_t), "spawn.keys"));
        GPE_TRY(spawn_alloc(c, (void **)&ws.vals, k * sizeof(uint32_t), 16 * sizeof(uint32_t), "spawn.vals"));
        // rec: k 16-byte records, read one at a time below k.  no slack
        GPE_TRY(spawn_alloc(c, (void **)&ws.rec, k * sizeof(uint4), 0, "spawn.rec"));
        // blocked / state: k words each, written and read by index below k.  no slack
        GPE_TRY(spawn_alloc(c, (void **)&ws.blocked, k * sizeof(uint32_t), 0, "spawn.blocked"));
        GPE_TRY(spawn_alloc(c, (void **)&ws.state, k * sizeof(uint32_t), 0, "spawn.state"));
        // rank: k words, scanned in place.  slack: the 16 words the scan's tile loads may read behind them
        GPE_TRY(spawn_alloc(c, (void **)&ws.rank, k * sizeof(uint32_t), 16 * sizeof(uint32_t), "spawn.rank"));
        // verdict: k bytes, written and copied out below k.  no slack
        GPE_TRY(spawn_alloc(c, (void **)&ws.verdict, k, 0, "spawn.verdict"));
        ws.cap = k;
    }
    // ctl: kSpawnCtlWords words.  no slack
    if (!ws.ctl) GPE_TRY(spawn_alloc(c, (void **)&ws.ctl, kSpawnCtlWords * sizeof(uint32_t), 0, "spawn.ctl"));
    GPE_TRY(sort_reserve(c, k));
    return scan_reserve(c, k);
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
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
    if (!finite || !isfinite(cell_size))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": the largest radius is not finite");
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
            c->tracers.stale = true;
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
// staging rows, 256-byte aligned parts, only the requested fields: pos | prev | radius
struct EditRows {
    uint64_t o_prev = 0, o_radius = 0, bytes = 0;
};
static EditRows edit_rows(const gpe_particle_edit *e)
{
    const uint64_t k = e->k;
    auto part = [k](bool on, uint64_t width) { return on ? (k * width + 255) / 256 * 256 : 0; };
    EditRows r;
    r.o_prev = part(e->pos_xy, 8);
    r.o_radius = r.o_prev + part(e->prev_xy, 8);
    r.bytes = r.o_radius + part(e->radius, 4);
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_edit_particles: not supported on a sharded context (gpe_shard_*, order "
                                            "keys or an active cell box)");
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
    if (is_sharded(c))
        return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported on a sharded context (gpe_shard_*, "
                                                                "order keys or an active cell box)");
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
gpe_status gpe_step(gpe_ctx *c, float dt, uint32_t flags)
{
    GPE_TRY(need_particles(c));
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(do_step(c, dt, flags));
    if (c->tracers.armed) GPE_TRY(tracers_after_step(c));
    return c->monitor.armed ? monitor_after_step(c) : GPE_OK;
}

gpe_status gpe_run(gpe_ctx *c, float dt, uint64_t steps, uint64_t resort_every, int32_t resort_first)
{
    GPE_TRY(need_particles(c));
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
        if (rc == GPE_OK && c->tracers.armed) rc = tracers_after_step(c);
        if (rc == GPE_OK && c->monitor.armed) rc = monitor_after_step(c);
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
    if (c->uid.on) return fail(c, GPE_ERR_UNSUPPORTED, "gpe_set_counts: not supported while uids are on");
    c->n = n_total;
    c->n_owned = n_owned;
    return GPE_OK;
}

gpe_status gpe_use_order_keys(gpe_ctx *c, int32_t enable)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (enable && c->uid.on)
        return fail(c, GPE_ERR_UNSUPPORTED, "gpe_use_order_keys: sharded runs carry order keys, not uids (uids are on)");
    c->use_order_keys = enable != 0;
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

gpe_status gpe_set_stream(gpe_ctx *c, void *hip_stream)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    resolve_pending(c);                                   // event pairs recorded on the stream being left
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (c->trace_origin) (void)hipEventRecord(c->trace_origin, c->stream);
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
    if (on && !c->trace_origin) GPE_TRY(mark_trace_origin(c));
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
