// gpe_internal.h -- shared declarations of the gfx950 implementation behind include/gpe.h.
// HIP for CDNA4 only: wave64, no portability layers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/gpe.h"
#include "k_collider.h"
#include "k_mover.h"
#include "native_policy.h"
#include "scope_events.h"
#include "scope_stamps.h"
#include "set_upload.h"

namespace gpe {

constexpr uint32_t kUnused = GPE_UNUSED_CELL_ID;
constexpr int kWave = 64;
// Streaming kernels cap their grid and grid-stride the rest (256 CUs x 8 blocks).
constexpr int kStreamBlock = 256;
constexpr int kMaxStreamGrid = 256 * 8;

inline int stream_grid(uint64_t items, int per_block = kStreamBlock)
{
    uint64_t g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > (uint64_t)kMaxStreamGrid) g = kMaxStreamGrid;
    return (int)g;
}

// ------------------------------------------------------------------------------------------------
// device helpers shared by several kernels (each restates a WGSL helper; citations are into
// /root/reference/src)
// ------------------------------------------------------------------------------------------------
// grid.wgsl:101-108 / home_cell_ids.wgsl:38-45
__host__ __device__ __forceinline__ uint32_t split_by_bits(uint32_t n)
{
    uint32_t x = n & 0x0000FFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
// grid.wgsl:112-114 ; u32(i32) is a bit cast
__device__ __forceinline__ uint32_t morton_encode(int32_t x, int32_t y)
{
    return split_by_bits((uint32_t)x) | (split_by_bits((uint32_t)y) << 1);
}
// collision_solver.wgsl:123-130
__device__ __forceinline__ uint32_t unsplit_by_bits(uint32_t n)
{
    uint32_t x = n & 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
// collision_solver.wgsl:55-58
__device__ __forceinline__ uint32_t cell_color(uint32_t cell_hash)
{
    return 1u + (unsplit_by_bits(cell_hash) & 1u) + (unsplit_by_bits(cell_hash >> 1) & 1u) * 2u;
}
// WGSL i32(f32): truncate, saturate, NaN -> 0.  v_cvt_i32_f32 does exactly that on gfx950, but
// the C++ cast is undefined out of range, so spell it out (the compiler folds it back).
__device__ __forceinline__ int32_t f32_to_i32_sat(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 0x7fffffff;
    if (f <= -2147483648.0f) return (int32_t)0x80000000;
    return (int32_t)f;
}
// grid.wgsl:53 / home_cell_ids.wgsl:27 : vec2<i32>(floor(pos / cell_size)) -- a true division.
__device__ __forceinline__ int32_t cell_coord(float p, float cell_size)
{
    return f32_to_i32_sat(floorf(p / cell_size));
}
// WGSL clamp(e, lo, hi) = min(max(e, lo), hi), written with compares so NaN/-0 behave as in the oracle
__device__ __forceinline__ float clamp_f(float x, float lo, float hi)
{
    float m = (x > lo) ? x : lo;
    return (m < hi) ? m : hi;
}
// grid.wgsl:117-129 is_obj_in_cell
__device__ __forceinline__ bool is_obj_in_cell(float px, float py, float sq_radius, int32_t cx,
                                               int32_t cy, float cs)
{
    float lo_x = (float)cx * cs, lo_y = (float)cy * cs;
    float hi_x = lo_x + cs, hi_y = lo_y + cs;
    float qx = clamp_f(px, lo_x, hi_x), qy = clamp_f(py, lo_y, hi_y);
    float dx = px - qx, dy = py - qy;
    float dist_sq = dx * dx + dy * dy;
    return dist_sq < sq_radius;
}

// ------------------------------------------------------------------------------------------------
// wave64 / block helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// The lanes of the wave for which `p` holds, as a mask.  (The builtin on the predicate itself: HIP's __ballot(int) turns
// the lane mask the compare has just produced into a 0 / 1 register and compares that again -- two VALU instructions per
// vote, and the tile kernels vote ~40 times per workgroup pass.)
__device__ __forceinline__ uint64_t ballot64(const bool p) { return __builtin_amdgcn_ballot_w64(p); }
// ... and back: the per-lane predicate of a (wave-uniform) lane mask.  Costs nothing: selects and branches take the
// mask as it is.  Votes on single comparisons combined by scalar ANDs, turned back into a predicate here, replace
// `a && b && c` where the combined predicate is also voted on (pair_response, k_native.hip).
__device__ __forceinline__ bool lanes_of(const uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// lane LANE of `v` = the wave-uniform `value`: one v_writelane_b32
template <int LANE>
__device__ __forceinline__ void write_lane(int &v, const int value)
{
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(value), "n"(LANE));
}

// number of set bits of `m` strictly below this lane
__device__ __forceinline__ uint32_t popc_below_lane(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// inclusive scan across the 64 lanes of a wave: six DPP adds (row shifts by 1, 2, 4, 8 inside the 16-lane rows, then
// the row totals broadcast from lane 15 into rows 1 and 3 and from lane 31 into rows 2 and 3) instead of six
// ds_bpermute round trips through the LDS crossbar with a select each.  A source lane outside the row / wave reads
// as 0 (bound_ctrl), which is the identity of the sum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v)
{
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
    v = dpp_add<0x111, 0xF>(v);        // row_shr:1
    v = dpp_add<0x112, 0xF>(v);        // row_shr:2
    v = dpp_add<0x114, 0xF>(v);        // row_shr:4
    v = dpp_add<0x118, 0xF>(v);        // row_shr:8
    v = dpp_add<0x142, 0xA>(v);        // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xC>(v);        // row_bcast:31 into rows 2 and 3
    return v;
}
// sum over the 64 lanes, the same in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}

// max over the 64 lanes, the same in every lane (the max-radius keys of k_remove.hip and k_edit.hip)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// exclusive scan of one value per thread over a 256-thread block; `total` receives the block sum.
// s_w: >= 4 words of LDS scratch.  Contains __syncthreads (all 256 threads must call it).
__device__ __forceinline__ uint32_t block256_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int lane = lane_id();
    const int w = (int)(threadIdx.x >> 6);
    uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
    uint32_t base = (w > 0 ? w0 : 0u) + (w > 1 ? w1 : 0u) + (w > 2 ? w2 : 0u);
    if (total) *total = w0 + w1 + w2 + w3;
    __syncthreads();
    return base + inc - v;
}

// LDS words shared by the lanes of ONE wave between barriers-free steps (per-wave counters, match tables).
// Not `volatile`: volatile accesses are left in the generic address space (flat_load/flat_store ... sc0 sc1
// followed by s_waitcnt vmcnt(0)), several times the cost of ds_read/ds_write.  Relaxed wavefront-scope atomics
// compile to plain ds_* instructions; wave_lds_order() keeps the compiler from moving them across each other
// (the LDS itself executes a wave's instructions in order).
template <typename T>
__device__ __forceinline__ T wave_lds_load(const T *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
template <typename T>
__device__ __forceinline__ void wave_lds_store(T *p, T v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// LDS histogram add for one wave-round: one atomic when the whole wave holds one digit (the common
// case for the high digits of nearly sorted keys), else one atomic per lane.
__device__ __forceinline__ void hist_add(uint32_t *s_hist, uint32_t d, bool valid)
{
    // Only scalar work on the critical path (ballots, one v_readlane): either the whole wave holds one
    // digit value -- one atomic -- or every lane issues its own fire-and-forget LDS atomic (the LDS
    // serialises lanes that hit the same bin; measured cheaper than peeling the values off with ballots:
    // the hash kernel went from 0.44 to 0.70 ms at 100 M particles with a four-value peel).
    const uint64_t m = ballot64(valid);
    if (m == 0) return;                                        // wave-uniform
    const int first = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m));
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, first);
    if (ballot64(valid && d != d0) == 0) {
        if (lane_id() == first) atomicAdd(&s_hist[d0], (uint32_t)__popcll(m));
        return;
    }
    if (valid) atomicAdd(&s_hist[d], 1u);
}

struct VerletParams {
    float dt_squared;
    float world_w, world_h;
    float acc_x, acc_y;          // FORCE_OF_GRAVITY (particle_integration.wgsl:21)
    uint32_t mouse_pressed;
    float mouse_x, mouse_y, mouse_strength;
};

// particle_integration.wgsl:34-76 for one particle
__device__ __forceinline__ void verlet_one(float cx, float cy, float qx, float qy, float r,
                                           const VerletParams &P, float &nx, float &ny)
{
    float vx = cx - qx, vy = cy - qy;                       // :40
    float ax = P.acc_x, ay = P.acc_y;                       // :42
    if (P.mouse_pressed == 1u) {                            // :44
        float dx = P.mouse_x - cx, dy = P.mouse_y - cy;     // :46
        float len = sqrtf(dx * dx + dy * dy);               // :50 normalize()
        ax = ax + (dx / len) * P.mouse_strength;            // :50,53
        ay = ay + (dy / len) * P.mouse_strength;
    }
    nx = (cx + vx) + ax * P.dt_squared;                     // :59
    ny = (cy + vy) + ay * P.dt_squared;
    nx = clamp_f(nx, r, P.world_w - r);                     // :70
    ny = clamp_f(ny, r, P.world_h - r);                     // :71
}

// ------------------------------------------------------------------------------------------------
// host-side context
// ------------------------------------------------------------------------------------------------
struct ScopeStat {
    std::string name;
    double total_ms = 0.0;
    uint64_t calls = 0;
};
struct HipScopeBackend {             // the event calls behind ScopeEvents (scope_events.h), on the context's stream
    using Event = hipEvent_t;
    hipStream_t stream;
    bool create(hipEvent_t *e) { return hipEventCreate(e) == hipSuccess; }
    void record(hipEvent_t e) { (void)hipEventRecord(e, stream); }
    void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct HipStampDev {                 // the device side of StampBackend (scope_stamps.h): gpe_api.hip
    gpe_ctx *c = nullptr;
    unsigned long long *buf = nullptr;           // "native.scope_stamps": one 64-bit timestamp per slot
    bool grow(uint32_t old_slots, uint32_t new_slots);
    void stamp(uint32_t slot);
};
struct TraceEvent {                  // one resolved scope instance (gpe_get_trace)
    int stat;
    double start_ms, dur_ms;         // start relative to the trace origin (gpe_set_profiling / gpe_reset_timings)
};

struct ScanWorkspace {           // reduce-then-scan tile sums, one array per recursion level
    std::vector<uint32_t *> level;
    std::vector<uint64_t> cap;
};

struct RemoveWorkspace {         // gpe_remove_particles* (k_remove.hip); allocated at first use, freed with the particles
    uint32_t *tile_count = nullptr;              // per-tile survivor counts, scanned in place
    unsigned long long *tile_key = nullptr;      // per-tile max of the survivors' bits(|radius|) << 32 | index
    uint64_t tiles_cap = 0;
    unsigned long long *max_key = nullptr;       // survivors' max of bits(|radius|) << 32 | index
    uint8_t *mask = nullptr;                     // the uploaded removal mask
    uint64_t mask_cap = 0;
};

struct QueryWorkspace {          // gpe_query_* / gpe_pick (k_query.hip); allocated at first use, freed with the particles
    uint32_t *tile_count = nullptr;              // per-tile match counts, scanned in place
    unsigned long long *tile_key = nullptr;      // gpe_pick: per-tile min of bits(d2) << 32 | index
    uint64_t tiles_cap = 0;
    unsigned long long *pick = nullptr;          // gpe_pick: the min over the tiles
    uint8_t *stage = nullptr;                    // the gathered rows of the requested fields
    uint64_t stage_cap = 0;                      // bytes
};

struct ContactsWorkspace {       // gpe_query_contacts (k_contacts.hip); allocated at first use, freed with the particles
    uint32_t *keys = nullptr, *vals = nullptr;   // clamped cell key and storage index per particle, sorted by the key
    uint4 *rec = nullptr;                        // per sorted slot: bits of x, y, radius and the storage index
    uint32_t *degree = nullptr;                  // per particle: its contacts
    uint32_t *upper = nullptr;                   // per particle: its contacts of higher index, scanned in place
    uint64_t cap = 0;                            // particles the five arrays above hold
    unsigned long long *tile_sum = nullptr;      // per workgroup of the count: the sum of its `upper`
    uint64_t tiles_cap = 0;
    unsigned long long *total = nullptr;         // the number of contacts
    uint8_t *stage = nullptr;                    // the gathered rows of the requested per-pair arrays
    uint64_t stage_cap = 0;                      // bytes
};

struct RayWorkspace {            // gpe_cast_rays (k_raycast.hip); allocated at first use, freed with the particles
    uint32_t *row_start = nullptr;               // kRayRowWords: per clamped row, its first slot of the sorted keys
    float2 *from = nullptr, *to = nullptr;       // the uploaded endpoints of one batch of rays
    uint32_t *index = nullptr, *uid = nullptr;   // per ray of the batch: the first hit's row
    float *t = nullptr, *radius = nullptr;
    float2 *pos = nullptr;
    uint64_t cap = 0;                            // rays the seven arrays above hold
};
constexpr uint32_t kRayRowWords = 65537;         // rows 0 .. 65535 of the clamped key and the end of the last one
constexpr uint32_t kRayMaxBatch = 1u << 20;      // rays per launch; gpe_cast_rays walks a longer list in batches

struct NearestWorkspace {        // gpe_query_nearest (k_nearest.hip); allocated at first use, freed with the particles
    uint32_t *row_start = nullptr;               // kRayRowWords: per clamped row, its first slot of the sorted keys
    float2 *points = nullptr;                    // the uploaded query points of one batch
    uint32_t *count = nullptr;                   // per point of the batch: neighbours delivered
    uint32_t *index = nullptr, *uid = nullptr;   // per slot (point x m) of the batch: the neighbours' rows
    float *dist2 = nullptr, *radius = nullptr;
    float2 *pos = nullptr;
    uint64_t cap = 0;                            // points the first two arrays hold
    uint64_t slots_cap = 0;                      // slots the five per-slot arrays hold
};
constexpr uint32_t kNearestMaxM = 64;            // GPE_NEAREST_MAX_M: the wave keeps one neighbour per lane
constexpr uint64_t kNearestMaxSlots = 1ull << 22;    // batch x m per launch; gpe_query_nearest walks a longer list in batches

struct ClustersWorkspace {       // gpe_query_clusters / gpe_query_cluster_of (k_clusters.hip); allocated at first use, freed with the particles
    uint32_t *parent = nullptr;                  // the union-find forest: parent[i] <= i; after the flatten free for label_uid
    uint32_t *label = nullptr;                   // per particle: the lowest index of its cluster
    uint32_t *root_size = nullptr;               // per root: the particles of its cluster (0 elsewhere)
    uint32_t *size = nullptr;                    // per particle: the particles of its cluster
    uint64_t cap = 0;                            // particles the four arrays above hold
    unsigned long long *tile_word = nullptr;     // per workgroup: its number of roots, later its largest size key
    uint64_t tiles_cap = 0;
    unsigned long long *words = nullptr;         // [0] the number of clusters, [1] the largest size << 32 | ~label
};

struct SpawnWorkspace {          // gpe_add_particles_free (k_spawn.hip); allocated at first use, freed with the particles
    float2 *pos = nullptr;                       // the uploaded candidates, input order
    float *radius = nullptr;
    uint32_t *keys = nullptr, *vals = nullptr;   // clamped cell key and input index per candidate, sorted by the key
    uint4 *rec = nullptr;                        // per sorted slot: bits of x, y, radius and the input index
    uint32_t *blocked = nullptr;                 // per candidate: 1 when a particle of the context touches it
    uint32_t *state = nullptr;                   // per candidate: its verdict (GPE_SPAWN_*), or kSpawnUndecided
    uint32_t *rank = nullptr;                    // per candidate: 1 when added, scanned in place
    uint8_t *verdict = nullptr;                  // per candidate: its verdict as the byte the host downloads
    uint64_t cap = 0;                            // candidates the nine arrays above hold
    uint32_t *ctl = nullptr;                     // kSpawnCtlWords: the candidates' cell box, the rounds' undecided counters
};
constexpr uint32_t kSpawnUndecided = 4u;         // SpawnWorkspace::state: waits for a candidate of lower index
constexpr int kSpawnRoundsPerLook = 8;           // separation rounds between two host reads of the undecided counters
// ctl words: [0] min cx, [1] min cy, [2] 65535 - max cx, [3] 65535 - max cy of the candidates inside the world test
// (one atomicMin each, all ones = no candidate); [kSpawnCtlRounds + r]: candidates still undecided after round r of a batch
constexpr int kSpawnCtlRounds = 4, kSpawnCtlWords = kSpawnCtlRounds + kSpawnRoundsPerLook;

struct EditWorkspace {           // gpe_edit_particles / gpe_kick_* (k_edit.hip); allocated at first use, freed with the particles
    uint32_t *keys = nullptr;                    // the caller's keys, resolved to storage indices in place, then sorted
    uint32_t *slots = nullptr;                   // each key's position in the caller's arrays, sorted with it
    uint64_t keys_cap = 0;
    uint8_t *fields = nullptr;                   // the staged rows of the requested fields: pos | prev | radius
    uint64_t fields_cap = 0;                     // bytes
    uint32_t *flag = nullptr;                    // [0] refusal bits (kEditBadIndex / kEditDuplicate), [1] keys that name a particle
    unsigned long long *tile_key = nullptr;      // radius edits: per-tile max of bits(|radius|) << 32 | index
    uint64_t tiles_cap = 0;
    unsigned long long *max_key = nullptr;       // ... and the max over the tiles
    unsigned long long *count = nullptr;         // gpe_kick_*: particles kicked (zeroed by the call)
};
constexpr uint32_t kEditBadIndex = 1u, kEditDuplicate = 2u;
constexpr uint32_t kEditPos = 1u, kEditPrev = 2u, kEditRadius = 4u;   // field mask of k_edit_apply

struct UidState {               // opt-in particle uids (gpe_enable_uids; k_uids.hip)
    bool on = false;
    uint64_t next = 0;                           // the uid the next added particle gets (at most 2^32)
    uint32_t *uids = nullptr;                    // cap entries; follows pos / prev / radius through every permutation
    uint32_t *uids_copy = nullptr;               // its partner in the copy set (swapped with it)
    // uid -> index map, allocated at first use: uids sorted ascending (keys) with their storage index (vals)
    uint32_t *map_keys = nullptr, *map_vals = nullptr;
    uint64_t map_cap = 0;
    bool map_valid = false;                      // cleared by everything that changes n, the order or the uids
    uint32_t map_max = 0;                        // the largest uid, with the map
    uint32_t *dup = nullptr;                     // duplicate flag of the last map build
    uint8_t *query = nullptr;                    // gpe_find_uids / _by_uid staging: queries and results
    uint64_t query_cap = 0;                      // bytes
};

struct TracerState {            // the tracer recorder (gpe_tracers_*; k_tracers.hip).  Observation state: no step reads it
    bool armed = false;
    bool stale = true;                           // the slot table is out of date (uid_slots_stale)
    uint32_t fields = 0;                         // GPE_TRACER_*
    uint64_t k = 0, every = 1, frames = 0;       // the configuration of gpe_tracers_begin
    uint64_t steps_seen = 0;                     // steps since begin
    uint64_t recorded = 0, held = 0;             // frames taken since begin / of them still in the ring (<= frames)
    uint32_t *keys = nullptr, *perm = nullptr;   // k each: the tracked uids ascending / the tracer each one is
    uint32_t lo = 0, hi = 0;                     // keys[0], keys[k - 1]
    uint32_t *slot_index = nullptr;              // k: each tracer's storage index, 0xffffffff for none (valid unless stale)
    float2 *ring_pos = nullptr, *ring_prev = nullptr;   // frames * k rows each, only the configured fields
    uint32_t *ring_index = nullptr;
    std::vector<uint64_t> step_of;               // host side of the ring: steps_seen when frame slot f was taken
};

// the run monitor (gpe_measure / gpe_monitor_*; k_monitor.hip).  Observation state: no step reads it
constexpr uint32_t kMonitorMaxBlocks = 2048;     // grid cap of the partial pass (256 CUs x 8 workgroups): one partial record each
constexpr uint64_t kMonitorPartialBytes = 80;    // sizeof(MonitorAcc), k_monitor.hip
struct MonitorState {
    bool armed = false;
    uint64_t every = 1, frames = 0;              // the configuration of gpe_monitor_begin
    float rest_speed = 0.f;
    uint64_t steps_seen = 0;                     // steps since begin
    uint64_t recorded = 0, held = 0;             // records taken since begin / of them still in the ring (<= frames)
    gpe_measures *ring = nullptr;                // frames records, written whole by k_monitor_final
    // kMonitorMaxBlocks partial records, then one gpe_measures: the device record of gpe_measure.  Allocated by the
    // first record taken, kept until gpe_destroy (a fixed size: no frame ever has to reallocate it)
    uint8_t *partials = nullptr;
};

// The cell-list lookup grid of the static colliders and of the force fields (collider_grid.h, field_grid.h; the holder
// and its upload: gpe_colliders.hip).  Rebuilt before the next pass when what it was built for has changed
struct CellListGrid {
    bool valid = false;
    float rb = 0.f, w = 0.f, h = 0.f;            // the radius bound (colliders only) and the world at the build (compared by bits)
    ColliderGridView view;
    uint32_t *cell_start = nullptr, *items = nullptr;
    uint64_t entries = 0;
};

// the static colliders (gpe_set_colliders; gpe_colliders.hip, k_colliders.hip).  Step state: gpe_step / gpe_run apply them
struct ColliderState {
    std::vector<gpe_collider> set;               // the colliders as the host gave them (empty: none, nothing is launched)
    float4 *rec = nullptr;                       // 2 per collider: (ax, ay, bx, by), (R, 0, 0, 0)
    unsigned long long *pushed = nullptr;        // one word: particles moved since the last gpe_set_colliders
    // the surfaces (gpe_set_surfaces; gpe_surfaces.hip, k_surface.h): empty / null: none, the plain pass is launched
    std::vector<gpe_surface> surfaces;           // one row per collider, as the host gave them (-0.0 stored as +0)
    float4 *surf = nullptr;                      // the same rows on the device
    uint64_t passes = 0;                         // passes enqueued since then
    CellListGrid grid;                           // built for gpe_max_radius and the world
};

// the sweep of the static colliders (gpe_set_collider_sweep; gpe_sweep.hip, k_sweep.hip, k_sweep.h).  A mode of their
// pass, like gravity: it outlives gpe_set_colliders and gpe_set_surfaces
struct SweepState {
    uint32_t mode = 0;                           // GPE_SWEEP_OFF / GPE_SWEEP_ON
    uint64_t passes = 0;                         // swept passes enqueued since the mode was last set
    unsigned long long *counts = nullptr;        // two words: particles swept, particles stopped, since then (null: never on)
};

// The node table of a step set that names its particles by uid (bonds, bends, areas): the distinct uids the set names,
// their storage slots and a CSR of each node's incidences (uid_nodes.h builds it, k_uid_nodes.h walks it; the set keeps
// its own incidence words beside it).  Device side, read by index below the stated count
struct UidNodeTable {
    uint64_t nodes = 0;                          // m: the distinct uids the set names
    bool stale = true;                           // node_slot is out of date (uid_slots_stale)
    uint64_t resolves = 0;                       // lookups since the set was given
    uint32_t *node_uid = nullptr;                // m: the nodes' uids, ascending
    uint32_t *node_slot = nullptr;               // m: each node's storage index, 0xffffffff for none (valid unless stale)
    uint32_t *row_start = nullptr;               // m + 1
};

// the distance bonds (gpe_set_bonds; gpe_bonds.hip, k_bonds.hip, bond_graph.h).  Step state: gpe_step / gpe_run relax them
struct BondState {
    std::vector<gpe_bond> set;                   // the bonds as the host gave them (empty: none, nothing is launched)
    uint32_t iterations = 1;
    uint64_t passes = 0;                         // since the last gpe_set_bonds
    UidNodeTable nt;                             // the uids the bonds name
    // device side, read by index below the stated count
    uint4 *rec = nullptr;                        // k: (node a, node b | anchor index, rest, w), bond_graph.h BondRecord
    float *max_length = nullptr;                 // k, or NULL when no bond can break
    float2 *anchors = nullptr;                   // one per anchor bond, or NULL
    uint32_t n_anchors = 0;
    uint32_t *inc = nullptr;                     // row_start[m] = 2 k - n_anchors: a node's bonds, bond << 1 | side
    float2 *corr = nullptr;                      // k: this relaxation's corrections
    uint8_t *state = nullptr;                    // k: 0 acted, 1 broken (sticky), 2 inert in this relaxation
    unsigned long long *broken = nullptr;        // one word: bonds broken
    // the colour tables (bond_colours.h): held only while the solver is coloured (BondSolverState), null otherwise
    uint32_t *order = nullptr;                   // k: the bond indices by (colour, index)
    uint32_t *colour_start = nullptr;            // colours + 1, the device's copy (the one-workgroup form reads it)
    std::vector<uint32_t> colour_begin;          // colours + 1, the host's copy (the per-colour launches' ranges)
    uint32_t colours = 0, largest_colour = 0;
};

// the bonds' solver (gpe_set_bond_solver; gpe_bonds.hip, k_bonds.hip, bond_colours.h).  A mode of their pass, like the
// colliders' sweep: it outlives gpe_set_bonds
struct BondSolverState {
    uint32_t mode = 0;                           // GPE_BOND_SOLVER_JACOBI / GPE_BOND_SOLVER_COLOURED
    uint32_t form = 0;                           // the last coloured pass's: 0 none yet, 1 per colour, 2 one workgroup
    uint64_t passes = 0;                         // coloured passes enqueued since the mode was last set
};

// the bend constraints (gpe_set_bends; gpe_bends.hip, k_bends.hip, bend_graph.h).  Step state: gpe_step / gpe_run relax
// them in front of the bonds
struct BendState {
    std::vector<gpe_bend> set;                   // the bends as the host gave them (empty: none, nothing is launched)
    uint32_t iterations = 1;
    uint64_t passes = 0;                         // since the last gpe_set_bends
    UidNodeTable nt;                             // the uids the bends name
    // device side, read by index below the stated count
    uint4 *rec = nullptr;                        // 2 k: (node a, hinge b, node c, rc), (rs, stiffness, 0, 0), bend_graph.h BendRecord
    uint32_t *inc = nullptr;                     // row_start[m] = 3 k: a node's bends, bend << 2 | role
    float4 *corr = nullptr;                      // k: this relaxation's corrections (da.x, da.y, dc.x, dc.y)
    uint8_t *state = nullptr;                    // k: 0 acted, 2 inert in this relaxation
    // the colour tables (bend_colours.h): held only while the solver is coloured (BendSolverState), null otherwise
    uint32_t *order = nullptr;                   // k: the bend indices by (colour, index)
    uint32_t *colour_start = nullptr;            // colours + 1, the device's copy (the one-workgroup form reads it)
    std::vector<uint32_t> colour_begin;          // colours + 1, the host's copy (the per-colour launches' ranges)
    uint32_t colours = 0, largest_colour = 0;
};

// the bends' solver (gpe_set_bend_solver; gpe_bends.hip, k_bends.hip, bend_colours.h).  A mode of their pass, like the
// bonds' solver: it outlives gpe_set_bends
struct BendSolverState {
    uint32_t mode = 0;                           // GPE_BEND_SOLVER_JACOBI / GPE_BEND_SOLVER_COLOURED
    uint32_t form = 0;                           // the last coloured pass's: 0 none yet, 1 per colour, 2 one workgroup
    uint64_t passes = 0;                         // coloured passes enqueued since the mode was last set
};

// the area constraints (gpe_set_areas; gpe_areas.hip, k_areas.hip, area_table.h).  Step state: gpe_step / gpe_run relax
// them behind the bends and in front of the bonds
struct AreaState {
    std::vector<gpe_area> set;                   // the loops as the host gave them (empty: none, nothing is launched)
    std::vector<uint32_t> member_uid_host;       // members: what gpe_get_areas gives back
    uint32_t iterations = 1;
    uint64_t members = 0;
    uint64_t passes = 0;                         // since the last gpe_set_areas
    UidNodeTable nt;                             // the uids the members name; nt.stale: member_slot is out of date too
    uint32_t class_start[6] = {0, 0, 0, 0, 0, 0};   // order[class_start[q], class_start[q + 1]): the loops of width 4 << q
    // device side, read by index below the stated count
    uint4 *rec = nullptr;                        // k: (first, count, rest_area, stiffness), area_table.h AreaRecord
    uint32_t *order = nullptr;                   // k: loop indices by width class
    uint32_t *member_node = nullptr;             // members: each member's node index
    uint32_t *member_slot = nullptr;             // members: node_slot of its node (valid unless stale)
    uint2 *inc = nullptr;                        // row_start[m] = members: a node's memberships, (member, loop)
    float2 *corr = nullptr;                      // members: this relaxation's corrections
    uint8_t *state = nullptr;                    // k: 0 acted, 2 inert in this relaxation
    float2 *value = nullptr;                     // k: (area, lambda) of the last relaxation, NaNs for an inert loop
};

// the rigid and soft bodies (gpe_set_bodies; gpe_bodies.hip, k_bodies.hip, body_table.h).  Step state: gpe_step / gpe_run match them
struct BodyState {
    std::vector<gpe_body> set;                   // the bodies as the host gave them (empty: none, nothing is launched)
    std::vector<uint32_t> member_uid_host;       // members: as the host gave them (gpe_get_bodies)
    std::vector<float> member_rest_host;         // 2 * members
    uint64_t members = 0;
    bool stale = true;                           // member_slot is out of date (uid_slots_stale)
    uint64_t passes = 0, resolves = 0;           // since the last gpe_set_bodies
    uint32_t class_start[7] = {0, 0, 0, 0, 0, 0, 0};   // order[class_start[q], class_start[q + 1]): the bodies of width 2 << q
    // device side, read by index below the stated count
    uint4 *rec = nullptr;                        // k: (first, count, stiffness, bd2), body_table.h BodyRecord
    uint32_t *order = nullptr;                   // k: body indices by width class
    uint32_t *member_uid = nullptr;              // members
    uint32_t *member_slot = nullptr;             // members: each member's storage index, 0xffffffff for none (valid unless stale)
    float2 *member_rest = nullptr;               // members
    float4 *pose = nullptr;                      // k: (cx, cy, co, si) of the last pass, NaNs while inert or broken
    uint8_t *state = nullptr;                    // k: 0 acted, 1 broken (sticky), 2 inert in the last pass
    unsigned long long *broken = nullptr;        // one word: bodies broken
};

// the force fields (gpe_set_fields; gpe_fields.hip, k_fields.hip, field_grid.h).  Step state: gpe_step / gpe_run apply them
struct FieldState {
    std::vector<gpe_field> set;                  // the fields as the host gave them (empty: none, nothing is launched)
    float4 *rec = nullptr;                       // 3 per field: k_field.h FieldRecord
    unsigned long long *touched = nullptr;       // one word: particles whose prev was written since the last gpe_set_fields
    uint64_t passes = 0;                         // passes enqueued since then
    CellListGrid grid;                           // built for the world; gpe_set_world clears `valid`, the tables stay
};

// the moving colliders (gpe_set_movers; gpe_movers.hip, k_movers.hip, k_mover.h, mover_grid.h).  Step state: gpe_step /
// gpe_run advance them on the device, rebuild their lookup grid there and apply them
struct MoverState {
    std::vector<gpe_mover> set;                  // the movers as the host gave them (empty: none, nothing is launched)
    MoverDef *def = nullptr;                     // one per mover: the rest capsule and the motion (k_mover.h)
    float *pose = nullptr;                       // 6 per mover: gpe_mover_pose, the posed capsule and the motion state
    float4 *rec = nullptr;                       // 2 per mover: the posed (ax, ay, bx, by), (R, 0, 0, 0): the pass's records
    unsigned long long *pushed = nullptr;        // one word: particles moved since the last gpe_set_movers
    // the surfaces (gpe_set_surfaces; gpe_surfaces.hip, k_surface.h): empty / null: none, the plain build and pass
    std::vector<gpe_surface> surfaces;           // one row per mover, as the host gave them (-0.0 stored as +0)
    float4 *surf = nullptr;                      // the same rows on the device
    float4 *old = nullptr;                       // one per mover: the posed capsule before the last advance (the build writes it)
    // the lookup grid, allocated once for the largest grid (kMoverGridMaxDim^2 cells): the masks (cells * words 64-bit
    // words), the summary (cells 32-bit words) and one 64-bit word `listed`, laid out for the view of the last build
    unsigned char *grid = nullptr;
    uint32_t words = 0;                          // mask words per cell: ceil(k / 64)
    uint64_t passes = 0;                         // passes enqueued since the last gpe_set_movers
    MoverGridView view;                          // the view of the last build
    bool built = false;                          // false: no pass has built a grid yet
    MoverLimits limits;                          // the dt contract's side of the set (k_mover.h)
};

struct MoverBuildArgs {
    const MoverDef *def = nullptr;
    float *pose = nullptr;
    float4 *rec = nullptr;
    float4 *old = nullptr;                       // with surfaces: the capsule before the advance, one per mover; else null
    uint32_t k = 0, words = 0;
    MoverGridView g;
    float rb = 0.f, dt = 0.f;
    unsigned long long *masks = nullptr;
    uint32_t *summary = nullptr;
    unsigned long long *listed = nullptr;
};

struct MoverPassArgs {
    const unsigned long long *masks = nullptr;   // view.gx * view.gy * words
    const uint32_t *summary = nullptr;           // view.gx * view.gy
    const float4 *rec = nullptr;                 // 2 per mover
    uint32_t k = 0, words = 0;
    ColliderGridView view;
    float world_w = 0.f, world_h = 0.f;
    unsigned long long *pushed = nullptr;
    const float4 *surf = nullptr;                // the surface form: one row per mover (e, mu, flags, reserved), ...
    const float4 *old = nullptr;                 // ... the capsules before the advance ...
    float2 *prev = nullptr;                      // ... and the previous positions it rewrites under a hit
};

// the sweep of the movers (gpe_set_mover_sweep; gpe_movers.hip, k_mover_sweep.hip, k_mover_sweep.h).  A mode of their
// pass, like gravity: not part of MoverState, so a new mover set leaves it alone.  The three buffers are allocated when
// the mode is first switched on, for kMoversMax movers, and kept until gpe_destroy
struct MoverCarry;
struct MoverSweepState : SweepState {
    MoverCarry *carry = nullptr;                 // kMoversMax: what each mover carries a point by in the last step
    float4 *old = nullptr;                       // kMoversMax: the posed capsules before the last advance
};

// what the swept build and the swept pass take beside MoverBuildArgs / MoverPassArgs (P.old, P.surf and P.prev as there)
struct MoverSweepArgs {
    MoverCarry *carry = nullptr;                 // one per mover: written by the build, read by the pass
    float2 *prev = nullptr;                      // the pass: read for every particle, written where a surface acted
    unsigned long long *counts = nullptr;        // the pass: two words, swept and stopped
};

struct SortWorkspace {
    uint32_t *keys_b = nullptr, *vals_b = nullptr;   // ping-pong partners, cap entries each
    uint64_t cap = 0;
    uint32_t *counts = nullptr;                      // [256][tiles] per-tile digit counts
    uint64_t counts_cap = 0;
    uint32_t *hist4 = nullptr;                       // 4 x 256 global digit histograms
};

struct OnesweepWorkspace {
    uint64_t *status = nullptr;      // [tiles][256] {epoch:30, flag:2, value:32}
    uint64_t status_cap = 0;
    uint32_t *hist4 = nullptr;       // 4 x 256 digit histograms
    uint32_t *bases4 = nullptr;      // 4 x 256 exclusive digit bases
    uint32_t *hist_plain = nullptr;  // 4 x 256: histograms of the sorts whose producer brings none
    uint32_t *ctl = nullptr;         // [0..3] tile tickets per pass, [4] error word
    uint32_t epoch = 0;
    bool hist_clean = false;         // the set the next native step adds into is zero: the native step keeps it so
    uint32_t hist_set = 0;           // which of the two sets of copies that is
};

// Straggler lists, ghost lists and rosters are indexed by the tile's position in the TILE BOX of the run: the whole cell
// box, or a sharded rank's active box (so that their memory follows the rank's share of the world, not the world).
struct TileBox {
    int32_t x0 = 0, y0 = 0, nx = 0, ny = 0;     // first tile (32x32 cells), tiles per row / column
    __host__ __device__ __forceinline__ bool holds(int tx, int ty) const { return tx >= x0 && ty >= y0 && tx < x0 + nx && ty < y0 + ny; }
    __host__ __device__ __forceinline__ uint32_t index(int tx, int ty) const { return (uint32_t)(ty - y0) * (uint32_t)nx + (uint32_t)(tx - x0); }
};
// pinned host words the native kernels report to (NativeState::host_stat; read by the step policy and by
// gpe_get_pipeline_info with a lag of the steps in flight)
constexpr int kStatWindowMax = 0;              // largest 24x24-cell window population of the last native step
constexpr int kStatArena = 1;                  // spill-arena slots handed out by the last native step
constexpr int kStatProbe = 2;                  // window population measured by the last asynchronous probe + 1 (0: none yet)
constexpr int kStatOverflow = 3;               // 32x32 tiles over capacity in the last native step
constexpr int kStatSubTiles = 4, kStatSpills = 5;   // quarters redone as 8x8 tiles / 8x8 tiles through the arena (diagnostics)
constexpr int kStatSorts = 6;                  // running count of steps whose radix passes ran (tile_ctl[kCtlSorts]), lagged
constexpr int kStatOverflowNew = 7;            // ... of kStatOverflow, the tiles the dense launch handed on itself (the others were known: hinted)
constexpr int kStatHalvesOver = 8;             // halves handed on to the over-capacity launch in the last native step
constexpr int kNativeCtlSorts = 14;         // tile_ctl word: running count of steps whose radix passes ran (native_launch.h kCtlSorts)
constexpr int kNativeCtlSortsSeen = 38;     // its copy in the line the tiles only read (native_launch.h kCtlSortsSeen)
// Native (N-key sort + LDS cell windows) pipeline state
struct NativeState {
    NativePolicy policy;             // the launch heuristics and their counters (native_policy.h)
    bool in_box = false;             // the configuration-time box check passed (density is the only possible obstacle)
    int32_t gx = 0, gy = 0;          // home cell columns / rows: cx in [0,gx), cy in [0,gy)
    int passes = 4;                  // radix passes needed for morton(gx-1, gy-1)
    uint32_t table_entries = 0;      // 8x8-cell block table length
    uint2 *block_table = nullptr;    // [morton >> 6] = (start, end) in the sorted order
    uint64_t table_cap = 0;
    uint32_t *keys = nullptr, *ids = nullptr;       // N each: hash output / sort ping
    uint32_t *keys_b = nullptr, *ids_b = nullptr;   // sort pong
    uint64_t cap = 0;
    uint32_t *codes = nullptr;       // per particle: cell relative to its sorted block | neighbour overlap mask | straggler (k_native_hash)
    uint32_t *gkeys = nullptr, *gids = nullptr, *gkeys_b = nullptr, *gids_b = nullptr;   // sharded runs: the ghosts' sort
    uint64_t gcap = 0;
    uint2 *gtable = nullptr;         // ... and their block table
    uint32_t *ghist = nullptr;       // ... and its digit histograms (two sets of kHistCopies copies, like os_ws.hist4)
    uint32_t ghist_set = 0;
    uint64_t gtable_cap = 0;
    const uint32_t *gsorted_ids_now = nullptr;   // the ghosts' indices in block order, this step (NULL: no ghost table)
    uint32_t *exc_count = nullptr;   // straggler lists: [2][exc_tiles] counts, then [2][exc_tiles][16] entries (one allocation)
    uint2 *exc_entry = nullptr;
    uint64_t exc_tiles = 0, exc_cap = 0;
    uint4 *roster_hdr = nullptr;           // tile rosters (native_launch.h, CollideArgs)
    uint32_t *roster_ids = nullptr;
    uint64_t roster_cap = 0;
    TileBox tb;                      // the tiles the straggler lists, ghost lists and rosters are kept for
    uint32_t *gho_count = nullptr;   // sharded runs: ghost lists, [2][exc_tiles] counts then [2][exc_tiles][kGhostSlots] ids
    uint64_t gho_cap = 0;
    const uint32_t *gho_count_now = nullptr, *gho_entry_now = nullptr, *ghost_sort_now = nullptr;   // what this step's tiles read
    const uint32_t *exc_count_now = nullptr;   // the set the current step's tiles read (NULL: the step sorts anyway)
    const uint2 *exc_entry_now = nullptr;
    uint32_t *sorted_key = nullptr;  // per particle: the block key it had when the radix passes last ran (written by their
                                     // first pass); the sorted ids and the block table describe that grouping
    bool sort_state_valid = false;   // sorted_key / sorted ids / block table belong to the current particle set and box
    uint64_t sorted_n = 0;           // ... of this many particles
    uint32_t step_seq = 0;           // native_prepare_step calls: its parity selects the per-step control words
    uint32_t collide_seq = 0;        // native_collide calls: numbers the dense launches for the tile hints (native_launch.h kCtlHints)
    const uint32_t *fresh_word = nullptr;   // tile_ctl word the tiles of the current step read (did the passes run?)
    uint32_t reason = GPE_REASON_NO_PARTICLES;   // why the native kernels do not run (GPE_REASON_*), NONE when they do
    uint64_t native_steps = 0, compat_steps = 0;
    bool always_sort = false;        // GPE_FLAG_SORT_EVERY_STEP (A/B measurements, tests): sort every step as rounds 1-2 did
    // Every radius was this one number, in plain_radius_lanes' range [1e-30, 1e30], when native_configure last looked
    // (every entry point that changes radii comes through it), and nothing has been able to change one since: the step
    // runs the kernels that take it as a constant.  Off on sharded contexts (order keys, an active box), once
    // gpe_device_ptr(GPE_RADIUS) has been handed out (native_radius_exposed) and under GPE_FLAG_GENERAL_RADII.
    bool uniform = false;
    float uniform_r = 0.0f;
    int32_t blocks_x = 0, blocks_y = 0;   // 8x8-cell blocks of the block box: table index = (by - by0) * blocks_x + (bx - bx0)
    int32_t bx0 = 0, by0 = 0;        // first block of the box (sharded runs: the rank's active box; else 0, 0)
    uint32_t *tile_ctl = nullptr;    // device control words (native_launch.h kCtl*)
    uint32_t *overflow1 = nullptr;   // packed (ty << 16 | tx) of 32x32 tiles over capacity
    uint64_t overflow_cap = 0;
    void *arena = nullptr;           // global spill arena for those tiles' particle arrays (37 B per slot)
    uint64_t arena_cap = 0;          // slots
    bool force = false;              // GPE_FLAG_NATIVE_FORCE (tests): no hand-over to the compat kernels
    bool print_stats = false;        // GPE_FLAG_NATIVE_STATS: print the step statistics every 128 steps
    uint32_t stat_calls = 0;
    uint32_t *host_stat = nullptr;   // pinned, 16 words (kStat* above): window maximum, arena use, probe answer, overflow tiles
    uint32_t window_max = 0;         // the same, measured synchronously at configuration time
    unsigned long long *dbg_stamps = nullptr;    // diagnostic builds (-DGPE_TILE_STAMPS / -DGPE_TILE_CYCLES): their device buffers
    uint4 *dbg_cycles = nullptr;
    uint64_t dbg_cycles_cap = 0;
};

// Device-resident halo exchange of a sharded run (k_shard.hip): particle counts live on the device, the host
// only keeps an upper bound.  Slots = the neighbouring ranks in ascending order, then this rank itself.
constexpr int kShardMaxSlots = 9;
// counts[] words.  Two sets of them (kShardSetWords apart), alternating with every unpack: the unpack kernel reads the
// old set in all its workgroups while one of them writes the new one.  The error word is sticky and shared: always
// word kShardError of set 0.
constexpr int kShardOwned = 0, kShardTotal = 1, kShardError = 2, kShardEpoch = 3, kShardHoles = 4;
constexpr int kShardSetWords = 8;
constexpr int kShardDoneTicket = 5;              // set 0: workgroups of the unpack launch that are through (the last one resets the send headers)
struct ShardSlots {                  // passed to the kernels by value
    uint32_t n_slots;
    uint32_t rank[kShardMaxSlots];
    uint32_t send_off[kShardMaxSlots], send_cap_mig[kShardMaxSlots], send_cap_gho[kShardMaxSlots];
    uint32_t recv_off[kShardMaxSlots], recv_cap_mig[kShardMaxSlots], recv_cap_gho[kShardMaxSlots];
    int8_t slot_of_rank[32];
};
constexpr uint32_t kShardErrSendOverflow = 1u;   // more rows for a neighbour than its segment takes
constexpr uint32_t kShardErrNoSlot = 2u;         // a particle needs a rank that is not a neighbour (moved > 1 block)
constexpr uint32_t kShardErrCapacity = 4u;       // owned + ghosts exceed the particle capacity
constexpr uint32_t kShardErrHoles = 8u;          // more migrants in one step than the hole list takes
constexpr uint32_t kShardErrRecvOverflow = 16u;  // a received header claims more rows than the segment holds
constexpr int kSegHeader = 4;                    // words: [n_migrants, n_ghosts, 0, 0]
constexpr int kMigWords = 6, kGhoWords = 4;      // migrant row: x y prev_x prev_y r key; ghost row: x y r key

// rows of one (slot, kind): a wave-aggregated append; every lane of the wave must call it
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool want)
{
    const uint64_t m = ballot64(want);
    if (m == 0) return 0xFFFFFFFFu;
    const int leader = (int)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    return want ? base + popc_below_lane(m) : 0xFFFFFFFFu;
}

// What a particle's NEW position means for the neighbours (k_shard.hip, "pack"): the owner of its block takes it over
// when that is another rank (a migrant: listed as a hole here), and every rank within one block of it gets a ghost copy.
// Shared by the pack kernel (k_shard_pack: all owned particles, the first pack of a run) and by the tiles of the
// native step, which pack their own particles as they write them back (k_native.hip: the pack kernel then never runs).
struct PackArgs {
    const uint8_t *owner = nullptr;              // gpe_shard_plan tables over the global block grid
    const uint32_t *dest_mask = nullptr;
    int32_t blocks_x = 0, blocks_y = 0;
    uint32_t my_rank = 0;
    uint32_t *send = nullptr, *counts = nullptr, *holes = nullptr;   // counts: the set in use (kShardOwned, kShardHoles)
    uint32_t *err = nullptr;                     // the sticky error word
    uint8_t *hole_flag = nullptr;
    uint32_t holes_cap = 0;
    // the tiles: a new position inside the `safe` box (world units: the rank's rectangle shrunk by one block + one cell on
    // every side that has a neighbour) concerns no other rank -- its block is this rank's and borders nobody
    float safe_x0 = 0.f, safe_y0 = 0.f, safe_x1 = 0.f, safe_y1 = 0.f;
    uint32_t on = 0;                             // 1: pack; 2: this launch runs behind the exchange -- a particle that would
                                                 // have to be packed is an error (it moved more than a block in one step)
    ShardSlots slots;
};

// mine: this lane holds an owned particle (local index i, new position p, previous position q).  Every lane of the
// wave must call it (ballots).
__device__ __forceinline__ void pack_particle(const PackArgs &P, const bool mine, const uint32_t i, const float2 p,
                                              const float2 q, const float rad, const uint32_t key, const float cell_size)
{
    uint32_t gho = 0;
    int mig = -1;
    if (mine) {
        int bx = cell_coord(p.x, cell_size) >> 3, by = cell_coord(p.y, cell_size) >> 3;
        bx = min(max(bx, 0), P.blocks_x - 1);
        by = min(max(by, 0), P.blocks_y - 1);
        const uint32_t b = (uint32_t)by * (uint32_t)P.blocks_x + (uint32_t)bx;
        const uint32_t owner = P.owner[b];
        gho = P.dest_mask[b] & 0x03FFFFFFu;             // ranks within one block of b, its owner excluded
        if (owner != P.my_rank) mig = (int)owner;       // b's owner takes the particle over
    }
    if (ballot64(gho != 0 || mig >= 0) == 0) return;    // interior wave
    uint32_t err = 0;
    {
        const uint32_t h = wave_append(&P.counts[kShardHoles], mig >= 0);
        if (mig >= 0) {
            if (h < P.holes_cap) { P.holes[h] = i; P.hole_flag[i] = 1; } else err |= kShardErrHoles;
            if (P.slots.slot_of_rank[mig & 31] < 0) err |= kShardErrNoSlot;
        }
    }
    uint32_t served = 0;
    for (uint32_t s = 0; s < P.slots.n_slots; ++s) {
        const uint32_t rk = P.slots.rank[s];
        uint32_t *seg = P.send + P.slots.send_off[s];
        const bool wm = mig == (int)rk;
        const bool wg = ((gho >> rk) & 1u) != 0;
        served |= wg ? (1u << rk) : 0u;
        const uint32_t rm = wave_append(seg + 0, wm);
        if (wm) {
            if (rm < P.slots.send_cap_mig[s]) {
                uint32_t *row = seg + kSegHeader + (uint64_t)rm * kMigWords;
                row[0] = __float_as_uint(p.x); row[1] = __float_as_uint(p.y);
                row[2] = __float_as_uint(q.x); row[3] = __float_as_uint(q.y);
                row[4] = __float_as_uint(rad); row[5] = key;
            } else err |= kShardErrSendOverflow;
        }
        const uint32_t rg = wave_append(seg + 1, wg);
        if (wg) {
            if (rg < P.slots.send_cap_gho[s]) {
                uint32_t *row = seg + kSegHeader + (uint64_t)P.slots.send_cap_mig[s] * kMigWords + (uint64_t)rg * kGhoWords;
                row[0] = __float_as_uint(p.x); row[1] = __float_as_uint(p.y);
                row[2] = __float_as_uint(rad); row[3] = key;
            } else err |= kShardErrSendOverflow;
        }
    }
    if (gho & ~served) err |= kShardErrNoSlot;
    if (err) atomicOr(P.err, err);
}

struct ShardState {
    bool on = false;                 // gpe_shard_configure was called
    bool active = false;             // between gpe_shard_begin and gpe_shard_counts: counts are on the device
    bool packed = false;             // the send buffer holds this step's rows
    bool have_rect = false;          // the plan told the rank's rectangle: the tiles of the step pack (no pack kernel)
    int32_t rect[4] = {0, 0, 0, 0};  // own rectangle in blocks, half-open: x0, y0, x1, y1
    uint32_t my_rank = 0;
    int32_t blocks_x = 0, blocks_y = 0;          // global block grid of the decomposition
    const uint8_t *owner = nullptr;              // caller's device tables (gpe_shard_plan)
    const uint32_t *dest_mask = nullptr;
    uint32_t *send = nullptr, *recv = nullptr;   // caller's device buffers
    ShardSlots slots;
    uint32_t *counts = nullptr;      // device, two sets of kShardSetWords words (kShard*)
    uint32_t parity = 0;             // the set in use: counts + parity * kShardSetWords (flips with every unpack)
    uint32_t *counts_now() const { return counts + parity * kShardSetWords; }
    uint32_t *host_counts = nullptr; // pinned mirror written by the unpack kernel
    uint32_t *holes = nullptr, *fill_src = nullptr, *fill_dst = nullptr;   // device, holes_cap each
    uint8_t *hole_flag = nullptr;    // device, one byte per particle slot
    uint64_t holes_cap = 0, flag_cap = 0;
    uint32_t begin_epoch = 0;        // epoch value at the last gpe_shard_begin
    uint64_t steps = 0;
    hipEvent_t fence[2] = {nullptr, nullptr};
    bool armed[2] = {false, false};
    // Exchange beside the step (round 4): the segments move on a stream of their own as soon as the tiles along the rank's
    // border have packed (ev_packed, recorded on the context's stream), while the interior tiles are still being resolved;
    // the next unpack waits for ev_exchanged.  overlap == false: everything on the context's stream, in order (rounds 1-3).
    bool overlap = false;
    hipStream_t xstream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_exchanged = nullptr;
    bool packed_recorded = false, exchanged_recorded = false;
    hipStream_t exchange_stream(hipStream_t main) const { return overlap && xstream ? xstream : main; }
    // moving the segments between ranks (gpe_comm.hip): an RCCL communicator or a caller-supplied transport
    void *comm = nullptr;            // ncclComm_t
    bool comm_owned = false;
    gpe_shard_transport_fn transport = nullptr;
    void *transport_user = nullptr;
};

// The sharded run's control plane (gpe_shard_ctl.hip): the decomposition this context is a rank of, the tables and
// segment buffers it owns, and who carries its collectives.
struct ShardCtl {
    bool ready = false;              // gpe_shard_setup has run
    bool home = false;               // every particle sits on its owner, counts on the host, ghosts dropped
    gpe_shard_layout layout;
    uint32_t rank = 0;
    float scale = 1.0f;              // capacity_scale of the neighbour segments
    double planned_per_block = 0.0;  // block population the segments were sized for
    uint8_t *d_owner = nullptr;      // library-owned device tables (gpe_shard_plan)
    uint32_t *d_mask = nullptr;
    uint64_t tables_cap = 0;         // blocks
    uint32_t *d_send = nullptr, *d_recv = nullptr;
    uint64_t send_cap = 0, recv_cap = 0;          // words allocated
    // the neighbour exchange spelled as an all-to-all (word offsets / counts per rank; zero for non-neighbours)
    uint64_t x_send_off[GPE_SHARD_MAX_RANKS] = {}, x_send_cnt[GPE_SHARD_MAX_RANKS] = {};
    uint64_t x_recv_off[GPE_SHARD_MAX_RANKS] = {}, x_recv_cnt[GPE_SHARD_MAX_RANKS] = {};
    uint32_t n_neighbours = 0;
    gpe_shard_collectives coll;      // caller-supplied collectives
    bool coll_set = false;
    gpe_local_group *group = nullptr;   // local group this context is a rank of
    uint32_t group_rank = 0;
    uint32_t *d_small = nullptr;     // device scratch for the small host-side collectives (kCtlSmallWords)
    uint32_t *d_hist = nullptr, *d_first = nullptr;   // re-sort: Morton-block histogram / first local index
    uint64_t hist_cap = 0;
    uint32_t *d_rows_send = nullptr, *d_rows_recv = nullptr;   // re-cut: particle rows on the move
    uint64_t rows_send_cap = 0, rows_recv_cap = 0;
    uint64_t resorts = 0, steps = 0, n_ghost = 0;
    uint32_t recuts = 0;
};
constexpr uint64_t kCtlSmallWords = 4096;

// Device memory (gpe_api.hip, "device memory"): every allocation of a context is in its registry.
struct DevAlloc {
    void *ptr = nullptr;             // what the owner holds: the payload's first byte
    void *base = nullptr;            // what the runtime returned (== ptr unless guarded)
    uint64_t payload = 0, slack = 0; // bytes kernels may write / bytes behind them that may only be read
    uint64_t total = 0;              // bytes allocated at base
    const char *tag = "";            // a string literal
};
constexpr uint64_t kGuardZone = 16384;   // bytes of a red zone at least: kHashBlock = 1024 lanes x a 16-byte store
struct GuardState {
    bool on = false;                 // GPE_FLAG_GUARD_ALLOCS
    uint32_t canary = 0, poison = 0; // gpe_config.guard_canary / guard_poison
    std::vector<DevAlloc> live;
    std::vector<DevAlloc> pinned;    // pinned host blocks the registry lists (state "pinned"): never scanned, one entry per block that exists
    std::vector<DevAlloc> released;  // guarded: one entry per tag that has been released, the last such allocation (ptr = base = NULL)
    hipError_t scan_failed = hipSuccess;   // a check at release could not run: that buffer's evidence is lost (sticky)
    std::vector<gpe_guard_zone> kept;   // damage found when a buffer was released (the first GPE_GUARD_MAX_ZONES)
    uint32_t kept_count = 0;
};

}  // namespace gpe

struct gpe_ctx {
    gpe_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;        // the stream every kernel, copy and RCCL call of this context goes to
    hipStream_t own_stream = nullptr;    // created by gpe_create; `stream` is either this or one lent by gpe_set_stream
    std::string last_error;

    uint64_t n = 0;          // particles taking part in collisions (owned + ghosts in a sharded run)
    uint64_t n_owned = 0;    // the first n_owned are integrated by K12 (== n unless sharded)
    uint64_t cap = 0;        // allocated particle capacity
    float max_radius = 0.f;  // ParticleSystem::max_radius
    float grid_max_radius = 0.f;
    float cell_size = 0.f;
    int32_t mouse_pressed = 0;
    float mouse_x = 0.f, mouse_y = 0.f;

    // particle_buffers.rs:4-10, two sets (particle_system.rs:17-18); colours are render-only
    float2 *pos = nullptr, *prev = nullptr;
    float *radius = nullptr;
    float2 *pos_copy = nullptr, *prev_copy = nullptr;
    float *radius_copy = nullptr;
    uint32_t *home_cell_ids = nullptr, *particle_ids = nullptr;   // particle_sort.rs:29-33
    // grid.rs:36-40 GridBuffers (4 slots per particle)
    uint32_t *cell_ids = nullptr, *object_ids = nullptr;
    // collision_cell_buffers.rs:6-10
    uint32_t *chunk_obj_count = nullptr;   // ceil(4n/4) = n entries
    uint32_t *collision_cells = nullptr;   // 4n entries
    uint32_t *indirect_args = nullptr;     // 3 entries (+1: K)
    // sharded runs: global object index of every local particle (in-cell order), active cell box
    uint32_t *order_keys = nullptr;
    bool use_order_keys = false;
    bool has_active_box = false;
    int32_t active_box[4] = {0, 0, 0, 0};   // cx0, cy0, cx1, cy1 (inclusive) holding this rank's particles

    gpe::SortWorkspace sort_ws;
    gpe::RemoveWorkspace remove_ws;
    gpe::UidState uid;
    gpe::TracerState tracers;
    gpe::MonitorState monitor;
    gpe::ColliderState colliders;
    gpe::SweepState sweep;
    gpe::BondState bonds;
    gpe::BondSolverState bond_solver;
    gpe::BendState bends;
    gpe::BendSolverState bend_solver;
    gpe::AreaState areas;
    gpe::BodyState bodies;
    gpe::FieldState fields;
    gpe::MoverState movers;
    gpe::MoverSweepState mover_sweep;
    gpe::QueryWorkspace query_ws;
    gpe::ContactsWorkspace contacts_ws;
    gpe::ClustersWorkspace clusters_ws;
    gpe::RayWorkspace ray_ws;
    gpe::NearestWorkspace nearest_ws;
    gpe::EditWorkspace edit_ws;
    gpe::SpawnWorkspace spawn_ws;
    gpe::ScanWorkspace scan_ws;
    gpe::OnesweepWorkspace os_ws;
    gpe::NativeState native;
    gpe::ShardState shard;
    gpe::ShardCtl ctl;
    gpe::GuardState guard;
    bool use_onesweep = true;        // GPE_SORT=safe selects the reduce-then-scan sort

    // profiling
    bool profiling = false;          // scopes record events now
    uint32_t profile_every = 0;      // 0 off, 1 every call, k > 1: every k-th step (gpe_set_profiling)
    uint64_t profile_step = 0;
    std::vector<gpe::ScopeStat> stats;
    // The scopes' boundaries: pool, pending pairs, shared boundaries.  On the context's own stream they are timestamp
    // slots (scope_stamps); on a stream lent by gpe_set_stream, or under GPE_FLAG_EVENT_SCOPES, events (scope_events).
    gpe::ScopeEvents<gpe::HipScopeBackend> scope_events;
    gpe::StampBackend<gpe::HipStampDev> stamp_be;
    gpe::ScopeEvents<gpe::StampRecorder<gpe::HipStampDev>> scope_stamps;
    double stamp_khz = 0.0;                       // the timestamp counter's rate (hipDeviceAttributeWallClockRate)
    bool stamp_origin = false;                    // slot 0 holds the trace origin
    hipEvent_t trace_origin = nullptr;            // recorded when profiling is switched on / timings are reset
    uint32_t *err_words = nullptr;                // pinned, 16 words: check_device_errors reads the sticky error words into it
    std::vector<gpe::TraceEvent> trace;           // the last kTraceCap resolved scopes, oldest first
};

namespace gpe {

// error plumbing -----------------------------------------------------------------------------
gpe_status fail(gpe_ctx *ctx, gpe_status code, const std::string &msg);
#define GPE_HIP(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (void)hipGetLastError(); /* reported here: not left for the next launch check */    \
            return gpe::fail((ctx), _e == hipErrorOutOfMemory ? GPE_ERR_OOM : GPE_ERR_HIP,      \
                             std::string(#expr) + ": " + hipGetErrorName(_e) + " (" +           \
                                 hipGetErrorString(_e) + ")");                                  \
        }                                                                                       \
    } while (0)
#define GPE_TRY(expr)                                                                           \
    do {                                                                                        \
        gpe_status _s = (expr);                                                                 \
        if (_s != GPE_OK) return _s;                                                            \
    } while (0)

// device memory -----------------------------------------------------------------------------
// The one allocator of device memory (gpe_api.hip).  payload_bytes: what kernels may write; slack_bytes: room behind it
// that may only be read (stated at the call site with its reader).  Unguarded the allocation is payload + slack bytes;
// guarded (GPE_FLAG_GUARD_ALLOCS) it is front zone | payload | rear zone, the slack inside the rear zone.  *ptr must not
// hold a live allocation (it is overwritten; NULL after a failure).  A failure leaves no sticky HIP error behind.
hipError_t gpe_dev_reserve(gpe_ctx *c, void **ptr, uint64_t payload_bytes, uint64_t slack_bytes, const char *tag);
// Frees *ptr (NULL: nothing) and forgets it.  Guarded: synchronises the context's streams and checks the zones first.
hipError_t gpe_dev_release(gpe_ctx *c, void **ptr);
template <class T>
inline hipError_t dev_reserve(gpe_ctx *c, T **p, uint64_t payload_bytes, uint64_t slack_bytes, const char *tag)
{
    return gpe_dev_reserve(c, (void **)p, payload_bytes, slack_bytes, tag);
}
template <class T>
inline hipError_t dev_release(gpe_ctx *c, T *&p)
{
    return gpe_dev_release(c, (void **)&p);
}

// the API's host side (gpe_api.hip, gpe_queries.hip, gpe_edits.hip, gpe_observe.hip): what the four files share ----
// One workspace buffer: payload exactly count elements, slack as stated at the call with its reader.  A failure reads
// "<who>: out of device memory" (or what `oom` says instead) / "<who>: <hipGetErrorName>".
template <typename T>
gpe_status ws_alloc(gpe_ctx *c, const char *who, T **p, uint64_t count, uint64_t slack_bytes, const char *tag,
                    const char *oom = "out of device memory")
{
    const hipError_t e = dev_reserve(c, p, count * sizeof(T), slack_bytes, tag);
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, std::string(who) + ": " + oom);
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string(who) + ": " + hipGetErrorName(e));
    return GPE_OK;
}

template <typename T>
gpe_status dev_alloc(gpe_ctx *c, T **p, uint64_t count, const char *tag)
{
    // payload: count elements.  slack: the round-up to 4 elements and 64 bytes -- no kernel is known to read them; they
    // keep the unguarded allocation at the size it always had (max(count, 4) * sizeof(T) + 64)
    // ("hipMalloc" is no caller's name: it keeps the text dev_alloc's failures always had, "hipMalloc: ...")
    const uint64_t payload = count * sizeof(T);
    return ws_alloc(c, "hipMalloc", p, count, std::max<uint64_t>(count, 4) * sizeof(T) + 64 - payload, tag);
}

template <typename T>
void dev_free(gpe_ctx *c, T *&p)
{
    (void)dev_release(c, p);
}

// The device calls behind SetUpload (set_upload.h), on the context's stream: tables through ws_alloc / dev_free, so tags,
// messages and guard zones are what they are everywhere.  A failing copy, fill or wait reads "<who>: <stage>: <hip name>".
struct HipUploadBackend {
    using Status = gpe_status;
    gpe_ctx *c;
    std::string &last_error() { return c->last_error; }
    gpe_status reserve(const char *who, void **p, uint64_t bytes, const char *tag) { return ws_alloc(c, who, (uint8_t **)p, bytes, 0, tag); }
    void release(void *p) { dev_free(c, p); }
    gpe_status done(const char *who, const char *stage, hipError_t e)
    {
        if (e == hipSuccess) return GPE_OK;
        (void)hipGetLastError();
        return fail(c, GPE_ERR_HIP, std::string(who) + ": " + (stage ? std::string(stage) + ": " : "") + hipGetErrorName(e));
    }
    gpe_status copy(const char *who, const char *stage, void *dst, const void *src, uint64_t bytes)
    {
        return done(who, stage, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    }
    gpe_status fill(const char *who, const char *stage, void *dst, int byte, uint64_t bytes)
    {
        return done(who, stage, hipMemsetAsync(dst, byte, bytes, c->stream));
    }
    gpe_status wait(const char *who, const char *stage) { return done(who, stage, hipStreamSynchronize(c->stream)); }
};
using HipSetUpload = SetUpload<HipUploadBackend>;

// A set's node table inside its upload transaction: the three tables reserved, the nodes and the rows copied, node_slot
// all ones (no node has a slot until the first pass looks them up).  The tags are literals, as everywhere: the registry
// keeps the pointers
inline void node_table_upload(HipSetUpload &up, UidNodeTable *T, const std::vector<uint32_t> &nodes,
                              const std::vector<uint32_t> &row_start, const char *node_uid_tag,
                              const char *node_slot_tag, const char *row_start_tag)
{
    const uint64_t m = nodes.size();
    up.reserve(&T->node_uid, m, node_uid_tag);
    up.reserve(&T->node_slot, m, node_slot_tag);
    up.reserve(&T->row_start, m + 1, row_start_tag);
    up.copy(T->node_uid, nodes.data(), m);
    up.copy(T->row_start, row_start.data(), m + 1);
    up.fill(T->node_slot, 0xff, m * sizeof(uint32_t));
    T->nodes = m;
    T->stale = true;
}
inline void node_table_free(gpe_ctx *c, UidNodeTable &T)
{
    dev_free(c, T.node_uid); dev_free(c, T.node_slot); dev_free(c, T.row_start);
}

// The 256-byte aligned staging layout of a result's requested parts: part() = the offset of the next part, which takes
// room only when it is requested; bytes = what the parts so far take.
struct StageLayout {
    uint64_t bytes = 0;
    uint64_t part(bool on, uint64_t len)
    {
        const uint64_t at = bytes;
        if (on) bytes += (len + 255) / 256 * 256;
        return at;
    }
};

constexpr uint64_t kUidLimit = 1ull << 32;                     // next_uid may reach 2^32: then no particle can be added
inline bool is_sharded(const gpe_ctx *c) { return c->shard.on || c->use_order_keys || c->has_active_box; }

// the refusals several entry points word alike (gpe_api.hip): fail() with "<who>: ..."
gpe_status refuse_sharded(gpe_ctx *c, const char *who);             // GPE_ERR_UNSUPPORTED: is_sharded(c)
gpe_status refuse_too_many(gpe_ctx *c, const char *who);            // GPE_ERR_UNSUPPORTED: more than 2^32 - 1 particles
gpe_status refuse_uid_off(gpe_ctx *c, const char *who);             // GPE_ERR_STATE: a uid output while uids are off
gpe_status refuse_radius_not_finite(gpe_ctx *c, const char *who);   // GPE_ERR_UNSUPPORTED
// GPE_ERR_UNSUPPORTED: the context holds <sets>, which <setter> with k = 0 clears (the one wording of every such refusal)
gpe_status refuse_holds(gpe_ctx *c, const char *who, const char *sets, const char *setter);
// gpe_api.hip
gpe_status need_particles(gpe_ctx *c);
// the sticky device-side error words; synchronises the context's stream once (wait_exchange: and the exchange stream, once)
gpe_status check_device_errors(gpe_ctx *c, bool wait_exchange = false);
gpe_status error_words_reserve(gpe_ctx *c);        // gpe_native.hip: c->err_words, once per context
void error_words_release(gpe_ctx *c);
gpe_status grow_particle_buffers(gpe_ctx *c, uint64_t cap);
gpe_status init_index_buffers(gpe_ctx *c, uint64_t lo, uint64_t hi);
// `bytes` from the device into host memory, then the sticky error words (that synchronises the stream)
inline gpe_status read_back(gpe_ctx *c, const void *device_ptr, void *host_ptr, uint64_t bytes)
{
    GPE_HIP(c, hipMemcpyAsync(host_ptr, device_ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    return check_device_errors(c);
}
// a get call of a set the host keeps: *k = its size, its first min(k, capacity) rows to out
template <typename T>
gpe_status rows_out(const std::vector<T> &set, T *out, uint64_t capacity, uint64_t *k)
{
    *k = set.size();
    const uint64_t m = std::min<uint64_t>(set.size(), capacity);
    if (m) memcpy(out, set.data(), m * sizeof(T));
    return GPE_OK;
}
// The storage order or the uids have changed: whatever keeps storage slots by uid looks them up again before its next use
inline void uid_slots_stale(gpe_ctx *c) { c->tracers.stale = c->bonds.nt.stale = c->bends.nt.stale = c->areas.nt.stale = c->bodies.stale = true; }
void refresh_cell_size(gpe_ctx *c);
gpe_status reconfigure(gpe_ctx *c);
gpe_status uid_map_ready(gpe_ctx *c);
gpe_status uid_query_reserve(gpe_ctx *c, uint64_t bytes);
// gpe_queries.hip (the region words of the circle and box calls are shared with the kicks), gpe_edits.hip
void query_release(gpe_ctx *c);
void contacts_release(gpe_ctx *c);
void clusters_release(gpe_ctx *c);
void ray_release(gpe_ctx *c);
void nearest_release(gpe_ctx *c);
void spawn_release(gpe_ctx *c);
void edit_release(gpe_ctx *c);
gpe_status circle_region(gpe_ctx *c, const char *who, float x, float y, float radius, float (&region)[5]);
gpe_status box_region(gpe_ctx *c, const char *who, float x0, float y0, float x1, float y1, float (&region)[5],
                      bool *empty);
// gpe_observe.hip: the tracers and the monitor of an armed context
gpe_status observers_after_step(gpe_ctx *c);       // after every step of gpe_step / gpe_run
void observers_release(gpe_ctx *c);
// The step sets (the X_after_step calls: see after_step, gpe_api.hip).
// gpe_colliders.hip: the static colliders of a context that holds some
inline bool has_colliders(const gpe_ctx *c) { return !c->colliders.set.empty(); }
gpe_status refuse_colliders(gpe_ctx *c, const char *who);   // GPE_ERR_UNSUPPORTED: sharding a context that holds colliders
gpe_status colliders_after_step(gpe_ctx *c);
void colliders_release(gpe_ctx *c);
// ... and the cell-list grid they share with the fields: G = the host tables under the two tags (synchronises); a
// failure reads "<who>: grid upload: ..." and leaves no grid, so the next pass tries again
void cell_grid_release(gpe_ctx *c, CellListGrid &G);
gpe_status cell_grid_upload(gpe_ctx *c, const char *who, CellListGrid &G, const ColliderGridView &view,
                            const std::vector<uint32_t> &cell_start, const std::vector<uint32_t> &items,
                            const char *cell_start_tag, const char *items_tag);
// gpe_sweep.hip: the swept form of that pass; the mode setter and the info getter it shares with the movers' sweep
gpe_status sweep_pass(gpe_ctx *c);                 // colliders_pass while the mode is on: the grid is ready
void sweep_release(gpe_ctx *c);
struct SweepTable { void **p; uint64_t bytes; const char *tag; };   // a buffer a mode keeps beside its counters
gpe_status sweep_mode_set(gpe_ctx *c, const char *who, SweepState &W, uint32_t mode, const char *tag,
                          std::initializer_list<SweepTable> more = {});
gpe_status sweep_mode_info(gpe_ctx *c, const char *who, const SweepState &W, gpe_sweep_info *info);
// gpe_surfaces.hip: the surfaces of the two sets; a new set drops its target's
void surfaces_drop(gpe_ctx *c, uint32_t target);   // GPE_SURFACES_OF_*: frees the rows, the next pass is the plain one
// The sets that name their particles by uid (uid_sets.h has what their entry points share; gpe_api.hip lists them in
// one table: their refusals, their passes behind a step, their release).  X_pass: one pass over the particles as they
// are now; X_release: the set and its tables go
inline bool has_bonds(const gpe_ctx *c) { return !c->bonds.set.empty(); }        // gpe_bonds.hip
gpe_status bonds_pass(gpe_ctx *c);
void bonds_release(gpe_ctx *c);
inline bool has_bends(const gpe_ctx *c) { return !c->bends.set.empty(); }        // gpe_bends.hip
gpe_status bends_pass(gpe_ctx *c);
void bends_release(gpe_ctx *c);
inline bool has_areas(const gpe_ctx *c) { return !c->areas.set.empty(); }        // gpe_areas.hip
gpe_status areas_pass(gpe_ctx *c);
void areas_release(gpe_ctx *c);
inline bool has_bodies(const gpe_ctx *c) { return !c->bodies.set.empty(); }      // gpe_bodies.hip
gpe_status bodies_pass(gpe_ctx *c);
void bodies_release(gpe_ctx *c);
// gpe_fields.hip: the force fields of a context that holds some
inline bool has_fields(const gpe_ctx *c) { return !c->fields.set.empty(); }
gpe_status refuse_fields(gpe_ctx *c, const char *who);      // GPE_ERR_UNSUPPORTED: sharding a context that holds fields
gpe_status fields_after_step(gpe_ctx *c, float dt);
void fields_world_changed(gpe_ctx *c);                      // gpe_set_world: the lookup grid follows before the next pass
void fields_release(gpe_ctx *c);

// gpe_movers.hip: the moving colliders of a context that holds some
inline bool has_movers(const gpe_ctx *c) { return !c->movers.set.empty(); }
gpe_status refuse_movers(gpe_ctx *c, const char *who);      // GPE_ERR_UNSUPPORTED: sharding a context that holds movers
gpe_status movers_check_dt(gpe_ctx *c, float dt, const char *who);  // GPE_ERR_INVALID_ARG: dt breaks the set's contract; before anything is launched
gpe_status movers_after_step(gpe_ctx *c, float dt);
void movers_release(gpe_ctx *c);
void mover_sweep_release(gpe_ctx *c);                       // gpe_destroy: the mode's counters and records
// The sharding entry points refuse a context that holds step sets: bonds, bodies, bends and areas (they name their particles by uid:
// the more telling refusal), then the call's own uid refusal when uids are on, then colliders, fields and movers
gpe_status refuse_step_sets(gpe_ctx *c, const char *who, const char *uid_refusal);

// profiling scope: a pair of timestamps on ctx->stream when ctx->profiling, else nothing -- slots of the stamp buffer
// (scope_stamps.h), or hipEvents where scope_uses_stamps() says no.  kSharedBoundaries: inside a ScopeRegion the scope
// takes the boundary a neighbouring scope recorded where nothing was enqueued between the two (scope_events.h); the
// timings and the trace read the same, a sampled step records fewer boundaries.
inline bool scope_uses_stamps(const gpe_ctx *c)
{
    return (c->cfg.flags & GPE_FLAG_EVENT_SCOPES) == 0 && c->stream == c->own_stream;
}
class Scope {
   public:
    enum Boundaries { kOwnEvents, kSharedBoundaries };
    // Timestamp slots, shared boundaries: the stamp of the scope's opening / closing is owed to the enqueue that
    // follows (scope_stamps.h) -- written by that launch's first workgroup when it is the hash or one of the two gated
    // sort kernels, by a kernel of its own right in front of it otherwise.  For boundaries whose next launch comes at once
    // and in front of short launches; without the hint a boundary is stamped at once, which is what the end of a long
    // kernel needs (the host must not delay it).  Timing only: the stamp lies between the same two launches either way.
    enum Carry : unsigned { kCarryNone = 0u, kCarryStart = 1u, kCarryStop = 2u };
    Scope(gpe_ctx *ctx, const char *name, Boundaries b = kOwnEvents, unsigned carry = kCarryNone);
    ~Scope();

   private:
    gpe_ctx *ctx_;
    int stat_ = -1;
    int start_ = -1;                 // slot of ctx->scope_events / ctx->scope_stamps
    bool shared_;
    bool stamps_ = false;
    unsigned carry_ = kCarryNone;
};
// Every enqueue onto c->stream inside a ScopeRegion says so (launches, async copies and memsets, event records other
// than the scopes' own): that is what lets two scopes there share a boundary event.
// A boundary's timestamp that is still owed is written first, by a kernel of its own (scope_stamps.h).
inline void note_enqueue(gpe_ctx *c)
{
    c->scope_events.note_enqueue();
    c->scope_stamps.note_enqueue();
    c->stamp_be.flush();
}
// For the launchers of the hash and of the two gated sort kernels, BEFORE their note_enqueue: where the kernel's first workgroup writes
// the owed timestamp (the kernel starts at that boundary), or NULL when none is owed.
inline unsigned long long *scope_stamp_for_next_launch(gpe_ctx *c)
{
    const int64_t slot = c->stamp_be.take();
    return slot < 0 ? nullptr : c->stamp_be.dev.buf + slot;
}
// A stretch of host code whose enqueues all call note_enqueue (native_collide).  Boundaries are never shared across
// its ends: the code outside enqueues without saying so.
class ScopeRegion {
   public:
    explicit ScopeRegion(gpe_ctx *c) : c_(c) { c_->scope_events.enter_region(); c_->scope_stamps.enter_region(); }
    ~ScopeRegion() { c_->stamp_be.flush(); c_->scope_events.leave_region(); c_->scope_stamps.leave_region(); }
    ScopeRegion(const ScopeRegion &) = delete;
    ScopeRegion &operator=(const ScopeRegion &) = delete;

   private:
    gpe_ctx *c_;
};

// kernel launchers (one translation unit each) --------------------------------------------------
// particles
gpe_status launch_home_cell_ids(gpe_ctx *c, const float2 *pos, uint64_t n, float cell_size,
                                uint32_t *home, uint32_t *ids);
gpe_status launch_rearrange(gpe_ctx *c, const float2 *pos, const float2 *prev, const float *radius,
                            const uint32_t *ids, uint64_t n, float2 *pos_out, float2 *prev_out,
                            float *radius_out);
gpe_status launch_verlet(gpe_ctx *c, float2 *pos, float2 *prev, const float *radius, uint64_t n,
                         float dt);
// grid
gpe_status launch_build_cell_ids(gpe_ctx *c, const float2 *pos, const float *radius, uint64_t n,
                                 float cell_size, uint32_t *cell_ids, uint32_t *object_ids);
// sort / scan
gpe_status sort_reserve(gpe_ctx *c, uint64_t n);
gpe_status sort_pairs(gpe_ctx *c, uint32_t *keys, uint32_t *vals, uint64_t n);
gpe_status sort_histogram(gpe_ctx *c, const uint32_t *keys, uint64_t n, uint32_t shift, uint32_t *hist256);
gpe_status sort_scatter_pass(gpe_ctx *c, const uint32_t *ka, const uint32_t *va, uint32_t *kb,
                             uint32_t *vb, uint64_t n, uint32_t shift);
gpe_status scan_reserve(gpe_ctx *c, uint64_t n);
gpe_status inclusive_scan(gpe_ctx *c, uint32_t *data, uint64_t n);
void sort_release(gpe_ctx *c);
void scan_release(gpe_ctx *c);
// onesweep (k_onesweep.hip)
constexpr int kHistCopies = 8;   // digit-histogram copies the hash kernel's workgroups flush into (same-line atomics serialise)
VerletParams verlet_params(const gpe_ctx *c, float dt);
gpe_status onesweep_reserve(gpe_ctx *c, uint64_t n);
void onesweep_release(gpe_ctx *c);
gpe_status onesweep_zero_hist(gpe_ctx *c);
// A sort that the device may skip (the native step, native_prepare_step): every pass returns at once when *need == 0.
// The first pass copies the keys in input order to key_copy and resets the block table (table_pairs uint4 entries),
// the last one sets *fresh and counts the sort.  Passed by value to the pass kernel.
struct OnesweepGate {
    const uint32_t *need = nullptr;
    uint32_t *key_copy = nullptr;           // first pass: key_copy[i] = (key % key_blocks_x) | (key / key_blocks_x) << 16
    uint32_t key_blocks_x = 1;             //   (the block's coordinates in the block box: what the hash's drift test needs)
    uint64_t key_div_magic = 0;            //   ceil(2^40 / key_blocks_x): key / key_blocks_x = key * magic >> 40, exact for key * blocks_x < 2^40
    uint4 *table_reset = nullptr;
    uint64_t table_pairs = 0;
    uint32_t *fresh = nullptr;
    uint32_t *sorts = nullptr;
    uint32_t *sorts_seen = nullptr;        // last pass: copy of the new *sorts (a word nobody updates atomically while tiles read it)
    int ticket_base = 0;                   // tile tickets at ctl[ticket_base + pass]
    const uint32_t *count_now = nullptr;   // first pass: *sorted_count = *count_now (NULL: n) -- the particles the grouping covers
    uint32_t *sorted_count = nullptr;
    unsigned long long *stamp = nullptr;   // a profiling boundary at this launch: its first workgroup stores wall_clock64() here
};
gpe_status onesweep_sort(gpe_ctx *c, uint32_t *keys, uint32_t *vals, uint32_t *keys_b, uint32_t *vals_b,
                         uint64_t n, int passes, bool hist_ready, bool iota_vals, uint32_t **out_keys,
                         uint32_t **out_vals, bool bases_ready = false, uint2 *table = nullptr,
                         uint32_t table_entries = 0,    // table: the last pass also fills the native block table
                         const uint32_t *hist_src = nullptr,   // bases_ready: histogram copies the passes scan themselves
                         const OnesweepGate *gate = nullptr);
// removal (k_remove.hip): mask != NULL selects the mask form, else the disc around (x, y) with rr = radius^2
uint64_t remove_tiles(uint64_t n);
gpe_status launch_remove_count(gpe_ctx *c, const uint8_t *mask, float x, float y, float rr, uint32_t *tile_count,
                               unsigned long long *tile_key, unsigned long long *max_key);
// *max_key = max over tile_key[0 .. tiles) (k_remove_max_key; also the fold of a radius edit's keys)
gpe_status launch_max_key_fold(gpe_ctx *c, const unsigned long long *tile_key, uint64_t tiles, unsigned long long *max_key);
// uids != NULL (uids on): each survivor's uid moves to uids_out as well
gpe_status launch_remove_scatter(gpe_ctx *c, const uint8_t *mask, float x, float y, float rr,
                                 const uint32_t *tile_scanned, const uint32_t *uids = nullptr,
                                 uint32_t *uids_out = nullptr);
// region queries and picking (k_query.hip): kind = a QueryKind of k_region.h (0 circle, 1 box, 2 segment); region =
// {x, y, -, -, radius^2} (circle), {x0, y0, x1, y1, -} (box) or {from x, from y, to x, to y, -} (segment)
uint64_t query_tiles(uint64_t n);
gpe_status launch_query_count(gpe_ctx *c, int kind, const float *region, uint32_t *tile_count);
// the matches ranked below capacity into the non-NULL outputs (uid_out: from c->uid.uids)
gpe_status launch_query_gather(gpe_ctx *c, int kind, const float *region, const uint32_t *tile_scanned,
                               uint32_t capacity, uint32_t *index_out, uint32_t *uid_out, float2 *pos_out,
                               float2 *prev_out, float *radius_out);
// *pick = min over the particles whose disc contains (x, y) of bits(d2) << 32 | index (~0 for none)
gpe_status launch_pick(gpe_ctx *c, float x, float y, unsigned long long *tile_key, unsigned long long *pick);
// contact queries (k_contacts.hip): keys[i] = the clamped cell of particle i under cell_size, vals[i] = i
uint64_t contacts_tiles(uint64_t n);
gpe_status launch_contacts_keys(gpe_ctx *c, float cell_size, uint32_t *keys, uint32_t *vals);
// rec[t] = the particle vals[t] (vals: sorted by key)
gpe_status launch_contacts_records(gpe_ctx *c, const uint32_t *vals, uint4 *rec);
// ... of any n rows (pos, radius): the candidates of gpe_add_particles_free
gpe_status launch_contacts_records_of(gpe_ctx *c, const float2 *pos, const float *radius, const uint32_t *vals, uint64_t n,
                                      uint4 *rec);
// degree[i], upper[i] = contacts of particle i / those of higher index; *total = the sum of upper (tile_sum: contacts_tiles(n))
gpe_status launch_contacts_count(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, uint32_t *degree, uint32_t *upper,
                                 unsigned long long *tile_sum, unsigned long long *total);
// the pairs ranked below capacity into the non-NULL outputs (scanned: inclusive scan of upper; uid_*: from c->uid.uids)
gpe_status launch_contacts_gather(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, const uint32_t *scanned,
                                  uint32_t capacity, uint32_t *index_a, uint32_t *index_b, uint32_t *uid_a, uint32_t *uid_b,
                                  float *overlap);
// ray casts (k_raycast.hip); keys / rec: the contact query's sorted cell keys and records under cell_size
// row_start[y] = the first sorted slot with key >= y << 16, y = 0 .. 65536 (kRayRowWords words)
gpe_status launch_ray_row_start(gpe_ctx *c, const uint32_t *keys, uint32_t *row_start);
// the first hit of each of the k <= kRayMaxBatch rays from[i] -> to[i] into row i of the non-NULL outputs (index
// GPE_RAY_MISS, uid GPE_UID_ABSENT and NaN for a miss; uid_out: from c->uid.uids).  Endpoints finite, within 131072 cells
gpe_status launch_ray_cast(gpe_ctx *c, const float2 *from, const float2 *to, uint32_t k, float cell_size,
                           const uint32_t *keys, const uint4 *rec, const uint32_t *row_start, uint32_t *index_out,
                           uint32_t *uid_out, float *t_out, float2 *pos_out, float *radius_out);
// nearest neighbours (k_nearest.hip); keys / rec / row_start as the ray cast takes them.  For each of the k points
// (k * m <= kNearestMaxSlots, 1 <= m <= kNearestMaxM; finite, within 131072 cells) the m candidates (d2 <= rr) with the
// least bits(d2) << 32 | index, ascending, into row i of the non-NULL per-slot outputs (GPE_NEAREST_NONE, GPE_UID_ABSENT
// and NaN past count_out[i]; uid_out: from c->uid.uids).  count_out is always written
gpe_status launch_nearest(gpe_ctx *c, const float2 *points, uint32_t k, uint32_t m, float max_distance, float cell_size,
                          const uint32_t *keys, const uint4 *rec, const uint32_t *row_start, uint32_t *count_out,
                          uint32_t *index_out, uint32_t *uid_out, float *dist2_out, float2 *pos_out, float *radius_out);
// contact clusters (k_clusters.hip); keys / rec: the contact query's sorted cell keys and records
// parent[i] = i, then every contact (i, j < i) unites the trees of i and j: parent[x] <= x, a component's root is its lowest index
gpe_status launch_clusters_hook(gpe_ctx *c, const uint32_t *keys, const uint4 *rec, uint32_t *parent);
// label[i] = root(i) (parent is compressed on the way); *count = the number of roots (tile_word: contacts_tiles(n))
gpe_status launch_clusters_flatten(gpe_ctx *c, uint32_t *parent, uint32_t *label, unsigned long long *tile_word,
                                   unsigned long long *count);
// root_size[r] = particles labelled r, size[i] = root_size[label[i]], label_uid[i] = uids[label[i]] (NULL: not wanted);
// *largest = max over the roots of size << 32 | (0xFFFFFFFF - label)
gpe_status launch_clusters_sizes(gpe_ctx *c, const uint32_t *label, uint32_t *root_size, uint32_t *size,
                                 uint32_t *label_uid, unsigned long long *tile_word, unsigned long long *largest);
// the particles labelled `want`, counted and gathered as launch_query_count / launch_query_gather do for a region
gpe_status launch_clusters_member_count(gpe_ctx *c, const uint32_t *label, uint32_t want, uint32_t *tile_count);
gpe_status launch_clusters_member_gather(gpe_ctx *c, const uint32_t *label, uint32_t want, const uint32_t *tile_scanned,
                                         uint32_t capacity, uint32_t *index_out, uint32_t *uid_out, float2 *pos_out,
                                         float2 *prev_out, float *radius_out);
// overlap-checked adds (k_spawn.hip); ws: the spawn workspace, k candidates uploaded into ws.pos / ws.radius
// keys[i] = candidate i's clamped cell under cell_size, vals[i] = i, state[i] = OUTSIDE_WORLD or kSpawnUndecided (the
// world test only when inside_world), ctl[0..3] = the cell box of the candidates that passed (set to all ones first)
gpe_status launch_spawn_keys(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, bool inside_world);
// blocked[i] = 1 for every candidate i a particle of the context touches, 0 for the others (keys / rec sorted);
// search false (every radius 0): nothing touches, no pass
gpe_status launch_spawn_pass(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, bool search);
// state[i]: undecided becomes BLOCKED_BY_PARTICLE when blocked[i], else stays (separate) or becomes ADDED
gpe_status launch_spawn_resolve(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, bool separate);
// one round of the separation over the undecided candidates; *left += those still undecided afterwards
gpe_status launch_spawn_round(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, uint32_t *left);
// rank[i] = 1 when state[i] is ADDED (to be scanned), verdict[i] = state[i] as a byte; then the added candidates go to
// old_n + rank[i] - 1 (rank scanned)
gpe_status launch_spawn_flags(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k);
gpe_status launch_spawn_scatter(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, uint64_t old_n);
// in-place edits (k_edit.hip).  Keyed edits: keys[i] becomes the storage index key i names (by_uid: looked up in the
// sorted uid map of n entries; GPE_UID_ABSENT for an absent uid or an index >= n, the latter also sets kEditBadIndex in
// flag[0]), slots[i] = i, flag[1] += the keys that name a particle.  flag zeroed by the caller.
gpe_status launch_edit_check(gpe_ctx *c, bool by_uid, uint32_t *keys, uint32_t *slots, uint64_t k, uint32_t *flag);
// keys sorted ascending: two equal neighbours other than GPE_UID_ABSENT set kEditDuplicate in flag[0]
gpe_status launch_edit_adjacent(gpe_ctx *c, const uint32_t *keys, uint64_t k, uint32_t *flag);
// particle keys[j] takes row slots[j] of every non-NULL field array (pos without prev: prev = the new pos too)
gpe_status launch_edit_apply(gpe_ctx *c, const uint32_t *keys, const uint32_t *slots, uint64_t k, const float2 *pos_rows,
                             const float2 *prev_rows, const float *radius_rows);
// *max_key = max over all particles of bits(|radius|) << 32 | index (the key of k_remove_count; tile_key: query_tiles(n))
gpe_status launch_edit_max_radius(gpe_ctx *c, unsigned long long *tile_key, unsigned long long *max_key);
// region as launch_query_count; op GPE_VEL_*; count != NULL: *count (zeroed here) receives the particles kicked
gpe_status launch_kick(gpe_ctx *c, bool box, const float *region, uint32_t op, float ax, float ay,
                       unsigned long long *count);
// tracer recorder (k_tracers.hip).  slot_index[perm[t]] = i for every particle i < n whose uid is keys[t] (keys: the k
// tracked uids ascending, lo / hi its ends); the other slots are left as they are (set to 0xffffffff by the caller)
gpe_status launch_tracers_resolve(gpe_ctx *c, const uint32_t *uids, uint64_t n, const uint32_t *keys, const uint32_t *perm,
                                  uint32_t k, uint32_t lo, uint32_t hi, uint32_t *slot_index);
// row j of the non-NULL frame arrays = pos / prev / index of particle slot_index[j] (< n), or quiet NaN / GPE_UID_ABSENT
gpe_status launch_tracers_sample(gpe_ctx *c, const uint32_t *slot_index, uint32_t k, const float2 *pos, const float2 *prev,
                                 uint64_t n, float2 *pos_row, float2 *prev_row, uint32_t *index_row);
// run monitor (k_monitor.hip).  partial: one partial record per workgroup of monitor_grid(n) <= kMonitorMaxBlocks into
// `partials`, from pos / prev [0, n), 1 <= n < 2^32; rs2 = rest_speed * rest_speed, W / H the world.  final: folds the
// monitor_grid(n) partials (none for n == 0) in index order and writes *out whole, uids (NULL: off) read at two indices
uint32_t monitor_grid(uint64_t n);
gpe_status launch_monitor_partial(gpe_ctx *c, const float2 *pos, const float2 *prev, uint64_t n, float rs2, float W,
                                  float H, void *partials);
gpe_status launch_monitor_final(gpe_ctx *c, const void *partials, uint64_t n, uint64_t step, const uint32_t *uids,
                                gpe_measures *out);
// static colliders (k_colliders.hip): one pass over pos[0, n) in place.  cell_start / items: the lookup grid `view`
// describes (view.gx * view.gy + 1 words; every item < k); rec: 2 k records; *pushed += the particles moved
gpe_status launch_colliders_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const uint32_t *cell_start,
                                 const uint32_t *items, const float4 *rec, uint32_t k, const ColliderGridView &view,
                                 unsigned long long *pushed, const float4 *surf = nullptr, float2 *prev = nullptr);
// distance bonds (k_bonds.hip): `iterations` relaxations of the k bonds of B over pos[0, n) in place, two launches each
gpe_status launch_bonds_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BondState &B, uint32_t k,
                             uint32_t m, uint32_t iterations);
// ... under the coloured solver: `iterations` coloured relaxations, B.order and B.colour_start as bond_colours.h built
// them for B.colours colours.  *form: 2 when the pass was one launch of one workgroup (m <= kBondLdsNodesMax), 1 when
// it was one launch per colour and relaxation
#ifndef GPE_BOND_LDS_NODES_MAX
#define GPE_BOND_LDS_NODES_MAX 1024              // (timing builds set 0 and 8192: every pass in one form, profiles/bond_solver/)
#endif
constexpr uint32_t kBondLdsNodesMax = GPE_BOND_LDS_NODES_MAX;       // policy: profiles/bond_solver/README.md
// the nodes the one-workgroup form declares LDS for, 12 B each: the policy's (12 KiB; a timing build of 8192: 96 KiB)
constexpr uint32_t kBondLdsNodesCap = kBondLdsNodesMax > 0 ? kBondLdsNodesMax : 1;
static_assert(kBondLdsNodesCap <= 8192, "12 B a node: 8192 nodes are 96 KiB of the 160 KiB a gfx950 workgroup may declare");
gpe_status launch_bonds_coloured(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BondState &B, uint32_t k,
                                 uint32_t m, uint32_t iterations, uint32_t *form);
// bend constraints (k_bends.hip): `iterations` relaxations of the k bends of B over pos[0, n) in place, two launches each
gpe_status launch_bends_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BendState &B, uint32_t k,
                             uint32_t m, uint32_t iterations);
// ... under the coloured solver: `iterations` coloured relaxations, B.order and B.colour_start as bend_colours.h built
// them for B.colours colours.  *form: 2 when the pass was one launch of one workgroup (m <= kBendLdsNodesMax), 1 when
// it was one launch per colour and relaxation
#ifndef GPE_BEND_LDS_NODES_MAX
#define GPE_BEND_LDS_NODES_MAX 1024              // (timing builds set 0 and 8192: every pass in one form, profiles/bend_solver/)
#endif
constexpr uint32_t kBendLdsNodesMax = GPE_BEND_LDS_NODES_MAX;       // policy: profiles/bend_solver/README.md
// the nodes the one-workgroup form declares LDS for, 12 B each: the policy's (12 KiB; a timing build of 8192: 96 KiB)
constexpr uint32_t kBendLdsNodesCap = kBendLdsNodesMax > 0 ? kBendLdsNodesMax : 1;
static_assert(kBendLdsNodesCap <= 8192, "12 B a node: 8192 nodes are 96 KiB of the 160 KiB a gfx950 workgroup may declare");
gpe_status launch_bends_coloured(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BendState &B, uint32_t k,
                                 uint32_t m, uint32_t iterations, uint32_t *form);
// area constraints (k_areas.hip): `iterations` relaxations of the k loops of A over pos[0, n) in place: one launch per
// non-empty width class, then one over the m nodes; launch_areas_expand: member_slot[i] = node_slot[member_node[i]]
gpe_status launch_areas_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const AreaState &A, uint32_t k,
                             uint32_t m, uint32_t iterations);
gpe_status launch_areas_expand(gpe_ctx *c, const AreaState &A);
// rigid and soft bodies (k_bodies.hip): one shape matching pass of the k bodies of B over pos[0, n) in place, one launch
// per non-empty width class
gpe_status launch_bodies_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BodyState &B, uint32_t k);
// force fields (k_fields.hip): one pass over prev[0, n) in place, pos read only.  cell_start / items: the lookup grid
// `view`, rec: 3 float4 per field.  *touched += the particles whose prev was written
gpe_status launch_fields_pass(gpe_ctx *c, const float2 *pos, float2 *prev, uint64_t n, const uint32_t *cell_start,
                              const uint32_t *items, const float4 *rec, uint32_t k, const ColliderGridView &view, float dt2,
                              unsigned long long *touched);
// the swept form (k_sweep.hip): prev[0, n) is read for every particle; counts: two words, swept and stopped
gpe_status launch_colliders_sweep(gpe_ctx *c, float2 *pos, float2 *prev, const float *radius, uint64_t n,
                                  const uint32_t *cell_start, const uint32_t *items, const float4 *rec, uint32_t k,
                                  const ColliderGridView &view, unsigned long long *pushed, unsigned long long *counts,
                                  const float4 *surf);
// moving colliders (k_movers.hip): the build advances, poses and lists the movers (the grid zeroed before it), the pass
// pushes pos[0, n) in place
gpe_status launch_movers_build(gpe_ctx *c, const MoverBuildArgs &B);
gpe_status launch_movers_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const MoverPassArgs &P);
// their swept form (k_mover_sweep.hip): the build also writes B.old (never null here) and W.carry and lists every mover
// where its motion reaches; the pass judges the paths relative to each mover.  P.old as the build wrote it; P.surf may
// be null; P.prev is unused (W.prev)
gpe_status launch_movers_sweep_build(gpe_ctx *c, const MoverBuildArgs &B, const MoverSweepArgs &W);
gpe_status launch_movers_sweep(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const MoverPassArgs &P,
                               const MoverSweepArgs &W);
// native pipeline: its host side (gpe_native.hip; the kernels and their launchers: k_native.hip, native_launch.h)
gpe_status native_configure(gpe_ctx *c);
bool native_should_run(gpe_ctx *c);
NativeStats native_read_stats(const NativeState &N);   // one reading of N.host_stat (allocated: native_configure)
void native_release(gpe_ctx *c);
// sharded runs (k_shard.hip)
gpe_status launch_shard_classify(gpe_ctx *c, const uint8_t *owner_of_block, const uint32_t *dest_mask_of_block,
                                 int32_t blocks_x, int32_t blocks_y, uint32_t my_rank, uint32_t *out_index,
                                 uint32_t *out_info, uint32_t *out_count, uint64_t out_capacity);
void shard_release(gpe_ctx *c);
void comm_release(gpe_ctx *c);
void ctl_release(gpe_ctx *c);
void shard_pack_args(gpe_ctx *c, PackArgs *P);
// collectives of a sharded run, carried by (in this order) the caller's callbacks, the local group, the RCCL communicator
gpe_status coll_all_reduce_u32(gpe_ctx *c, uint32_t *d_buf, uint64_t count, uint32_t op);
gpe_status coll_all_to_all_u32(gpe_ctx *c, const uint32_t *d_send, const uint64_t *send_off, const uint64_t *send_cnt,
                               uint32_t *d_recv, const uint64_t *recv_off, const uint64_t *recv_cnt,
                               hipStream_t on = nullptr);   // (on: the stream handed to the caller's callback; default the context's)
// the same over the RCCL communicator (gpe_comm.hip) and over a local group (gpe_group.hip)
gpe_status rccl_all_reduce_u32(gpe_ctx *c, uint32_t *d_buf, uint64_t count, uint32_t op);
gpe_status rccl_all_to_all_u32(gpe_ctx *c, const uint32_t *d_send, const uint64_t *send_off, const uint64_t *send_cnt,
                               uint32_t *d_recv, const uint64_t *recv_off, const uint64_t *recv_cnt);
gpe_status group_all_reduce_u32(gpe_ctx *c, uint32_t *d_buf, uint64_t count, uint32_t op);
gpe_status group_all_to_all_u32(gpe_ctx *c, const uint32_t *d_send, const uint64_t *send_off, const uint64_t *send_cnt,
                                uint32_t *d_recv, const uint64_t *recv_off, const uint64_t *recv_cnt);
gpe_status group_exchange_segments(gpe_ctx *c, hipStream_t xs);   // the per-step neighbour exchange, event-ordered (no stream sync)
void group_leave(gpe_ctx *c);
gpe_status resort_for_shard(gpe_ctx *c);          // ParticleSort::sort on the owned particles (gpe_api.hip do_resort)
gpe_status shard_ensure_flag_capacity(gpe_ctx *c);
std::string shard_error_text(uint32_t flags);
gpe_status step_for_shard(gpe_ctx *c, float dt);           // one ordinary step (gpe_api.hip do_step)
gpe_status grow_for_shard(gpe_ctx *c, uint64_t capacity);  // reallocate the particle buffers, keeping the first c->n
gpe_status reconfigure_native(gpe_ctx *c);
// verlet != nullptr: K12 is applied to the first n_owned particles as they are written back (pos_out = integrated
// position, prev = resolved position) -- the separate integration launch is then skipped
gpe_status native_collide(gpe_ctx *c, const float2 *pos_in, float2 *pos_out, const VerletParams *verlet = nullptr);
// collision cells + solver
gpe_status launch_count_chunks(gpe_ctx *c, const uint32_t *cell_ids, uint64_t total, uint32_t *chunk_counts);
gpe_status launch_build_collision_cells(gpe_ctx *c, const uint32_t *cell_ids, uint64_t total,
                                        const uint32_t *scanned, uint64_t num_chunks,
                                        uint32_t *collision_cells, uint32_t *indirect_args);
gpe_status launch_solve_color(gpe_ctx *c, const uint32_t *collision_cells, const uint32_t *scanned,
                              uint64_t num_chunks, const uint32_t *cell_ids, const uint32_t *object_ids,
                              uint64_t total, float2 *pos, const float *radius, float stiffness,
                              uint32_t color);

}  // namespace gpe
