/*
 * gpe.h -- C-ABI of the MI355X-native particle step (libgpe.so).
 *
 * Drop-in boundary for the per-timestep particle pipeline of MarcVivas/gpu-physics-engine:
 * everything State::update() (src/state.rs:115-131) calls except the camera update, i.e. the
 * module API of src/particles, src/grid, src/physics and the two GPU primitives in src/utils.
 * The reference exports no FFI of its own (Cargo.toml:6-7 builds cdylib+rlib with nothing
 * extern "C"), so each entry point below names the Rust method a host shim would forward to it.
 * Citations are relative to /root/reference/src.  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *  - plain pointers and sizes only; positions are interleaved (x,y) f32 pairs (glam::Vec2).
 *  - the library owns all device memory; the caller owns every host array passed in or out.
 *  - every function returns gpe_status (0 = OK, negative = error) and never unwinds;
 *    gpe_last_error() gives the message of the last failure on that context (or globally when
 *    ctx is NULL).  The reference unwrap()s/panics instead (gpu_buffer.rs:266-268).
 *  - one in-order hipStream per context; calls on one context are not re-entrant.
 *    gpe_step/gpe_run and the per-module calls are asynchronous; gpe_download/gpe_sync block.
 */
#ifndef GPE_H
#define GPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_ABI_VERSION 1u
#define GPE_UNUSED_CELL_ID 0xffffffffu    /* grid/grid.rs:22  UNUSED_CELL_ID            */
#define GPE_MAX_CELLS_PER_OBJECT 4u       /* grid/grid.rs:18  MAX_CELLS_PER_OBJECT      */
#define GPE_COUNTING_CHUNK_SIZE 4u        /* physics/collision_cell_builder.rs:13       */

typedef struct gpe_ctx gpe_ctx;
typedef int32_t gpe_status;

enum {
    GPE_OK = 0,
    GPE_ERR_INVALID_ARG = -1,
    GPE_ERR_HIP = -2,          /* a HIP runtime call failed (message has the hipError name)  */
    GPE_ERR_OOM = -3,
    GPE_ERR_STATE = -4,        /* call order violated (e.g. step before set_particles)       */
    GPE_ERR_UNSUPPORTED = -5,
    GPE_ERR_NO_DEVICE = -6     /* no gfx950 device visible: there is NO CPU fallback         */
};

/* Which kernels gpe_step() runs.  Both produce identical positions
 * (tests/test_gpu_native.py::test_native_equals_compat_1m, _100m; each against the oracle: test_gpu_parity_step.py).
 * COMPAT materialises the reference's own intermediate buffers every step (4N (cell,object)
 * pairs, chunk counts, collision-cell list) -- needed for bit-exact comparison with the
 * reference tests.  NATIVE is the MI355X design: N-key sort + LDS-staged cell windows. */
enum { GPE_MODE_COMPAT = 0, GPE_MODE_NATIVE = 1 };

enum { GPE_STEP_RESORT = 1u };            /* gpe_step flags: Morton re-sort first (state.rs:122) */

typedef struct gpe_config {
    uint32_t struct_size;          /* = sizeof(gpe_config), for ABI growth                    */
    int32_t  device;               /* HIP device ordinal, -1 = current device                 */
    float    world_width;          /* state.rs:35  (3048)                                     */
    float    world_height;         /* state.rs:35  (1048)                                     */
    float    gravity_x;            /* particle_integration.wgsl:21 FORCE_OF_GRAVITY (0,0)     */
    float    gravity_y;
    float    cell_size_multiplier; /* grid.rs:20  CELL_SIZE_MULTIPLIER = 2.2                  */
    float    stiffness;            /* collision_solver.wgsl:2  STIFFNESS = 0.6                */
    float    mouse_strength;       /* particle_integration.wgsl:22  = 150                     */
    uint32_t mode;                 /* GPE_MODE_*                                              */
    uint32_t profiling;            /* as gpe_set_profiling: 0 off, 1 every scope, k every k-th step */
    uint32_t flags;                /* GPE_FLAG_* (0 = the defaults); was reserved[0]          */
    uint32_t guard_canary;         /* GPE_FLAG_GUARD_ALLOCS: the canary and poison words of this context, 0 = the   */
    uint32_t guard_poison;         /* defaults 0x3C3 / 0x2A5; were reserved[0..1] (gpe_guard_check)                  */
    uint32_t reserved[2];
} gpe_config;

/* gpe_config.flags -- switches for tests and measurements; the reference has no counterpart (state.rs:34-70 builds one
 * pipeline).  None of them changes a result bit. */
enum {
    GPE_FLAG_NATIVE_FORCE = 1u,      /* never hand an over-dense scene to the COMPAT kernels (windows then spill)   */
    GPE_FLAG_SORT_EVERY_STEP = 2u,   /* NATIVE: run the radix passes every step instead of when a particle has left */
                                     /* the reach of the kept block table (what rounds 1-2 did; for A/B timing)     */
    GPE_FLAG_NATIVE_STATS = 4u,      /* print the tile statistics to stderr every 128 steps                          */
    GPE_FLAG_SAFE_SORT = 8u,         /* per-module sorts by the communication-free reduce-then-scan radix sort       */
                                     /* (k_radix_sort.hip) instead of onesweep: an in-GPU cross-check                */
    GPE_FLAG_COUNTING_SORT_TILES = 16u, /* NATIVE: the dense launch builds its member lists by a counting sort      */
                                     /* (rounds 1-2) instead of direct cell slots; for A/B timing                    */
    GPE_FLAG_XCD_EIGHTHS = 64u,      /* NATIVE: every XCD works through one contiguous eighth of the tile rows       */
                                     /* (rounds 1-3) instead of interleaved bands of rows; for A/B timing            */
    GPE_FLAG_NO_HALF_TILES = 128u,   /* NATIVE: tiles the direct-slot launch hands on go straight to the 16x16 / 8x8 */
                                     /* windows (rounds 1-3), not first through 32x16 direct-slot halves -- neither  */
                                     /* the half-tile launch nor the dense launch's front workgroups; A/B timing     */
    GPE_FLAG_SHARD_OVERLAP = 256u,   /* sharded runs: the neighbour exchange on a stream of its own beside the       */
                                     /* interior tiles, the tiles along the rank's border first (off by default: on  */
                                     /* one GPU the two cross-stream waits cost more than the exchange they hide)    */
    GPE_FLAG_FUSED_HISTOGRAMS = 512u,/* NATIVE: the hash kernel counts the radix digits every step (rounds 1-3)      */
                                     /* instead of a gated launch counting them when a sort is due; for A/B timing   */
    GPE_FLAG_GUARD_ALLOCS = 1024u,   /* tests: every device allocation of the context sits between two red zones     */
                                     /* filled with a canary, its fresh payload is poisoned (gpe_guard_check)        */
    GPE_FLAG_HASH_INDEX64 = 2048u,   /* NATIVE, diagnostic: the hash kernel indexes with 64 bits at every particle    */
                                     /* count (by default only where an index could pass 2^31); for tests, A/B timing */
    GPE_FLAG_EVENT_SCOPES = 4096u,   /* profiling scopes record hipEvents (as they did up to now) instead of writing  */
                                     /* the GPU's timestamp counter into a device buffer; for A/B timing.  A context  */
                                     /* on a stream lent by gpe_set_stream records events either way                  */
    GPE_FLAG_GENERAL_RADII = 8192u   /* NATIVE: keep the kernels that read every particle's radius even when all radii */
                                     /* are one ordinary number (gpe_pipeline_info.uniform_radius); for tests, A/B timing */
};

/* Fills *cfg with the reference's compile-time constants. */
gpe_status gpe_config_default(gpe_config *cfg);

/* State::new (state.rs:34-70) minus window/renderer: creates the HIP context (stream, events).
 * Fails with GPE_ERR_NO_DEVICE when no GPU is visible. */
gpe_status gpe_create(const gpe_config *cfg, gpe_ctx **out);
gpe_status gpe_destroy(gpe_ctx *ctx);
const char *gpe_last_error(const gpe_ctx *ctx);
uint32_t gpe_abi_version(void);

/* ---- particles (src/particles/particle_system.rs) ----------------------------------------- */
/* ParticleSystem::new_from_buffers (:49-99) / generate_initial_particles (:102-161).
 * prev_xy == NULL => previous = current (zero velocity, :126-127).  Also (re)creates the Grid
 * (grid.rs:74-149) and CollisionSystem (collision_system.rs:14-22) buffers for n particles and
 * sets max_radius = the radius of largest magnitude (:51). */
gpe_status gpe_set_particles(gpe_ctx *ctx, const float *pos_xy, const float *prev_xy,
                             const float *radius, uint64_t n);
/* ParticleSystem::add_particles (:163-220) + Grid::refresh_grid (grid.rs:265-291) +
 * CollisionSystem::refresh (collision_system.rs:24-28): append n particles (prev = pos),
 * grow every dependent buffer (amortised x2 like gpu_buffer.rs:54-56), recompute cell size. */
gpe_status gpe_add_particles(gpe_ctx *ctx, const float *pos_xy, const float *radius, uint64_t n);
/* Remove every particle i (storage order, as gpe_download(GPE_POS) returns it) with remove[i] != 0.
 * n must equal gpe_len.  n_removed may be NULL.  Synchronises, like gpe_add_particles.
 * The survivors keep their order and their pos / prev / radius bits; afterwards the context is what
 * gpe_set_particles(survivors' pos, prev, radius) would leave on it (capacity and the native step /
 * sort counters aside): gpe_len, gpe_max_radius (largest magnitude, last on ties, sign kept), cell
 * size, HOME_CELL_IDS = unused, PARTICLE_IDS = iota, grid arrays, native eligibility.  Compacted on
 * the device (csrc/k_remove.hip): the mask (n bytes) is the only upload.
 * Nothing removed: GPE_OK, *n_removed = 0, the context untouched.  Every particle removed:
 * GPE_ERR_INVALID_ARG, the context untouched.  NULL mask or n != gpe_len: GPE_ERR_INVALID_ARG; no
 * particles: GPE_ERR_STATE; a sharded context (gpe_shard_*, order keys, active box): GPE_ERR_UNSUPPORTED. */
gpe_status gpe_remove_particles(gpe_ctx *ctx, const uint8_t *remove, uint64_t n, uint64_t *n_removed);
/* Remove every particle whose centre p has (p.x-x)*(p.x-x) + (p.y-y)*(p.y-y) <= radius*radius, in
 * IEEE binary32 with one rounding per operation, left to right, no FMA (numpy float32 gives the same
 * set).  radius must be finite and >= 0 (else GPE_ERR_INVALID_ARG); otherwise as gpe_remove_particles. */
gpe_status gpe_remove_particles_in_circle(gpe_ctx *ctx, float x, float y, float radius, uint64_t *n_removed);
/* ParticleSystem::len (:275) / get_max_radius (:291) */
gpe_status gpe_len(const gpe_ctx *ctx, uint64_t *n);
gpe_status gpe_max_radius(const gpe_ctx *ctx, float *r);
/* ParticleSystem::sort_by_cell_id (:236-243) -> ParticleSort::sort (particle_sort.rs:58-69):
 * K1 home cell ids, stable sort of (home cell, particle id), K4 rearrange.  The live and copy
 * sets are swapped instead of copied back (particle_rearrange.rs:205-238). */
gpe_status gpe_morton_resort(gpe_ctx *ctx);
/* ParticleSystem::update_positions (:245-247) -> K12 verlet_integration */
gpe_status gpe_integrate(gpe_ctx *ctx, float dt);
/* mouse_click_callback / mouse_move_callback (:221-227, particle_integration.rs:176-185) */
gpe_status gpe_set_mouse(gpe_ctx *ctx, int32_t pressed, float x, float y);
/* world size used by K12's wall clamp (ParticleIntegration::new, particle_integration.rs:34-48;
 * new_from_buffers hard-codes 1920x1080, particle_system.rs:86) */
gpe_status gpe_set_world(gpe_ctx *ctx, float width, float height);
gpe_status gpe_set_gravity(gpe_ctx *ctx, float gx, float gy);
/* Read back the step constants the context holds, however they were set (gpe_create's config or the
 * setters above): world size, gravity, and the mouse button state and position (pressed 0 / 1). */
gpe_status gpe_world(const gpe_ctx *ctx, float *width, float *height);
gpe_status gpe_gravity(const gpe_ctx *ctx, float *gx, float *gy);
gpe_status gpe_mouse(const gpe_ctx *ctx, int32_t *pressed, float *x, float *y);

/* ---- particle uids (not in the reference) ----------------------------------------------------------- */
/* The library moves particles around in storage: a re-sort permutes them, a removal compacts them, set / add rebuild
 * or append.  A uid is an opt-in u32 per particle that the library carries through every one of those moves, so that
 * a host can keep its own per-particle data (colours, tracers, "the particle I spawned") keyed by uid.  (Not to be
 * confused with GPE_PARTICLE_IDS, the re-sort's permutation scratch, particle_system.rs:254.)
 *  - Off by default.  While off, every other entry point behaves and launches exactly as without uids.
 *  - While on:  gpe_set_particles gives uid = storage index (0..n-1) and next = n;  gpe_add_particles gives the k new
 *    particles next .. next+k-1 in input order and next += k -- GPE_ERR_STATE, nothing added, when next + k > 2^32;
 *    re-sorts (gpe_morton_resort, GPE_STEP_RESORT in gpe_step / gpe_run) permute the uids with pos / prev / radius;
 *    gpe_remove_particles* compact them with the survivors; gpe_reserve and growth keep them.  Uids are never reused.
 *  - gpe_download / gpe_array_bytes / gpe_device_ptr(GPE_UIDS): u32[n], in storage order like GPE_POS.
 *  - Sharded runs carry GPE_ORDER_KEYS instead: gpe_enable_uids / gpe_set_uids on a context with shard state, order
 *    keys or an active cell box, and gpe_shard_set_particles / gpe_use_order_keys(ctx, 1) / gpe_set_counts on a
 *    context whose uids are on, return GPE_ERR_UNSUPPORTED.
 *  - A NULL context or array: GPE_ERR_INVALID_ARG.
 * Lookups go through a uid -> index map (the uids sorted on the device, csrc/k_uids.hip), rebuilt by the first lookup
 * after anything has changed the uids or their order. */
#define GPE_UID_ABSENT 0xffffffffu
/* enable != 0, off -> on: uid = storage index (0..n-1), next = n (also with no particles yet).  On -> on: nothing
 * changes.  enable == 0: the uids are dropped (their buffers freed). */
gpe_status gpe_enable_uids(gpe_ctx *ctx, int32_t enable);
/* Replace every particle's uid: uids[i] for storage index i; n must equal gpe_len (>= 1, else GPE_ERR_STATE).  The
 * uids must be pairwise distinct (checked on the device).  Afterwards uids are on and next = max(uids) + 1 (2^32 for a
 * uid 0xffffffff).  A duplicate, NULL uids or a wrong n: GPE_ERR_INVALID_ARG and the previous uid state -- on / off,
 * values, next -- untouched.  Synchronises. */
gpe_status gpe_set_uids(gpe_ctx *ctx, const uint32_t *uids, uint64_t n);
/* The uid the next added particle gets (at most 2^32).  GPE_ERR_STATE while uids are off: how a host asks whether
 * they are on. */
gpe_status gpe_next_uid(const gpe_ctx *ctx, uint64_t *next);
/* next <= the largest current uid or next > 2^32: GPE_ERR_INVALID_ARG.  GPE_ERR_STATE while uids are off. */
gpe_status gpe_set_next_uid(gpe_ctx *ctx, uint64_t next);
/* For each of the k uids: index_out[i] = the particle's current storage index, or GPE_UID_ABSENT; pos_xy_out[2i..2i+1],
 * prev_xy_out[2i..2i+1], radius_out[i] = that particle's bits, or quiet NaN for an absent uid.  Every output may be
 * NULL.  Duplicate queries are allowed, k == 0 is OK.  Blocks like gpe_download.  GPE_ERR_STATE while uids are off. */
gpe_status gpe_find_uids(gpe_ctx *ctx, const uint32_t *uids, uint64_t k, uint32_t *index_out, float *pos_xy_out,
                         float *prev_xy_out, float *radius_out);
/* Remove the particles whose uid is among the k uids (absent ones are ignored, a duplicate counts once).  Otherwise
 * exactly gpe_remove_particles with that mask: survivors keep their order, nothing removed leaves the context
 * untouched, removing every particle is GPE_ERR_INVALID_ARG.  GPE_ERR_STATE while uids are off. */
gpe_status gpe_remove_particles_by_uid(gpe_ctx *ctx, const uint32_t *uids, uint64_t k, uint64_t *n_removed);

/* ---- tracers (not in the reference) ----------------------------------------------------------------------------
 * Where k particles named by uid were during a run, without stopping it: an opt-in recorder that writes one frame
 * -- one row per tracer -- into a device-resident ring after every every-th step (csrc/k_tracers.hip).  The writes are
 * stream-ordered: gpe_step and gpe_run stay as asynchronous as they are, and only gpe_tracers_read synchronises.  A
 * context that is not armed launches exactly what it launches without this section.
 *  - Steps: a step is one gpe_step or one iteration of gpe_run.  The per-module calls (gpe_integrate,
 *    gpe_solve_collisions, gpe_grid_*, gpe_morton_resort, ...) and the steps of a sharded run are not steps.  The
 *    recorder keeps steps_seen: 0 at gpe_tracers_begin, + 1 after each step, across calls -- gpe_run(7) followed by
 *    gpe_run(5) samples like gpe_run(12).
 *  - Frames: a frame is taken after a step when steps_seen % every == 0 and holds the state that step left behind.
 *    gpe_tracers_sample takes a frame at the current steps_seen without changing it (the frame at step 0).
 *  - Rows: row j of a frame belongs to uids[j].  If a particle with that uid exists at that moment the row holds the
 *    bits of its pos, the bits of its prev and its storage index -- copied, no arithmetic.  Otherwise it holds quiet
 *    NaNs and GPE_UID_ABSENT: a particle that was removed, one not yet added (it shows up in the first frame after
 *    gpe_add_particles has handed out that uid), or uids switched off in the meantime.  Tracers are followed through
 *    re-sorts, removals, adds, growth, gpe_set_particles and gpe_set_uids.
 *  - Ring: the ring keeps the newest `frames` frames.  gpe_tracers_read delivers the newest min(count, capacity) of
 *    them, oldest first, into every non-NULL array; host memory past those entries is left untouched.  With every array
 *    NULL the call only reports count and recorded.  GPE_TRACERS_CONSUME empties the ring after delivery; recorded
 *    keeps counting.  An array for a field that was not configured: GPE_ERR_INVALID_ARG, nothing written.  Blocks like
 *    gpe_download.
 *  - Nothing a step can see changes: positions, prev, radii, uids, the uid -> index map and its validity, the native
 *    step / sort counters, the kept block table and the rosters are left alone; the recorder neither builds nor
 *    invalidates the uid map (it keeps a table of its own: each tracer's storage index, re-resolved on the stream by one
 *    pass over the uids before the first frame after anything has moved the particles or changed their uids).  An armed
 *    context steps bit for bit like one that is not.
 *  - Errors: a NULL ctx / cfg / uids / out, a struct_size below the struct's, k == 0, k > GPE_TRACERS_MAX, every == 0,
 *    frames == 0, no field or an unknown field bit, an unknown read flag, or two equal uids (checked on the host, before
 *    anything is allocated): GPE_ERR_INVALID_ARG.  A sharded context (gpe_shard_*, order keys or an active cell box):
 *    GPE_ERR_UNSUPPORTED.  gpe_tracers_begin while uids are off, with no particles or while already armed, and
 *    gpe_tracers_sample / _read / _end while not armed: GPE_ERR_STATE.  A ring that does not fit: GPE_ERR_OOM, and the
 *    context stays unarmed.  gpe_destroy frees the recorder; it is observation state, not step state. */
#define GPE_TRACERS_MAX 65536u
enum { GPE_TRACER_POS = 1u, GPE_TRACER_PREV = 2u, GPE_TRACER_INDEX = 4u };   /* fields */
enum { GPE_TRACERS_CONSUME = 1u };                                           /* read flag */
typedef struct gpe_tracer_config {
    uint32_t struct_size;   /* in: sizeof(gpe_tracer_config)                          */
    uint32_t fields;        /* in: GPE_TRACER_*, at least one, no unknown bit         */
    uint64_t k;             /* in: 1 .. GPE_TRACERS_MAX                               */
    const uint32_t *uids;   /* in: u32[k], pairwise distinct; row j of a frame = uids[j] */
    uint64_t every;         /* in: >= 1: a frame after every every-th step            */
    uint64_t frames;        /* in: >= 1: ring capacity in frames                      */
} gpe_tracer_config;        /* 40 bytes */
typedef struct gpe_tracer_frames {
    uint32_t struct_size;   /* in */
    uint32_t flags;         /* in: 0 or GPE_TRACERS_CONSUME                           */
    uint64_t capacity;      /* in: frames each non-NULL array has room for            */
    uint64_t count;         /* out: frames held in the ring (<= config.frames)        */
    uint64_t recorded;      /* out: frames taken since begin (held + overwritten + consumed) */
    uint64_t *step;         /* out, may be NULL: u64[capacity], steps since begin at which the frame was taken */
    float    *pos_xy;       /* out, may be NULL: f32[capacity * k * 2]                */
    float    *prev_xy;      /* out, may be NULL: f32[capacity * k * 2]                */
    uint32_t *index;        /* out, may be NULL: u32[capacity * k] storage index at that moment */
} gpe_tracer_frames;        /* 64 bytes */
/* Arms the recorder: steps_seen = recorded = 0, the ring empty.  Synchronises (the uids are uploaded). */
gpe_status gpe_tracers_begin(gpe_ctx *ctx, const gpe_tracer_config *cfg);
gpe_status gpe_tracers_sample(gpe_ctx *ctx);            /* one frame now, stream-ordered, no sync */
gpe_status gpe_tracers_read(gpe_ctx *ctx, gpe_tracer_frames *out);
/* Disarms the recorder and frees its buffers (the frames not read are lost).  Synchronises. */
gpe_status gpe_tracers_end(gpe_ctx *ctx);

/* ---- run monitor (not in the reference) ------------------------------------------------------------------------
 * What the whole system is doing while it runs -- has it settled, is it blowing up, did a NaN appear and where, how far
 * does the cloud extend, what are the total momentum and kinetic energy -- without stopping the run: one fixed record
 * of scalars, computed by a full-pass reduction on the device (csrc/k_monitor.hip).  gpe_measure takes one record now;
 * gpe_monitor_begin arms a recorder that writes one record per frame into a device-resident ring after every every-th
 * step, stream-ordered: only gpe_monitor_read and gpe_monitor_end synchronise.  A context that is not armed launches
 * exactly what it launches without this section.
 *  - The record.  For storage index i, p = pos[i], q = prev[i]:  vx = p.x - q.x; vy = p.y - q.y; v2 = vx*vx + vy*vy,
 *    IEEE binary32, one rounding per operation, left to right, no FMA.  That is the displacement per step: the recorder
 *    does not know dt and does not divide.  A particle is irregular when any of p.x, p.y, q.x, q.y is not finite or v2
 *    is not finite (an overflowing difference or square); every other particle is regular.  All fields except n,
 *    irregular and first_irregular* range over the regular particles only: every term is finite, no sum can turn NaN.
 *  - Extent: min and max in the total order of the sign-magnitude bit pattern, so -0 < +0; the delivered bits are
 *    those of an actual particle coordinate.  Fastest particle: selected by the key
 *    bits(v2) << 32 | (0xFFFFFFFF - index): the largest v2, the lowest storage index on a tie.
 *  - Absent values: an index that does not exist is 0xFFFFFFFF; a uid is GPE_UID_ABSENT while uids are off or when
 *    the index does not exist, otherwise uids[index] at that moment -- the handle that stays valid after the next
 *    re-sort.
 *  - Sums: each binary32 term converted exactly to double and added in double.  For a sum S of terms t_i over m
 *    regular particles the delivered D satisfies |D - S| <= m * 2^-52 * sum|t_i|; where every partial sum is exactly
 *    representable D is exact.  No floating-point atomics: the launch geometry and the order in which partial sums are
 *    combined are functions of n alone, so two measurements of the same arrays give identical bytes -- in either mode,
 *    on any context, by gpe_measure or as a monitor frame.
 *  - Steps: a step is one gpe_step or one iteration of gpe_run.  The per-module calls and the steps of a sharded run
 *    are not steps.  The recorder keeps steps_seen: 0 at gpe_monitor_begin, + 1 after each step, across calls --
 *    gpe_run(7) followed by gpe_run(5) samples like gpe_run(12).
 *  - Frames: a frame is taken after a step when steps_seen % every == 0 and measures the state that step left behind:
 *    whichever pos / prev / uids are live, gpe_len and the world at that moment, so frames follow removals, adds,
 *    growth, edits, gpe_set_particles and uids being switched on or off between runs.  gpe_monitor_sample takes a frame
 *    at the current steps_seen without changing it (the frame at step 0).
 *  - Ring: the ring keeps the newest `frames` records.  gpe_monitor_read delivers the newest min(count, capacity) of
 *    them, oldest first; host memory past those entries is left untouched.  With frames == NULL the call only reports
 *    count and recorded.  GPE_MONITOR_CONSUME empties the ring after delivery; recorded keeps counting.  Blocks like
 *    gpe_download.
 *  - Nothing a step can see changes: an armed context steps bit for bit like one that is not; counters, the kept block
 *    table, the rosters and the uid map are left alone.  Tracers and the monitor may be armed together and are
 *    independent.
 *  - Errors: a NULL ctx / cfg / out, a struct_size below the struct's, every == 0, frames == 0, non-zero config flags,
 *    an unknown read flag, a rest_speed that is NaN or negative (+inf and -0.0 are accepted): GPE_ERR_INVALID_ARG.  A
 *    sharded context (gpe_shard_*, order keys or an active cell box) or more than 2^32 - 1 particles:
 *    GPE_ERR_UNSUPPORTED.  gpe_monitor_begin while armed or with no particles, gpe_monitor_sample / _read / _end while
 *    not armed: GPE_ERR_STATE.  A ring that does not fit: GPE_ERR_OOM, and the context stays unarmed.  gpe_measure with
 *    no particles returns GPE_OK with n = 0 and the "none" values; on any error of gpe_measure the record is not
 *    written.  gpe_destroy frees the recorder; it is observation state, not step state. */
enum { GPE_MONITOR_CONSUME = 1u };                                           /* read flag */
typedef struct gpe_measures {
    uint64_t step;        /* monitor frame: steps since gpe_monitor_begin; gpe_measure: 0                   */
    uint64_t n;           /* gpe_len at that moment                                                         */
    uint64_t irregular;   /* number of irregular particles                                                  */
    uint64_t moving;      /* regular particles with v2 > rest_speed*rest_speed (binary32 product; == is at rest) */
    uint64_t outside;     /* regular particles with !(p.x >= 0 && p.x <= W && p.y >= 0 && p.y <= H), W,H as gpe_world */
    double   sum_x, sum_y, sum_vx, sum_vy, sum_v2;   /* sums of the binary32 terms, each converted exactly to double */
    float    min_x, min_y, max_x, max_y;             /* extent of the regular centres; none: +inf,+inf,-inf,-inf     */
    float    max_v2;      /* largest v2 among the regular particles; none: +0                              */
    uint32_t max_v2_index, max_v2_uid;               /* its storage index (lowest on a tie) and uid                 */
    uint32_t first_irregular, first_irregular_uid;   /* lowest irregular storage index and its uid                  */
    uint32_t reserved;    /* 0 */
} gpe_measures;           /* 120 bytes */
typedef struct gpe_monitor_config {
    uint32_t struct_size;   /* in: sizeof(gpe_monitor_config)                         */
    uint32_t flags;         /* in: 0                                                  */
    uint64_t every;         /* in: >= 1: a frame after every every-th step            */
    uint64_t frames;        /* in: >= 1: ring capacity in records                     */
    float    rest_speed;    /* in: >= 0 (+inf, -0.0 accepted): the moving threshold, displacement per step */
    uint32_t reserved;      /* in: ignored                                            */
} gpe_monitor_config;       /* 32 bytes */
typedef struct gpe_monitor_frames {
    uint32_t struct_size;   /* in */
    uint32_t flags;         /* in: 0 or GPE_MONITOR_CONSUME                           */
    uint64_t capacity;      /* in: records `frames` has room for                      */
    uint64_t count;         /* out: records held in the ring (<= config.frames)       */
    uint64_t recorded;      /* out: records taken since begin (held + overwritten + consumed) */
    gpe_measures *frames;   /* out, may be NULL: gpe_measures[capacity]               */
} gpe_monitor_frames;       /* 40 bytes */
/* One record now, step = 0.  Blocks like gpe_download. */
gpe_status gpe_measure(gpe_ctx *ctx, float rest_speed, gpe_measures *out);
/* Arms the recorder: steps_seen = recorded = 0, the ring empty. */
gpe_status gpe_monitor_begin(gpe_ctx *ctx, const gpe_monitor_config *cfg);
gpe_status gpe_monitor_sample(gpe_ctx *ctx);            /* a frame now at the current steps_seen, stream-ordered, no sync */
gpe_status gpe_monitor_read(gpe_ctx *ctx, gpe_monitor_frames *out);
/* Disarms the recorder and frees the ring (the records not read are lost).  Synchronises. */
gpe_status gpe_monitor_end(gpe_ctx *ctx);

/* ---- static colliders (not in the reference) ----------------------------------------------------------------------
 * Obstacles the particles cannot enter: a floor, a funnel, a shelf, a peg.  A collider is a capsule, the segment a -> b
 * thickened by radius R >= 0 (a == b: a disc; R == 0: a thin wall; a chain: a polyline).  While a context holds a set,
 * gpe_step and every iteration of gpe_run run one pass over the particles after the step and before the tracers and
 * the monitor, stream-ordered, on the device (csrc/k_colliders.hip); a tracer or monitor frame sees the projected
 * state.  The per-module calls (gpe_integrate and the rest) run no pass: gpe_apply_colliders is their hook.  A context
 * without colliders launches exactly what it launches without this section.
 *  - The pass.  For a particle with centre p and stored radius r and collider j, in IEEE binary32, one rounding per
 *    operation, left to right, no FMA, `/` and sqrtf correctly rounded (csrc/k_collider.h is the one definition):
 *      a = |r|;  dx = bx-ax; dy = by-ay; fx = px-ax; fy = py-ay;  A = dx*dx + dy*dy
 *      u = 0; if A > 0: u = (fx*dx + fy*dy) / A;  u = (u > 0) ? u : 0;  u = (u < 1) ? u : 1          (NaN -> 0)
 *      qx = fx - u*dx; qy = fy - u*dy;  h = qx*qx + qy*qy;  s = R + a
 *      touched when h < s*s (strict; a NaN anywhere: not touched);  d = sqrtf(h);  depth = s - d
 *      normal: d > 0: (qx/d, qy/d);  else A > 0: L = sqrtf(A), ((-dy)/L, dx/L);  else (1, 0)
 *    Every collider is judged from the position the pass starts with, and only the touched collider with the largest
 *    key bits(depth) << 32 | (0xFFFFFFFF - j) acts: the deepest penetration, the lowest index on a tie.  The particle
 *    moves to (px + nx*depth, py + ny*depth), then K12's clamp: clamp(x, r, W - r), clamp(y, r, H - r), W, H as
 *    gpe_world.  Only pos is written, prev stays: the Verlet velocity loses its component into the obstacle
 *    (inelastic).  A particle no collider touches keeps every bit.  Deepest-only makes the result a function of
 *    (p, r, colliders) alone: the overlapping capsules of a polyline do not push twice at a joint; a corner is
 *    resolved over two steps.
 *  - Without the sweep (below) there is no swept test: a wall thinner than one step's displacement is tunnelled
 *    through.  Make walls thick, or switch the sweep on.
 *  - The sweep.  gpe_set_collider_sweep(ctx, GPE_SWEEP_ON) makes the pass judge a particle by its path prev -> pos of
 *    this step instead of by pos alone (csrc/k_sweep.h is the one definition, csrc/k_sweep.hip the pass; the same
 *    arithmetic rules).  With m = pos - prev and s_j = R_j + |r|:
 *      1. m not finite, or exactly zero in both components: the rule above, on pos (a resting particle gets its bits).
 *      2. the contact of collider j on x(t) = prev + t m: t_j = 0 where prev is touched; else the least t in [0, 1] at
 *         which the path, approaching, meets the band's side or the discs about a and b and the capsule's distance
 *         there obeys d_j <= s_j + 2^-19 (|prevx| + |prevy| + |posx| + |posy|); else t_j = 1 where pos is touched.  With
 *         x_j = x(t_j), d_j and the normal n_j taken there: depth_j = (s_j - d_j) + n_j . (x_j - pos); the contact
 *         counts when depth_j > 0 (a particle moving out of an obstacle it started in has none).
 *      3. the least t_j wins, then the greatest depth_j, then the lowest j.
 *      4. q = clamp(pos + n * depth) as above; with surfaces on the set and a row not flagged GPE_SURFACE_PLAIN, the
 *         surface rule with that normal and depth gives q and prev'.
 *      5. if any collider has a contact on prev -> q with depth_j > 2^-10 * s_j, the particle stops at its first
 *         contact: pos = clamp(x_1 + n_1 * max(s_1 - d_1, 0)), prev untouched, no surface.  Otherwise pos = q (and
 *         prev = prev' where a surface acted).
 *    So a particle ends at a point whose path from prev enters nothing deeper than that slop, or at the first point where
 *    it touched anything; a corner still takes two steps.  What stays a limit: the movers have no sweep
 *    of this mode's making (GPE_SWEEP_ON here leaves their pass plain; theirs is gpe_set_mover_sweep, below); prev is the
 *    position after the step's collision response, so a particle the collision solver shoves across a wall in one step
 *    is not caught (a wall has to be thicker than one collision push, not than one displacement); a particle that
 *    starts on the wrong side of a wall stays there.  The sweep is a mode of the pass, like gravity: allowed with no
 *    colliders set, kept by gpe_set_colliders, gpe_set_surfaces and everything colliders survive.  Off (the default),
 *    the kernels and the bits are those of a context that never heard of it.  gpe_set_collider_sweep waits for the
 *    stream and zeroes the sweep's counters; a mode other than GPE_SWEEP_OFF / GPE_SWEEP_ON: GPE_ERR_INVALID_ARG; on a
 *    sharded context: GPE_ERR_UNSUPPORTED.  gpe_get_sweep_info: passes run in the swept form since the last
 *    gpe_set_collider_sweep, the particles whose winner had 0 < t < 1 (swept) and those that stopped (step 5), summed;
 *    it synchronises.
 *  - Colliders are step state, not observation state: the set survives gpe_set_particles, adds, removals, edits,
 *    re-sorts, growth, gpe_set_world and uids being switched on or off; gpe_destroy frees it.
 *  - The pass finds a particle's colliders through a coarse grid over the world, rebuilt before the next pass when
 *    |gpe_max_radius| or the world has changed (that rebuild synchronises).  No result depends on the grid: a particle
 *    outside it, with a NaN coordinate or with a radius above the bound it was built for is tested against every
 *    collider.
 *  - gpe_set_colliders replaces the set (k == 0 clears it and frees its buffers) and zeroes passes and pushed; it may be
 *    called before there are particles and synchronises like gpe_add_particles.  A host that moves an obstacle calls
 *    it once a frame, or makes it a mover (below).  gpe_get_colliders delivers the first min(k, capacity) colliders into out (may be NULL with
 *    capacity 0) and the number set into *k.  gpe_apply_colliders with no colliders or no particles: GPE_OK, nothing
 *    done.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL colliders with k > 0, k > GPE_COLLIDERS_MAX, a
 *    non-finite coordinate, a radius that is NaN, infinite or negative (-0.0 is accepted as 0), non-zero flags, a
 *    struct_size below the struct's: GPE_ERR_INVALID_ARG.  gpe_set_colliders on a sharded context (gpe_shard_*, order
 *    keys or an active cell box), and gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and gpe_set_counts on a
 *    context that holds colliders: GPE_ERR_UNSUPPORTED. */
#define GPE_COLLIDERS_MAX 4096u
typedef struct gpe_collider { float ax, ay, bx, by, radius; uint32_t flags; } gpe_collider;   /* 24 bytes; flags = 0 */
typedef struct gpe_colliders_info {
    uint32_t struct_size, k;          /* in / colliders set                                             */
    uint64_t passes;                  /* passes run since the last gpe_set_colliders                    */
    uint64_t pushed;                  /* particles moved by those passes, summed (integer atomics only) */
    uint32_t grid_x, grid_y;          /* the lookup grid in use (diagnostic; no result depends on it)   */
    uint64_t list_entries;            /* (cell, collider) entries in it                                 */
} gpe_colliders_info;                 /* 40 bytes */
gpe_status gpe_set_colliders(gpe_ctx *ctx, const gpe_collider *colliders, uint64_t k);
gpe_status gpe_get_colliders(const gpe_ctx *ctx, gpe_collider *out, uint64_t capacity, uint64_t *k);
gpe_status gpe_apply_colliders(gpe_ctx *ctx);                              /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_colliders_info(gpe_ctx *ctx, gpe_colliders_info *info); /* synchronises (reads the device counters) */
#define GPE_SWEEP_OFF 0u
#define GPE_SWEEP_ON 1u
typedef struct gpe_sweep_info {
    uint32_t struct_size, mode;       /* in / GPE_SWEEP_*                                               */
    uint64_t passes;                  /* swept passes run since the last gpe_set_collider_sweep         */
    uint64_t swept;                   /* particles whose winning contact lay at 0 < t < 1, summed       */
    uint64_t stopped;                 /* particles that stopped at their first contact, summed          */
} gpe_sweep_info;                     /* 32 bytes */
gpe_status gpe_set_collider_sweep(gpe_ctx *ctx, uint32_t mode);            /* synchronises */
gpe_status gpe_get_collider_sweep(const gpe_ctx *ctx, uint32_t *mode);
gpe_status gpe_get_sweep_info(gpe_ctx *ctx, gpe_sweep_info *info);         /* synchronises (reads the device counters) */

/* ---- moving colliders (not in the reference) ----------------------------------------------------------------------
 * Obstacles that move: a piston, a lift, a sliding gate, a paddle wheel, a mixer blade.  A mover is a capsule at rest
 * (as gpe_collider) plus a motion: GPE_MOVER_LINEAR slides it along a velocity, for ever (travel == 0) or back and forth
 * over a distance (travel > 0); GPE_MOVER_ROTATE turns it about a pivot at omega radians per second, counter-clockwise,
 * full turns.  The movers are a second set beside the static colliders, independent of them.  While a context holds a
 * set, gpe_step and every iteration of gpe_run advance every mover by dt ON THE DEVICE, rebuild the movers' lookup grid
 * there and run one pass over the particles, stream-ordered, no host round trip (csrc/k_movers.hip): a memset and two
 * launches per step.  Order: step -> bends -> areas -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor: the static
 * walls keep the last word over a piston that squeezes particles against them.  The per-module calls run no pass:
 * gpe_apply_movers(dt) is their hook.  A context without movers launches and allocates exactly what it does without
 * this section.
 *  - The motion (csrc/k_mover.h is the one definition), in IEEE binary32, one rounding per operation, left to right, no
 *    FMA, `/` and sqrtf correctly rounded, no libm sin / cos.  The state of a mover is (q0, q1).
 *    At set time: speed = sqrtf(vx*vx + vy*vy);  u = v / speed, or (0, 0) when speed == 0.
 *    LINEAR, (q0, q1) = (g, sgn), fresh (0, +1):  d = speed*dt;  g1 = g + sgn*d;  with travel > 0: if g1 > travel:
 *      g1 = travel - (g1 - travel), sgn = -sgn; else if g1 < 0: g1 = -g1, sgn = -sgn; then g1 is clamped into
 *      [0, travel].  The posed end points are rest + (g1*ux, g1*uy).
 *    ROTATE, (q0, q1) = (c, s), fresh (1, 0):  x = omega*dt;  x == 0 keeps the state bit for bit;  else x2 = x*x,
 *      sa = x + x*(x2*(S0 + x2*(S1 + x2*(S2 + x2*S3)))),  S = -1/6, 1/120, -1/5040, 1/362880 as binary32,
 *      ca = 1 + x2*(C0 + x2*(C1 + x2*(C2 + x2*(C3 + x2*C4)))),  C = -1/2, 1/24, -1/720, 1/40320, -1/3628800,
 *      c2 = c*ca - s*sa;  s2 = s*ca + c*sa;  m = sqrtf(c2*c2 + s2*s2);  (c, s) = (c2/m, s2/m).
 *      A posed end point is p + (rx*c - ry*s, rx*s + ry*c) with r = rest - p.
 *    Over |x| <= 0.5 the polynomial is within 3.9e-8 of sin and cos; the orientation stays within 2^-21 of unit length
 *    and its angle within steps * 2^-22 rad of steps * omega*dt.
 *  - The dt contract: |omega*dt| <= 0.5 for every ROTATE mover (the polynomial's range), and speed*|dt| <= travel for
 *    every LINEAR mover with travel > 0 (one reflection per step suffices); dt is finite.  It is checked on the host,
 *    against the set's largest |omega| and, among the movers that go back and forth, the largest speed and the smallest
 *    travel, before gpe_step, gpe_run and gpe_apply_movers launch anything: a violation is GPE_ERR_INVALID_ARG and the
 *    context is as if the call had not been made.
 *  - The pass.  After the advance every particle is pushed out of the posed mover it penetrates deepest: the static
 *    colliders' touch, key, normal and clamp (above), unchanged, every mover judged from the position the pass starts
 *    with.  Only pos is written, prev stays: in a Verlet engine that hands the particle the wall's velocity.  A particle
 *    no mover touches keeps every bit.
 *  - Without the movers' sweep (next item) there is no swept test: a mover must be thicker than one step's relative
 *    displacement of mover and particle.  Make movers thick, or switch their sweep on.
 *  - The movers' sweep.  gpe_set_mover_sweep(ctx, GPE_SWEEP_ON) makes the pass judge a particle by its path RELATIVE TO
 *    EACH MOVER over the step (csrc/k_mover_sweep.h is the one definition, csrc/k_mover_sweep.hip the build and the
 *    pass; the same arithmetic rules).  With C0_j and C1_j mover j's capsule before and after this step's advance:
 *      1. y0_j = prev carried rigidly with mover j over the step: LINEAR: prev + (a1 - a0); ROTATE: prev turned about
 *         the pivot by (cd, sd) = (c1*c0 + s1*s0, s1*c0 - c1*s0).  A mover whose state did not change: y0_j = prev,
 *         bit for bit.  The relative path is taken as the chord y0_j -> pos.
 *      2. pos - y0_j not finite, or exactly zero: mover j judges the particle by the plain touch at pos, a contact with
 *         t = 1.  (A particle at rest under a mover at rest: the plain pass's contact.)
 *      3. a turning ROTATE mover is considered only if the world path prev -> pos comes within (arm_j + R_j) + |r| of
 *         its pivot, arm_j the farthest end of the rest capsule from the pivot: the chord of a fast particle can cut
 *         through a disc its true path never enters.
 *      4. the contact of the static sweep (above) on y0_j -> pos against C1_j; the least t wins, then the greatest depth,
 *         then the lowest j.
 *      5. q = clamp(pos + n * depth); with a surface on the winner (not GPE_SURFACE_PLAIN, pos - prev finite) the
 *         surface rule with that normal and depth and the wall's displacement at the contact gives q and prev'.
 *      6. verified once: if any mover has a contact (1 to 4 with q for pos) deeper than 2^-10 * s_j the particle stops
 *         at its first contact, prev untouched, no surface.
 *    Guaranteed: a particle that starts the step on one side of a blade, relative to the blade, and whose chord crosses
 *    the blade's stretch does not end on the other side.  Not: the chord is off by up to |omega*dt| * |pos - prev| / 4
 *    between its ends (fast particles near rotors); the collision solver's own pushes are not swept; a particle that
 *    starts inside the capsule is pushed as before; two movers closing on one particle are resolved by the first
 *    contact and the one verification, no further.  In this mode the build lists a mover in every cell its motion
 *    reaches (a LINEAR mover's parallelogram, a ROTATE mover's disc); no result depends on the grid.  The mode is step
 *    state like gravity, independent of gpe_set_collider_sweep: allowed with no movers set, kept by gpe_set_movers
 *    (also with k == 0), gpe_set_surfaces, gpe_set_mover_poses and everything movers survive; gpe_apply_movers follows
 *    it.  Off (the default), the kernels and the bits are those of a context that never heard of it.
 *    gpe_set_mover_sweep waits for the stream and zeroes the two counters; a mode other than GPE_SWEEP_OFF /
 *    GPE_SWEEP_ON: GPE_ERR_INVALID_ARG; on a sharded context: GPE_ERR_UNSUPPORTED.  gpe_get_mover_sweep_info fills a
 *    gpe_sweep_info: passes run in the swept form since the last gpe_set_mover_sweep, the particles whose winner had
 *    0 < t < 1 (swept) and those that stopped (6), summed; it synchronises.
 *  - The set and the poses are step state: they survive gpe_set_particles, adds, removals, edits, re-sorts, growth and
 *    gpe_set_world; gpe_destroy frees them.  Movers name no particle.
 *  - The pass finds a particle's movers through a coarse grid (at most 128 x 128 cells) of bit masks, built on the
 *    device every step from the posed capsules for |gpe_max_radius| and the world as they are then.  No result depends
 *    on the grid: a particle outside it, with a NaN coordinate or with a radius above the bound is tested against every
 *    mover.
 *  - gpe_set_movers replaces the set (k == 0 clears it and frees its buffers), resets every pose to its fresh state and
 *    zeroes passes and pushed; it synchronises like gpe_add_particles.  gpe_get_movers delivers the first
 *    min(k, capacity) movers into out (may be NULL with capacity 0) and the number set into *k; a radius of -0.0 reads
 *    back as +0.  gpe_get_mover_poses does the same with the current capsule and state of every mover, and
 *    synchronises.  gpe_set_mover_poses restores the states (k must be the set's size): ax .. by of the input are
 *    ignored and recomputed from the state.  gpe_apply_movers(dt) advances once and runs one pass now, stream-ordered,
 *    no sync; with no movers or no particles: GPE_OK, nothing done.  gpe_get_movers_info synchronises; `listed` is the
 *    number of (cell, mover) bits the last build set.
 *  - Errors (the previous set and poses stay untouched): a NULL ctx, NULL movers with k > 0, k > GPE_MOVERS_MAX, a value
 *    that is not finite (a velocity whose speed overflows included), a radius that is NaN or negative (-0.0 is accepted
 *    as 0), an unknown kind, flags or reserved not 0, travel < 0; for gpe_set_mover_poses a k that is not the set's
 *    size, a state that is not finite, a LINEAR sgn that is not +1 or -1, a g outside [0, travel] when travel > 0; a
 *    struct_size below the struct's: GPE_ERR_INVALID_ARG.  gpe_set_movers on a sharded context, and
 *    gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and gpe_set_counts on a context that holds movers:
 *    GPE_ERR_UNSUPPORTED. */
#define GPE_MOVERS_MAX 1024u
enum { GPE_MOVER_LINEAR = 0, GPE_MOVER_ROTATE = 1 };
typedef struct gpe_mover {
    float ax, ay, bx, by, radius;     /* the capsule at rest (as gpe_collider)                               */
    uint32_t kind;                    /* GPE_MOVER_*                                                         */
    float vx, vy;                     /* LINEAR: velocity, world units per second                            */
    float travel;                     /* LINEAR: > 0: back and forth over this distance along v; 0: for ever */
    float px, py;                     /* ROTATE: the pivot                                                   */
    float omega;                      /* ROTATE: radians per second, counter-clockwise, full turns           */
    uint32_t flags;                   /* 0                                                                   */
    uint32_t reserved;                /* 0                                                                   */
} gpe_mover;                          /* 56 bytes */
typedef struct gpe_mover_pose { float ax, ay, bx, by, q0, q1; } gpe_mover_pose;   /* 24 bytes: the posed capsule, the state */
typedef struct gpe_movers_info {
    uint32_t struct_size, k;          /* in / movers set                                                */
    uint64_t passes;                  /* passes run since the last gpe_set_movers                       */
    uint64_t pushed;                  /* particles moved by those passes, summed (integer atomics only) */
    uint32_t grid_x, grid_y;          /* the lookup grid of the last build (diagnostic)                 */
    uint32_t mask_words, reserved;    /* 64-bit mask words per cell: ceil(k / 64)                       */
    uint64_t listed;                  /* (cell, mover) bits the last build set                          */
} gpe_movers_info;                    /* 48 bytes */
gpe_status gpe_set_movers(gpe_ctx *ctx, const gpe_mover *movers, uint64_t k);
gpe_status gpe_get_movers(const gpe_ctx *ctx, gpe_mover *out, uint64_t capacity, uint64_t *k);
gpe_status gpe_get_mover_poses(gpe_ctx *ctx, gpe_mover_pose *out, uint64_t capacity, uint64_t *k);   /* synchronises */
gpe_status gpe_set_mover_poses(gpe_ctx *ctx, const gpe_mover_pose *poses, uint64_t k);
gpe_status gpe_apply_movers(gpe_ctx *ctx, float dt);                       /* advance + one pass now, stream-ordered, no sync */
gpe_status gpe_get_movers_info(gpe_ctx *ctx, gpe_movers_info *info);       /* synchronises (reads the device counters) */
gpe_status gpe_set_mover_sweep(gpe_ctx *ctx, uint32_t mode);               /* GPE_SWEEP_*; synchronises */
gpe_status gpe_get_mover_sweep(const gpe_ctx *ctx, uint32_t *mode);
gpe_status gpe_get_mover_sweep_info(gpe_ctx *ctx, gpe_sweep_info *info);   /* synchronises (reads the device counters) */

/* ---- surface materials (not in the reference) ----------------------------------------------------------------------
 * Bounce and friction, per obstacle: a ball that rebounds from the floor, a particle that slides to a halt, a shelf
 * things stay on, a drum or a plate that drags its load along.  A surface is one row per static collider or per mover:
 * restitution e in [0, 1], friction mu >= 0, flags.  Without surfaces the two passes write pos only (above).  While a
 * set holds surfaces its pass runs in a second form (csrc/k_colliders.hip, csrc/k_movers.hip: the same lookup, the same
 * winner) that also reads and writes prev for the particles an obstacle touches -- and for no others: a particle
 * nothing touches costs what it costs without surfaces.  gpe_step, gpe_run, gpe_apply_colliders and gpe_apply_movers
 * all pick it up; the order of the passes stays.  A context that sets no surface launches, allocates and computes
 * exactly what it does without this section.
 *  - The rule (csrc/k_surface.h is the one definition).  The acting obstacle is chosen exactly as above: the deepest
 *    penetration, the lowest index on a tie, every obstacle judged from the position the pass starts with.  Inputs: that
 *    position p, the previous position prev, the radius r, the normal n and the depth of the touch, its clamped
 *    parameter u, and the wall's displacement w at the contact over this step.  IEEE binary32, one rounding per
 *    operation, left to right, no FMA, `/` and sqrtf correctly rounded:
 *      q   = (px + nx*depth, py + ny*depth)                      the plain pass's push, the same bits
 *      v   = p - prev;   rel = v - w
 *      vn  = relx*nx + rely*ny
 *      t   = (relx - vn*nx, rely - vn*ny)                        the tangential part, t0 = t
 *      on  = (vn < 0) ? (-e)*vn : vn                             approaching: reflected and damped; separating: kept
 *      jn  = on - vn                                             the normal velocity change, >= 0
 *      tl  = sqrtf(tx*tx + ty*ty);   s = mu*jn
 *      if s < tl:  k = (tl - s)/tl;  t = (tx*k, ty*k)            sliding: Coulomb, the change bounded by mu*jn
 *      else:       t = (0, 0)                                    sticking
 *      out = ((wx + on*nx) + tx, (wy + on*ny) + ty)              the velocity the particle leaves with
 *      pos' = clamp(q - (t0 - t))                                K12's clamp as in the plain pass
 *      prev' = pos' - out
 *    The tangential velocity that friction removes is taken out of the position too; without that a particle that
 *    sticks on a slope creeps down by g*dt^2*sin every step.  With mu = 0, t0 - t is +0 and pos' carries the bits of
 *    the plain pass.  A particle nothing touches keeps every bit of pos and prev.
 *  - The wall's displacement.  A static collider: w = (0, 0).  A mover: what the contact point moved in this step's
 *    advance.  The posed capsule before the advance is (a0, b0), after it (a1, b1), the touch is taken against
 *    (a1, b1):  wa = a1 - a0; wb = b1 - b0; w = wa + u*(wb - wa)  per component.  The old capsule is a function of the
 *    state (q0, q1) alone: gpe_get_mover_poses / gpe_set_mover_poses carry all a host needs to continue a run.
 *  - Two escapes keep the bits of the plain rule, pos pushed and prev untouched: a row whose flags has
 *    GPE_SURFACE_PLAIN (a host gives a material to some obstacles only), and a particle whose p - prev is not finite
 *    in either component.
 *  - What a surface is not.  It has no effect on particle-particle contacts: a pile above its bottom layer is as
 *    slippery as before.  There is no rolling and no spin.  A corner is still resolved by the deepest obstacle, over
 *    two steps; there is still no swept test.  Friction sees the normal velocity change of this pass only: a particle
 *    pressed on a wall by its neighbours and not by its own velocity feels little of it.
 *  - gpe_set_surfaces: row j belongs to collider j (GPE_SURFACES_OF_COLLIDERS) or mover j (GPE_SURFACES_OF_MOVERS) of
 *    the set held at the call; k must equal that set's size; k == 0 clears the surfaces and frees their buffer.  It
 *    synchronises like gpe_set_colliders.  gpe_set_colliders and gpe_set_movers drop their target's surfaces (k == 0
 *    included): a new set gets new surfaces.  Surfaces are step state: they survive everything their set survives.
 *    gpe_get_surfaces delivers the first min(k, capacity) rows into out (may be NULL with capacity 0) and the number
 *    set into *k (0: none); -0.0 reads back as +0.
 *  - Errors (the previous surfaces stay untouched): a NULL ctx, NULL rows with k > 0, an unknown target, a k that is
 *    not 0 and not the set's size, a restitution that is NaN or outside [0, 1], a friction that is NaN, infinite or
 *    negative, an unknown flag, a non-zero reserved; for gpe_get_surfaces a NULL k or NULL out with a capacity:
 *    GPE_ERR_INVALID_ARG.  gpe_set_surfaces with k > 0 on a sharded context: GPE_ERR_UNSUPPORTED. */
enum { GPE_SURFACES_OF_COLLIDERS = 0, GPE_SURFACES_OF_MOVERS = 1 };
enum { GPE_SURFACE_PLAIN = 1u };
typedef struct gpe_surface { float restitution, friction; uint32_t flags, reserved; } gpe_surface;   /* 16 bytes */
gpe_status gpe_set_surfaces(gpe_ctx *ctx, uint32_t target, const gpe_surface *rows, uint64_t k);
gpe_status gpe_get_surfaces(const gpe_ctx *ctx, uint32_t target, gpe_surface *out, uint64_t capacity, uint64_t *k);

/* ---- distance bonds (not in the reference) ------------------------------------------------------------------------
 * Ties between particles: a rope, a chain, a cloth, a soft body, a pinned object, a sheet that tears.  A bond holds two
 * particles, named by uid (gpe_enable_uids must be on), at a rest length; an anchor bond (GPE_BOND_ANCHOR) holds one
 * particle to a fixed point.  While a context holds a set, gpe_step and every iteration of gpe_run run one pass after
 * the step, BEFORE the static colliders (walls keep the last word) and the tracers and the monitor, stream-ordered, on
 * the device (csrc/k_bonds.hip): step -> bends -> areas -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor.  The per-module calls run no pass:
 * gpe_apply_bonds is their hook.  A context without bonds launches and allocates exactly what it does without this
 * section.
 *  - One relaxation (csrc/k_bond.h is the one definition).  Every bond is judged from the positions the relaxation
 *    starts with, in IEEE binary32, one rounding per operation, left to right, no FMA, `/` and sqrtf correctly
 *    rounded; a = particle uid_a, b = particle uid_b or the anchor point:
 *      dx = bx-ax; dy = by-ay;  h = dx*dx + dy*dy;  d = sqrtf(h)
 *      inert this relaxation unless d > 0 and d < +inf         (NaN, coincident centres, overflow: left alone)
 *      if max_length > 0 and d > max_length: the bond breaks   (strict; sticky: it never acts again)
 *      e = d - rest_length;  f = e / d;  g = f * w;  cx = g*dx;  cy = g*dy
 *    a receives (+cx, +cy), b (-cx, -cy); w = 0.5f * stiffness for a pair, stiffness for an anchor (whose point
 *    receives nothing).  A bond one of whose uids names no live particle is inert and NOT broken: it acts again when
 *    the uid reappears (gpe_set_uids).  A particle with at least one acting bond moves to p + acc, acc summed from
 *    +0.0f over its acting bonds in ascending bond index (inert and broken bonds are skipped, not added as zero), then
 *    K12's clamp with its stored radius: clamp(x, r, W - r), clamp(y, r, H - r).  Only pos is written: prev and radius
 *    never, so the velocity change is the one Verlet implies.  Every other particle keeps every bit, unclamped.
 *  - A pass relaxes the set `iterations` times (Jacobi: no relaxation reads what it has written itself), so the
 *    result depends on the set and the particles alone, never on launch order, storage order or mode.
 *  - What a bond is not: there is no angular constraint (a chain folds freely: the bends below, gpe_set_bends, hold
 *    angles); Jacobi relaxation converges slowly
 *    along stiff long chains, which need iterations; a rest length below the sum of the two radii fights the collision
 *    solver, which pushes the pair apart again in the next step.
 *  - The set and its broken flags are step state: they survive adds, removals, edits, kicks, re-sorts, growth,
 *    gpe_set_mode and gpe_set_particles (which renumbers the uids from 0: the bonds then name the new particles).  After
 *    a call that moves, adds or removes particles the next pass looks its uids up again (that synchronises once); every
 *    other pass only enqueues.
 *  - gpe_set_bonds replaces the set (k == 0 clears it and frees its buffers), clears the broken flags and zeroes the
 *    counters; it synchronises.  A bond given with GPE_BOND_BROKEN starts broken: that is how a snapshot restores one;
 *    the bit is not kept in the record.  -0.0 in rest_length / max_length is stored as +0.  The same pair may be
 *    listed twice: both bonds act.  gpe_get_bonds delivers the first min(k, capacity) records into out and their
 *    broken flags (1 / 0) into broken_out (each may be NULL) and the number set into *k; it synchronises.
 *    gpe_apply_bonds with no bonds or no particles: GPE_OK, nothing done.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL bonds with k > 0, k > GPE_BONDS_MAX, iterations
 *    outside 1 .. GPE_BOND_ITER_MAX, a rest_length or max_length that is NaN, infinite or negative, a stiffness that is
 *    NaN or outside [0, 1], unknown flag bits, uid_a == GPE_UID_ABSENT, uid_a == uid_b, an anchor whose uid_b is not
 *    GPE_UID_ABSENT or a pair whose uid_b is, a non-finite anchor coordinate, a uid with more than GPE_BOND_MAX_DEGREE
 *    bonds, a struct_size below the struct's: GPE_ERR_INVALID_ARG.  Uids off: GPE_ERR_STATE.  gpe_set_bonds on a
 *    sharded context, and gpe_enable_uids(ctx, 0), gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and
 *    gpe_set_counts on a context that holds bonds: GPE_ERR_UNSUPPORTED. */
#define GPE_BONDS_MAX        4194304u   /* a 1 M-particle sheet has about 2 M structural bonds */
#define GPE_BOND_MAX_DEGREE  1024u      /* bonds per particle: one lane walks them in order */
#define GPE_BOND_ITER_MAX    32u
#define GPE_BOND_ANCHOR      1u         /* flags: uid_b unused, a is tied to (anchor_x, anchor_y) */
#define GPE_BOND_BROKEN      2u         /* flags, gpe_set_bonds only: the bond starts broken */
typedef struct gpe_bond {               /* 32 bytes */
    uint32_t uid_a, uid_b;              /* uid_b == GPE_UID_ABSENT iff GPE_BOND_ANCHOR */
    float rest_length;                  /* finite, >= 0 */
    float stiffness;                    /* in [0, 1]: the share of the error removed per relaxation */
    float max_length;                   /* finite, >= 0; 0: never breaks; else breaks once its length > max_length */
    uint32_t flags;
    float anchor_x, anchor_y;           /* finite; read only with GPE_BOND_ANCHOR */
} gpe_bond;
typedef struct gpe_bonds_info {
    uint32_t struct_size, iterations;  /* in / relaxations per pass                                        */
    uint64_t k, nodes;                 /* bonds set / distinct uids they name                              */
    uint64_t passes;                   /* passes enqueued since the last gpe_set_bonds                     */
    uint64_t live, broken;             /* bonds not broken / broken (integer atomics only); live + broken = k */
    uint64_t resolves;                 /* times the uids were looked up again since the last gpe_set_bonds */
} gpe_bonds_info;                      /* 56 bytes */
gpe_status gpe_set_bonds(gpe_ctx *ctx, const gpe_bond *bonds, uint64_t k, uint32_t iterations);
gpe_status gpe_get_bonds(gpe_ctx *ctx, gpe_bond *out, uint8_t *broken_out, uint64_t capacity, uint64_t *k);
gpe_status gpe_apply_bonds(gpe_ctx *ctx);                          /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_bonds_info(gpe_ctx *ctx, gpe_bonds_info *info); /* synchronises (reads the device counter) */

/* ---- the bonds' solver: Jacobi or coloured Gauss-Seidel (not in the reference) ------------------------------------
 * A mode of the bonds' pass, off (GPE_BOND_SOLVER_JACOBI) by default; step state like gpe_set_collider_sweep: allowed
 * with no set present, it outlives gpe_set_bonds, every add, removal, edit and re-sort, and gpe_set_world.  Jacobi
 * judges every bond from the positions a relaxation starts with: stable only up to a stiffness of 1 / (bonds per
 * particle), and slow along chains.  GPE_BOND_SOLVER_COLOURED relaxes the bonds one colour after the other, every
 * bond seeing the corrections of the colours before it: stiffness 1 is stable whatever the degree, and a hanging rope
 * keeps about a quarter of the excess stretch Jacobi leaves it at the same number of relaxations.  The place of the
 * pass, gpe_get_bonds, gpe_get_bonds_info, gpe_apply_bonds and the broken flags are the same in both modes.
 *  - The colouring (csrc/bond_colours.h is the one definition) is a function of the set alone.  In ascending bond
 *    index j, colour[j] = the least c >= 0 that no bond of lower index has taken at particle uid_a, nor at uid_b for a
 *    pair (an anchor occupies uid_a only).  Broken bonds, bonds whose uid no particle has and both twins of a bond
 *    listed twice are coloured too.  No two bonds of one colour share a particle.
 *  - One coloured relaxation: for c = 0 .. colours - 1, every bond of colour c is judged as above (the same d, break,
 *    e, f, g, cx, cy, the same w) from the positions as they are NOW; where it acts, a moves to
 *    clamp(a + (cx, cy)) and, for a pair, b to clamp(b + (-cx, -cy)), K12's clamp with the particle's own radius; where
 *    it breaks, it is broken from then on; inert otherwise.  Within a colour no position has two writers, so the
 *    result equals a sequential sweep of the bonds in (colour, index) order: a binary32 function of the set and the
 *    particles alone, never of launch order, storage order or pipeline mode -- but the order of the colours, and so
 *    the order of the bonds in the set, is part of the result.  A pass runs `iterations` such relaxations and writes
 *    pos only.
 *  - What it is not: the bends and the areas stay Jacobi; a set that needs more than GPE_BOND_COLOURS_MAX colours is
 *    refused (greedy needs at most 2 * degree - 1, so every set of at most 32 bonds per particle fits; a hub of 200
 *    bonds stays with Jacobi); there is no coloured solver in sharded runs.
 *  - gpe_set_bond_solver synchronises; over a set it builds (COLOURED) or frees (JACOBI) the colour tables, keeps the
 *    set, its broken flags and its counters, and zeroes `passes` and `form` of the info below.  Under COLOURED,
 *    gpe_set_bonds builds the tables with the set.  With the mode JACOBI the kernels launched, the buffers held and
 *    every bit are those of a context that never heard of the mode.
 *  - gpe_get_bond_solver_info: the mode; colours and largest_colour of the set held (0 without one, or under JACOBI);
 *    form: how the last coloured pass ran -- 0 none yet, 1 one launch per colour and relaxation, 2 one launch of one
 *    workgroup that keeps the set's particles in LDS, taken when the set names at most lds_nodes_max particles; both
 *    forms give the same bits.
 *  - Errors (the previous set, mode and tables stay untouched): a NULL ctx, an unknown mode, a struct_size below the
 *    struct's, and -- from gpe_set_bond_solver(COLOURED) over a set as from gpe_set_bonds under COLOURED -- a set
 *    that needs more than GPE_BOND_COLOURS_MAX colours (the message names the count): GPE_ERR_INVALID_ARG.  A sharded
 *    context: GPE_ERR_UNSUPPORTED -- for either mode, JACOBI included, though it is what such a context runs anyway:
 *    the call is refused as a whole there, like gpe_set_collider_sweep, and gpe_get_bond_solver reads JACOBI. */
#define GPE_BOND_COLOURS_MAX      64u
#define GPE_BOND_SOLVER_JACOBI    0u
#define GPE_BOND_SOLVER_COLOURED  1u
typedef struct gpe_bond_solver_info {
    uint32_t struct_size, mode;        /* in / GPE_BOND_SOLVER_*                                               */
    uint32_t colours, largest_colour;  /* of the set held under COLOURED: colours / bonds in the fullest one  */
    uint32_t form, lds_nodes_max;      /* the last coloured pass's launch form (0, 1, 2) / form 2's node limit */
    uint64_t passes;                   /* coloured passes enqueued since the last gpe_set_bond_solver          */
} gpe_bond_solver_info;                /* 32 bytes */
gpe_status gpe_set_bond_solver(gpe_ctx *ctx, uint32_t mode);          /* synchronises */
gpe_status gpe_get_bond_solver(gpe_ctx *ctx, uint32_t *mode);
gpe_status gpe_get_bond_solver_info(gpe_ctx *ctx, gpe_bond_solver_info *info);

/* ---- bend constraints (not in the reference) ----------------------------------------------------------------------
 * Angles between bonded particles: a rope with stiffness, grass and hair that spring back, a cloth that resists
 * folding, an articulated shape that holds a rest angle.  A bend names three distinct particles by uid (gpe_enable_uids
 * must be on): a, the hinge b, and c, and holds the angle from u = a - b to v = c - b at a rest angle, given as
 * (rest_cos, rest_sin) so that neither side needs libm.  It tells a fold to the left from a fold to the right, and
 * is stiff to first order at a straight rest pose; a distance bond from a to c is neither.  While a context holds a
 * set, gpe_step and every iteration of gpe_run run one pass after the step, IN FRONT OF the distance bonds (lengths
 * keep the last word over angles, walls over both), stream-ordered, on the device (csrc/k_bends.hip):
 * step -> bends -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor (area constraints, where held,
 * run between the bends and the bonds: step -> bends -> areas -> bonds).  The per-module calls run no
 * pass: gpe_apply_bends is their hook.  A context without bends launches and allocates exactly what it does without
 * this section.
 *  - One relaxation (csrc/k_bend.h is the one definition).  Every bend is judged from the positions the relaxation
 *    starts with, in IEEE binary32, one rounding per operation, left to right, no FMA, `/` and sqrtf correctly
 *    rounded; rc = rest_cos, rs = rest_sin:
 *      ux = ax-bx; uy = ay-by; vx = cx-bx; vy = cy-by
 *      lu = ux*ux + uy*uy;  lv = vx*vx + vy*vy
 *      tx = rc*ux - rs*uy;  ty = rs*ux + rc*uy            (u turned by the rest angle)
 *      cr = tx*vy - ty*vx;  dt = tx*vx + ty*vy
 *      den = sqrtf(lu*lv)
 *      inert this relaxation unless lu > 0, lv > 0, den > 0 and den < +inf   (NaN fails every comparison)
 *      s = cr / den;  if dt < 0: s = (cr < 0) ? -1 : +1   (more than 90 degrees off: the largest correction)
 *      inert if s != s
 *      gax = uy/lu; gay = -ux/lu;  gcx = -vy/lv; gcy = vx/lv;  gbx = -(gax+gcx); gby = -(gay+gcy)
 *      q = ((gax*gax + gay*gay) + (gcx*gcx + gcy*gcy)) + (gbx*gbx + gby*gby)
 *      inert unless q > 0 and q < +inf
 *      m = s * stiffness;  lam = -m / q
 *      da = (lam*gax, lam*gay);  dc = (lam*gcx, lam*gcy);  db = (-(da.x + dc.x), -(da.y + dc.y))
 *    This is the position-based-dynamics step on C = sin(deviation) with equal masses: the three corrections sum to
 *    zero.  An exact fold-back (cr == 0, dt < 0) turns with s = +1.  A bend one of whose uids names no live particle
 *    is inert: it acts again when the uid reappears (gpe_set_uids).  A particle with at least one acting bend moves to
 *    p + acc, acc summed from +0.0f over its acting bends in ascending bend index (inert bends are skipped, not added
 *    as zero; the hinge's share is formed as -(da + dc) where it is added), then K12's clamp with its stored radius:
 *    clamp(x, r, W - r), clamp(y, r, H - r).  Only pos is written: prev and radius never.  Every other particle keeps
 *    every bit, unclamped.  Bends do not break.
 *  - A pass relaxes the set `iterations` times (Jacobi: no relaxation reads what it has written itself), so the
 *    result depends on the set and the particles alone, never on launch order, storage order or mode.
 *  - What a bend is not: Jacobi relaxation is weak along long chains (a 32-particle cantilever droops almost as
 *    without bends); a stiffness above about 0.5 on a chain overshoots, because each interior particle sits in three
 *    bends; a bend shortens its arms to second order, and the bonds behind it restore them.  There are no breaking
 *    bends, no motorised rest angles, no per-particle mass, no bends in sharded runs, and bend and bond relaxations
 *    are not interleaved.  (gpe_set_bend_solver, below, relaxes the set colour after colour in place of Jacobi: it
 *    lifts the limit on the stiffness, not the weakness along long chains.)
 *  - The set is step state: it survives adds, removals, edits, kicks, re-sorts, growth, gpe_set_mode, gpe_set_world
 *    and gpe_set_particles (which renumbers the uids from 0: the bends then name the new particles).  After a call
 *    that moves, adds or removes particles the next pass looks its uids up again (that synchronises once); every other
 *    pass only enqueues.
 *  - gpe_set_bends replaces the set (k == 0 clears it and frees its buffers) and zeroes the counters; it
 *    synchronises.  -0.0 in rest_cos / rest_sin / stiffness is stored as +0.  The same triple may be listed twice:
 *    both bends act.  gpe_get_bends delivers the first min(k, capacity) records into out and the number set into *k.
 *    gpe_apply_bends with no bends or no particles: GPE_OK, nothing done.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL bends with k > 0, k > GPE_BENDS_MAX, iterations
 *    outside 1 .. GPE_BEND_ITER_MAX, a uid that is GPE_UID_ABSENT, two of the three uids equal, a rest_cos or rest_sin
 *    that is not finite or |rest_cos^2 + rest_sin^2 - 1| > 2^-20 in binary32, a stiffness that is NaN or outside
 *    [0, 1], nonzero flags or reserved, a uid with more than GPE_BEND_MAX_DEGREE bends, a struct_size below the
 *    struct's: GPE_ERR_INVALID_ARG.  Uids off: GPE_ERR_STATE.  gpe_set_bends on a sharded context, and
 *    gpe_enable_uids(ctx, 0), gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and gpe_set_counts on a context
 *    that holds bends: GPE_ERR_UNSUPPORTED. */
#define GPE_BENDS_MAX        4194304u   /* a 1 M-particle sheet has about 2 M bends along rows and columns */
#define GPE_BEND_MAX_DEGREE  1024u      /* bends per particle, any role: one lane walks them in order */
#define GPE_BEND_ITER_MAX    32u
typedef struct gpe_bend {               /* 32 bytes */
    uint32_t uid_a, uid_b, uid_c;       /* distinct, none GPE_UID_ABSENT; b is the hinge */
    float rest_cos, rest_sin;           /* finite; |rest_cos^2 + rest_sin^2 - 1| <= 2^-20 in binary32 */
    float stiffness;                    /* in [0, 1] */
    uint32_t flags, reserved;           /* both 0 */
} gpe_bend;
typedef struct gpe_bends_info {
    uint32_t struct_size, iterations;  /* in / relaxations per pass                                        */
    uint64_t k, nodes;                 /* bends set / distinct uids they name                              */
    uint64_t passes;                   /* passes enqueued since the last gpe_set_bends                     */
    uint64_t resolves;                 /* times the uids were looked up again since the last gpe_set_bends */
} gpe_bends_info;                      /* 40 bytes */
gpe_status gpe_set_bends(gpe_ctx *ctx, const gpe_bend *bends, uint64_t k, uint32_t iterations);
gpe_status gpe_get_bends(const gpe_ctx *ctx, gpe_bend *out, uint64_t capacity, uint64_t *k);
gpe_status gpe_apply_bends(gpe_ctx *ctx);                          /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_bends_info(gpe_ctx *ctx, gpe_bends_info *info);

/* ---- the bends' solver: Jacobi or coloured Gauss-Seidel (not in the reference) ------------------------------------
 * A mode of the bends' pass, off (GPE_BEND_SOLVER_JACOBI) by default, shaped like gpe_set_bond_solver and independent
 * of it; step state: allowed with no set present, it outlives gpe_set_bends, every add, removal, edit and re-sort, and
 * gpe_set_world.  Jacobi judges every bend from the positions a relaxation starts with: on a chain every interior
 * particle sits in three bends, so a stiffness above about 0.5 overshoots.  GPE_BEND_SOLVER_COLOURED relaxes the bends
 * one colour after the other, every bend seeing the corrections of the colours before it: stiffness 1 is stable, and
 * an 8-particle cantilever with one relaxation per pass droops less than half as far as under Jacobi at stiffness 0.5
 * (4.78 against 10.44 on the CPU model; 12.20 without bends).  The place of the pass, gpe_get_bends,
 * gpe_get_bends_info and gpe_apply_bends are the same in both modes.
 *  - The colouring (csrc/bend_colours.h is the one definition) is a function of the set alone.  In ascending bend
 *    index j, colour[j] = the least c >= 0 that no bend of lower index has taken at particle uid_a, at the hinge uid_b
 *    or at uid_c.  Bends whose uid no particle has and both twins of a bend listed twice are coloured too.  No two
 *    bends of one colour share a particle.  A chain listed in order takes 3 colours.
 *  - One coloured relaxation: for c = 0 .. colours - 1, every bend of colour c is judged as above (the same da, dc,
 *    the same inert verdicts) from the positions as they are NOW; where it acts, it moves its three particles itself:
 *    a to clamp(a + da), c to clamp(c + dc) and the hinge to clamp(b + (-(da.x + dc.x), -(da.y + dc.y))), K12's clamp
 *    with the particle's own radius; a bend with an absent uid or an inert verdict moves nothing.  Within a colour no
 *    position has two writers, so the result equals a sequential sweep of the bends in (colour, index) order: a
 *    binary32 function of the set and the particles alone, never of launch order, storage order or pipeline mode --
 *    but the order of the colours, and so the order of the bends in the set, is part of the result.  A pass runs
 *    `iterations` such relaxations and writes pos only.
 *  - What it is not: it is for short stiff pieces (grass, hair segments, hinges, cloth folds) at stiffness 1, not for
 *    long beams -- a 16-particle cantilever droops 26 to 27 against 28.2 free with either solver, because the rule
 *    converges slowly along a chain whatever its order.  The areas stay Jacobi, and the bonds have a solver of their
 *    own.  Bends and bonds are still separate passes: their relaxations are not interleaved.  A set that needs more
 *    than GPE_BEND_COLOURS_MAX colours is refused (greedy needs at most 3 * (degree - 1) + 1, so every set of at most 22
 *    bends per particle fits); there is no coloured solver in sharded runs.
 *  - gpe_set_bend_solver synchronises; over a set it builds (COLOURED) or frees (JACOBI) the colour tables, keeps the
 *    set and its counters, and zeroes `passes` and `form` of the info below.  Under COLOURED, gpe_set_bends builds the
 *    tables with the set.  With the mode JACOBI the kernels launched, the buffers held and every bit are those of a
 *    context that never heard of the mode.
 *  - gpe_get_bend_solver_info: the mode; colours and largest_colour of the set held (0 without one, or under JACOBI);
 *    form: how the last coloured pass ran -- 0 none yet, 1 one launch per colour and relaxation, 2 one launch of one
 *    workgroup that keeps the set's particles in LDS, taken when the set names at most lds_nodes_max particles; both
 *    forms give the same bits.
 *  - Errors (the previous set, mode and tables stay untouched): a NULL ctx, an unknown mode, a struct_size below the
 *    struct's, and -- from gpe_set_bend_solver(COLOURED) over a set as from gpe_set_bends under COLOURED -- a set
 *    that needs more than GPE_BEND_COLOURS_MAX colours (the message names the count): GPE_ERR_INVALID_ARG.  A sharded
 *    context: GPE_ERR_UNSUPPORTED -- for either mode; the call is refused as a whole there, and gpe_get_bend_solver
 *    reads JACOBI. */
#define GPE_BEND_COLOURS_MAX      64u
#define GPE_BEND_SOLVER_JACOBI    0u
#define GPE_BEND_SOLVER_COLOURED  1u
typedef struct gpe_bend_solver_info {
    uint32_t struct_size, mode;        /* in / GPE_BEND_SOLVER_*                                               */
    uint32_t colours, largest_colour;  /* of the set held under COLOURED: colours / bends in the fullest one  */
    uint32_t form, lds_nodes_max;      /* the last coloured pass's launch form (0, 1, 2) / form 2's node limit */
    uint64_t passes;                   /* coloured passes enqueued since the last gpe_set_bend_solver          */
} gpe_bend_solver_info;                /* 32 bytes */
gpe_status gpe_set_bend_solver(gpe_ctx *ctx, uint32_t mode);          /* synchronises */
gpe_status gpe_get_bend_solver(gpe_ctx *ctx, uint32_t *mode);
gpe_status gpe_get_bend_solver_info(gpe_ctx *ctx, gpe_bend_solver_info *info);

/* ---- area constraints (not in the reference) -----------------------------------------------------------------------
 * Closed loops of particles that keep their area: a balloon, a tyre, a water drop, a jelly cell that squashes under
 * load and recovers, a foam of cells that share walls, an inflatable that is pumped up while the run goes on.  A loop
 * is `count` members (3 .. GPE_AREA_MAX_MEMBERS), each a particle named by uid (gpe_enable_uids must be on), in order
 * around a closed polygon, with a signed rest_area (positive when the members turn from +x towards +y) and a stiffness
 * in [0, 1].  Inside one loop a uid appears once; a uid may be a member of up to GPE_AREA_MAX_DEGREE loops (shared
 * cell walls, a two-chamber balloon).  While a context holds a set, gpe_step and every iteration of gpe_run run one
 * pass after the step, behind the bends and IN FRONT OF the distance bonds (lengths keep the last word over areas as
 * over angles, walls over all three), stream-ordered, on the device (csrc/k_areas.hip):
 * step -> bends -> areas -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor.  The per-module
 * calls run no pass: gpe_apply_areas is their hook.  A context without areas launches and allocates exactly what it
 * does without this section.
 *  - One relaxation (csrc/k_area.h is the one definition).  Every loop is judged from the positions the relaxation
 *    starts with, in IEEE binary32, one rounding per operation, left to right, no FMA, `/` correctly rounded.  For
 *    member j let n = (j + 1) % count and m = (j + count - 1) % count:
 *      q_j = p_j - p_0                                     (componentwise: member 0 is the origin)
 *      t_j = q_j.x * q_n.y - q_n.x * q_j.y;   A2 = S(t);   area = 0.5f * A2;   C = area - rest_area
 *      g_j = (0.5f * (q_n.y - q_m.y), 0.5f * (q_m.x - q_n.x));   D = S(g_j.x * g_j.x + g_j.y * g_j.y)
 *      inert this relaxation unless 0 < D < +inf and C is finite   (NaN fails every comparison)
 *      s = C * stiffness;   lambda = -(s / D);   corr_j = (lambda * g_j.x, lambda * g_j.y)
 *    S is the canonical sum of the bodies (csrc/k_body.h): with G = the smallest power of two >= count, at most 64,
 *    lane l of G adds v_l, v_(l+G), ... from +0.0f, then the halving tree partial[l] += partial[l + off], off = G/2
 *    .. 1.  Its order depends on count alone.  A loop with a member whose uid names no live particle is inert: it is
 *    not broken and acts again when the uid reappears (gpe_set_uids).  A particle with at least one acting loop moves
 *    to p + acc, acc summed from +0.0f over its memberships of acting loops in ascending member index (inert loops
 *    are skipped, not added as zero), then K12's clamp with its stored radius: clamp(x, r, W - r), clamp(y, r, H - r).
 *    Only pos is written: prev and radius never.  Every other particle keeps every bit, unclamped.  Loops do not
 *    break: a balloon tears through its bonds' max_length.
 *  - A pass relaxes the set `iterations` times (Jacobi: no relaxation reads what it has written itself), so the
 *    result depends on the set and the particles alone, never on launch order, storage order or mode.
 *  - What an area is not: it is Jacobi, so a stiffness above 1 / (loops per particle) overshoots; a rest_area whose
 *    sign differs from the current area drives the loop through a fold; there is no per-member mass, no breaking, no
 *    areas in sharded runs, and area and bond relaxations are not interleaved.
 *  - The set is step state: it survives adds, removals, edits, kicks, re-sorts, growth, gpe_set_mode, gpe_set_world
 *    and gpe_set_particles (which renumbers the uids from 0: the loops then name the new particles).  After a call
 *    that moves, adds or removes particles the next pass looks its uids up again (that synchronises once); every other
 *    pass only enqueues.
 *  - gpe_set_areas replaces the set (k == 0 clears it and frees its buffers) and zeroes the counters; it synchronises.
 *    areas[j] owns member_uid[first .. first + count); the ranges tile [0, members) in any order.  -0.0 in rest_area /
 *    stiffness is stored as +0.  gpe_get_areas delivers the first min(k, capacity) records into out, the first
 *    min(members, member_capacity) uids into member_uid_out, and the numbers set into *k and *members.
 *    gpe_apply_areas with no areas or no particles: GPE_OK, nothing done.  gpe_get_area_values delivers (area, lambda)
 *    per loop as of the last relaxation run, two NaNs for a loop that was inert in it or has not run yet; it
 *    synchronises.  gpe_set_area_targets replaces the rest areas of loops first .. first + k - 1 in place (the pump):
 *    it may synchronise, allocates nothing, and keeps the looked-up slots and every counter; gpe_get_areas delivers
 *    the new values.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL areas or member_uid with k > 0, k > GPE_AREAS_MAX,
 *    members > GPE_AREA_MEMBERS_MAX, a count outside 3 .. GPE_AREA_MAX_MEMBERS, ranges that overlap, leave members
 *    unused or run past `members`, a uid that is GPE_UID_ABSENT, a uid twice in one loop, a uid in more than
 *    GPE_AREA_MAX_DEGREE loops, a rest_area that is not finite, a stiffness that is NaN or outside [0, 1], iterations
 *    outside 1 .. GPE_AREA_ITER_MAX, nonzero flags or reserved, a struct_size below the struct's, a target range past
 *    the set: GPE_ERR_INVALID_ARG.  Uids off: GPE_ERR_STATE.  gpe_set_areas on a sharded context, and
 *    gpe_enable_uids(ctx, 0), gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and gpe_set_counts on a context
 *    that holds areas: GPE_ERR_UNSUPPORTED. */
#define GPE_AREAS_MAX         4194304u  /* loops in a set */
#define GPE_AREA_MAX_MEMBERS  4096u     /* members of one loop: 64 rounds of one wave */
#define GPE_AREA_MEMBERS_MAX  16777216u /* members of all loops together */
#define GPE_AREA_MAX_DEGREE   64u       /* loops per uid: one lane walks them in order */
#define GPE_AREA_ITER_MAX     32u
typedef struct gpe_area {               /* 24 bytes */
    uint32_t first, count;              /* members [first, first + count) of member_uid, in order around the polygon */
    float rest_area;                    /* finite, signed */
    float stiffness;                    /* in [0, 1] */
    uint32_t flags, reserved;           /* both 0 */
} gpe_area;
typedef struct gpe_areas_info {
    uint32_t struct_size, iterations;  /* in / relaxations per pass                                        */
    uint64_t k, members, nodes;        /* loops set / members of all loops / distinct uids they name       */
    uint64_t passes;                   /* passes enqueued since the last gpe_set_areas                     */
    uint64_t resolves;                 /* times the uids were looked up again since the last gpe_set_areas */
} gpe_areas_info;                      /* 48 bytes */
gpe_status gpe_set_areas(gpe_ctx *ctx, const gpe_area *areas, uint64_t k, const uint32_t *member_uid, uint64_t members,
                         uint32_t iterations);
gpe_status gpe_get_areas(const gpe_ctx *ctx, gpe_area *out, uint64_t capacity, uint64_t *k, uint32_t *member_uid_out,
                         uint64_t member_capacity, uint64_t *members);
gpe_status gpe_apply_areas(gpe_ctx *ctx);                          /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_areas_info(gpe_ctx *ctx, gpe_areas_info *info);
gpe_status gpe_get_area_values(gpe_ctx *ctx, float *area_lambda, uint64_t capacity, uint64_t *k);   /* synchronises */
gpe_status gpe_set_area_targets(gpe_ctx *ctx, uint64_t first, uint64_t k, const float *rest_area);

/* ---- rigid and soft bodies (not in the reference) ------------------------------------------------------------------
 * Groups of particles that keep their shape: a box, a wheel, a brick, a jelly blob.  A body is `count` members (2 ..
 * GPE_BODY_MAX_MEMBERS), each a particle named by uid (gpe_enable_uids must be on) with a rest position (rx, ry) in any
 * frame (only the offsets matter), a stiffness in [0, 1] and a break_distance >= 0 (0: never breaks).  A uid appears
 * at most once in the whole set.  While a context holds a set, gpe_step and every iteration of gpe_run run one shape
 * matching pass (Mueller et al. 2005) after the step, behind the distance bonds and BEFORE the static colliders, on
 * the device (csrc/k_bodies.hip): step -> bends -> areas -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor.  A bond can hang a body
 * from an anchor; walls keep the last word.  The per-module calls run no pass: gpe_apply_bodies is their hook.  A
 * context without bodies launches and allocates exactly what it does without this section.
 *  - The pass (csrc/k_body.h is the one definition), IEEE binary32, one rounding per operation, left to right, no
 *    FMA, `/` and sqrtf correctly rounded.  A member whose uid names no live particle is absent in this pass; L is the
 *    number of live members; a body with L < 2 is inert in this pass (not broken).
 *    S(v), the canonical sum over the body's members, depends on count alone: G = the smallest power of two >= count,
 *    at most 64; partial[l] = +0.0f; lane l adds v_l, v_(l+G), v_(l+2G), ... in that order (an absent member adds
 *    +0.0f); then for off = G/2 .. 1: partial[l] = partial[l] + partial[l + off] for l < off; S = partial[0].
 *      fL = (float)L;  rbar = (S(rx)/fL, S(ry)/fL);  c = (S(px)/fL, S(py)/fL)
 *      per live member: q = r - rbar;  d = p - c;  a = qx*dx + qy*dy;  b = qx*dy - qy*dx
 *      A = S(a);  B = S(b);  h = sqrtf(A*A + B*B);  inert unless h > 0 and h < +inf   (NaN, overflow, coincident
 *      members, underflow);  co = A/h;  si = B/h
 *      per live member: gx = cx + (co*qx - si*qy);  gy = cy + (si*qx + co*qy);  e = g - p;  e2 = ex*ex + ey*ey
 *      with break_distance > 0: any live member with e2 > bd2 (bd2 = break_distance*break_distance, rounded once on
 *      the host; strict) breaks the body: sticky, it never acts again, nothing moves in the pass in which it breaks
 *      otherwise every live member moves to (px + stiffness*ex, py + stiffness*ey), then K12's clamp with its stored
 *      radius: clamp(x, r, W - r), clamp(y, r, H - r).  Only pos is written: prev and radius never, so the velocity
 *      change is the one Verlet implies.
 *    The body's pose (cx, cy, co, si) is kept per body: four NaNs while the body is inert or broken, and before the
 *    first pass.  The result depends on the set and the particles alone, never on storage order or mode.
 *  - What a body is not: a collider or a collision deforms a body until the next pass; bodies whose members overlap at
 *    rest fight the collision solver; a break_distance below one step's collision push breaks at the first touch;
 *    there is no per-member mass (every member weighs the same, as in the collision response), no joint between
 *    bodies and no swept test.
 *  - The set and its broken flags are step state: they survive adds, removals, edits, kicks, re-sorts, growth,
 *    gpe_set_mode and gpe_set_particles (which renumbers the uids from 0: the bodies then name the new particles).
 *    After a call that moves, adds or removes particles the next pass looks its uids up again (that synchronises
 *    once); every other pass only enqueues.
 *  - gpe_set_bodies replaces the set (k == 0 clears it and frees its buffers), clears the broken flags and zeroes the
 *    counters; it synchronises.  Body j owns members [first, first + count) of member_uid and member_rest_xy (x, y
 *    interleaved).  A body given with GPE_BODY_BROKEN starts broken: that is how a snapshot restores one; the bit is
 *    not kept in the record.  -0.0 in break_distance is stored as +0.  gpe_get_bodies delivers the first min(k,
 *    capacity) records and their broken flags (1 / 0), the first min(members, member_capacity) member uids and rest
 *    positions (each output may be NULL) and the numbers set into *k and *members; it synchronises.
 *    gpe_get_body_poses delivers the first min(k, capacity) poses as of the last pass, 4 floats each; it synchronises.
 *    gpe_apply_bodies with no bodies or no particles: GPE_OK, nothing done.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL arrays with k > 0, k > GPE_BODIES_MAX, members >
 *    GPE_BODY_MEMBERS_MAX, a count outside 2 .. GPE_BODY_MAX_MEMBERS, member ranges that overlap, run past `members` or
 *    leave members unused, a uid equal to GPE_UID_ABSENT or named twice, a non-finite rest coordinate, a stiffness that
 *    is NaN or outside [0, 1], a break_distance that is NaN, infinite or negative, unknown flag bits, a non-zero
 *    reserved, a struct_size below the struct's: GPE_ERR_INVALID_ARG.  Uids off: GPE_ERR_STATE.  gpe_set_bodies on a
 *    sharded context, and gpe_enable_uids(ctx, 0), gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and
 *    gpe_set_counts on a context that holds bodies: GPE_ERR_UNSUPPORTED. */
#define GPE_BODIES_MAX        1048576u
#define GPE_BODY_MAX_MEMBERS  4096u
#define GPE_BODY_MEMBERS_MAX  16777216u   /* members of the whole set */
#define GPE_BODY_BROKEN       1u          /* flags, gpe_set_bodies only: the body starts broken */
typedef struct gpe_body {                 /* 24 bytes */
    uint32_t first, count;                /* members [first, first + count) */
    float stiffness;                      /* in [0, 1]: the share of the way to the matched pose per pass */
    float break_distance;                 /* finite, >= 0; 0: never breaks */
    uint32_t flags, reserved;
} gpe_body;
typedef struct gpe_bodies_info {
    uint32_t struct_size, reserved;    /* in / 0                                                             */
    uint64_t k, members;               /* bodies set / members of the whole set                              */
    uint64_t passes;                   /* passes enqueued since the last gpe_set_bodies                      */
    uint64_t live, broken;             /* bodies not broken / broken (an integer counter); live + broken = k */
    uint64_t resolves;                 /* times the uids were looked up again since the last gpe_set_bodies  */
} gpe_bodies_info;                     /* 56 bytes */
gpe_status gpe_set_bodies(gpe_ctx *ctx, const gpe_body *bodies, uint64_t k, const uint32_t *member_uid,
                          const float *member_rest_xy, uint64_t members);
gpe_status gpe_get_bodies(gpe_ctx *ctx, gpe_body *out, uint8_t *broken_out, uint64_t capacity, uint64_t *k,
                          uint32_t *member_uid_out, float *member_rest_xy_out, uint64_t member_capacity,
                          uint64_t *members);
gpe_status gpe_apply_bodies(gpe_ctx *ctx);                            /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_body_poses(gpe_ctx *ctx, float *pose_xycs, uint64_t capacity, uint64_t *k);   /* synchronises */
gpe_status gpe_get_bodies_info(gpe_ctx *ctx, gpe_bodies_info *info);  /* synchronises (reads the device counter) */

/* ---- force fields (not in the reference) ----------------------------------------------------------------------------
 * What pushes the particles inside a run: a fan, a gravity well, a whirlpool, a pool of mud, a conveyor belt.  A field
 * is a region (everywhere, a closed disc, a closed box) and a kind (a uniform acceleration, a pull toward a pole, a
 * swirl around a pole, a drag).  While a context holds a set, gpe_step and every iteration of gpe_run run one pass over
 * the particles after the step, BEHIND the static colliders and before the tracers and the monitor, stream-ordered, on
 * the device (csrc/k_fields.hip): step -> bends -> areas -> bonds -> bodies -> movers -> colliders -> fields -> tracers / monitor.  A field is
 * judged at the position the step ends with; a tracer or monitor frame sees the new velocity; the velocity acts from
 * the next step on.  The per-module calls (gpe_integrate and the rest) run no pass: gpe_apply_fields is their hook.  A
 * context without fields launches and allocates exactly what it does without this section.
 *  - The pass.  For a particle with c = pos and q = prev, and dt2 = dt * dt (one binary32 product, as the step forms
 *    it), in IEEE binary32, one rounding per operation, left to right, no FMA, `/` and sqrtf correctly rounded
 *    (csrc/k_field.h is the one definition).  Field j MATCHES by the predicates of the region queries and the kicks on
 *    the centre c alone (csrc/k_region_pred.h): CIRCLE the closed disc (c.x-x0)*(c.x-x0) + (c.y-y0)*(c.y-y0) <= rr
 *    with rr = x1 * x1; BOX the closed box x0 <= c.x && c.x <= x1 && y0 <= c.y && c.y <= y1; EVERYWHERE always (a NaN
 *    coordinate included).  The particle's radius plays no part.  Start with A = (0, 0), s = 1, accel = drag = false;
 *    over the matching fields in ASCENDING index:
 *      UNIFORM: g = (fx, fy)
 *      RADIAL:  dx = px - c.x; dy = py - c.y; len = sqrtf(dx*dx + dy*dy); w = strength
 *               LINEAR falloff: t = len / reach; w1 = 1 - t; w1 = (w1 > 0) ? w1 : 0; w = strength * w1
 *               g = ((dx / len) * w, (dy / len) * w);  if !(len > 0): g = (0, 0)
 *               (on its pole a field contributes nothing; the reference's mouse attractor divides by its zero length
 *               there and yields NaN)
 *      VORTEX:  as RADIAL with g = (((-dy) / len) * w, (dx / len) * w): strength > 0 turns counter-clockwise where x
 *               points right and y up
 *      UNIFORM, RADIAL, VORTEX: A.x = A.x + g.x; A.y = A.y + g.y; accel = true
 *      DRAG:    s = s * strength; drag = true
 *    Then drags act first, accelerations second:
 *      if drag:  v = c - q; v = v * s; q = c - v            (gpe_kick_* with GPE_VEL_SCALE)
 *      if accel: q.x = q.x - A.x * dt2; q.y = q.y - A.y * dt2   (gpe_kick_* with GPE_VEL_ADD)
 *    A particle no field matches keeps every bit of prev and is not stored.  The order is part of the result: the
 *    sums are not associative.  pos, radii, uids, the kept block table, the rosters and the native step / sort counters
 *    are never touched, exactly as after a kick.  The payload of a NaN that the arithmetic itself produces is not
 *    specified.
 *  - An EVERYWHERE UNIFORM field is gravity delayed by one step: the step adds gravity before it moves the particle,
 *    a field changes the velocity the NEXT step moves it with.  It is therefore not bit-identical to gpe_set_gravity.
 *  - Fields are step state, not observation state: the set survives gpe_set_particles, adds, removals, edits,
 *    re-sorts, growth, gpe_set_world and uids being switched on or off; gpe_destroy frees it.
 *  - The pass finds a particle's fields through a coarse grid over the world that depends on the set and the world
 *    alone, rebuilt before the next pass when the world has changed (that rebuild synchronises).  No result depends on
 *    the grid: a particle outside it or with a NaN coordinate is tested against every field.
 *  - gpe_set_fields replaces the set (k == 0 clears it and frees its buffers) and zeroes passes and touched; it may be
 *    called before there are particles and synchronises like gpe_add_particles.  Fields do not move or vary in time: a
 *    host that wants that calls it once a frame.  -0.0 as a circle's radius is stored as +0.  gpe_get_fields delivers
 *    the first min(k, capacity) fields into out (may be NULL with capacity 0) and the number set into *k.
 *    gpe_apply_fields with no fields or no particles: GPE_OK, nothing done.
 *  - Errors (the previous set stays untouched): a NULL ctx, NULL fields with k > 0, k > GPE_FIELDS_MAX, an unknown
 *    shape, kind or falloff, non-zero flags, any float that is not finite, a negative circle radius (-0.0 is accepted
 *    as 0), a falloff other than NONE on UNIFORM or DRAG, LINEAR with a reach that is not > 0, a DRAG strength outside
 *    [0, 1], a dt that is not finite in gpe_apply_fields, a struct_size below the struct's: GPE_ERR_INVALID_ARG.  A box
 *    with x0 > x1 or y0 > y1 is accepted and matches nothing.  gpe_set_fields on a sharded context (gpe_shard_*, order
 *    keys or an active cell box), and gpe_shard_set_particles, gpe_use_order_keys(ctx, 1) and gpe_set_counts on a
 *    context that holds fields: GPE_ERR_UNSUPPORTED. */
#define GPE_FIELDS_MAX 4096u
enum { GPE_FIELD_EVERYWHERE = 0, GPE_FIELD_CIRCLE = 1, GPE_FIELD_BOX = 2 };                      /* shape   */
enum { GPE_FIELD_UNIFORM = 0, GPE_FIELD_RADIAL = 1, GPE_FIELD_VORTEX = 2, GPE_FIELD_DRAG = 3 };  /* kind    */
enum { GPE_FALLOFF_NONE = 0, GPE_FALLOFF_LINEAR = 1 };                                           /* falloff */
typedef struct gpe_field {
    uint32_t shape, kind, falloff, flags;   /* flags = 0                                                              */
    float x0, y0, x1, y1;   /* CIRCLE: centre (x0, y0), radius x1, y1 = 0.  BOX: [x0, x1] x [y0, y1].  EVERYWHERE: all 0 */
    float px, py;           /* RADIAL / VORTEX: the pole                                                              */
    float fx, fy;           /* UNIFORM: the acceleration, in gravity's units                                          */
    float strength;         /* RADIAL: > 0 toward the pole.  VORTEX: > 0 counter-clockwise.  DRAG: the share of the
                               velocity kept per step, in [0, 1]                                                      */
    float reach;            /* LINEAR falloff: the distance from the pole at which the field has faded to 0           */
} gpe_field;                /* 56 bytes */
typedef struct gpe_fields_info {
    uint32_t struct_size, k;          /* in / fields set                                                 */
    uint64_t passes;                  /* passes run since the last gpe_set_fields                        */
    uint64_t touched;                 /* particles whose prev those passes wrote, summed (integer atomics only) */
    uint32_t grid_x, grid_y;          /* the lookup grid in use (diagnostic; no result depends on it)    */
    uint64_t list_entries;            /* (cell, field) entries in it                                     */
} gpe_fields_info;                    /* 40 bytes */
gpe_status gpe_set_fields(gpe_ctx *ctx, const gpe_field *fields, uint64_t k);
gpe_status gpe_get_fields(const gpe_ctx *ctx, gpe_field *out, uint64_t capacity, uint64_t *k);
gpe_status gpe_apply_fields(gpe_ctx *ctx, float dt);                 /* one pass now, stream-ordered, no sync */
gpe_status gpe_get_fields_info(gpe_ctx *ctx, gpe_fields_info *info); /* synchronises (reads the device counter) */

/* ---- region queries and picking (not in the reference) ------------------------------------------------------
 * Which particles lie in a region, or under a point, without downloading every position: full passes over the
 * particles on the device (csrc/k_query.hip) that change nothing on the context.  Positions, prev, radii, uids, the
 * uid map, the native step / sort counters, the kept block table and the rosters are left alone; the steps after a
 * query are bit-identical to those of a context that was never queried.  Each call blocks like gpe_download.
 *  - Circle: p matches when (p.x-x)*(p.x-x) + (p.y-y)*(p.y-y) <= radius*radius in IEEE binary32, one rounding per
 *    operation, left to right, no FMA: the predicate and argument check of gpe_remove_particles_in_circle, so the set a
 *    circle query returns is exactly the set that removal with the same arguments removes.  radius must be finite and
 *    >= 0, else GPE_ERR_INVALID_ARG.
 *  - Box: p matches when x0 <= p.x && p.x <= x1 && y0 <= p.y && p.y <= y1 (closed; infinite bounds give half-planes).
 *    A NaN bound: GPE_ERR_INVALID_ARG.  x0 > x1 or y0 > y1: an empty box, GPE_OK with count 0.
 *  - Pick: among the particles whose own disc contains (x, y) -- dx*dx + dy*dy <= r*r in binary32 as above, r the
 *    particle's radius (a negative radius acts as its magnitude) -- the one with the smallest dx*dx + dy*dy, the lowest
 *    storage index on a tie.  count is 0 or 1.
 *  - Output: the first min(count, capacity) matches in ascending storage index go into every non-NULL array, all
 *    arrays filled from the same particles; host memory past those entries is left untouched.  With every array NULL
 *    the call only counts.
 *  - Errors: a NULL context, a NULL out or a struct_size below sizeof(gpe_query_result): GPE_ERR_INVALID_ARG; uid
 *    requested while uids are off: GPE_ERR_STATE; a sharded context (gpe_shard_*, order keys or an active cell box):
 *    GPE_ERR_UNSUPPORTED.  On any error count is 0 (when out is usable) and no output array is written.
 *  - No particles: GPE_OK, count 0. */
typedef struct gpe_query_result {
    uint32_t struct_size;   /* in: sizeof(gpe_query_result)                                            */
    uint32_t reserved;      /* in: 0                                                                   */
    uint64_t capacity;      /* in: entries each non-NULL array below has room for                      */
    uint64_t count;         /* out: number of matches (may exceed capacity)                            */
    uint32_t *index;        /* out, may be NULL: storage indices (as gpe_download(GPE_POS)), ascending  */
    uint32_t *uid;          /* out, may be NULL: their uids; non-NULL while uids are off: GPE_ERR_STATE */
    float    *pos_xy;       /* out, may be NULL: f32[2 * capacity]                                     */
    float    *prev_xy;      /* out, may be NULL: f32[2 * capacity]                                     */
    float    *radius;       /* out, may be NULL: f32[capacity]                                         */
} gpe_query_result;
gpe_status gpe_query_circle(gpe_ctx *ctx, float x, float y, float radius, gpe_query_result *out);
gpe_status gpe_query_box(gpe_ctx *ctx, float x0, float y0, float x1, float y1, gpe_query_result *out);
gpe_status gpe_pick(gpe_ctx *ctx, float x, float y, gpe_query_result *out);

/* ---- contact queries (not in the reference) ------------------------------------------------------------------
 * Which particles are touching right now, and how many neighbours each one has, without downloading positions and
 * radii for a neighbour search on the host: a cell-binned search on the device (csrc/k_contacts.hip) in scratch of
 * its own.
 *  - Contact predicate: particles i != j are in contact when dx*dx + dy*dy < (ri + rj)*(ri + rj), dx = xi - xj,
 *    dy = yi - yj, in IEEE binary32, one rounding per operation, left to right, no FMA (numpy float32 gives the same
 *    answer).  Radii are taken as stored (a negative radius enters the sum with its sign).  This is are_colliding of
 *    collision_solver.wgsl:60-64 on the squared distance itself.  It is symmetric in i and j, because the squares of
 *    negated differences are equal.  Coincident centres are a contact when the radius sum is non-zero.  A NaN anywhere
 *    makes the comparison false.  This is the geometric predicate, not the step's: the step squares a rounded square
 *    root and skips distance <= 1e-4, so the two may differ at those two edges.
 *  - overlap = (ri + rj) - sqrtf(dx*dx + dy*dy), the square root correctly rounded: the penetration depth, the bits
 *    numpy float32 gives.
 *  - degree[i] = the number of j in contact with i.  The array always has gpe_len entries, whatever capacity is.
 *  - count = the number of unordered pairs = sum(degree) / 2, summed in 64 bits.
 *  - Pairs are ordered ascending by index_a, then ascending by index_b (index_a < index_b).  The first
 *    min(count, capacity) pairs go into every non-NULL per-pair array, all arrays filled from the same pairs; host
 *    memory past those entries is left untouched.  With every array NULL the call only counts.
 *  - More than 2^32 - 1 contacts cannot be listed (the 32-bit scan cannot rank them): when a per-pair array is requested
 *    and count > 0xFFFFFFFF the call returns GPE_ERR_UNSUPPORTED and writes no per-pair array.  This is the one error
 *    that leaves count set; degree is delivered too.
 *  - The search uses a cell size of its own, gpe_compute_cell_size(|gpe_max_radius|): a gpe_grid_set_max_radius
 *    override changes nothing about the result.  A contact implies a centre distance below 2 max|r|, so the 3 x 3 cell
 *    neighbourhood is complete.  (gpe_max_radius bounds every |radius| after set / remove / edit; gpe_add_particles
 *    keeps max(max_radius, r) as the reference does, so it does too unless a negative radius of larger magnitude was
 *    added.)  That cell size not finite (an infinite radius): GPE_ERR_UNSUPPORTED.  0 (every radius 0): GPE_OK, count
 *    0, every degree 0.
 *  - Positions may be anything gpe_set_particles accepts -- outside the world, negative, 1e30, +-inf, NaN: the result
 *    is exactly the predicate's, and the search never reads or writes out of bounds for them.
 *  - The query changes nothing on the context: positions, prev, radii, uids, the uid map, GPE_HOME_CELL_IDS and the
 *    other scratch index arrays, the native step / sort counters, the kept block table and the rosters are left alone;
 *    the steps after a query are bit-identical to those of a context that was never queried.  It works in both modes
 *    and at any point between steps, and blocks like gpe_download.
 *  - Errors: a NULL context, a NULL out or a struct_size below sizeof(gpe_contact_result): GPE_ERR_INVALID_ARG; a uid
 *    array while uids are off: GPE_ERR_STATE; a sharded context (gpe_shard_*, order keys or an active cell box) and
 *    more than 2^32 - 1 particles: GPE_ERR_UNSUPPORTED.  On these errors count is 0 (when out is usable) and nothing is
 *    written.
 *  - No particles, or one particle: GPE_OK, count 0. */
typedef struct gpe_contact_result {
    uint32_t struct_size;   /* in: sizeof(gpe_contact_result)                                   */
    uint32_t reserved;      /* in: 0                                                            */
    uint64_t capacity;      /* in: pairs each non-NULL per-pair array has room for              */
    uint64_t count;         /* out: number of contacts (exact, may exceed capacity and 2^32)    */
    uint32_t *index_a;      /* out, may be NULL: storage index of the lower particle            */
    uint32_t *index_b;      /* out, may be NULL: storage index of the higher particle (a < b)   */
    uint32_t *uid_a;        /* out, may be NULL: their uids; non-NULL while uids are off:       */
    uint32_t *uid_b;        /*                   GPE_ERR_STATE                                  */
    float    *overlap;      /* out, may be NULL: f32[capacity] penetration depth                */
    uint32_t *degree;       /* out, may be NULL: u32[gpe_len] contacts of every particle        */
} gpe_contact_result;       /* 72 bytes */
gpe_status gpe_query_contacts(gpe_ctx *ctx, gpe_contact_result *out);

/* ---- contact clusters (not in the reference) -----------------------------------------------------------------
 * Which particles make up one clump: the connected components of the graph whose edges are the contacts of
 * gpe_query_contacts, labelled on the device (csrc/k_clusters.hip) in scratch of its own, without downloading the pair
 * list for a union-find on the host -- a settled pile may have more contacts than can be listed at all.
 *  - Two particles are in one cluster when a chain of contacts joins them.  "Contact" is exactly the predicate of
 *    gpe_query_contacts: the same binary32 operations, radii as stored, a NaN anywhere compares false.
 *  - The search uses the contact query's own cell size, gpe_compute_cell_size(|gpe_max_radius|): a
 *    gpe_grid_set_max_radius override changes nothing about the result.
 *  - label[i] = the lowest storage index among the particles of i's cluster.  A particle without contacts is its own
 *    cluster, label[i] == i.  size[i] = the number of particles in i's cluster.  label_uid[i] = the uid of particle
 *    label[i].  count = the number of i with label[i] == i, singletons included.  largest_size / largest_label: the
 *    size of the largest cluster and its label, the lowest label among the clusters of that size.
 *  - The per-particle arrays always have gpe_len entries.
 *  - The result is a function of the particles alone: everything is integers, and the lowest index of a component does
 *    not depend on the launch geometry or on which wave wins a race.  Two calls return identical arrays.
 *  - Positions may be anything gpe_set_particles accepts, as for gpe_query_contacts.
 *  - The query changes nothing on the context: positions, prev, radii, uids, the uid map, GPE_HOME_CELL_IDS and the
 *    other scratch index arrays, the native step / sort counters, the kept block table and the rosters are left alone;
 *    the steps after a query are bit-identical to those of a context that was never queried.  It works in both modes
 *    and at any point between steps, and blocks like gpe_download.
 *  - No particles: GPE_OK, count 0.  One particle, or every radius 0 (a cell size of 0): every particle is its own
 *    cluster -- count = gpe_len, largest_size = 1, largest_label = 0; the arrays are filled on the host.
 *  - Errors, as gpe_query_contacts: a NULL context, a NULL out or a struct_size below sizeof(gpe_cluster_result):
 *    GPE_ERR_INVALID_ARG; label_uid requested while uids are off: GPE_ERR_STATE; a sharded context (gpe_shard_*, order
 *    keys or an active cell box), more than 2^32 - 1 particles, and a cell size that is not finite (an infinite radius)
 *    with more than one particle: GPE_ERR_UNSUPPORTED.  On any error count is 0 (when out is usable) and no array is
 *    written. */
typedef struct gpe_cluster_result {
    uint32_t struct_size;    /* in: sizeof(gpe_cluster_result)                                        */
    uint32_t reserved;       /* in: 0                                                                 */
    uint64_t count;          /* out: number of clusters, singletons included                          */
    uint32_t largest_size;   /* out: particles in the largest cluster                                 */
    uint32_t largest_label;  /* out: its label (the lowest label among clusters of that size)         */
    uint32_t *label;         /* out, may be NULL: u32[gpe_len]                                        */
    uint32_t *size;          /* out, may be NULL: u32[gpe_len] particles in i's cluster               */
    uint32_t *label_uid;     /* out, may be NULL: u32[gpe_len] uid of particle label[i]; uids off: GPE_ERR_STATE */
} gpe_cluster_result;        /* 48 bytes */
gpe_status gpe_query_clusters(gpe_ctx *ctx, gpe_cluster_result *out);

/* Flood select: the members of the cluster that holds the particle named by storage index (GPE_CLUSTER_BY_INDEX) or by
 * uid (GPE_CLUSTER_BY_UID), delivered exactly as the region queries deliver rows.  count may exceed capacity; the first
 * min(count, capacity) members, in ascending storage index, go into every non-NULL array; host memory past those
 * entries is left untouched; with every array NULL the call only counts.  A particle without contacts is the one member
 * of its cluster.  An absent uid: GPE_OK with count 0.
 *  - Errors: GPE_CLUSTER_BY_INDEX with key >= gpe_len, or an unknown key_kind: GPE_ERR_INVALID_ARG;
 *    GPE_CLUSTER_BY_UID while uids are off: GPE_ERR_STATE; otherwise those of gpe_query_circle and of
 *    gpe_query_clusters above.  On any error count is 0 (when out is usable) and no array is written.
 *  - The context is left untouched as by gpe_query_clusters, except that a lookup by uid may rebuild a stale uid ->
 *    index map, as gpe_find_uids does. */
enum { GPE_CLUSTER_BY_INDEX = 0, GPE_CLUSTER_BY_UID = 1 };
gpe_status gpe_query_cluster_of(gpe_ctx *ctx, uint32_t key_kind, uint32_t key, gpe_query_result *out);

/* ---- ray casts and segment queries (not in the reference) -----------------------------------------------------
 * What a ray hits first (line of sight, a laser, a fan of distance sensors) and which particles a stroke crosses (a
 * cut, a line eraser), without downloading positions and radii: gpe_cast_rays walks the contact query's cell-binned
 * table along each ray on the device (csrc/k_raycast.hip), gpe_query_segment is a full pass (csrc/k_query.hip).
 *  - Both apply one function (csrc/k_ray.h) to the segment from o = (ox, oy) to e = (ex, ey) and a particle with centre
 *    c and stored radius r, in IEEE binary32, one rounding per operation, left to right, no FMA, `/` and sqrtf
 *    correctly rounded (numpy float32 gives the same bits):
 *        a = |r|;  rr = a*a;                     if !(a > 0): miss         (radius 0 or NaN is never hit; a negative
 *        dx = ex-ox; dy = ey-oy; fx = ox-cx; fy = oy-cy                     radius acts as its magnitude, as in gpe_pick)
 *        A = dx*dx + dy*dy;  C = fx*fx + fy*fy
 *        if C <= rr: touched, t = +0             (the origin lies in the closed disc; also the zero-length ray)
 *        if !(A > 0): miss
 *        B = fx*dx + fy*dy;  u = (-B) / A
 *        qx = fx + u*dx;  qy = fy + u*dy;  h = qx*qx + qy*qy
 *        if !(h <= rr): miss
 *        w = sqrtf((rr - h) / A);  t = u - w
 *        touched iff t >= 0 && t <= 1            (a t of -0 counts as, and is delivered as, +0)
 *    A NaN anywhere makes a comparison false: a miss.  This is the closest-approach form; it has no B*B - A*C
 *    cancellation.
 *  - gpe_cast_rays: for ray i the result is the touched particle with the smallest t, the lowest storage index on a
 *    tie.  Every output array may be NULL; hits is always set.  A miss delivers GPE_RAY_MISS, GPE_UID_ABSENT and quiet
 *    NaNs.
 *  - The cast's search uses the contact query's own cell size, gpe_compute_cell_size(|gpe_max_radius|): a
 *    gpe_grid_set_max_radius override plays no part, and the caveat about a negative radius of larger magnitude added
 *    later is that of gpe_query_contacts.  That cell size not finite (an infinite radius): GPE_ERR_UNSUPPORTED.  0
 *    (every radius 0): GPE_OK, every ray misses.
 *  - Endpoints, checked on the host over the caller's arrays before anything is written: every coordinate must be
 *    finite and, while the cell size is positive, satisfy |v| <= 131072 * cell_size; else GPE_ERR_INVALID_ARG.  Any
 *    supported world passes (65 000 cells per axis is the native limit); a host clips longer rays itself.  The bound
 *    keeps the rounding of the walk's own arithmetic a small fraction of a cell, which is what makes the walk complete.
 *  - Particle positions may be anything gpe_set_particles accepts -- outside the world, 1e30, +-inf, NaN: the result
 *    is exactly the function's, and nothing reads or writes out of bounds for them.
 *  - Both calls change nothing on the context, as gpe_query_contacts: positions, prev, radii, uids, the uid map, the
 *    scratch index arrays, the native step / sort counters, the kept block table and the rosters are left alone; the
 *    steps after a call are bit-identical to those of a context that was never queried.  They work in both modes and at
 *    any point between steps, and block like gpe_download.
 *  - Errors of gpe_cast_rays: a NULL context, a NULL cast, a struct_size below sizeof(gpe_ray_cast), non-zero flags, a
 *    NULL from_xy or to_xy with k > 0: GPE_ERR_INVALID_ARG; uid requested while uids are off: GPE_ERR_STATE; a sharded
 *    context (gpe_shard_*, order keys or an active cell box) and more than 2^32 - 1 particles: GPE_ERR_UNSUPPORTED.  On
 *    every error hits is 0 (when the struct is usable) and no output is written.
 *  - k == 0: GPE_OK, hits 0.  No particles: GPE_OK, every ray misses. */
#define GPE_RAY_MISS 0xffffffffu
typedef struct gpe_ray_cast {
    uint32_t struct_size;   /* in: sizeof(gpe_ray_cast)                                       */
    uint32_t flags;         /* in: 0; anything else GPE_ERR_INVALID_ARG                       */
    uint64_t k;             /* in: number of rays                                             */
    const float *from_xy;   /* in: f32[2k]                                                    */
    const float *to_xy;     /* in: f32[2k]                                                    */
    uint32_t *index;        /* out, may be NULL: storage index of the first hit, GPE_RAY_MISS */
    uint32_t *uid;          /* out, may be NULL: its uid, GPE_UID_ABSENT for a miss           */
    float    *t;            /* out, may be NULL: fraction of the way from `from` to `to`; quiet NaN for a miss */
    float    *pos_xy;       /* out, may be NULL: f32[2k] the hit particle's centre; NaN for a miss */
    float    *radius;       /* out, may be NULL: f32[k] its stored radius; NaN for a miss     */
    uint64_t hits;          /* out: rays that hit something                                   */
} gpe_ray_cast;             /* 80 bytes */
gpe_status gpe_cast_rays(gpe_ctx *ctx, gpe_ray_cast *cast);

/* Everything the segment from (x0, y0) to (x1, y1) crosses: a particle matches when the function above says touched.
 * Delivery, errors and the untouched context are exactly those of gpe_query_box.  A non-finite endpoint:
 * GPE_ERR_INVALID_ARG; there is no bound on its magnitude, the full pass needs none.  The first hit of gpe_cast_rays
 * for the same segment is the member of this set with the least t; a miss there means the set is empty. */
gpe_status gpe_query_segment(gpe_ctx *ctx, float x0, float y0, float x1, float y1, gpe_query_result *out);

/* ---- nearest neighbours (not in the reference) -----------------------------------------------------------------
 * Which particles are closest to this point (a snapping cursor, a proximity sensor, the 8 neighbours of each tracer, an
 * agent that looks around), without downloading the positions: gpe_query_nearest walks the contact query's cell-binned
 * table outward from each of k points on the device (csrc/k_nearest.hip) and keeps the m closest.
 *  - The predicate is the circle query's.  For the point (x, y) and a particle centre p, in IEEE binary32, one rounding
 *    per operation, left to right, no FMA (numpy float32 gives the same bits):
 *        d2 = (p.x-x)*(p.x-x) + (p.y-y)*(p.y-y);  rr = max_distance*max_distance
 *        candidate iff d2 <= rr                   (a NaN anywhere compares false; +inf <= +inf holds)
 *    Radii play no part: this is the distance between the point and the centre.  gpe_pick remains the call for "what is
 *    under the cursor".
 *  - For point i the neighbours are the min(m, candidates) candidates with the least key bits(d2) << 32 | index: d2 is
 *    at least +0, so its bits order as its values, and the lowest storage index wins a tie.  They are delivered in
 *    ascending key order into row i (m slots) of every non-NULL array; the slots count[i] .. m-1 of a row get
 *    GPE_NEAREST_NONE, GPE_UID_ABSENT and quiet NaNs.  found is always set.
 *  - For a finite max_distance the candidates are exactly the members of gpe_query_circle(x, y, max_distance), and
 *    count[i] = min(m, that count).  +inf means no cutoff (particles whose d2 overflows to +inf are then candidates, and
 *    come last); -0.0 is accepted as 0.
 *  - A point that coincides with a particle finds that particle at d2 = +0.  A host that wants the neighbours OF a
 *    particle asks for m + 1 and drops the first row entry (the lowest index among coincident particles comes first).
 *  - The cell size of the search is gpe_compute_cell_size(|gpe_max_radius|), the contact query's own, when that is
 *    finite and > 0; a gpe_grid_set_max_radius override plays no part.  Otherwise (every radius 0, or an infinite
 *    radius) it is max(world_width, world_height) / 1024 in binary32, and when that is not finite and positive either:
 *    GPE_ERR_UNSUPPORTED.  The result never depends on the cell size; only the bound on the query points does.
 *  - Query points, checked on the host over the caller's array before anything is written: every coordinate must be
 *    finite and satisfy |v| <= 131072 * cell_size, else GPE_ERR_INVALID_ARG (the rule of gpe_cast_rays, for the same
 *    reason: it keeps the rounding of the walk's own arithmetic a small fraction of a cell).  A context without
 *    particles has no cell size: the coordinates need only be finite there.
 *  - Particle positions may be anything gpe_set_particles accepts -- outside the world, 1e30, +-inf, NaN: the result
 *    is exactly the predicate's, and nothing reads or writes out of bounds for them.
 *  - The call changes nothing on the context, as gpe_query_contacts: positions, prev, radii, uids, the uid map, the
 *    scratch index arrays, the native step / sort counters, the kept block table and the rosters are left alone; the
 *    steps after a call are bit-identical to those of a context that was never asked.  It works in both modes and at any
 *    point between steps, and blocks like gpe_download.
 *  - Errors: a NULL context, a NULL query, a struct_size below sizeof(gpe_nearest_query), non-zero flags, m == 0 or
 *    m > GPE_NEAREST_MAX_M, a max_distance that is NaN or negative, a NULL point_xy with k > 0: GPE_ERR_INVALID_ARG; uid
 *    requested while uids are off: GPE_ERR_STATE; a sharded context (gpe_shard_*, order keys or an active cell box) and
 *    more than 2^32 - 1 particles: GPE_ERR_UNSUPPORTED.  On every error found is 0 (when the struct is usable) and no
 *    output is written.
 *  - k == 0: GPE_OK, found 0.  No particles: GPE_OK, every count 0, the rows filled with the values above. */
#define GPE_NEAREST_NONE 0xffffffffu
#define GPE_NEAREST_MAX_M 64
typedef struct gpe_nearest_query {
    uint32_t struct_size;   /* in: sizeof(gpe_nearest_query)                                   */
    uint32_t flags;         /* in: 0; anything else GPE_ERR_INVALID_ARG                         */
    uint64_t k;             /* in: number of query points                                       */
    const float *point_xy;  /* in: f32[2k]                                                      */
    uint32_t m;             /* in: neighbours wanted per point, 1 .. GPE_NEAREST_MAX_M          */
    float    max_distance;  /* in: >= 0 or +inf (no cutoff)                                     */
    uint32_t *count;        /* out, may be NULL: u32[k] neighbours delivered for point i (<= m) */
    uint32_t *index;        /* out, may be NULL: u32[k*m] storage indices, row i = point i      */
    uint32_t *uid;          /* out, may be NULL: u32[k*m]                                       */
    float    *dist2;        /* out, may be NULL: f32[k*m] the d2 above                          */
    float    *pos_xy;       /* out, may be NULL: f32[2*k*m]                                     */
    float    *radius;       /* out, may be NULL: f32[k*m] stored radius                         */
    uint64_t found;         /* out: sum of count over all points                                */
} gpe_nearest_query;        /* 88 bytes */
gpe_status gpe_query_nearest(gpe_ctx *ctx, gpe_nearest_query *q);

/* ---- editing particles in place (not in the reference) --------------------------------------------------------
 * Change particles that exist, on the device (csrc/k_edit.hip), without the download / gpe_set_particles detour that
 * would drop the uids, the kept block table and the native counters.  Two kinds of call:
 *
 * Keyed edits (gpe_edit_particles): new pos, prev or radius for the k particles named by storage index or by uid --
 * drag, throw, resize the particle gpe_pick found.
 *  - Fields: a non-NULL array supplies element i for the particle key i names; a NULL array leaves that field of every
 *    named particle alone.  pos_xy without prev_xy: prev = the new pos (at rest, as gpe_add_particles leaves a new
 *    particle).  Bits are copied, no arithmetic: any float is accepted, as gpe_set_particles accepts it.
 *  - Leaves behind, when pos or radius was edited: what gpe_set_particles(edited pos, edited prev, edited radius) would
 *    leave, as far as a step can see -- every later step, with or without re-sorts, in either mode, is bit-identical to
 *    that of such a fresh context.  Capacity, the native step / sort counters, the uids and the uid map are kept (the
 *    order does not change); the scratch index arrays (GPE_HOME_CELL_IDS and friends) keep what the last call left in
 *    them.  The native pipeline is re-derived as after a removal: the kept block table, rosters and hints are dropped,
 *    the box check runs again -- a particle moved outside [0, world] shows up as GPE_REASON_OUT_OF_BOX, and moving it
 *    back returns the context to the NATIVE kernels.
 *  - radius non-NULL: gpe_max_radius is recomputed on the device over all particles (largest magnitude, last on ties,
 *    sign kept, as after a removal), gpe_grid_max_radius is set to it and the cell size follows.  radius NULL: max
 *    radius, the grid max radius (a gpe_grid_set_max_radius override included) and the cell size are untouched.
 *  - Only prev_xy: nothing is re-derived; the kept block table stays in use.
 *  - Absent uids are skipped, as in gpe_remove_particles_by_uid; edited = k minus those.  Uids are resolved through
 *    the uid -> index map, rebuilt first if stale.
 *  - GPE_ERR_INVALID_ARG, the context untouched: two keys naming one particle (found on the device), an index >=
 *    gpe_len, every field array NULL, a NULL ctx / edit / keys, struct_size below sizeof(gpe_particle_edit), an unknown
 *    key_kind.  GPE_ERR_STATE: GPE_EDIT_BY_UID while uids are off; no particles.  GPE_ERR_UNSUPPORTED: a sharded
 *    context (gpe_shard_*, order keys or an active cell box).  k == 0: GPE_OK, nothing changes.  On any error edited = 0.
 *  - Synchronises, like gpe_add_particles.
 *
 * Region velocity edits (gpe_kick_circle / gpe_kick_box): add to, set or scale the Verlet velocity pos - prev of every
 * particle in a circle or a box -- the push, stop and damp brush.  One pass over the particles that writes prev only.
 *  - Region: the predicate and the argument check of gpe_query_circle / gpe_query_box; a kick touches exactly the
 *    particles the query with the same arguments returns.
 *  - Per matching particle and component, in IEEE binary32 with one rounding per operation and no FMA (numpy float32
 *    gives the same bits):  GPE_VEL_ADD  prev = prev - a  (a = 0 changes no bit, except that a prev of -0 becomes +0 for
 *    a = -0);  GPE_VEL_SET  prev = pos - a  (a = 0 freezes: prev = pos exactly);  GPE_VEL_SCALE  v = pos - prev,
 *    v = v * a, prev = pos - v.  ax acts on x, ay on y; both must be finite and op known, else GPE_ERR_INVALID_ARG.
 *  - Leaves alone: positions, radii, uids, the uid map, the kept block table, the rosters and the counters
 *    (gpe_get_pipeline_info's native_sorts and roster_stamp are the same before and after); nothing is re-derived.
 *  - n_kicked == NULL: stream-ordered, no synchronisation, like gpe_step -- a host may issue one per frame between
 *    steps.  n_kicked != NULL: the matches are counted and the call blocks to read the count.
 *  - An empty region (radius 0 off any particle, x0 > x1) and a context without particles: GPE_OK, count 0.  Invalid
 *    region arguments: GPE_ERR_INVALID_ARG; a sharded context: GPE_ERR_UNSUPPORTED.  On any error *n_kicked = 0. */
enum { GPE_EDIT_BY_INDEX = 0, GPE_EDIT_BY_UID = 1 };
typedef struct gpe_particle_edit {
    uint32_t struct_size;      /* in: sizeof(gpe_particle_edit)                                     */
    uint32_t key_kind;         /* in: GPE_EDIT_BY_*                                                 */
    uint64_t k;                /* in: number of keys                                                */
    const uint32_t *keys;      /* in: storage indices (as gpe_download(GPE_POS)) or uids            */
    const float *pos_xy;       /* in, may be NULL: f32[2k] new positions                            */
    const float *prev_xy;      /* in, may be NULL: f32[2k] new previous positions                   */
    const float *radius;       /* in, may be NULL: f32[k]  new radii                                */
    uint64_t edited;           /* out: particles written (k minus absent uids)                      */
} gpe_particle_edit;
gpe_status gpe_edit_particles(gpe_ctx *ctx, gpe_particle_edit *edit);

enum { GPE_VEL_ADD = 0, GPE_VEL_SET = 1, GPE_VEL_SCALE = 2 };
gpe_status gpe_kick_circle(gpe_ctx *ctx, float x, float y, float radius,
                           uint32_t op, float ax, float ay, uint64_t *n_kicked);
gpe_status gpe_kick_box(gpe_ctx *ctx, float x0, float y0, float x1, float y1,
                        uint32_t op, float ax, float ay, uint64_t *n_kicked);

/* ---- adding particles where there is room (not in the reference) -----------------------------------------------
 * gpe_add_particles appends whatever it is given, as the reference's add_particles does (particle_system.rs:163-220) --
 * also on top of particles that exist, the commonest way to blow a pile apart.  gpe_add_particles_free filters the k
 * candidates of a brush on the device first (csrc/k_spawn.hip): the candidates are binned by cell, the particles of the
 * context stream past them once, and only the candidates with room are appended.  Nothing is downloaded but k verdicts.
 *
 * Every candidate gets exactly one verdict; the first rule that applies wins:
 *  1. GPE_SPAWN_OUTSIDE_WORLD, only with GPE_SPAWN_INSIDE_WORLD: with a = fabsf(r) the candidate passes when
 *     x >= a && x <= W - a && y >= a && y <= H - a, in IEEE binary32 with one rounding per operation, W and H as gpe_world
 *     returns them.  A NaN fails the test.  Without the flag nothing is rejected here, as gpe_add_particles rejects
 *     nothing.
 *  2. GPE_SPAWN_BLOCKED_BY_PARTICLE: the candidate is in contact with at least one particle of the context.  "In contact"
 *     is the predicate of gpe_query_contacts -- dx*dx + dy*dy < (ri + rj)*(ri + rj), the same binary32 operations, radii
 *     as stored, a NaN anywhere compares false (such a candidate is never blocked).
 *  3. GPE_SPAWN_BLOCKED_BY_CANDIDATE, only with GPE_SPAWN_SEPARATE: of the candidates rules 1 and 2 left, taken in
 *     ascending input index, a candidate is blocked when it is in contact with a candidate of lower input index that was
 *     itself ADDED.  This sequential greedy rule defines the result; the device reaches it in rounds whose number, but
 *     not whose outcome, depends on the launch geometry and on the order in which waves run.
 *  4. GPE_SPAWN_ADDED otherwise.
 * Without GPE_SPAWN_DRY_RUN the ADDED candidates are appended in input order, and the context is what
 * gpe_add_particles(those candidates' pos, radius) would have left: gpe_len, prev = pos, gpe_max_radius = fmaxf over the
 * appended radii only, the grid max radius and the cell size, the index buffers, growth by doubling, the native
 * re-derivation; with uids on the appended particles get next .. next + added - 1 in input order (next + added > 2^32:
 * GPE_ERR_STATE, nothing added).  Every later step, in either mode, with or without re-sorts, is bit-identical to that of
 * a twin context that made the plain add.  added == 0 and a dry run leave the context untouched, as gpe_query_contacts
 * does: nothing a step can see changes, and the counters, the kept block table, the rosters, the uid map and the scratch
 * index arrays stay as they were.  Synchronises, like gpe_add_particles.
 *  - The search uses a cell size of its own, gpe_compute_cell_size(R), R = the larger of |gpe_max_radius| and the largest
 *    |radius| among the candidates: a contact implies a centre distance below 2 R, so the 3 x 3 cell neighbourhood is
 *    complete.  A gpe_grid_set_max_radius override plays no part.  R (or that cell size) not finite:
 *    GPE_ERR_UNSUPPORTED.  R == 0: nothing touches, rules 2 and 3 block nobody.
 *  - Positions of particles and of candidates may be anything gpe_set_particles accepts -- 1e30, +-inf, NaN, negative:
 *    the verdicts are exactly the predicate's, and the search never reads or writes out of bounds for them.
 *  - Errors: a NULL ctx or spawn, a NULL pos_xy or radius with k > 0, unknown flag bits, a struct_size below
 *    sizeof(gpe_particle_spawn): GPE_ERR_INVALID_ARG; no particles yet: GPE_ERR_STATE, as gpe_add_particles; a sharded
 *    context (gpe_shard_*, order keys or an active cell box), or gpe_len + k above the 2^30 - 1 particles
 *    gpe_add_particles allows: GPE_ERR_UNSUPPORTED.  k == 0: GPE_OK, added = 0.  On any error added = 0, verdict is not
 *    written and the context is untouched -- except that a NULL ctx and a struct_size below sizeof(gpe_particle_spawn)
 *    leave `added` as it was too: the first is refused before the struct is looked at, and the second declares a struct
 *    that ends before `added`, its last field. */
enum { GPE_SPAWN_SEPARATE = 1u, GPE_SPAWN_INSIDE_WORLD = 2u, GPE_SPAWN_DRY_RUN = 4u };
enum { GPE_SPAWN_ADDED = 0, GPE_SPAWN_BLOCKED_BY_PARTICLE = 1, GPE_SPAWN_BLOCKED_BY_CANDIDATE = 2,
       GPE_SPAWN_OUTSIDE_WORLD = 3 };
typedef struct gpe_particle_spawn {
    uint32_t struct_size;     /* in: sizeof(gpe_particle_spawn)                                       */
    uint32_t flags;           /* in: GPE_SPAWN_*; unknown bits: GPE_ERR_INVALID_ARG                   */
    uint64_t k;               /* in: number of candidates                                             */
    const float *pos_xy;      /* in: f32[2k]                                                          */
    const float *radius;      /* in: f32[k]                                                           */
    uint8_t  *verdict;        /* out, may be NULL: u8[k], GPE_SPAWN_* per candidate, input order      */
    uint64_t added;           /* out: candidates with verdict ADDED (also in a dry run)               */
} gpe_particle_spawn;         /* 48 bytes */
gpe_status gpe_add_particles_free(gpe_ctx *ctx, gpe_particle_spawn *spawn);

/* ---- grid (src/grid/grid.rs) ---------------------------------------------------------------- */
/* Grid::compute_cell_size (:159-161) */
float gpe_compute_cell_size(float max_obj_radius);
/* Grid::new_without_camera(ctx, max_obj_radius, &particles) (:74): override the radius the cell
 * size is derived from (default: the particle system's max radius, Grid::new :66-71).
 * Below max_radius / 1.1 the cell is narrower than the largest particle: such a particle can lie in two
 * cells of one colour, and the colour passes then move it from two lanes at once (so does the reference's
 * collision_solver.wgsl).  The step still runs, but its bits are not reproducible; at or above that
 * radius every step is. */
gpe_status gpe_grid_set_max_radius(gpe_ctx *ctx, float max_obj_radius);
gpe_status gpe_cell_size(const gpe_ctx *ctx, float *cell_size);     /* Grid::cell_size (:163) */
/* The radius the cell size is derived from: the last gpe_grid_set_max_radius value, or gpe_max_radius
 * after set / add / remove (cell size = this * 2.2 in binary32, which is not exactly invertible). */
gpe_status gpe_grid_max_radius(const gpe_ctx *ctx, float *max_obj_radius);
gpe_status gpe_grid_build(gpe_ctx *ctx);     /* Grid::build_cell_ids (:296-306), K5          */
gpe_status gpe_grid_sort(gpe_ctx *ctx);      /* Grid::sort_map (:310-312), 4N-pair sort      */
gpe_status gpe_grid_update(gpe_ctx *ctx);    /* Grid::update (:322-332) = build + sort       */

/* ---- physics (src/physics/collision_system.rs) ---------------------------------------------- */
/* CollisionSystem::solve_collisions (:30-39): collision-cell list (K6, scan, K10) then the four
 * colour passes (K11).  Operates on the pair list left by gpe_grid_update. */
gpe_status gpe_solve_collisions(gpe_ctx *ctx);
/* CollisionCellBuilder::build_collision_cells alone (collision_cell_builder.rs:211-236) */
gpe_status gpe_build_collision_cells(gpe_ctx *ctx);

/* ---- step (src/state.rs:115-131) ------------------------------------------------------------ */
/* One State::update(): [re-sort] -> grid update -> solve collisions -> integrate. */
gpe_status gpe_step(gpe_ctx *ctx, float dt, uint32_t flags);
/* `steps` updates with no host synchronisation in between; re-sorts on the first step when
 * resort_first != 0 (particle_system.rs:45) and then every resort_every steps (0 = never;
 * the reference re-sorts every 4 s of wall clock, particle_system.rs:13-14,229-231). */
gpe_status gpe_run(gpe_ctx *ctx, float dt, uint64_t steps, uint64_t resort_every, int32_t resort_first);
gpe_status gpe_sync(gpe_ctx *ctx);
gpe_status gpe_set_mode(gpe_ctx *ctx, uint32_t mode);

/* Which kernels does the next gpe_step() run, and if not the NATIVE ones, why not?  The reference has one pipeline
 * and no switch (state.rs:34-70); here mode NATIVE (the default) falls back to the COMPAT kernels -- same bits -- for
 * the inputs listed below, and this call is how a host sees it.  Synchronises (it reads a device counter). */
enum { GPE_PIPELINE_COMPAT = 0, GPE_PIPELINE_NATIVE = 1 };
enum {
    GPE_REASON_NONE = 0,             /* the NATIVE kernels run                                                     */
    GPE_REASON_MODE_COMPAT = 1,      /* gpe_config.mode / gpe_set_mode asked for COMPAT                            */
    GPE_REASON_NO_PARTICLES = 2,     /* nothing to step yet                                                        */
    GPE_REASON_OUT_OF_BOX = 3,       /* a particle lay outside [0, world] when the context was configured          */
    GPE_REASON_GRID_TOO_WIDE = 4,    /* more than 65000 cells along an axis (16-bit cell coordinates)              */
    GPE_REASON_TABLE_TOO_LARGE = 5,  /* more than 2^27 8x8-cell blocks (a block table above 1 GiB)                 */
    GPE_REASON_DENSE_WINDOWS = 6     /* a 24x24-cell window holds more than 16384 particles (24576 to enter): held */
                                     /* on COMPAT, probed every 256 steps, returns by itself when it thins out     */
};
typedef struct gpe_pipeline_info {
    uint32_t struct_size;        /* in: sizeof(gpe_pipeline_info)                                                  */
    uint32_t pipeline;           /* GPE_PIPELINE_*: what the next step runs                                        */
    uint32_t reason;             /* GPE_REASON_*                                                                   */
    uint32_t sort_passes;        /* NATIVE: 8-bit radix passes of one sort of the block keys                       */
    uint64_t native_steps;       /* steps run on the NATIVE kernels since gpe_create                               */
    uint64_t compat_steps;       /* ... on the COMPAT kernels                                                      */
    uint64_t native_sorts;       /* NATIVE steps whose radix passes ran (the others reused the kept block table)   */
    uint32_t window_max;         /* largest 24x24-cell window population last reported by the tiles                */
    uint32_t roster_stamp;       /* the sort count the tile rosters are checked against (the tiles' own copy of    */
                                 /* native_sorts, low 32 bits: the two are equal or the rosters would be stale)    */
    /* what the tiles of the last reported NATIVE step did (lagged by the steps in flight; a host that fills in a   */
    /* struct_size up to roster_stamp gets the fields above only):                                                   */
    uint32_t overflow_tiles;     /* 32x32 tiles handed to the over-capacity launch                                  */
    uint32_t overflow_subtiles;  /* 16x16 quarters of those redone as four 8x8 tiles                                */
    uint32_t overflow_spills;    /* 8x8 tiles staged in the global spill arena                                      */
    uint32_t arena_slots;        /* spill-arena slots handed out                                                    */
    /* (a host that fills in a struct_size up to arena_slots gets the fields above only)                            */
    uint32_t uniform_radius;     /* NATIVE: 1 while the step runs the kernels that take ONE radius as a constant -- */
                                 /* every radius was the same number in [1e-30, 1e30] when the context was last    */
                                 /* configured, on one device, and gpe_device_ptr(GPE_RADIUS) not handed out since */
} gpe_pipeline_info;
gpe_status gpe_get_pipeline_info(gpe_ctx *ctx, gpe_pipeline_info *info);

/* ---- downloads (GpuBuffer::download, utils/gpu_buffer.rs:96-175) ---------------------------- */
typedef enum gpe_array {
    GPE_POS = 0,               /* current_positions   f32[2n]   particle_system.rs:258-265        */
    GPE_PREV = 1,              /* previous_positions  f32[2n]                                     */
    GPE_RADIUS = 2,            /* radii               f32[n]                                      */
    GPE_HOME_CELL_IDS = 3,     /* u32[n]   ParticleSystem::download_home_cell_ids (:250)          */
    GPE_PARTICLE_IDS = 4,      /* u32[n]   ParticleSystem::download_particle_ids (:254)           */
    GPE_CELL_IDS = 5,          /* u32[4n]  Grid::download_cell_ids (grid.rs:314)                  */
    GPE_OBJECT_IDS = 6,        /* u32[4n]  Grid::download_object_ids (grid.rs:318)                */
    GPE_COLLISION_CELLS = 7,   /* u32[4n]  CollisionSystem::download_collision_cells (:41)        */
    GPE_NUM_COLLISION_CELLS = 8, /* u32[1] last element of the scanned chunk counts               */
    GPE_CHUNK_OBJ_COUNT = 9,   /* u32[n]   CollisionCellBuilder::chunk_obj_count (scanned)        */
    GPE_INDIRECT_ARGS = 10,    /* u32[3]   collision_cell_builder.wgsl:96-109                     */
    GPE_ORDER_KEYS = 11,       /* u32[n]   sharded runs: global object index of each local particle */
    GPE_UIDS = 12              /* u32[n]   particle uids (gpe_enable_uids); GPE_ERR_STATE while off  */
} gpe_array;
/* Blocks until the stream is idle, then copies exactly `bytes` (must equal the array's size). */
gpe_status gpe_download(gpe_ctx *ctx, gpe_array what, void *dst, uint64_t bytes);
gpe_status gpe_array_bytes(const gpe_ctx *ctx, gpe_array what, uint64_t *bytes);
/* Render hand-off (particle_drawer.wgsl:11-13 reads these three as storage buffers): the device
 * pointer stays valid until the next set/add_particles or morton_resort (GPE_UIDS: the same). */
gpe_status gpe_device_ptr(gpe_ctx *ctx, gpe_array what, void **device_ptr, uint64_t *bytes);

/* ---- GPU primitives (src/utils/radix_sort, src/utils/prefix_sum) ----------------------------- */
/* GpuBuffer<u32> stand-in for the primitive tests (utils/gpu_buffer.rs:31-47,96-175). */
gpe_status gpe_buffer_alloc(gpe_ctx *ctx, uint64_t bytes, void **device_ptr);
gpe_status gpe_buffer_free(gpe_ctx *ctx, void *device_ptr);
gpe_status gpe_buffer_upload(gpe_ctx *ctx, void *device_ptr, const void *src, uint64_t bytes);
gpe_status gpe_buffer_download(gpe_ctx *ctx, const void *device_ptr, void *dst, uint64_t bytes);
/* GPUSorter::sort (radix_sort.rs:199-217): stable ascending sort of n (u32 key, u32 payload)
 * pairs, result in the caller's buffers.  Device pointers. */
gpe_status gpe_sort_pairs_u32(gpe_ctx *ctx, uint32_t *d_keys, uint32_t *d_payload, uint64_t n);
/* GPUSorter::build_histogram (radix_sort.rs:180-188): 256-bin histogram of (key >> shift) & 255
 * over all n keys (the reference keeps one per workgroup; with n <= 11520 there is one). */
gpe_status gpe_sort_histogram_u32(gpe_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint32_t shift,
                                  uint32_t *d_hist256);
/* GPUSorter::scatter (radix_sort.rs:190-198): ONE stable pass on the 8-bit digit at `shift`,
 * from (keys_a, payload_a) into (keys_b, payload_b). */
gpe_status gpe_sort_scatter_pass_u32(gpe_ctx *ctx, const uint32_t *d_keys_a, const uint32_t *d_payload_a,
                                     uint32_t *d_keys_b, uint32_t *d_payload_b, uint64_t n, uint32_t shift);
/* PrefixSum::execute (prefix_sum.rs:143-160): in-place inclusive u32 scan, wrap-around add. */
gpe_status gpe_inclusive_scan_u32(gpe_ctx *ctx, uint32_t *d_data, uint64_t n);

/* ---- sharding support (the reference is single-device, so no counterpart there) ---- */
/* One context per GPU holds the particles whose home cell that rank owns, followed by ghost copies of
 * the neighbours' particles within 5 cells of its region (the dependency cone of the four colour passes).
 * Ghosts take part in collisions but are not integrated; their results are discarded.  The host side
 * (gpu-physics-engine_amd/sharded.py) moves migrants and ghosts between ranks over RCCL point-to-point. */
/* Grow every buffer to hold `capacity` particles, keeping the current ones. */
gpe_status gpe_reserve(gpe_ctx *ctx, uint64_t capacity);
gpe_status gpe_capacity(const gpe_ctx *ctx, uint64_t *capacity);
/* The first n_owned of the n_total resident particles are this rank's own (integrated by K12); the rest
 * are ghosts written by the caller through gpe_device_ptr(GPE_POS / GPE_RADIUS / GPE_ORDER_KEYS). */
gpe_status gpe_set_counts(gpe_ctx *ctx, uint64_t n_total, uint64_t n_owned);
/* Order the members of a cell by GPE_ORDER_KEYS[local index] (the particle's index in the unsharded
 * system) instead of by local index, so a sharded run reproduces the single-device pair order. */
gpe_status gpe_use_order_keys(gpe_ctx *ctx, int32_t enable);
/* Cells [cx0..cx1] x [cy0..cy1] contain every resident particle: the native tile grid is cut to it. */
gpe_status gpe_set_active_cells(gpe_ctx *ctx, int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1);
/* The context's hipStream_t, so that a host framework can enqueue its own packing / exchange work in
 * order with the library's kernels. */
gpe_status gpe_stream_handle(gpe_ctx *ctx, void **hip_stream);
/* Run on a stream the CALLER owns (hipStream_t; it must outlive the context or the next gpe_set_stream).  A host
 * framework that allocates, frees or communicates on the context's stream (torch's caching allocators and
 * ProcessGroupNCCL remember the stream of every buffer they handle) lends its own stream instead of borrowing
 * the library's: the library never destroys a borrowed stream.  NULL returns to the library's own stream.
 * Synchronises the stream in use before switching. */
gpe_status gpe_set_stream(gpe_ctx *ctx, void *hip_stream);
/* Re-derive the native pipeline's configuration after the caller changed particles in place. */
gpe_status gpe_refresh(gpe_ctx *ctx);
/* For every owned particle whose 8x8-cell block (row-major blocks_x x blocks_y over the world) is owned by
 * another rank (a migrant) and/or borders other ranks (a ghost for them), append (local index, info):
 * info bits 0-25 = the block's destination-rank mask, bits 26-30 = 1 + the block's owner when that is not
 * my_rank (at most 26 ranks).  *d_out_count (device, zeroed by the caller) receives the number appended
 * (entries beyond out_capacity are dropped). */
gpe_status gpe_shard_classify(gpe_ctx *ctx, const uint8_t *d_owner_of_block, const uint32_t *d_dest_mask_of_block,
                              int32_t blocks_x, int32_t blocks_y, uint32_t my_rank, uint32_t *d_out_index,
                              uint32_t *d_out_info, uint32_t *d_out_count, uint64_t out_capacity);

/* Device-resident exchange (k_shard.hip): the same protocol without a host round trip per step.  The caller owns
 * two device buffers of u32 words and moves the neighbour segments between ranks (RCCL send/recv, fixed sizes):
 * after pack, segment s of d_send goes to rank slot_rank[s] and lands in that rank's d_recv segment for this rank.
 * Segment = [n_migrants, n_ghosts, 0, 0][cap_mig rows of 6 words: x y prev_x prev_y r key][cap_gho rows of 4 words:
 * x y r key].  Slots are the neighbouring ranks in ascending order followed by this rank (its own segment of
 * d_send holds the migrants that stay behind as ghosts; it is not sent).  Both sides must agree on the capacities.
 * Needs order keys, the native pipeline and an active box; every rank region at least two blocks wide. */
typedef struct gpe_shard_plan {
    uint32_t struct_size;          /* = sizeof(gpe_shard_plan)                                   */
    uint32_t rank, world_size, n_slots;
    int32_t  blocks_x, blocks_y;   /* block grid of the whole world (tables below)               */
    const uint8_t  *d_owner_of_block;
    const uint32_t *d_dest_mask_of_block;
    uint32_t slot_rank[9];
    uint32_t send_off[9], send_cap_mig[9], send_cap_gho[9];   /* word offsets into d_send, rows   */
    uint32_t recv_off[9], recv_cap_mig[9], recv_cap_gho[9];   /* word offsets into d_recv, rows   */
    uint32_t *d_send, *d_recv;
    int32_t  own_x0, own_y0, own_x1, own_y1;   /* the rank's rectangle in blocks, half-open (all 0: not told).  Told, the  */
                                               /* tiles of the step pack their own particles as they write them back and   */
                                               /* no pack kernel runs (struct_size without these four is accepted too)     */
} gpe_shard_plan;
gpe_status gpe_shard_configure(gpe_ctx *ctx, const gpe_shard_plan *plan);
/* Counts go to the device (owned = total = the host's owned count, ghosts dropped); packs the first segments. */
gpe_status gpe_shard_begin(gpe_ctx *ctx);
/* Consume d_recv: fill the migrants' holes, append arriving migrants, then ghosts.  No host sync. */
gpe_status gpe_shard_unpack(gpe_ctx *ctx);
/* gpe_shard_unpack + one step (State::update without re-sort) + pack of the next segments.  No host sync. */
gpe_status gpe_shard_step(gpe_ctx *ctx, float dt);
/* The counts as last mirrored to pinned host memory: no synchronisation, they lag by the steps in flight (<= ~64).
 * For capacity planning (grow the buffers before the device-side total reaches the capacity). */
gpe_status gpe_shard_peek(gpe_ctx *ctx, uint64_t *n_owned, uint64_t *n_total);
/* Synchronises and returns the device-side counts; leave != 0 also returns the context to host-side counts
 * (owned particles only), e.g. before a Morton re-sort or a download.  Reports exchange errors. */
gpe_status gpe_shard_counts(gpe_ctx *ctx, uint64_t *n_owned, uint64_t *n_total, int32_t leave);

/* Moving the packed segments between the ranks, inside the library: RCCL point-to-point over xGMI.  One grouped
 * ncclSend / ncclRecv pair per neighbouring rank on the context's stream (fixed sizes, nothing to wait for on the
 * host), so a host in any language drives a sharded run with gpe_shard_run alone between two re-sorts.
 * librccl.so.1 is loaded at the first of these calls (dlopen: a process that already holds RCCL, e.g. under
 * torch.distributed, shares its copy). */
#define GPE_COMM_ID_BYTES 128u
/* ncclGetUniqueId: call on one rank, hand the 128 bytes to every rank (any side channel). */
gpe_status gpe_comm_unique_id(uint8_t *id128);
/* ncclCommInitRank on the context's device: collective over the world_size ranks of the decomposition
 * (rank numbers = gpe_shard_plan.rank / slot_rank).  The communicator belongs to the context. */
gpe_status gpe_shard_comm_init(gpe_ctx *ctx, const uint8_t *id128, uint32_t rank, uint32_t world_size);
/* Use a communicator the caller created (ncclComm_t); the caller keeps ownership. */
gpe_status gpe_shard_comm_attach(gpe_ctx *ctx, void *nccl_comm);
gpe_status gpe_shard_comm_destroy(gpe_ctx *ctx);
/* Any other transport (tests: gloo through host memory): fn must enqueue / perform the transfer of every neighbour
 * segment of d_send into the peers' d_recv in order with hip_stream and return 0.  NULL removes it. */
typedef int32_t (*gpe_shard_transport_fn)(void *user, const uint32_t *d_send, uint32_t *d_recv, void *hip_stream);
gpe_status gpe_shard_set_transport(gpe_ctx *ctx, gpe_shard_transport_fn fn, void *user);
/* Send the segments packed by gpe_shard_begin / gpe_shard_step and receive the neighbours' (communicator or transport). */
gpe_status gpe_shard_exchange(gpe_ctx *ctx);
/* `steps` x (gpe_shard_exchange, gpe_shard_step): the step loop of a sharded run between two re-sorts, no host
 * synchronisation (the host stays at most ~64 steps ahead of the device). */
gpe_status gpe_shard_run(gpe_ctx *ctx, float dt, uint64_t steps);
/* Do librccl.so.1 and every entry point used above resolve on this machine?  (No GPU needed.) */
gpe_status gpe_comm_probe(void);

/* ---- sharded control plane: decomposition, set-up, global re-sort, load re-cut, the scheduled run -----------------
 * Everything a host needs to drive a sharded run through this header alone (no Python, no torch): the reference's
 * State::update schedule (state.rs:115-131: re-sort gate, then the step) across ranks.  One context per rank -- one
 * process per GPU, or one thread per context inside one process (gpe_local_group_*).  The collective calls below
 * (marked so) must be made by every rank, in the same order. */
#define GPE_SHARD_MAX_RANKS 26u
/* The world cut into px x py rectangles of 8x8-cell blocks (rank = j * px + i owns block columns xcuts[i]..xcuts[i+1],
 * block rows ycuts[j]..ycuts[j+1]).  A plain value: every rank builds the same one from the same arguments. */
typedef struct gpe_shard_layout {
    uint32_t struct_size;                       /* = sizeof(gpe_shard_layout)                                  */
    uint32_t world_size, px, py;
    float    world_width, world_height, cell_size;
    int32_t  cells_x, cells_y;                  /* home cell columns / rows: floor(world / cell) + 1           */
    int32_t  blocks_x, blocks_y;                /* 8x8-cell blocks                                             */
    int32_t  xcuts[27];                         /* px + 1 entries rising from 0 to blocks_x (27 = MAX_RANKS + 1) */
    int32_t  ycuts[27];                         /* py + 1 entries rising from 0 to blocks_y                    */
} gpe_shard_layout;
/* Host only (no GPU needed).  px = py = 0: the process grid as square as possible, px <= py.  xcuts / ycuts NULL: equal
 * widths; else px + 1 / py + 1 entries (what gpe_shard_recut derives from the particle quantiles). */
gpe_status gpe_shard_layout_build(float world_width, float world_height, float cell_size, uint32_t world_size,
                                  uint32_t px, uint32_t py, const int32_t *xcuts, const int32_t *ycuts,
                                  gpe_shard_layout *out);
/* Owner rank of each of n host positions (interleaved x,y; the kernels' own f32 arithmetic: floor(p / cell) >> 3,
 * clamped to the block grid): how a host deals the initial particles to the ranks. */
gpe_status gpe_shard_layout_owner_of(const gpe_shard_layout *layout, const float *pos_xy, uint64_t n, uint8_t *owner_out);
/* Cut `bins` block columns (rows) into `parts` runs of about equal particle count, every run at least min_width blocks
 * wide: cuts_out receives parts + 1 entries.  Pure function (every rank derives the same cuts from the same histogram). */
gpe_status gpe_shard_quantile_cuts(const uint64_t *hist, uint32_t bins, uint32_t parts, uint32_t min_width, int32_t *cuts_out);

/* What the control plane needs from "the other ranks", when it is not the in-library RCCL communicator
 * (gpe_shard_comm_init / _attach) or a local group (gpe_local_group_join): two collectives over device memory, both
 * ordered with hip_stream; they may block the host.  Return 0 on success. */
enum { GPE_REDUCE_SUM = 0, GPE_REDUCE_MAX = 1 };
typedef struct gpe_shard_collectives {
    uint32_t struct_size;
    uint32_t reserved;
    void *user;
    /* in-place all-reduce of `count` u32 words at d_buf over all ranks (op: GPE_REDUCE_*) */
    int32_t (*all_reduce_u32)(void *user, uint32_t *d_buf, uint64_t count, uint32_t op, void *hip_stream);
    /* for every rank r: send_count[r] words at d_send + send_off[r] go to rank r, which finds them at its d_recv +
     * recv_off[this rank]; recv_count[r] words arrive from rank r.  (ncclSend / ncclRecv pairs in one group.) */
    int32_t (*all_to_all_u32)(void *user, const uint32_t *d_send, const uint64_t *send_off, const uint64_t *send_count,
                              uint32_t *d_recv, const uint64_t *recv_off, const uint64_t *recv_count, void *hip_stream);
} gpe_shard_collectives;
/* NULL: back to the in-library communicator.  The struct is copied. */
gpe_status gpe_shard_set_collectives(gpe_ctx *ctx, const gpe_shard_collectives *coll);

/* Several contexts of ONE process as the ranks of a sharded run: one host thread per context (every collective call
 * blocks until all ranks have made it), segments and collectives moved by hipMemcpyAsync / kernels between the
 * contexts' buffers (same device, or peers).  What a single-process host -- the reference's State owns one device,
 * renderer/wgpu_context.rs:42-49 -- grows into on a multi-GPU node without a collective library. */
typedef struct gpe_local_group gpe_local_group;
gpe_status gpe_local_group_create(uint32_t world_size, gpe_local_group **out);
gpe_status gpe_local_group_destroy(gpe_local_group *group);
/* The context becomes rank `rank` of the group: its collectives and its segment transport are the group's. */
gpe_status gpe_local_group_join(gpe_ctx *ctx, gpe_local_group *group, uint32_t rank);
/* A rank that failed leaves the others waiting in a collective: this wakes them all with an error. */
gpe_status gpe_local_group_abort(gpe_local_group *group);

/* ParticleSystem::new_from_buffers (particle_system.rs:49-99) for one rank: its n owned particles with their global
 * indices (order_key[i] = the particle's index in the unsharded system), buffers sized for `capacity` particles
 * (0: 1.3 n + 4096; ghosts and arrivals need room).  prev_xy NULL: previous = current. */
gpe_status gpe_shard_set_particles(gpe_ctx *ctx, const float *pos_xy, const float *prev_xy, const float *radius,
                                   const uint32_t *order_key, uint64_t n, uint64_t capacity);
/* COLLECTIVE.  Makes the context rank `rank` of `layout`: agrees on the cell size of the whole system (2.2 x the
 * largest radius over all ranks, grid.rs:159-161) and checks the layout was cut with it, switches the order keys on,
 * cuts the tile grid to the rank's rectangle + ghost ring, sizes the neighbour segments from the densest rank's block
 * population x capacity_scale (1.0; both ends of a pair get the same numbers, and the set-up compares them: a send and
 * a receive of different lengths would wait for ever), allocates the tables and segment buffers inside the library and
 * configures the device-resident exchange (gpe_shard_configure).  Needs collectives: a communicator, a local group or
 * gpe_shard_set_collectives; every rectangle at least two blocks wide, at most 8 neighbours. */
gpe_status gpe_shard_setup(gpe_ctx *ctx, const gpe_shard_layout *layout, uint32_t rank, float capacity_scale);
/* The layout in use (gpe_shard_recut replaces it). */
gpe_status gpe_shard_get_layout(const gpe_ctx *ctx, gpe_shard_layout *out);
/* COLLECTIVE.  ParticleSort::sort (particle_sort.rs:58-69) across the ranks: every particle goes home to its owner
 * (exchange + unpack, ghosts dropped), then K1 + stable sort by home-cell key + K4 on the owned particles in the order
 * of their old global indices, and the NEW global indices -- the particle's position in the single-device sorted order --
 * from one all-reduce of the histogram over Morton blocks (a block of 64 consecutive keys = one 8x8-cell block = one
 * owner): index = particles of all ranks in earlier blocks + position inside the block.  Leaves the context with
 * host-side counts; the next gpe_shard_run_scheduled / gpe_shard_begin starts the device-resident loop again. */
gpe_status gpe_shard_resort(gpe_ctx *ctx);
/* COLLECTIVE; call where gpe_shard_resort may be called (it is called BY gpe_shard_run_scheduled before its re-sorts).
 * When the most loaded rank owns more than `above` x the mean (1.25; <= 0: never): new cuts at the particle quantiles of
 * the all-reduced block-column / block-row histograms, every particle moved to its new owner (one all-to-all), tables,
 * tile grid and segments re-planned.  Results do not depend on the cuts.  *recut (may be NULL) = 1 when they changed. */
gpe_status gpe_shard_recut(gpe_ctx *ctx, float above, int32_t *recut);
/* COLLECTIVE.  State::update (state.rs:115-131) `steps` times for this rank: a re-sort (gpe_shard_recut at 1.25, then
 * gpe_shard_resort) before step 0 when resort_first != 0 and before every resort_every-th step (0: never), and
 * gpe_shard_run for the steps in between -- no host synchronisation except at the re-sorts. */
gpe_status gpe_shard_run_scheduled(gpe_ctx *ctx, float dt, uint64_t steps, uint64_t resort_every, int32_t resort_first);
/* The rank's owned particles as host arrays (synchronises; the counts come from the device): up to `capacity` of
 * them, *n_owned receives their number.  order_key_out / pos_xy_out / prev_xy_out may each be NULL. */
gpe_status gpe_shard_download_owned(gpe_ctx *ctx, uint32_t *order_key_out, float *pos_xy_out, float *prev_xy_out,
                                    uint64_t capacity, uint64_t *n_owned);
/* Counters of the control plane since gpe_shard_setup. */
typedef struct gpe_shard_stats {
    uint32_t struct_size;
    uint32_t recuts;             /* gpe_shard_recut calls that changed the cuts                          */
    uint64_t resorts;            /* gpe_shard_resort calls                                               */
    uint64_t steps;              /* steps run by gpe_shard_run_scheduled                                 */
    uint64_t n_owned, n_ghost;   /* as of the last synchronising call                                    */
    uint32_t n_neighbours;
    uint32_t transport;          /* 0 none, 1 RCCL inside the library, 2 local group, 3 caller callbacks */
} gpe_shard_stats;
gpe_status gpe_shard_get_stats(gpe_ctx *ctx, gpe_shard_stats *out);

/* ---- profiling (wgpu_profiler scopes threaded through every reference call) ------------------ */
typedef struct gpe_timing {
    char     name[64];    /* the reference's scope label, e.g. "Sort map" (grid.rs:329); kernel-level
                             entries are "<scope>/<kernel>"                                   */
    double   total_ms;    /* sum over calls since the last gpe_reset_timings                  */
    uint64_t calls;
} gpe_timing;
/* on = 0: off; 1: every scope of every call; k > 1: the scopes of every k-th step only (sampled --
   an event pair per kernel costs about as much as a small kernel). */
gpe_status gpe_set_profiling(gpe_ctx *ctx, uint32_t on);
gpe_status gpe_reset_timings(gpe_ctx *ctx);
/* Synchronises, then writes up to *count entries; *count receives the number available. */
gpe_status gpe_get_timings(gpe_ctx *ctx, gpe_timing *out, uint32_t *count);

/* The reference's `--features benchmark` build writes every finished frame's scopes as a Chrome trace
 * (state.rs:108-112, wgpu_profiler::chrometrace): one entry per recorded scope instance, start relative to the
 * last gpe_reset_timings (or to the gpe_set_profiling call that switched profiling on).  The newest 65536
 * instances are kept.  Same calling convention as gpe_get_timings; gpu-physics-engine_amd/engine.py
 * (Context.write_chrome_trace) turns them into the JSON chrome://tracing loads. */
typedef struct gpe_trace_event {
    char   name[64];
    double start_ms;
    double duration_ms;
} gpe_trace_event;
gpe_status gpe_get_trace(gpe_ctx *ctx, gpe_trace_event *out, uint32_t *count);

/* ---- guarded device allocations (tests; DESIGN.md "device memory: payload, slack, red zones") ---------- */
/* With GPE_FLAG_GUARD_ALLOCS every device allocation of the context is front zone | payload | rear zone: the
 * payload is what kernels may write, the zones (>= 16 KiB each, the read-only slack of the allocation lies at
 * the head of the rear one) are filled with a canary word and the fresh payload with a poison word.
 * gpe_guard_check, stream-ordered behind the context's work, compares every zone of every live allocation with
 * the canary (one kernel), synchronises and fills *out; zones found damaged when their buffer was released or
 * regrown are kept and reported by every later call.  Damage is a finding, not an error: the status is GPE_OK,
 * the text of the first damaged zone goes to gpe_last_error.  Without the flag: GPE_OK, damaged = 0.  GPE_ERR_HIP when
 * the check itself failed, now or when a buffer was released (its evidence is gone: the report would not be complete).
 * gpe_config.guard_canary / guard_poison choose the words: each nonzero and below 1024, and different from the other --
 * such a word is a nonzero finite f32, and used as an index of 16-byte elements it stays inside a red zone; anything
 * else fails gpe_create with GPE_ERR_INVALID_ARG.  Without the flag the two words are ignored. */
#define GPE_GUARD_MAX_ZONES 8
enum { GPE_GUARD_FRONT = 0, GPE_GUARD_REAR = 1 };
typedef struct gpe_guard_zone {
    char     tag[32];        /* the allocation's tag, e.g. "native.codes"                                  */
    uint32_t side;           /* GPE_GUARD_FRONT / GPE_GUARD_REAR                                           */
    uint32_t first_word;     /* the aligned 32-bit word that holds the first damaged byte                 */
    int64_t  first_offset;   /* first / last damaged byte: front zone relative to the payload's first     */
    int64_t  last_offset;    /* byte (negative), rear zone relative to the first byte behind the payload  */
    uint64_t payload_bytes;
} gpe_guard_zone;
typedef struct gpe_guard_report {
    uint32_t struct_size;    /* in: sizeof(gpe_guard_report)                                               */
    uint32_t damaged;        /* damaged zones, those kept from released buffers included                   */
    uint32_t listed;         /* min(damaged, GPE_GUARD_MAX_ZONES): entries of zones[] filled               */
    uint32_t allocations;    /* live allocations checked                                                   */
    gpe_guard_zone zones[GPE_GUARD_MAX_ZONES];
} gpe_guard_report;
gpe_status gpe_guard_check(gpe_ctx *ctx, gpe_guard_report *out);
/* The registry of the context's device allocations (kept with and without the flag): one line
 * "tag payload_bytes slack_bytes live\n" per live allocation, then, with the flag, one
 * "tag payload_bytes slack_bytes released\n" per tag of which an allocation has been released (its last one; those
 * were checked when they went), then one "tag bytes 0 pinned\n" per pinned host block the context has allocated (the
 * error words gpe_sync reads: one per context).  What the tests prove a growth with, and the coverage list of
 * profiles/guard/ is from.
 * NUL-terminated, truncated to capacity; *needed (may be NULL) receives the bytes the whole text takes. */
gpe_status gpe_guard_registry(gpe_ctx *ctx, char *text, uint64_t capacity, uint64_t *needed);

#ifdef __cplusplus
}
#endif
#endif /* GPE_H */
