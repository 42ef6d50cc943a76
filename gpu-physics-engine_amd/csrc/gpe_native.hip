// gpe_native.hip -- the host side of the native step (GPE_MODE_NATIVE): its buffers, the lagged statistics the kernels
// publish, the configuration-time checks and the step itself -- hash -> [sort -> block table] -> collide -- with every
// decision about what to launch (native_policy.h).  The kernels and their launchers are k_native.hip's; the two sides
// meet in native_launch.h, and nothing here is device code.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>

#include "gpe_internal.h"
#include "native_launch.h"

namespace gpe {

// The device buffers of NativeState.  release: free and forget; reserve: a fresh buffer of `bytes` in place of the old one
// (whose contents are not kept).  After a failed reserve the pointer is NULL and the error is the caller's: GPE_HIP for a
// buffer the path needs.  An optional buffer is released through GPE_HIP first (a failing hipFree stays an error) and
// then reserved: only the failed allocation means "run without".
// payload / slack: bytes the kernels may write / bytes behind them that are only read (gpe_dev_reserve).
template <class T>
static hipError_t release(gpe_ctx *c, T *&p)
{
    return dev_release(c, p);
}
template <class T>
static hipError_t reserve(gpe_ctx *c, T *&p, size_t payload, size_t slack, const char *tag)
{
    hipError_t e = release(c, p);
    if (e == hipSuccess) e = dev_reserve(c, &p, payload, slack, tag);
    return e;
}

void native_release(gpe_ctx *c)
{
    NativeState &N = c->native;
    void *bufs[] = {N.block_table, N.keys, N.ids, N.keys_b, N.ids_b, N.codes, N.sorted_key, N.gkeys, N.gids, N.gkeys_b,
                    N.gids_b, N.gtable, N.ghist, N.exc_count, N.gho_count, N.roster_hdr, N.roster_ids, N.tile_ctl,
                    N.overflow1, N.arena};
    for (void *b : bufs) (void)release(c, b);
    (void)release(c, N.dbg_stamps);
    (void)release(c, N.dbg_cycles);
    if (N.host_stat) (void)hipHostFree(N.host_stat);
    N = NativeState();
}

static gpe_status arena_reserve(gpe_ctx *c, uint64_t want);

// The pinned words check_device_errors (gpe_api.hip) copies the sticky device-side error words into: once per context,
// at the first synchronising call, so that gpe_sync enqueues its copies before it waits and waits once.  (Here, beside
// the step's own pinned statistics: pinned host memory has two homes in the library, this file and k_shard.hip.)
gpe_status error_words_reserve(gpe_ctx *c)
{
    if (c->err_words) return GPE_OK;
    GPE_HIP(c, hipHostMalloc((void **)&c->err_words, 64, hipHostMallocDefault));
    memset(c->err_words, 0, 64);
    DevAlloc a;                                        // listed by gpe_guard_registry, state "pinned"
    a.ptr = a.base = c->err_words; a.payload = a.total = 64; a.tag = "ctl.error_words";
    c->guard.pinned.push_back(a);
    return GPE_OK;
}

void error_words_release(gpe_ctx *c)
{
    if (!c->err_words) return;
    auto &pinned = c->guard.pinned;                    // (the registry lists blocks that exist)
    for (size_t i = pinned.size(); i-- > 0;)
        if (pinned[i].ptr == c->err_words) pinned.erase(pinned.begin() + i);
    (void)hipHostFree(c->err_words);
    c->err_words = nullptr;
}

// The words the tiles publish (k_native_hash, k_native_publish_probe) while the host reads them: each word on its own.
NativeStats native_read_stats(const NativeState &N)
{
    assert(N.host_stat != nullptr);
    const auto word = [&](int k) { return __atomic_load_n(&N.host_stat[k], __ATOMIC_RELAXED); };
    NativeStats s;
    s.window_max = word(kStatWindowMax);
    s.arena = word(kStatArena);
    s.probe = word(kStatProbe);
    s.overflow = word(kStatOverflow);
    s.sub_tiles = word(kStatSubTiles);
    s.spills = word(kStatSpills);
    s.sorts = word(kStatSorts);
    s.overflow_new = word(kStatOverflowNew);
    s.halves_over = word(kStatHalvesOver);
    return s;
}

// Diagnostics.  GPE_FLAG_NATIVE_STATS: the step statistics every 128 native_should_run calls.
static void native_print_stats(gpe_ctx *c, const NativeStats &s)
{
    NativeState &N = c->native;
    if (N.print_stats && (++N.stat_calls & 127u) == 0)
        fprintf(stderr, "[gpe native] call %u: window max %u, arena slots used %u of %llu, 32x32 tiles over capacity %u, "
                        "quarters redone as 8x8 tiles %u, 8x8 tiles through the arena %u\n", N.stat_calls,
                s.window_max, s.arena, (unsigned long long)N.arena_cap, s.overflow, s.sub_tiles, s.spills);
}

#ifdef GPE_TILE_STAMPS
// -DGPE_TILE_STAMPS builds: the collide launches' phase stamps (CollideArgs::stamps), printed every 20 native_collide
// calls.  Returns the stamps of this call's launches.
static unsigned long long *native_tile_stamps(gpe_ctx *c)
{
    unsigned long long *&g_stamps = c->native.dbg_stamps;
    // ([0, 64): the dense launch's tiles; [64, 128): the windows of the over-capacity launch)
    if (!g_stamps && reserve(c, g_stamps, 128 * 8, 0, "native.dbg_stamps") == hipSuccess) (void)hipMemset(g_stamps, 0, 128 * 8);
    static int g_calls = 0;
    if (++g_calls % 20 == 0) for (int part = 0; part < 2; ++part) {
        unsigned long long h[64];
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemcpy(h, g_stamps + 64 * part, sizeof(h), hipMemcpyDeviceToHost);
        fprintf(stderr, part == 0 ? "[dense launch]\n" : "[over-capacity launch]\n");
        for (int cls = 0; cls < 3; ++cls)
            fprintf(stderr, "[P5 waves] %s: busy %.0f  barrier wait %.0f cycles per colour pass (%llu wave-passes)\n",
                    cls == 0 ? "group waves" : cls == 1 ? "single waves" : "idle waves", h[40 + cls] ? (double)h[32 + cls] / h[40 + cls] : 0.0,
                    h[40 + cls] ? (double)h[36 + cls] / h[40 + cls] : 0.0, h[40 + cls]);
        fprintf(stderr, "[tile stamps] n=%llu", (unsigned long long)c->n);
        if (h[47])
            fprintf(stderr, "[P5 cells] per colour pass: %.1f one-lane cells, %.1f lane-group cells, %.2f whole-wave cells of %.1f members (largest %.1f);"
                    " a wave spends %.0f cycles in them and the rows; %.2f row cells; whole-wave cells by members <=16 / <=32 / <=64 / more: %.2f %.2f %.2f %.2f\n",
                    (double)h[44] / h[47], (double)h[45] / h[47], (double)h[46] / h[47],
                    h[46] ? (double)h[49] / h[46] : 0.0, (double)h[50] / h[47], (double)h[48] / (double)(h[40] + h[41] + h[42]),
                    (double)h[51] / h[47], (double)h[52] / h[47], (double)h[53] / h[47], (double)h[54] / h[47], (double)h[55] / h[47]);
        double all = 0;
        for (int i = 0; i < 14; ++i) all += (double)h[i];
        for (int i = 0; i < 14; ++i)
            fprintf(stderr, "  P%d %.0f (%.1f%%)", i, h[16 + i] ? (double)h[i] / (double)h[16 + i] : 0.0, all > 0 ? 100.0 * (double)h[i] / all : 0.0);
        fprintf(stderr, "  (tiles %llu of %llu started)\n", h[16 + 6], h[16 + 0]);
        if (part == 1) (void)hipMemset(g_stamps, 0, 128 * 8);
    }
    return g_stamps;
}
#endif

// hash -> [sort -> block table].  *sorted_ids receives the particle ids grouped by 8x8-cell block.
// The radix passes are enqueued every step but run only when the hash kernel finds a particle that has left the
// reach of the grouping they last produced (kDrift* cells beyond its block): the sorted ids and the block table are
// kept across steps, the per-particle codes carry the particle's cell (mod 128) and whether it is still within reach of
// its old block, and the tiles look up more blocks than they keep particles from.  Decided on the device, step by step; the host waits for nothing.
// In the benchmark cloud (gravity off) a sort is needed every few dozen steps, in free fall every 5-25 steps.
// always_sort: this call must not rely on the kept grouping (configuration-time probes).
static gpe_status native_prepare_step(gpe_ctx *c, uint32_t **sorted_ids, bool always_sort = false)
{
    NativeState &N = c->native;
    const uint64_t n = c->n;
    constexpr size_t kHistSet = (size_t)kHistCopies * 4 * 256;          // words of one set of digit histograms
    if (!c->os_ws.hist_clean) {                                        // another sort used the histograms since
        note_enqueue(c);
        GPE_HIP(c, hipMemsetAsync(c->os_ws.hist4, 0, 2 * kHistSet * sizeof(uint32_t), c->stream));
        c->os_ws.hist_clean = true;
        c->os_ws.hist_set = 0;
    }
    uint32_t *hist_now = c->os_ws.hist4 + (size_t)c->os_ws.hist_set * kHistSet;
    uint32_t *hist_next = c->os_ws.hist4 + (size_t)(c->os_ws.hist_set ^ 1u) * kHistSet;
    c->os_ws.hist_set ^= 1u;
    const uint32_t parity = (N.step_seq++) & 1u;
    // The kept grouping can be used when it belongs to these particles and this box.  Sharded runs (ghosts come and go
    // every step, padding keys) and one-pass sorts (the table would be reset and filled by the same launch) always sort.
    // A sharded run with its counts on the device (k_shard.hip) keeps the grouping of its OWNED particles the same way:
    // their indices are stable (a hole left by a migrant is filled from the tail, an arrival is appended: both reach
    // the tiles as stragglers until the next sort), while the ghosts -- new every step -- are grouped by a small sort
    // of their own, every step, into a second block table.  Other sharded set-ups (host-side counts) always sort.
    // A scene in which nearly every step sorts anyway (a crushed pile: a third of the particles move further than the
    // kept table reaches, every step) gains nothing from the kept table and pays for it in the hash kernel (the old
    // keys, the drift test: 1.2 instead of 0.6 ms at 100 M).  The passes' own counter says so (lagged): the policy's
    // sort hold then sorts unconditionally for a while, and the table gets another try after it.
    // Who counts the radix digits of a step that keeps its table (k_native_hash, fuse_hist): the hash kernel, fused, while
    // many recent steps sorted (a falling or crushed cloud before the sort hold takes over -- the separate launch reads all
    // keys again, 0.2-0.4 ms at 100 M when it runs, against the 0.075 ms per step the fused count costs the hash);
    // otherwise the gated launch, which returns at once on the steps that do not sort.
    const PreparePlan plan = N.policy.prepare(native_read_stats(N), always_sort, N.always_sort,
                                              (c->cfg.flags & GPE_FLAG_FUSED_HISTOGRAMS) != 0);
    const bool sharded = c->shard.on || c->use_order_keys || c->has_active_box;
    const bool kept_sharded = c->shard.on && c->shard.active && c->use_order_keys && N.gkeys != nullptr && !N.always_sort;
    const bool gated = N.passes >= 2 && (!sharded || kept_sharded);
    const bool reuse = gated && plan.keep_table && N.sort_state_valid && (kept_sharded || N.sorted_n == n) &&
                       N.exc_count != nullptr;                         // (no room for the straggler lists: sort every step)
    const uint64_t pairs = ((uint64_t)N.table_entries + 1) / 2;        // the table is allocated in 16-byte units
    const bool fuse_hist = plan.fuse_hist;
    // The keys have two readers, the gated histogram and the first radix pass, and both return at once on a step that does
    // not sort.  So a step that keeps its table and leaves the digits to the gated launch stores none (4 of the 24 B the
    // hash moves per particle): the gated launch forms them from the positions when it runs.  Not on sharded set-ups
    // (padding keys, ghosts); steps that fuse the histogram or sort unconditionally store them as they always did.
    const bool late_keys = reuse && !fuse_hist && !sharded;
    const bool uniform = N.uniform && !sharded;                        // (sharded: switched off where it begins, and here)
    HashGhosts hg;
    hg.sorted_count = N.tile_ctl + kCtlSortedCount;
    uint64_t g_bound = 0;
    if (kept_sharded) {
        // upper bound of the ghost count from the pinned mirror (lags by the steps in flight), as for the total
        const ShardState &SH = c->shard;
        g_bound = c->cap;
        const uint32_t epoch = __atomic_load_n(&SH.host_counts[kShardEpoch], __ATOMIC_ACQUIRE);
        if ((int32_t)(epoch - SH.begin_epoch) > 0) {
            const uint64_t gh = SH.host_counts[kShardTotal] >= SH.host_counts[kShardOwned]
                                    ? SH.host_counts[kShardTotal] - SH.host_counts[kShardOwned] : 0;
            g_bound = std::min<uint64_t>(c->cap, gh + std::max<uint64_t>(16384, gh / 4));
        }
        g_bound = std::min<uint64_t>(g_bound, n);
        hg.owned = SH.counts_now() + kShardOwned;
        hg.gkeys = N.gkeys; hg.gids = N.gids; hg.g_bound = g_bound;
        hg.gtable2 = (uint4 *)N.gtable; hg.gtable_pairs = pairs;
        hg.ghist_now = N.ghist + (size_t)N.ghist_set * kHistSet;       // (two sets, alternating over the steps that use them:
        hg.ghist_next = N.ghist + (size_t)(N.ghist_set ^ 1u) * kHistSet;   //  this step's hash zeroes the next one's)
        N.ghist_set ^= 1u;
        hg.ghost_sort = N.tile_ctl + kCtlGhostSort + parity;
        hg.ghost_sort_next = N.tile_ctl + kCtlGhostSort + (parity ^ 1u);
        if (N.gho_count && N.gho_cap >= N.exc_tiles) {                 // ghost lists: two sets by step parity, like the stragglers'
            hg.gl_count = N.gho_count + (size_t)parity * N.exc_tiles;
            hg.gl_count_next = N.gho_count + (size_t)(parity ^ 1u) * N.exc_tiles;
            hg.gl_entry = N.gho_count + 2 * N.exc_tiles + (size_t)parity * N.exc_tiles * kGhostSlots;
        }
    }
    // (block key / blocks_x = key * magic >> 40: OnesweepGate::key_div_magic)
    const uint64_t div_magic = ((1ull << 40) + (uint64_t)N.blocks_x - 1) / (uint64_t)N.blocks_x;
    {
        // (what follows the hash is the gated histogram or the first gated radix pass: either carries the boundary
        // behind it; the hash carries the one in front of itself -- stamped at once by a kernel of its own, that boundary
        // put the host's time to marshal the hash's launch into the scope whenever the GPU had caught up with the host,
        // which a small scene does the more often the faster its kernels are)
        Scope s(c, "native/hash", Scope::kSharedBoundaries, Scope::kCarryStart | Scope::kCarryStop);
        // at least 4 keys per lane (measured: profiles/r01/tune_hash.txt)
        // (two particles per thread until the grid is full: 14.0 against 14.3 us at 1 M with four, 15.2 with one --
        // the kernel is launch and latency there; from 4 M particles on the grid is kHashGridMax either way)
        const int grid = (int)std::min<uint64_t>(kHashGridMax, std::max<uint64_t>(1, n / (2ull * kHashBlock)));
        const uint32_t *n_valid = (c->shard.on && c->shard.active) ? c->shard.counts_now() + kShardTotal : nullptr;
        launch_native_hash(c, kept_sharded, grid, c->pos, c->radius, uniform, N.uniform_r, n, n_valid,
                           c->cell_size, N.gx, N.gy, N.bx0, N.by0, N.blocks_x, N.blocks_y, N.table_entries,
                           late_keys ? nullptr : N.keys,
                           N.codes, N.passes, hist_now, hist_next, c->os_ws.ctl, N.tile_ctl,
                           (uint4 *)N.block_table, gated ? 0ull : pairs,    // gated: the first radix pass resets the table
                           N.host_stat, reuse ? N.sorted_key : nullptr, parity, div_magic,
                           N.exc_count ? N.exc_count + (size_t)parity * N.exc_tiles : nullptr,
                           N.exc_count ? N.exc_entry + (size_t)parity * N.exc_tiles * kExcSlots : nullptr,
                           N.exc_count ? N.exc_count + (size_t)(parity ^ 1u) * N.exc_tiles : nullptr, N.tb,
                           (uint32_t)std::max<uint64_t>(64, n >> 11),       // more stragglers than 0.05 % of the particles: sort
                           fuse_hist ? 1u : 0u, hg, (c->cfg.flags & GPE_FLAG_HASH_INDEX64) != 0);
        GPE_HIP(c, hipGetLastError());
    }
    uint32_t *sk = nullptr, *sv = nullptr;
    {
        // the last radix pass also fills the block table (first / one-past-last position of every block, by
        // atomic min / max at the ends of each tile's key runs); every pass derives its digit bases from hist_now
        Scope s(c, "native/sort", Scope::kSharedBoundaries);
        OnesweepGate g;
        g.need = N.tile_ctl + kCtlNeedSort + parity;
        if (reuse && !fuse_hist) {
            // (the hash kernel counted nothing: see fuse_hist there)
            const int hgrid = (int)std::min<uint64_t>(kHistGatedGridMax, std::max<uint64_t>(1, n / (4ull * kHistGatedBlock)));
            HistKeys hk;
            if (late_keys) {
                hk.pos = c->pos; hk.cell_size = c->cell_size;
                hk.gx = N.gx; hk.gy = N.gy; hk.bx0 = N.bx0; hk.by0 = N.by0; hk.blocks_x = N.blocks_x; hk.blocks_y = N.blocks_y;
            }
            launch_native_hist_gated(c, hgrid, N.keys, n, N.passes, hist_now, g.need, hk);
            GPE_HIP(c, hipGetLastError());
        }
        g.fresh = N.tile_ctl + kCtlFresh + parity;
        g.sorts = N.tile_ctl + kCtlSorts;
        g.sorts_seen = N.tile_ctl + kCtlSortsSeen;
        if (gated) {
            g.key_copy = N.sorted_key; g.table_reset = (uint4 *)N.block_table; g.table_pairs = pairs;
            g.key_blocks_x = (uint32_t)N.blocks_x;
            g.key_div_magic = div_magic;
            g.count_now = hg.owned; g.sorted_count = N.tile_ctl + kCtlSortedCount;
        }
        GPE_TRY(onesweep_sort(c, N.keys, N.ids, N.keys_b, N.ids_b, n, N.passes, true, true, &sk, &sv, true,
                              N.block_table, N.table_entries, hist_now, &g));
    }
    (void)sk;
    N.gsorted_ids_now = nullptr;
    if (kept_sharded && g_bound > 0) {
        // the ghosts' own grouping: (block key, particle index) pairs written by the hash, sorted every step; the last
        // pass fills the ghosts' block table
        Scope s(c, "shard/ghost-sort", Scope::kSharedBoundaries);
        uint32_t *gk = nullptr, *gv = nullptr;
        OnesweepGate gg;                                               // (its own tile tickets; runs when a ghost list ran over,
        gg.ticket_base = 8;                                            //  or always when there are no lists)
        gg.need = hg.ghost_sort;
        GPE_TRY(onesweep_sort(c, N.gkeys, N.gids, N.gkeys_b, N.gids_b, g_bound, N.passes, true, false, &gk, &gv, true,
                              N.gtable, N.table_entries, hg.ghist_now, &gg));
        (void)gk;
        N.gsorted_ids_now = gv;
    }
    N.sort_state_valid = gated;           // (the passes of this call ran, or the kept state was and stays valid)
    N.sorted_n = n;
    N.fresh_word = N.tile_ctl + kCtlFresh + parity;
    N.gho_count_now = hg.gl_count;
    N.gho_entry_now = hg.gl_entry;
    N.ghost_sort_now = hg.ghost_sort;
    N.exc_count_now = reuse ? N.exc_count + (size_t)parity * N.exc_tiles : nullptr;
    N.exc_entry_now = reuse ? N.exc_entry + (size_t)parity * N.exc_tiles * kExcSlots : nullptr;
    *sorted_ids = sv;
    return GPE_OK;
}

// (Re)derive the cell box from the world and the cell size, size the workspaces, and check on the
// device that (a) every particle lies inside the box and (b) no 24x24-cell window holds more particles
// than the smallest LDS cell window stages.  Called from the configuration entry points (set/add
// particles, set world, set max radius, set mode) -- never on the step path; synchronises.
gpe_status native_configure(gpe_ctx *c)
{
    NativeState &N = c->native;
    N.policy.configure(N.host_stat ? native_read_stats(N).sorts : 0u);   // (host_stat: from an earlier configuration)
    N.in_box = false;
    N.uniform = false;                   // (decided below, from the radii as they are now)
    N.sort_state_valid = false;          // particles, box or keys changed: the kept grouping is of something else
    N.always_sort = (c->cfg.flags & GPE_FLAG_SORT_EVERY_STEP) != 0;
    N.reason = GPE_REASON_NO_PARTICLES;
    if (c->n == 0 || !(c->cell_size > 0.0f)) return GPE_OK;
    // largest home coordinate a clamped particle can take: floor(world / cell_size)
    // (K12 clamps to [r, world - r], particle_integration.wgsl:70-71)
    const float fx = floorf(c->cfg.world_width / c->cell_size), fy = floorf(c->cfg.world_height / c->cell_size);
    N.reason = GPE_REASON_GRID_TOO_WIDE;
    if (!(fx >= 0.0f) || !(fy >= 0.0f) || fx > 65000.0f || fy > 65000.0f) return GPE_OK;   // 16-bit cell coords
    N.gx = (int32_t)fx + 1;
    N.gy = (int32_t)fy + 1;
    // The sort key is the particle's 8x8-cell BLOCK, row-major over the box: the tiles look particles up per
    // block and order the members of a cell themselves, so the order inside a block is free.  Against the
    // Morton id of the home cell (what the reference sorts by) that is 6 bits less plus the padding Morton
    // interleaving adds to a non-square box: one radix pass less at 1 M (2 instead of 3) and at 100 M (3 / 4).
    N.bx0 = N.by0 = 0;
    N.blocks_x = (N.gx + 7) >> 3;
    N.blocks_y = (N.gy + 7) >> 3;
    if (c->has_active_box) {
        // sharded: the block box is this rank's active box (own blocks + ghost ring), so the keys stay as short
        // as a single-device run of the same size has them
        const int32_t b0x = std::max(0, c->active_box[0] >> 3), b0y = std::max(0, c->active_box[1] >> 3);
        const int32_t b1x = std::min(N.blocks_x - 1, c->active_box[2] >> 3), b1y = std::min(N.blocks_y - 1, c->active_box[3] >> 3);
        if (b1x >= b0x && b1y >= b0y) {
            N.bx0 = b0x; N.by0 = b0y;
            N.blocks_x = b1x - b0x + 1; N.blocks_y = b1y - b0y + 1;
        }
    }
    N.table_entries = (uint32_t)N.blocks_x * (uint32_t)N.blocks_y;
    int bits = 0;
    // key == table_entries is the padding key of a sharded run (k_native_hash): it needs its bits too
    const uint32_t max_key = c->shard.on ? N.table_entries : N.table_entries - 1;
    while (bits < 32 && (max_key >> bits) != 0) ++bits;
    N.passes = (bits + 7) / 8;
    if (N.passes < 1) N.passes = 1;
    N.reason = GPE_REASON_TABLE_TOO_LARGE;
    if (N.table_entries > (1u << 27)) return GPE_OK;                   // > 1 GiB of table: stay on compat
    // The block table.  payload: the whole 16-byte pairs that cover its entries (the reset writes pairs: `pairs` in
    // native_prepare_step).  slack: what is left of the two spare entries -- read by nobody known, the size it always had.
    const size_t table_payload = (((size_t)N.table_entries + 1) / 2) * sizeof(uint4);
    const size_t table_slack = ((size_t)N.table_entries + 2) * sizeof(uint2) - table_payload;
    // One word per particle.  payload: cap words.  slack: 16 words the radix passes' tile loads may read behind them.
    const size_t particle_words_bytes = c->cap * sizeof(uint32_t), particle_words_slack = 16 * sizeof(uint32_t);
    if (N.table_cap < N.table_entries) {
        N.table_cap = 0;
        GPE_HIP(c, reserve(c, N.block_table, table_payload, table_slack, "native.block_table"));
        N.table_cap = N.table_entries;
    }
    if (N.cap < c->cap) {
        N.cap = 0;
        N.gcap = 0;                                                    // (the ghost buffers follow below)
        const std::pair<uint32_t **, const char *> words[] = {
            {&N.keys, "native.keys"}, {&N.ids, "native.ids"}, {&N.keys_b, "native.keys_b"}, {&N.ids_b, "native.ids_b"},
            {&N.codes, "native.codes"}, {&N.sorted_key, "native.sorted_key"}};
        for (const auto &b : words)
            GPE_HIP(c, reserve(c, *b.first, particle_words_bytes, particle_words_slack, b.second));
        N.cap = c->cap;
    }
    if (c->shard.on && (N.gcap < c->cap || N.gtable_cap < N.table_entries)) {
        // sharded runs: the ghosts' sort buffers and block table
        N.gcap = 0; N.gtable_cap = 0;
        const std::pair<uint32_t **, const char *> words[] = {
            {&N.gkeys, "native.gkeys"}, {&N.gids, "native.gids"}, {&N.gkeys_b, "native.gkeys_b"}, {&N.gids_b, "native.gids_b"}};
        for (const auto &b : words)
            GPE_HIP(c, reserve(c, *b.first, particle_words_bytes, particle_words_slack, b.second));
        N.gcap = c->cap;
        GPE_HIP(c, reserve(c, N.gtable, table_payload, table_slack, "native.gtable"));
        N.gtable_cap = N.table_entries;
        if (!N.ghist) {
            GPE_HIP(c, reserve(c, N.ghist, 2 * (size_t)kHistCopies * 4 * 256 * sizeof(uint32_t), 0, "native.ghist"));
            GPE_HIP(c, hipMemsetAsync(N.ghist, 0, 2 * (size_t)kHistCopies * 4 * 256 * sizeof(uint32_t), c->stream));
        }
    }
    const uint64_t tiles = (uint64_t)((N.gx + kTileMain - 1) / kTileMain) * ((N.gy + kTileMain - 1) / kTileMain);
    {
        // straggler lists: per 32x32 tile of the cell box a count and kExcSlots entries, two sets (step parity)
        // the tile box: the whole cell box, or a sharded rank's active box
        N.tb.x0 = 0; N.tb.y0 = 0; N.tb.nx = (N.gx + 31) / 32; N.tb.ny = (N.gy + 31) / 32;
        if (c->has_active_box) {
            const int32_t cx0 = std::max(0, c->active_box[0]), cy0 = std::max(0, c->active_box[1]);
            const int32_t cx1 = std::min(N.gx - 1, c->active_box[2]), cy1 = std::min(N.gy - 1, c->active_box[3]);
            if (cx1 >= cx0 && cy1 >= cy0) {
                N.tb.x0 = cx0 / 32; N.tb.y0 = cy0 / 32;
                N.tb.nx = cx1 / 32 - N.tb.x0 + 1; N.tb.ny = cy1 / 32 - N.tb.y0 + 1;
            }
        }
        N.exc_tiles = (uint64_t)N.tb.nx * (uint64_t)N.tb.ny;
        if (N.exc_cap < N.exc_tiles) {
            N.exc_entry = nullptr; N.exc_cap = 0;
            GPE_HIP(c, release(c, N.exc_count));
            // (264 B per tile and set: a sparse scene in a huge world -- up to 8 M tiles -- may not get them; the run
            // then sorts every step, native_prepare_step, instead of failing to configure)
            const size_t bytes = 2 * N.exc_tiles * sizeof(uint32_t) + 16 + 2 * N.exc_tiles * kExcSlots * sizeof(uint2);
            // payload: the counts of both sets, rounded up to the entries' 8-byte alignment, and the entries.  slack: what
            // the 16 bytes of alignment allowance leave over (8 or 12 bytes), read by nobody
            const size_t payload = ((2 * N.exc_tiles + 1) & ~1ull) * sizeof(uint32_t) + 2 * N.exc_tiles * kExcSlots * sizeof(uint2);
            if (reserve(c, N.exc_count, payload, bytes - payload, "native.exc") == hipSuccess) N.exc_cap = N.exc_tiles;
        }
        if (N.exc_count) {
            // (entries behind the counts of both sets, 8-byte aligned)
            N.exc_entry = (uint2 *)(N.exc_count + ((2 * N.exc_tiles + 1) & ~1ull));
            GPE_HIP(c, hipMemsetAsync(N.exc_count, 0, 2 * N.exc_tiles * sizeof(uint32_t), c->stream));
        }
    }
    // Rosters scale with the world's tile count, not with n (6160 B per tile): at the benchmark density that is 16 B per
    // particle; a sparse scene in a large world would pay gigabytes for lists of a few ids each.  Beyond 16 roster
    // slots per particle (4 x the benchmark's ratio) the run does without them.
    const bool rosters_pay = N.exc_tiles * (uint64_t)kRosterCap <= 16ull * std::max<uint64_t>(c->n, 1u << 16);
    if (!rosters_pay && N.roster_hdr) {
        N.roster_cap = 0;
        GPE_HIP(c, release(c, N.roster_hdr));
        GPE_HIP(c, release(c, N.roster_ids));
    }
    if (c->shard.on && c->has_active_box && N.gho_cap < N.exc_tiles) {
        // ghost lists (sharded runs): a count and kGhostSlots ids per tile, two sets.  Optional: without them the ghosts
        // are sorted into their block table every step
        N.gho_cap = 0;
        GPE_HIP(c, release(c, N.gho_count));
        // payload: counts and ids of both sets.  slack: 64 bytes read by nobody known (the size it always had)
        if (reserve(c, N.gho_count, 2 * N.exc_tiles * (1 + (size_t)kGhostSlots) * sizeof(uint32_t), 64, "native.gho") == hipSuccess)
            N.gho_cap = N.exc_tiles;
    }
    if (N.gho_count) GPE_HIP(c, hipMemsetAsync(N.gho_count, 0, 2 * N.exc_tiles * sizeof(uint32_t), c->stream));
    if (rosters_pay && N.exc_count &&
        (c->cfg.flags & (GPE_FLAG_SORT_EVERY_STEP | GPE_FLAG_COUNTING_SORT_TILES)) == 0) {
        // tile rosters (CollideArgs): 16 + 4 kRosterCap bytes per 32x32 tile.  Optional: a device that has no room for
        // them runs without (every step then looks its blocks up)
        if (N.roster_cap < N.exc_tiles) {
            N.roster_cap = 0;
            GPE_HIP(c, release(c, N.roster_hdr));
            GPE_HIP(c, release(c, N.roster_ids));
            if (reserve(c, N.roster_hdr, N.exc_tiles * sizeof(uint4), 0, "native.roster_hdr") == hipSuccess &&
                reserve(c, N.roster_ids, N.exc_tiles * (size_t)kRosterCap * sizeof(uint32_t), 0, "native.roster_ids") == hipSuccess)
                N.roster_cap = N.exc_tiles;
            else { (void)release(c, N.roster_hdr); (void)release(c, N.roster_ids); }
        }
        // (stamp 0 is never current: the tiles compare with sorts + 1)
        if (N.roster_hdr) GPE_HIP(c, hipMemsetAsync(N.roster_hdr, 0, N.exc_tiles * sizeof(uint4), c->stream));
    }
    if (N.overflow_cap < tiles) {
        N.overflow_cap = 0;
        // payload: all of it -- the lists are laid out over the whole allocation; no slack
        GPE_HIP(c, reserve(c, N.overflow1, (3 * tiles + 32 + 2 * kHintMax) * sizeof(uint32_t), 0, "native.overflow"));   // (the tiles, then their halves: CollideArgs::overflow2, then the hints)
        N.overflow_cap = tiles;
    }
    {
        // spill arena: every particle can be staged by the 9 windows around it, but a scene that dense has
        // left the native path long before (native_should_run); one slot per particle, 1 M .. 32 M slots
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(c->cap, 1ull << 20), 32ull << 20);
        GPE_TRY(arena_reserve(c, std::max<uint64_t>(want, N.arena_cap)));
    }
    if (!N.tile_ctl) {
        GPE_HIP(c, reserve(c, N.tile_ctl, kCtlWords * sizeof(uint32_t), 0, "native.tile_ctl"));
        GPE_HIP(c, hipMemsetAsync(N.tile_ctl, 0, kCtlWords * sizeof(uint32_t), c->stream));
    }
    if (!N.host_stat) GPE_HIP(c, hipHostMalloc((void **)&N.host_stat, 64, hipHostMallocDefault));
    memset(N.host_stat, 0, 64);
    GPE_TRY(onesweep_reserve(c, c->cap));
    GPE_HIP(c, hipMemsetAsync(N.tile_ctl, 0, kCtlSorts * sizeof(uint32_t), c->stream));
    // One radius for all?  The same pass over the particles answers it.  Not asked where the general kernels stay anyway:
    // sharded contexts (ghosts arrive with radii of their own; order-key tiles), GPE_FLAG_GENERAL_RADII.
    const bool ask_radii = !c->shard.on && !c->use_order_keys && !c->has_active_box && (c->cfg.flags & GPE_FLAG_GENERAL_RADII) == 0;
    GPE_HIP(c, hipMemsetAsync(N.tile_ctl + kCtlRadiusBits, 0, 2 * sizeof(uint32_t), c->stream));
    launch_native_check_box(c, c->pos, c->n,
                            (c->shard.on && c->shard.active) ? c->shard.counts_now() + kShardTotal : nullptr, c->cell_size, N.gx, N.gy,
                            N.tile_ctl + kCtlError, ask_radii ? c->radius : nullptr, N.tile_ctl + kCtlRadiusBits);
    GPE_HIP(c, hipGetLastError());
    uint32_t flag = 1;
    uint32_t radius_bits[2] = {0u, 0u};
    GPE_HIP(c, hipMemcpyAsync(&flag, N.tile_ctl + kCtlError, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipMemcpyAsync(radius_bits, N.tile_ctl + kCtlRadiusBits, sizeof(radius_bits), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    if (ask_radii && ~radius_bits[0] == radius_bits[1]) {
        // (plain_radius_lanes' range, k_pair.h: positive, finite, 1 / r finite -- the radii for which equal radii make
        // both weights of a pair exactly 0.5)
        float r;
        memcpy(&r, &radius_bits[1], sizeof(r));
        if (r >= 1e-30f && r <= 1e30f) { N.uniform = true; N.uniform_r = r; }
    }
    GPE_HIP(c, hipMemsetAsync(N.tile_ctl, 0, kCtlSorts * sizeof(uint32_t), c->stream));         // the check's verdict is not a step error
    N.reason = GPE_REASON_OUT_OF_BOX;
    if (flag != 0) return GPE_OK;                                      // a particle outside the box: compat kernels
    N.in_box = true;
    // window population of the current state
    const bool prof = c->profiling;
    c->profiling = false;
    uint32_t *ids = nullptr;
    gpe_status st = native_prepare_step(c, &ids, true);
    c->profiling = prof;
    GPE_TRY(st);
    launch_native_window_max(c, N.block_table, N.table_entries, N.blocks_x, N.blocks_y, N.tile_ctl + kCtlWindowMax);
    GPE_HIP(c, hipGetLastError());
    uint32_t wmax = 0xffffffffu;
    GPE_HIP(c, hipMemcpyAsync(&wmax, N.tile_ctl + kCtlWindowMax, sizeof(wmax), hipMemcpyDeviceToHost, c->stream));
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    GPE_HIP(c, hipMemsetAsync(N.tile_ctl, 0, kCtlSorts * sizeof(uint32_t), c->stream));
    N.window_max = wmax;
    // gpe_config.flags: keep over-dense scenes on the native kernels (their windows then go through the spill arena);
    // print the step statistics every 128 steps; sort every step
    N.force = (c->cfg.flags & GPE_FLAG_NATIVE_FORCE) != 0;
    N.print_stats = (c->cfg.flags & GPE_FLAG_NATIVE_STATS) != 0;
    N.reason = N.policy.admit(wmax, N.force) ? GPE_REASON_NONE : GPE_REASON_DENSE_WINDOWS;
    return GPE_OK;
}

// The spill arena: every particle of a dense region can be staged by the 9 windows around it.  One slot per
// particle to start with (1 M .. 32 M slots); native_should_run doubles it when a step used more than half.
static gpe_status arena_reserve(gpe_ctx *c, uint64_t want)
{
    NativeState &N = c->native;
    if (N.arena_cap >= want) return GPE_OK;
    // the new arena first: on failure the old one stays in place (a run that must stay on the native kernels keeps
    // working with it) and the error is the caller's to report
    void *fresh = nullptr;
    // payload: the slots.  slack: 256 bytes the 16-byte loads of the last slots' arrays may read behind them
    const hipError_t e = reserve(c, fresh, want * kArenaBytesPerSlot, 256, "native.arena");
    if (e == hipErrorOutOfMemory) return fail(c, GPE_ERR_OOM, "native collide: out of device memory for the spill arena");
    if (e != hipSuccess) return fail(c, GPE_ERR_HIP, std::string("hipMalloc (spill arena): ") + hipGetErrorName(e));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (kernels in flight may still use the old one)
    const hipError_t freed = release(c, N.arena);                         // (reported below: the new arena is in place either way)
    N.arena = fresh;
    N.arena_cap = want;
    GPE_HIP(c, freed);
    return GPE_OK;
}

// While a dense scene is held on the compat kernels: measure the window population of the current state WITHOUT a
// host synchronisation -- hash + sort + window maximum are enqueued, the answer lands in pinned memory and is read
// by a later call.  (Round 1 re-ran native_configure here: two stream synchronisations and possibly a reallocation
// inside gpe_run every 256 steps.)
static gpe_status native_probe_async(gpe_ctx *c)
{
    NativeState &N = c->native;
    const bool prof = c->profiling;
    c->profiling = false;
    uint32_t *ids = nullptr;
    const gpe_status st = native_prepare_step(c, &ids, true);
    c->profiling = prof;
    GPE_TRY(st);
    launch_native_window_max(c, N.block_table, N.table_entries, N.blocks_x, N.blocks_y, N.tile_ctl + kCtlWindowMax);
    launch_native_publish_probe(c, N.tile_ctl, N.host_stat);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

// Should this step take the native kernels?  The tiles report the step's largest 24x24-cell window population and
// the spill-arena slots they used to pinned host memory (asynchronously, so the values lag by the steps still in
// flight; gpe_run bounds that).  Windows above the handover population (one-lane O(n^2) cells that overlapping
// windows would repeat) send the context to the compat kernels -- unless the run needs the native ones (order keys
// of a sharded run: there the dense windows keep going through the spill arena).  A held context probes the state
// every 256 steps without synchronising and returns when the windows have thinned out.  Nothing here frees or
// allocates on ordinary steps; the arena grows (one synchronisation) when a step has used more than half of it.
bool native_should_run(gpe_ctx *c)
{
    NativeState &N = c->native;
    if (c->cfg.mode != GPE_MODE_NATIVE || !N.host_stat) return false;   // (no host_stat: never configured this far)
    const bool must_stay = N.force || c->use_order_keys;
    const NativeStats s = native_read_stats(N);
    native_print_stats(c, s);
    // (a failed growth leaves the old arena in place and the step goes on with it when it must stay: a window it cannot
    // hold raises kErrTileOverflow, which gpe_sync reports -- never a silent hand-over of a run that must stay native)
    const RunPlan p = N.policy.run(s, must_stay, N.in_box, N.arena_cap,
                                   [&](uint64_t slots) { return arena_reserve(c, slots) == GPE_OK; });
    // (the host's side of the handshake: it resets the words the plan has consumed)
    if (p.arena_reset) __atomic_store_n(&N.host_stat[kStatArena], 0u, __ATOMIC_RELAXED);
    if (p.readmitted || p.resume) N.reason = GPE_REASON_NONE;
    if (p.hand_over) N.reason = GPE_REASON_DENSE_WINDOWS;
    if (p.resume) __atomic_store_n(&N.host_stat[kStatWindowMax], s.probe - 1u, __ATOMIC_RELAXED);
    if (p.hand_over || p.resume || p.probe) __atomic_store_n(&N.host_stat[kStatProbe], 0u, __ATOMIC_RELAXED);
    if (p.probe) (void)native_probe_async(c);
    return p.run;
}

// Hinted tiles (kCtlHints): the dense launch's first workgroups redo them as halves.  With rosters only (the hint travels
// in the roster header the tile loads anyway), and only while tiles have run over lately (lagged statistic, hinted tiles
// included): the kernel that carries the front workgroups is 3 % slower than the plain one.  Until it is launched a
// registered tile simply tries itself again.  (Up to 8 M particles, and while the front workgroups can take at least half
// of the tiles that run over: the 3 % are 1.5 us of the 1 M launch, against ~20 us of half-tile launch behind it, but
// 0.1 ms at 100 M.)
static void native_hint_policy(gpe_ctx *c, const NativeStats &s, CollideArgs *A)
{
    const HintPlan h = c->native.policy.hints(s, A->roster_hdr != nullptr, (c->cfg.flags & GPE_FLAG_NO_HALF_TILES) != 0, c->n);
    A->hints_on = h.hints_on ? 1u : 0u;
    A->front_wgs = h.front_wgs;
}

// pos_in (step-start positions) -> pos_out (after the four colour passes), every particle written.
gpe_status native_collide(gpe_ctx *c, const float2 *pos_in, float2 *pos_out, const VerletParams *verlet)
{
    NativeState &N = c->native;
    uint32_t *sorted_ids = nullptr;
    // Everything this function enqueues says so (note_enqueue: here, the launchers of k_native.hip, onesweep_sort), so
    // its scopes share the events at their common boundaries: 7 records on a sampled kept-table step instead of 12.
    ScopeRegion region(c);
    GPE_TRY(native_prepare_step(c, &sorted_ids));
    CollideArgs A;
    A.pos_in = pos_in;
    A.radius = c->radius;
    A.uniform = (N.uniform && !c->shard.on && !c->use_order_keys && !c->has_active_box) ? 1u : 0u;
    A.uniform_r = N.uniform_r;
    A.pos_out = pos_out;
    A.sorted_ids = sorted_ids;
    A.codes = N.codes;
    A.fresh = N.fresh_word;
    A.gtable = N.gsorted_ids_now ? N.gtable : nullptr;
    A.gsorted_ids = N.gsorted_ids_now;
    A.exc_count = N.exc_count_now;
    A.exc_entry = N.exc_entry_now;
    A.tb = N.tb;
    A.gho_count = N.gsorted_ids_now ? N.gho_count_now : nullptr;     // (kept sharded run with ghosts this step)
    A.gho_entry = N.gho_entry_now;
    A.ghost_sort = N.ghost_sort_now;
    A.roster_hdr = (N.roster_cap >= N.exc_tiles) ? N.roster_hdr : nullptr;
    A.roster_ids = N.roster_ids;
    A.sorts_seen = N.tile_ctl + kCtlSortsSeen;
    A.roster_write = N.exc_count_now != nullptr ? 1u : 0u;            // (this step could do without a sort: the table is kept)
    A.table = N.block_table;
    A.entries = N.table_entries;
    A.blocks_x = N.blocks_x;
    A.blocks_y = N.blocks_y;
    A.bx0 = N.bx0;
    A.by0 = N.by0;
    A.counts = (c->shard.on && c->shard.active) ? c->shard.counts_now() + kShardOwned : nullptr;
    A.cell_size = c->cell_size;
    A.stiffness = c->cfg.stiffness;
    A.gx = N.gx;
    A.gy = N.gy;
    A.tile_ctl = N.tile_ctl;
    A.overflow1 = N.overflow1;
    A.overflow1_cap = (uint32_t)N.overflow_cap;
    A.overflow2 = N.overflow1 + N.overflow_cap + 16;
    A.quarters_of_halves = 0u;
    A.hints = N.overflow1 + 3 * N.overflow_cap + 32;                   // 2 x kHintMax words behind the two lists
    A.hint_parity = N.collide_seq & 1u;
    A.step_stamp = N.collide_seq + 16u;                                // (never the 0 of a cleared roster header)
    ++N.collide_seq;
    A.front_wgs = 0u;
    A.hints_on = 0u;
    {
        // arena layout: px | py | rad | id | hm | mem (4 per slot) | sblk
        float *f = (float *)N.arena;
        const uint64_t m = N.arena_cap;
        A.arena_px = f; A.arena_py = f + m; A.arena_rad = f + 2 * m;
        A.arena_id = (uint32_t *)(f + 3 * m); A.arena_hm = (uint32_t *)(f + 4 * m);
        A.arena_mem = (uint32_t *)(f + 5 * m);
        A.arena_sblk = (uint8_t *)(f + 9 * m);
        A.arena_cap = (uint32_t)m;
    }
    A.order_keys = c->use_order_keys ? c->order_keys : nullptr;
    A.tile_x0 = A.tile_y0 = 0;
    A.prev = c->prev;
    A.n_owned = c->n_owned;
    A.fuse_verlet = verlet ? 1u : 0u;
    if (verlet) A.vp = *verlet; else memset(&A.vp, 0, sizeof(A.vp));
    A.stamps = nullptr;
    A.frame_l = A.frame_r = A.frame_b = A.frame_t = 0;
    A.pack = PackArgs();
    if (c->shard.on && c->shard.active && c->shard.have_rect && verlet && A.order_keys) shard_pack_args(c, &A.pack);
#ifdef GPE_TILE_STAMPS
    note_enqueue(c);                                                   // (it may copy and clear the stamps)
    A.stamps = native_tile_stamps(c);
#endif
    int32_t cx0 = 0, cy0 = 0, cx1 = N.gx - 1, cy1 = N.gy - 1;
    if (c->has_active_box) {                                           // sharded: only this rank's cells
        cx0 = std::max(cx0, c->active_box[0]); cy0 = std::max(cy0, c->active_box[1]);
        cx1 = std::min(cx1, c->active_box[2]); cy1 = std::min(cy1, c->active_box[3]);
        if (cx1 < cx0 || cy1 < cy0) { cx1 = cx0; cy1 = cy0; }
    }
    A.tile_x0 = cx0 / kTileMain;
    A.tile_y0 = cy0 / kTileMain;
    A.tiles_x = cx1 / kTileMain - A.tile_x0 + 1;
    A.tiles_y = cy1 / kTileMain - A.tile_y0 + 1;
    const uint32_t total = (uint32_t)A.tiles_x * (uint32_t)A.tiles_y;
    const NativeStats stats = native_read_stats(N);                   // (this call's decisions all read this one)
    bool direct_form = false;                                          // the dense launch runs direct-slot tiles
    {
        Scope s(c, verlet ? "native/collide+verlet" : "native/collide", Scope::kSharedBoundaries);
        A.band_tiles = dense_launch_band((uint32_t)A.tiles_x, (uint32_t)A.tiles_y, (c->cfg.flags & GPE_FLAG_XCD_EIGHTHS) != 0);
        const uint32_t grid = dense_launch_grid((uint32_t)A.tiles_x, (uint32_t)A.tiles_y, A.band_tiles);
        // Which form of the tile?  The direct-slot form is the faster one while tiles fit it; it holds 928 particles and
        // hands a tile on when its cells crowd (more than 96 memberships beyond a cell's sixth, a cell of more than 64).
        // In a compressed scene (the 100 M cloud after a few hundred steps of gravity) most tiles would take that
        // detour through the over-capacity launch, while the counting-sort form holds 1192 particles and resolves
        // crowded cells in place.  So the choice follows the tiles' own report (lagged by the steps in flight; either
        // form is exact): counting-sort tiles once more than 2 % of the direct-slot tiles ran over; back to direct
        // slots when no 24x24-cell window has held more than 512 particles (2.3 x the mean of the benchmark density; a
        // direct-slot window overflows around 350) and no tile has run over for 64 steps.
        // (order-key windows carry four more bytes per particle: in the direct form that leaves 728 slots, 1.27 x the
        // mean tile's particles, and too many tiles run over; the counting-sort form holds 1024)
        // (order-key windows: the direct form needs the ghost lists of a kept sharded run; every other sharded set-up
        // looks its ghosts up in the block tables, which only the counting-sort form does)
        const bool legacy = N.policy.counting_sort(stats, total, (c->cfg.flags & GPE_FLAG_COUNTING_SORT_TILES) != 0,
                                                   A.order_keys != nullptr && A.gho_count == nullptr);
        direct_form = !legacy;
        if (legacy) {
            if (A.order_keys)
                launch_collide(c, CollideForm::DenseOrd, grid, A);
            else
                launch_collide(c, CollideForm::Dense, grid, A);
        } else if (A.order_keys) {
            // A sharded step whose tiles pack (A.pack.on) and whose exchange runs beside it (ShardState::overlap): the frame
            // of the tile grid first -- the tiles whose particles can come to lie outside the pack's safe box: their cells
            // reach within a block and a cell (the most a particle may move per step, + the box's margin) of it -- then
            // the event the exchange waits for, then the interior tiles, which must not have anything to pack.
            ShardState &SH = c->shard;
            bool split = false;
            if (A.pack.on == 1u && SH.overlap && SH.ev_packed) {
                const int reach = 8 + 1 + 8 + 1;                       // cells: from a tile's edge to the safe box's edge
                const int rx0 = SH.rect[0] * 8, ry0 = SH.rect[1] * 8, rx1 = SH.rect[2] * 8, ry1 = SH.rect[3] * 8;
                const bool nb_l = SH.rect[0] > 0, nb_r = SH.rect[2] < SH.blocks_x, nb_d = SH.rect[1] > 0, nb_u = SH.rect[3] < SH.blocks_y;
                int fl = 0, fr = 0, fb = 0, ft = 0;
                for (int t = 0; t < A.tiles_x; ++t) {
                    const int c0 = (A.tile_x0 + t) * kTileMain, c1 = c0 + kTileMain - 1;
                    if (nb_l && c0 < rx0 + reach) fl = t + 1;
                    if (nb_r && c1 >= rx1 - reach && fr == 0) fr = A.tiles_x - t;
                }
                for (int t = 0; t < A.tiles_y; ++t) {
                    const int c0 = (A.tile_y0 + t) * kTileMain, c1 = c0 + kTileMain - 1;
                    if (nb_d && c0 < ry0 + reach) fb = t + 1;
                    if (nb_u && c1 >= ry1 - reach && ft == 0) ft = A.tiles_y - t;
                }
                if (fl + fr < A.tiles_x && fb + ft < A.tiles_y) {
                    split = true;
                    A.frame_l = fl; A.frame_r = fr; A.frame_b = fb; A.frame_t = ft;
                    const uint32_t frame = (uint32_t)((fb + ft) * A.tiles_x + (A.tiles_y - fb - ft) * (fl + fr));
                    if (frame) {
                        launch_collide(c, CollideForm::BorderOrd, frame, A);
                        GPE_HIP(c, hipGetLastError());
                    }
                    note_enqueue(c);
                    GPE_HIP(c, hipEventRecord(SH.ev_packed, c->stream));
                    SH.packed_recorded = true;
                    // the interior: a tile box of its own (bands as above), nothing to pack
                    A.tile_x0 += fl; A.tile_y0 += fb; A.tiles_x -= fl + fr; A.tiles_y -= fb + ft;
                    A.pack.on = 2u;
                    A.band_tiles = dense_launch_band((uint32_t)A.tiles_x, (uint32_t)A.tiles_y, (c->cfg.flags & GPE_FLAG_XCD_EIGHTHS) != 0);
                    const uint32_t igrid = dense_launch_grid((uint32_t)A.tiles_x, (uint32_t)A.tiles_y, A.band_tiles);
                    launch_collide(c, CollideForm::DirectOrd, igrid, A);
                }
            }
            if (!split) {
                native_hint_policy(c, stats, &A);
                if (A.front_wgs)
                    launch_collide(c, CollideForm::DirectOrdFront, grid + A.front_wgs, A);
                else
                    launch_collide(c, CollideForm::DirectOrd, grid, A);
            }
        } else {
            native_hint_policy(c, stats, &A);
            if (A.front_wgs)
                launch_collide(c, CollideForm::DirectFront, grid + A.front_wgs, A);
            else
                launch_collide(c, CollideForm::Direct, grid, A);
        }
        GPE_HIP(c, hipGetLastError());
    }
    {
        // tiles whose window exceeded the LDS capacity: 16x16 tiles, 8x8 tiles, spill arena.  (Measured and dropped:
        // running this launch on a second stream beside the dense one -- the stream fork/join costs ~8 us per step,
        // more than the normally empty launch it hides; it only pays in clustered scenes.)
        // The launch takes its work items from a ticket counter, so ANY grid is correct; an empty launch of 1024
        // workgroups (8 waves and 36 KB of LDS each) costs ~6 us, 8 % of the 1 M step.  While the tiles have reported no
        // over-capacity tile for a while (the statistic lags by the steps in flight) the grid is 128 workgroups; the
        // first reported tile brings the full grid back.  A surprise only makes that one step's launch slower.
        // A context whose windows were thin when it was configured (at most kWindowQuietStart: NativePolicy::admit) starts
        // that way -- small grid, no half-tile launch -- instead of paying both for its first 96 and 32 steps, and after
        // every gpe_add_particles / gpe_set_particles again; one that was dense then starts with both.
        Scope s(c, "native/collide-dense-regions", Scope::kSharedBoundaries);
        // (quiet_steps: since the dense launch last handed a tile on ITSELF -- hinted tiles do not count, they never reach
        // list 1; dense_quiet: since anything reached list 1 or list 2)
        // The half-tile launch: while the direct-slot launch has handed tiles on lately (lagged; either way is exact --
        // without it the over-capacity launch takes the tiles of list 1).  Not behind counting-sort tiles: what does not
        // fit their 1192 particles is dense enough for the windows.
        // (A scene in which more than 2 % of the tiles run over has its dense launch on counting-sort tiles by then --
        // `crowded` above: this launch is for the few tiles of a clumped cloud, not for piles; keeping the direct-slot form
        // with halves behind it up to 50 % of the tiles was measured: step 2000 of the 100 M soak 35.5 instead of 31.0 ms.)
        // (With front workgroups in the dense launch list 1 only holds tiles that ran over for the FIRST time -- one every
        // ~60 steps in the clumped 1 M cloud, which no lagged statistic foresees: the over-capacity launch takes those as
        // quarters, and the half-tile launch comes back when list 1 stays occupied, i.e. the hints are full.)
        // (The small over-capacity grid only where the empty launch matters: from a few million particles on its 6 us are
        // noise, and a surprise -- the statistic lags by up to 64 steps -- would cost those steps milliseconds each; with
        // front workgroups also while the lists have held few work items lately, a first-time tile being four.)
        const OverflowPlan op = N.policy.overflow(stats, A.front_wgs, direct_form, (c->cfg.flags & GPE_FLAG_NO_HALF_TILES) != 0, c->n);
        if (op.halves_grid) {
            A.quarters_of_halves = 1u;
            if (A.order_keys)
                launch_collide(c, CollideForm::HalvesOrd, op.halves_grid, A);
            else
                launch_collide(c, CollideForm::Halves, op.halves_grid, A);
            GPE_HIP(c, hipGetLastError());
        }
        const uint32_t ogrid = op.overflow_grid;
#ifdef GPE_TILE_STAMPS
        A.stamps += 64;
#endif
        if (A.order_keys)
            launch_collide(c, CollideForm::OverflowOrd, ogrid, A);
        else
            launch_collide(c, CollideForm::Overflow, ogrid, A);
        GPE_HIP(c, hipGetLastError());
    }
    // (a sharded step that did not split its tiles: everything has packed now)
    if (A.pack.on == 1u && c->shard.overlap && c->shard.ev_packed) {
        note_enqueue(c);
        GPE_HIP(c, hipEventRecord(c->shard.ev_packed, c->stream));
        c->shard.packed_recorded = true;
    }
    return GPE_OK;
}

}  // namespace gpe
