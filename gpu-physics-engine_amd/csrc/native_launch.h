// native_launch.h -- the seam between the two sides of the native step: the kernels and their launchers (k_native.hip)
// and the host side that sizes the buffers, reads the statistics and decides what to launch (gpe_native.hip).  What the
// host fills and the kernels read, the constants both sides size things by, and one launcher per family of launch sites;
// no kernel is declared here.
#pragma once

#include "gpe_internal.h"

namespace gpe {

// tile_ctl words (the first four are cleared every step, the error word is sticky)
constexpr int kCtlOverflow1 = 0;               // 32x32 tiles over capacity this step
constexpr int kCtlOverflow2 = 1;               // 32x16 halves of those the half-tile launch could not take either
constexpr int kCtlHalfTicket = 7;              // next work item of the half-tile launch
constexpr int kCtlWindowMax = 2;               // largest 24x24-cell window population seen this step
constexpr int kCtlArena = 3;                   // particles handed out of the global spill arena this step
constexpr int kCtlOverflowTicket = 4;          // next work item of the over-capacity launch
constexpr int kCtlSubTiles = 5;                // 16x16 quarters redone as four 8x8 tiles this step
constexpr int kCtlSpills = 6;                  // 8x8 tiles staged in the global spill arena this step
constexpr int kCtlPerStepWords = 8;            // words [0, 8) are cleared every step
// HINTS: a tile the direct-slot dense launch hands on is, as a rule, over capacity on the next step too (a clump lives for
// hundreds of steps).  It registers itself for the next collide launch -- hints[next parity][k], k from tile_ctl[kCtlHints
// + next parity], and that launch's number in the fourth word of its roster header -- and there the FIRST kHintMax * 2
// workgroups of the dense launch redo it as two 32x16 halves while the others resolve their tiles: nothing waits behind
// the dense launch for it (the half-tile launch there cost the 1 M step ~20 us from step ~1000 of the benchmark run on).
// The tile's own workgroup sees the number in the header it loads anyway and returns; the half workgroup registers the
// tile again, kHintAge launches long -- then the tile tries itself once (it may fit again) and, if it still runs over, is
// registered afresh by the launch that takes it off list 1.  Launches are
// numbered by native_collide itself (not by step: a host may collide twice on one grid); the list a launch has used is
// cleared behind it by its over-capacity launch.  Exact whatever the lists hold: a tile is skipped by its own workgroup
// iff its header carries this launch's number or the next one's (registered again already, by a front workgroup -- or by
// itself, which is past the test), and a front workgroup takes a listed tile iff the header carries one of the two.
constexpr int kCtlHints = 11;                  // [launch parity] tiles registered for the launch of that parity
constexpr int kCtlHintsSeen = 13;              // hinted tiles of the last launch (statistics)
// (kHintMax, the tiles a launch may register: native_policy.h, whose hint policy sizes the front workgroups by it)
constexpr int kCtlError = 8;                   // sticky
// Two words each, indexed by the parity of the step (native_prepare_step counts them): a step's hash kernel clears
// the NEXT step's word while its own is being set, so no workgroup of a launch races with another's reset.
// (The words the tiles only READ -- fresh, sorted count -- live in a 128-byte line of their own, the L2's granule: the
// first line holds the words every tile and every work item of the over-capacity launch hammers with atomics (overflow
// count, work ticket, window maximum, arena), and a load from a line under atomic fire queues behind them: with
// `fresh` next to the ticket P0 of a tile took 11.5 k instead of 5.9 k cycles and the over-capacity launch 6.3 instead
// of 4.1 ms at step 1000 of the 100 M soak.)
constexpr int kCtlNeedSort = 34;               // [parity] the hash found a particle outside the drift its code can express
constexpr int kCtlFresh = 36;                  // [parity] the radix passes ran: the block table describes THIS step's positions
constexpr int kCtlSorts = kNativeCtlSorts;     // steps whose radix passes ran (running count, gpe_get_pipeline_info)
constexpr int kCtlStragglers0 = 9, kCtlStragglers1 = 15;   // [parity] stragglers found by the step's hash so far
constexpr int kCtlSortedCount = 32;            // particles the kept grouping covers (written by the first radix pass)
constexpr int kCtlSortsSeen = kNativeCtlSortsSeen;   // copy of kCtlSorts in the line the tiles only read (written by the last radix pass)
constexpr int kCtlRadiusBits = 42;             // [2] configuration time only: ~(smallest), largest bit pattern of the radii (k_native_check_box)
constexpr int kCtlGhostSort = 40;              // [parity] sharded: a tile's ghost list ran over -- the ghosts' radix passes run and the tiles look the ghosts up in their block table
constexpr int kCtlWords = 64;                  // tile_ctl is this long (two 128-byte lines)
// A particle beyond that reach (a straggler: in a cloud without damping a few particles are always fast) does not
// force a sort by itself: the hash kernel hands it, with its cell, to every 32x32 tile whose cell window holds it
// (at most four), kExcSlots per tile, and marks its code so that the tiles skip it in the old block's list.  Only a
// tile's list running over raises kCtlNeedSort.  Two sets of lists, by step parity (reset like the control words).
constexpr uint32_t kExcSlots = 16;
// Sharded runs: the ghosts (copies of the neighbours' particles, new every step) reach the tiles the same way -- the hash
// kernel lists every ghost for the 32x32 tiles whose window holds its cell, kGhostSlots per tile (a tile on the rank's
// border sees ~60-150 at the benchmark density).  Only when a list runs over do the ghosts get sorted into a block
// table of their own (rounds 1-3 did that every step: two radix launches).
constexpr uint32_t kGhostSlots = 256;
constexpr uint64_t kArenaBytesPerSlot = 37;     // px, py, rad, id, hm (4 B each), 4 member entries (16 B), block (1 B)
                                                // (at most kArenaMaxSlots: native_policy.h)
constexpr int kTileMain = 32;                  // cells: the tiles of the dense launch
// Sharded runs with the counts on the device (k_shard.hip): the first *owned particles are the rank's own and take
// part in the kept grouping; the ghosts behind them change every step, so they are grouped by a small sort of their
// own every step (gkeys / gids, g_bound pairs, the ghost block table).  All NULL / 0 otherwise.
struct HashGhosts {
    const uint32_t *owned = nullptr;
    uint32_t *gkeys = nullptr, *gids = nullptr;
    uint64_t g_bound = 0;
    uint4 *gtable2 = nullptr;
    uint64_t gtable_pairs = 0;
    const uint32_t *sorted_count = nullptr;    // tile_ctl[kCtlSortedCount]
    uint32_t *ghist_now = nullptr, *ghist_next = nullptr;   // the ghost sort's digit histograms (kHistCopies copies, two sets)
    // ghost lists (kGhostSlots ids per tile of the tile box): this step's, and the next step's counts to reset
    uint32_t *gl_count = nullptr, *gl_entry = nullptr, *gl_count_next = nullptr;
    uint32_t *ghost_sort = nullptr, *ghost_sort_next = nullptr;   // tile_ctl[kCtlGhostSort + parity], ... of the next step
};
// What the gated histogram launch needs to form the keys itself (block_key_of) on a step whose hash stored none; pos ==
// NULL: the hash stored them.  One kernel argument: the launch sits between the hash and the radix passes of every step,
// and on a small scene the host's time to marshal it is on the step's critical path.
struct HistKeys {
    const float2 *pos = nullptr;
    float cell_size = 0.0f;
    int32_t gx = 0, gy = 0, bx0 = 0, by0 = 0, blocks_x = 0, blocks_y = 0;
};
constexpr int kHashBlock = 1024;
constexpr int kHashGridMax = 2048;
constexpr int kHistGatedBlock = 1024, kHistGatedGridMax = 2048;
#ifndef GPE_QMAX_MAIN_VALUE
#define GPE_QMAX_MAIN_VALUE 3                  // looked-up particles per thread of a 32x32 tile's workgroup
#endif
struct CollideArgs {
    const float2 *pos_in;
    const float *radius;
    // every particle has the radius uniform_r (NativeState::uniform): the direct-slot launches and the half-tile launch run
    // their windows without a radius array; the other forms read `radius` as ever
    uint32_t uniform;
    float uniform_r;
    float2 *pos_out;
    const uint32_t *sorted_ids;
    const uint32_t *codes;       // per particle: cell mod 128 (7 + 7 bits) | neighbour overlap mask (8 bits) | kCodeStraggler
    const uint2 *gtable;         // sharded runs: (start, end) of every block among the GHOSTS, sorted every step (else NULL)
    const uint32_t *gsorted_ids; // ... and their particle indices in that order
    const uint32_t *exc_count;   // stragglers handed to each 32x32 tile this step (NULL: none, the run always sorts)
    const uint2 *exc_entry;      // kExcSlots x (particle, cell x | y << 16) per tile
    TileBox tb;                  // the tiles those lists, the ghost lists and the rosters are kept for
    const uint32_t *gho_count;   // sharded runs: ghosts listed for each tile this step (NULL: none / not sharded)
    const uint32_t *gho_entry;   // kGhostSlots x particle index per tile
    const uint32_t *ghost_sort;  // tile_ctl[kCtlGhostSort + parity]: != 0 when a ghost list ran over this step -- the
                                 // ghosts are then looked up in their block table (gtable) instead
    const uint32_t *fresh;       // tile_ctl[kCtlFresh + parity]: != 0 when the radix passes ran this step (the table is
                                 // of NOW: nobody is a straggler, the lists and the rosters are not used)
    const uint2 *table;
    uint32_t entries;
    int32_t blocks_x, blocks_y;  // table index of block (bx, by) = (by - by0) * blocks_x + (bx - bx0)
    int32_t bx0, by0;            // first block of the block box (0, 0 unless sharded)
    const uint32_t *counts;      // sharded runs: [0] = owned particles, kept on the device; else NULL
    float cell_size;
    float stiffness;
    int32_t gx, gy;              // cell box
    int32_t tiles_x, tiles_y;    // tile grid of the dense launch
    uint32_t band_tiles;         // ... dealt to the XCDs in bands of this many consecutive tiles (dense_launch_tile)
    // sharded runs that exchange beside the step: the FRAME of the tile grid (frame_l / _r columns, frame_b / _t rows: the
    // tiles whose particles can come to lie outside the pack's safe box) is resolved first, by k_collide_border
    int32_t frame_l, frame_r, frame_b, frame_t;
    int32_t tile_x0, tile_y0;    // its first tile (sharded runs cut the grid to the rank's active box)
    const uint32_t *order_keys;  // sharded runs: in-cell order by order_keys[local index]; else NULL
    uint32_t *tile_ctl;          // kCtl* words
    uint32_t *overflow1;         // packed (ty << 16 | tx) of over-capacity 32x32 tiles
    uint32_t overflow1_cap;
    // While tiles run over the direct-slot form (the host's lagged statistic) a launch between the dense and the
    // over-capacity one redoes each as two 32x16 HALVES in the same direct-slot form (k_collide_halves: half the cells,
    // so 1.6 x the particles per cell fit, at the dense launch's cost per particle); the halves it cannot take either
    // are listed in overflow2 (packed ty16 << 16 | tx32) and the over-capacity launch works through that list.
    uint32_t *overflow2;
    uint32_t quarters_of_halves; // list 1 was taken by the half-tile launch: the over-capacity launch only takes overflow2 (two quarters per half)
    // hints (kCtlHints): hints[parity * kHintMax + k] = ty << 16 | tx; front_wgs == 0: no hints this launch
    uint32_t *hints;
    uint32_t step_stamp, front_wgs, hint_parity;
    uint32_t hints_on;           // tiles that run over register themselves (front_wgs != 0: ... and this launch redoes the registered ones)
    // spill arena (global memory) for the particle arrays of such tiles
    float *arena_px, *arena_py, *arena_rad;
    uint32_t *arena_id, *arena_hm, *arena_mem;   // arena_mem holds 4 entries per particle
    uint8_t *arena_sblk;
    uint32_t arena_cap;
    // K12 fused into the write-back (particle_integration.wgsl:25-77) when fuse_verlet != 0
    float2 *prev;
    uint64_t n_owned;
    uint32_t fuse_verlet;
    VerletParams vp;
    // Tile rosters (direct-slot tiles of a run that keeps its block table): the particles a tile's lookup finds do not
    // change between two sorts, so the tile that looks them up right after a sort writes them down -- roster_ids[tile *
    // kRosterCap ..], roster_hdr[tile] = (count | 0xFFFFFFFF: more than the tile stages, stamp = sorts so far + 1, largest
    // 24x24-cell window population, -) -- and the steps until the next sort start from that list: one coalesced load
    // issued with the kernel's first instructions instead of table lookup -> scan -> slot map -> ids (three barriers and
    // a dependent global round trip).  A roster whose stamp is not the current one is ignored and rewritten.
    uint4 *roster_hdr;           // NULL: no rosters
    uint32_t *roster_ids;
    const uint32_t *sorts_seen;  // tile_ctl[kCtlSortsSeen]
    uint32_t roster_write;       // this run keeps its table: write rosters down
    unsigned long long *stamps;  // diagnostic builds only (-DGPE_TILE_STAMPS): cycles per phase, thread 0
    // sharded runs: the tiles along the rank's border pack their own particles for the neighbours as they write them
    // back (gpe_internal.h, pack_particle); pack.on == 0 otherwise
    PackArgs pack;
};
constexpr int kRosterCap = GPE_QMAX_MAIN_VALUE * 512;   // == TileDirect<32, .., 512>::RAWCAP

// The launchers (k_native.hip): each enqueues one kernel on c->stream and does nothing else -- the caller checks
// hipGetLastError where it always did.  The block size belongs to the kernel, so the launcher supplies it.
// (uniform: the instantiation that takes uniform_r for every particle's radius -- NativeState::uniform; keys == NULL: a
// kept-table step whose keys nobody reads unless it sorts, launch_native_hist_gated forms them then)
void launch_native_hash(gpe_ctx *c, bool ghosts, int grid, const float2 *pos, const float *radius, bool uniform,
                        float uniform_r, uint64_t n, const uint32_t *n_valid_ptr, float cell_size, int32_t gx, int32_t gy, int32_t bx0, int32_t by0,
                        int32_t blocks_x, int32_t blocks_y, uint32_t pad_key, uint32_t *keys, uint32_t *codes, int digits,
                        uint32_t *hist4, uint32_t *hist_next, uint32_t *os_ctl, uint32_t *tile_ctl, uint4 *table2,
                        uint64_t table_pairs, uint32_t *host_stat, const uint32_t *sorted_key, uint32_t parity,
                        uint64_t div_magic, uint32_t *exc_count, uint2 *exc_entry, uint32_t *exc_count_next, TileBox tb,
                        uint32_t straggler_limit, uint32_t fuse_always, const HashGhosts &G, bool index64);
// (K.pos != NULL: the hash stored no keys; the launch forms them from the positions, stores and counts them)
void launch_native_hist_gated(gpe_ctx *c, int grid, uint32_t *keys, uint64_t n, int digits, uint32_t *hist4,
                              const uint32_t *need, const HistKeys &K);
// (these two cover their n / entries with a grid-stride loop: stream_grid)
void launch_native_check_box(gpe_ctx *c, const float2 *pos, uint64_t n, const uint32_t *n_valid_ptr, float cell_size,
                             int32_t gx, int32_t gy, uint32_t *flag, const float *radius, uint32_t *radius_bits);
void launch_native_window_max(gpe_ctx *c, const uint2 *table, uint32_t entries, int32_t blocks_x, int32_t blocks_y,
                              uint32_t *out_max);
void launch_native_publish_probe(gpe_ctx *c, uint32_t *tile_ctl, uint32_t *host_stat);
// The collide kernels that are launched.  Ord: the order-key instantiation (sharded runs); Front: the dense launch
// carries front workgroups for the hinted tiles (the grid includes them).
enum class CollideForm {
    Dense, DenseOrd,                                   // counting-sort tiles
    Direct, DirectFront, DirectOrd, DirectOrdFront,    // direct-slot tiles
    BorderOrd,                                         // the frame of a sharded step that exchanges beside its interior
    Halves, HalvesOrd,                                 // the half-tile launch
    Overflow, OverflowOrd,                             // the over-capacity launch
};
void launch_collide(gpe_ctx *c, CollideForm form, uint32_t grid, const CollideArgs &A);
// The dense launch's tile grid (defined beside dense_launch_tile, whose mapping they mirror).
uint32_t dense_launch_band(uint32_t tiles_x, uint32_t tiles_y, bool eighths);
uint32_t dense_launch_grid(uint32_t tiles_x, uint32_t tiles_y, uint32_t band_tiles);

}  // namespace gpe
