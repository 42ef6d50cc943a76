// k_native.hip -- the MI355X-native collision pipeline (GPE_MODE_NATIVE).
//
// The reference sorts 4N (cell, object) pairs every step and resolves collisions cell by cell through
// global memory in four colour launches (~520 B/particle/step).  Here:
//
//   hash     key[i] = row-major index of particle i's 8x8-cell block, code[i] = its cell inside the block + the
//            overlap mask of its 8 neighbour cells; the four radix histograms and digit bases (fused); resets
//            the block table and the per-step control words
//   sort     onesweep over N (key, id) pairs (k_onesweep.hip); its last pass also fills the block table:
//            (start, end) of every block in the sorted order
//   collide  one workgroup per 32x32-cell tile: look the blocks of tile +- 8 cells up, keep the particles
//            whose home cell lies within 5 cells of the tile in LDS (positions, radii, ids gathered through
//            the sorted ids), rebuild the reference's per-cell member lists (home + phantom cells, members
//            in ascending object index), run ALL FOUR colour passes there, write back the tile's own
//            particles with the Verlet integration (K12) applied.
//
// Exactness: cell membership is frozen from the step-start positions
// (grid.wgsl:39-97), pairs of a cell run sequentially in ascending object index on live positions
// (collision_solver.wgsl:66-118), colours run 1..4.  A colour-k cell is exact when every cell that
// shares a particle with it was exact in colours < k; with the tile's own particles needing cells
// within +-1, the cells needed at colour k lie within +-(5-k) of the tile and their members' home
// cells within +-5 (the cell window; the block lookup reaches +-8).  Halo cells are recomputed redundantly by the neighbouring tiles (same
// inputs, same operation order => same bits), so no inter-tile communication and no global colour
// barrier is needed.  Positions are double-buffered (read pos_in, write pos_out) because neighbours
// read a tile's step-start positions while it writes its results.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "gpe_internal.h"
#include "k_cells.h"
#include "k_pair.h"
#include "native_launch.h"

namespace gpe {

constexpr int kNatThreads = 512;
constexpr int kNatWaves = kNatThreads / 64;

// exclusive scan of one value per thread over the whole workgroup (kNatWaves waves)
__device__ __forceinline__ uint32_t nat_block_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int lane = lane_id();
    const int w = (int)(threadIdx.x >> 6);
    const uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kNatWaves; ++i) {
        const uint32_t x = s_w[i];
        if (i < w) base += x;
        all += x;
    }
    if (total) *total = all;
    // no barrier behind the reads of s_w: its next writer (this function again) sits behind other barriers
    return base + inc - v;
}
constexpr int kHalo = 8;                       // cells = one 8x8 block: the granule of the block table lookups
// Cells a tile really needs around itself (tiles start at even cell coordinates, T is even).  Colour - 1 =
// (x & 1) + 2 (y & 1) (collision_solver.wgsl:55-58), a particle spans at most 2 x 2 cells, and a cell only depends on
// cells of EARLIER colours that share a member with it -- its horizontal, vertical or diagonal neighbours, by parity:
//   colour 4 (odd, odd)   <- colour 3 left / right, colour 2 below / above, colour 1 diagonal
//   colour 3 (even, odd)  <- colour 2 diagonal, colour 1 below / above
//   colour 2 (odd, even)  <- colour 1 left / right
// The tile's own particles sit in cells within 1 of the tile [x0, x1] x [y0, y1] (x0, y0 even; x1, y1 odd), so the
// cells that must be exact are
//   colour 4: x in [x0-1, x1]   y in [y0-1, y1]        colour 3: x in [x0-2, x1+1] y in [y0-1, y1]
//   colour 2: x in [x0-3, x1+2] y in [y0-2, y1+1]      colour 1: x in [x0-4, x1+3] y in [y0-2, y1+1]
// and their members' home cells lie within [x0-5, x1+4] x [y0-3, y1+2]: the cell window.  (A square window of
// tile +- 5 holds 16 % more cells, and the square colour zones 12 % more cells to resolve.)
constexpr int kConeLeft = 4, kConeRight = 3, kConeDown = 2, kConeUp = 1;   // colour-1 cells beyond the tile's edges
constexpr uint32_t kErrOutOfBox = 1u;          // a particle outside the configured cell box
constexpr uint32_t kErrTileOverflow = 2u;      // an 8x8 tile region over LDS capacity (no result!)
constexpr uint32_t kErrBoundExceeded = 16u;    // sharded run: the device-side particle count passed the host's bound
// (the tile_ctl words -- kCtl* -- with the tile hints they carry, the list sizes kExcSlots / kGhostSlots and the arena's
// slot size are the host's too: native_launch.h)
constexpr uint32_t kHintAge = 240;             // a hint entry: age << 22 | ty << 11 | tx (at most 2048 tiles per axis: 16-bit cells)
// How far a particle may have left the 8x8-cell block it was sorted into (cells beyond the block's extent, per
// direction) and still be found by every tile that needs it.  A tile looks up the blocks of tile +- 8 cells but keeps
// only the window [x0-5, x1+4] x [y0-3, y1+2] (kCone* + 1): a kept particle that moved right by dr cells comes from a
// block that starts at >= (x0-5) - 7 - dr, inside the lookup (>= x0-15, block-aligned: x0-8) while dr <= 3; moved left:
// its block starts at <= x1+4+dl <= x1+8 while dl <= 4; up: >= (y0-3) - 7 - du >= y0-15 while du <= 5; down: <= y1+2+dd
// <= y1+8 while dd <= 6.
constexpr int kDriftLeft = 4, kDriftRight = 3, kDriftDown = 6, kDriftUp = 5;
// The code word of a particle (k_native_hash -> tiles): its cell MOD 128 per axis (a tile's lookup region plus the drift
// spans fewer than 128 cells, so the value names one cell of it) | the overlap mask of the 8 neighbour cells | straggler.
constexpr uint32_t kCodeCellMask = 127u;
constexpr int kCodeYShift = 7, kCodeOverlapShift = 14;
constexpr uint32_t kCodeStraggler = 1u << 22;
static_assert(kDriftRight <= kHalo - (kConeLeft + 1) && kDriftLeft <= kHalo - (kConeRight + 1), "x drift inside the lookup slack");
static_assert(kDriftUp <= kHalo - (kConeDown + 1) && kDriftDown <= kHalo - (kConeUp + 1), "y drift inside the lookup slack");
static_assert(64 + 2 * kHalo + kDriftLeft + kDriftRight < 128 && 32 + 2 * kHalo + kDriftDown + kDriftUp < 128, "a lookup region + drift names every cell mod 128 once");
// window coordinate of the cell a code names, for a window whose first cell is o (any sign): in [0, 128)
__device__ __forceinline__ int code_window_x(uint32_t code, int o) { return (int)((code - (uint32_t)o) & kCodeCellMask); }
__device__ __forceinline__ int code_window_y(uint32_t code, int o) { return (int)(((code >> kCodeYShift) - (uint32_t)o) & kCodeCellMask); }
// (the pinned host words the kernels report to -- kStat* -- are declared in gpe_internal.h: gpe_get_pipeline_info reads them too)
// tile sizes (cells) and LDS capacities (particles staged per region)
#ifndef GPE_CAP_MAIN
#define GPE_CAP_MAIN 1192
#endif
constexpr int kCapMain = GPE_CAP_MAIN;             // (kTileMain: native_launch.h)
// The sub-tile windows take the same LDS as the main one, so the launch for over-capacity tiles also runs four
// workgroups per CU (with 1920 / 2048-particle windows it ran two: half the waves to hide latency with).
// (Round 4: 1600-particle sub-tile windows, three workgroups per CU at 80 VGPRs, looked-up capacity 8 x 512 -- against
// 1200 / four per CU / 64 VGPRs / 6 x 512: -1.4 % at step 1250 and -7.5 % at step 2000 of the 100 M soak; 2000-particle
// windows at two per CU and 128 VGPRs, which spill nothing: +5 % / -7 %.  profiles/r04/soak_marks_overflow_windows.txt)
#ifndef GPE_CAP_MID
#define GPE_CAP_MID 1600
#endif
#ifndef GPE_CAP_SMALL
#define GPE_CAP_SMALL 1600
#endif
#ifndef GPE_QMAX_MID
#define GPE_QMAX_MID 8
#endif
#ifndef GPE_OVF_WAVES
#define GPE_OVF_WAVES 6                        // waves per SIMD the over-capacity launch is compiled for (512 VGPRs / this)
#endif
constexpr int kTileMid = 16, kCapMid = GPE_CAP_MID;
constexpr int kTileSmall = 8, kCapSmall = GPE_CAP_SMALL;
// sharded (order-key) instantiations: 4 more bytes per slot for the local index, so 1024 slots in the same LDS
#ifndef GPE_CAP_ORD
#define GPE_CAP_ORD 1024
#endif
constexpr int kCapOrd = GPE_CAP_ORD;
// population of a 3x3-block (24x24-cell) window = what an 8x8 sub-tile looks up (it keeps ~56 % of it):
constexpr uint32_t kWindowReport = 512;     // tiles report windows above this population
// (the handover and eligibility populations, kWindowHandover / kWindowEligible, are the step policy's: native_policy.h)

// ---------------------------------------------------------------------------------------------------
// hash: per particle R pos 8 B, radius 4 B, old key 4 B (kept table); W code 4 B, key 4 B -- 24 B.  Two of the five never
// change the result on the steps of a run that keeps its table: the UNIFORM instantiation takes the one radius all
// particles have as a kernel argument (NativeState::uniform), and a kept-table step whose digits the gated launch counts
// stores no key (keys == NULL: k_native_hist_gated derives the keys itself on the steps that sort) -- 16 B.
// Fused 4-digit histogram for the onesweep passes on the steps that sort anyway.
// (home_cell_ids.wgsl:24-31 computes the Morton id of the home cell; the key kept here is the row-major index
// of its 8x8-cell block; the particle id is implicit in the first pass.)
// The workgroup that flushes its histogram last also turns the histograms into the digit bases of the four
// passes and resets the tile tickets (k_os_prepare's job): one launch less on the step path.
// ---------------------------------------------------------------------------------------------------
// (the overlap mask of the 8 neighbour cells, neighbour_overlap_mask: k_cells.h)
//
// Every workgroup flushes up to 256 bins per digit with device-scope atomics (they resolve beyond the per-XCD
// L2s), so the workgroups are large (1024 lanes).  The kernel is bound by instruction issue and latency, not by
// HBM: two workgroups per CU (64 VGPRs: two positions per lane in flight instead of eight) and up to 2048 of them
// take it from 544 to 454 us at 100 M particles and from 98 to 84 us at 16 M, the extra flushes included
// (profiles/r02/ab_hash_occupancy.txt).
// (kHashBlock, kHashGridMax and HashGhosts: native_launch.h)
constexpr int kHashBatch = 2;                  // positions loaded per lane before any of them is ranked
// The sort key of a particle at p: its 8x8-cell block, row-major over the block box; 0 and `out` for a particle outside
// the cell box or the block box (flagged by the hash).  cx, cy: its home cell.  One expression for the two kernels that
// form keys -- the hash, and the gated histogram on the steps whose hash stored none.
__device__ __forceinline__ uint32_t block_key_of(const float2 p, const float cell_size, const int32_t gx, const int32_t gy,
                                                 const int32_t bx0, const int32_t by0, const int32_t blocks_x,
                                                 const int32_t blocks_y, int32_t &cx, int32_t &cy, bool &out)
{
    cx = cell_coord(p.x, cell_size);
    cy = cell_coord(p.y, cell_size);
    const int32_t lbx = (cx >> 3) - bx0, lby = (cy >> 3) - by0;
    out = (cx < 0) | (cx >= gx) | (cy < 0) | (cy >= gy) | (lbx < 0) | (lbx >= blocks_x) | (lby < 0) | (lby >= blocks_y);
    // (24-bit multiply-add: both factors are below 2^13 for an in-box cell; a full-rate instruction where the 32-bit
    // multiply takes four issue slots -- the hash is bound by issue at 100 M, not by HBM)
    return out ? 0u : __umul24((uint32_t)lby, (uint32_t)blocks_x) + (uint32_t)lbx;
}
// GHOSTS: a sharded run with its counts on the device (HashGhosts); the ordinary instantiation carries none of that code.
// Index: the type of the particle indices, the stride and the round counters.  uint32_t while every index the loop forms
// stays below 2^31 (launch_native_hash: 1 M and 100 M particles both do) -- an address is then base + zero-extended index,
// where the 64-bit form multiplies, shifts and adds register pairs on the VALU for each of the five arrays a particle
// touches; uint64_t beyond that.  Same stores, same atomics in the same order, same bits either way.
// UNIFORM: every particle has the radius uniform_r (NativeState::uniform): `radius` is not read.
template <bool GHOSTS, typename Index, bool UNIFORM = false>
__global__ __launch_bounds__(kHashBlock, 8) void k_native_hash(const float2 *__restrict__ pos,
                                                            const float *__restrict__ radius, uint64_t n64,
                                                            const uint32_t *__restrict__ n_valid_ptr,
                                                            float cell_size, int32_t gx, int32_t gy,
                                                            int32_t bx0, int32_t by0, int32_t blocks_x,
                                                            int32_t blocks_y, uint32_t pad_key,
                                                            uint32_t *__restrict__ keys,
                                                            uint32_t *__restrict__ codes, int digits,
                                                            uint32_t *hist4, uint32_t *__restrict__ hist_next,
                                                            uint32_t *__restrict__ os_ctl, uint32_t *tile_ctl,
                                                            uint4 *__restrict__ table2, uint64_t table_pairs,
                                                            uint32_t *__restrict__ host_stat,
                                                            const uint32_t *__restrict__ sorted_key, uint32_t parity,
                                                            float uniform_r, uint32_t *__restrict__ exc_count,
                                                            uint2 *__restrict__ exc_entry,
                                                            uint32_t *__restrict__ exc_count_next, TileBox tb,
                                                            uint32_t straggler_limit, uint32_t fuse_always, HashGhosts G,
                                                            unsigned long long *stamp)
{
    // (a sampled step's boundary in front of this launch: scope_stamps.h)
    if (stamp && blockIdx.x == 0 && threadIdx.x == 0) *stamp = wall_clock64();
    // sorted_key[i] = the block key particle i had when the radix passes last ran (they keep it up to date,
    // k_onesweep.hip): the sorted ids and the block table still describe THAT grouping.  As long as every particle
    // is within kDrift* cells of its old block, the tiles find it through the old table (they look up more than they
    // keep) and this step needs no sort: the code carries the particle's cell RELATIVE to the old block.  Particles
    // beyond that go to per-tile straggler lists (kExcSlots); a list running over raises tile_ctl[kCtlNeedSort +
    // parity]; the radix passes that follow look at the word and return at once when it is 0.
    // sorted_key == NULL: always sort (first step, sharded runs, one-pass sorts).
    // (uniform_r stands where the block key's division magic stood until the division moved to the radix pass that
    // writes sorted_key: the kernel takes as many arguments as it did -- on a small scene the host's time to marshal a
    // launch is on the step's critical path)
    __shared__ uint32_t s_hist[4 * 256];
    __shared__ uint32_t s_ghist[GHOSTS ? 4 * 256 : 1];                 // (the ghosts' keys, sharded runs)
    __shared__ uint32_t s_sort_known;                                  // a wave of this workgroup has seen the straggler limit passed
    // The digit histograms of the owned particles' keys feed the radix passes -- which run on ~1 % of the steps of a run
    // that keeps its block table (7-12 % at 100 M in free fall).  Such a run leaves them to a gated launch of its own
    // behind this kernel (k_native_hist_gated: it returns at once unless need_sort was raised); only a step that sorts
    // anyway (no kept table: first step, sort_hold, a run that sorts every step) counts them here, fused.
    const bool fuse_hist = sorted_key == nullptr || fuse_always != 0u;   // (fuse_always: the host asks for the fused count as rounds 1-3 had it)
    // (kernel-uniform) a step that counts nothing here neither zeroes s_hist nor reads it back in the flush
    const bool ghost_hist = GHOSTS && (G.gkeys != nullptr || G.ghist_now != nullptr);
    if (fuse_hist) s_hist[threadIdx.x] = 0;
    if (GHOSTS) s_ghist[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_sort_known = 0u;
    // What a step accumulates into is reset here instead of by a launch of its own (a launch costs ~6 us, 5 % of
    // the step at 1 M particles): the block table (filled two kernels later), and -- workgroup 0 -- the per-step
    // control words, after handing the previous step's window statistic to the host (pinned memory), the radix
    // passes' tile tickets, and the digit histograms the NEXT step's hash adds into (two sets, alternating steps:
    // this step's set is read by the radix passes that follow, nobody touches the other one meanwhile).
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < table_pairs; i += (uint64_t)gridDim.x * blockDim.x)
        table2[i] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);      // (first, one past last) = (max, 0): empty
    if (GHOSTS)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G.gtable_pairs; i += (uint64_t)gridDim.x * blockDim.x)
        G.gtable2[i] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);   // the ghosts' block table: rebuilt every step
    if (exc_count_next) {                                              // the next step's straggler lists
        const uint64_t nt = (uint64_t)tb.nx * (uint64_t)tb.ny;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += (uint64_t)gridDim.x * blockDim.x)
            exc_count_next[i] = 0;
    }
    if (GHOSTS && G.gl_count_next) {                                   // ... and ghost lists
        const uint64_t nt = (uint64_t)tb.nx * (uint64_t)tb.ny;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += (uint64_t)gridDim.x * blockDim.x)
            G.gl_count_next[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < kCtlPerStepWords) {
        if (host_stat) {                                               // last step's statistics (kStat*), lagged
            if (threadIdx.x == kCtlWindowMax) host_stat[kStatWindowMax] = tile_ctl[kCtlWindowMax];
            if (threadIdx.x == kCtlArena) host_stat[kStatArena] = tile_ctl[kCtlArena];
            if (threadIdx.x == kCtlOverflow1) {
                // (+ the hinted tiles of the last launch)
                const uint32_t fresh_over = tile_ctl[kCtlOverflow1];
                host_stat[kStatOverflow] = fresh_over + tile_ctl[kCtlHintsSeen];
                host_stat[kStatOverflowNew] = fresh_over;
            }
            if (threadIdx.x == kCtlOverflow2) host_stat[kStatHalvesOver] = tile_ctl[kCtlOverflow2];
            if (threadIdx.x == kCtlSubTiles) host_stat[kStatSubTiles] = tile_ctl[kCtlSubTiles];
            if (threadIdx.x == kCtlSpills) host_stat[kStatSpills] = tile_ctl[kCtlSpills];
            if (threadIdx.x == 7) host_stat[kStatSorts] = tile_ctl[kCtlSorts];
        }
        tile_ctl[threadIdx.x] = 0;
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < kHistCopies * 4 * 256; i += kHashBlock) hist_next[i] = 0;
        if (GHOSTS && G.ghist_next)
            for (int i = threadIdx.x; i < kHistCopies * 4 * 256; i += kHashBlock) G.ghist_next[i] = 0;
        if (threadIdx.x < 16) os_ctl[threadIdx.x] = 0;                 // tile tickets (owned [0..3], ghosts [8..11]) + error word [4]
        if (threadIdx.x == 0) {                                        // the next step's words; this step's if it must sort
            tile_ctl[kCtlNeedSort + (parity ^ 1u)] = 0;
            tile_ctl[kCtlFresh + (parity ^ 1u)] = 0;
            tile_ctl[parity ? kCtlStragglers0 : kCtlStragglers1] = 0;
            if (GHOSTS && G.ghost_sort_next) *G.ghost_sort_next = 0u;
            if (GHOSTS && G.gkeys && !G.gl_count) atomicOr(G.ghost_sort, 1u);   // (no lists: the ghosts are always sorted)
            if (!sorted_key) atomicOr(&tile_ctl[kCtlNeedSort + parity], 1u);
        }
    }
    __syncthreads();
    const Index n = (Index)n64;
    const Index stride = (Index)gridDim.x * (Index)blockDim.x;
    const Index rounds = (n + stride - 1) / stride;
    const Index first_idx = (Index)blockIdx.x * (Index)blockDim.x + (Index)threadIdx.x;
    // Sharded runs keep the particle count on the device (the exchange changes it every step without a host
    // round trip): the host passes an upper bound n, slots [nv, n) are padding that sorts behind every block.
    Index nv = n;
    if (n_valid_ptr) {
        const uint32_t have = *n_valid_ptr;
        if ((uint64_t)have > n64) { if (threadIdx.x == 0) atomicOr(&tile_ctl[kCtlError], kErrBoundExceeded); }
        else nv = (Index)have;
    }
    // owned particles [0, n_own), ghosts [n_own, nv); indices from sorted_cnt on are not in the kept grouping
    Index n_own = nv;
    if (GHOSTS && G.owned) n_own = min((Index)*G.owned, nv);
    const Index sorted_cnt = (sorted_key && G.sorted_count) ? (Index)*G.sorted_count : ~(Index)0;
    if (GHOSTS && G.gkeys) {
        // ghost slots behind the last one the particle loop below reaches: padding (sorts behind every block)
        const uint64_t first = (uint64_t)(n - n_own);
        for (uint64_t j = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < G.g_bound; j += (uint64_t)gridDim.x * blockDim.x) {
            G.gkeys[j] = pad_key; G.gids[j] = 0u;
        }
        if ((uint64_t)(nv - n_own) > G.g_bound && threadIdx.x == 0) atomicOr(&tile_ctl[kCtlError], kErrBoundExceeded);
    }
    bool oob = false, drifted = false;
    bool sort_known = sorted_key == nullptr;                           // (wave-uniform) the radix passes will run this step
    for (Index r0 = 0; r0 < rounds; r0 += kHashBatch) {
        float2 p[kHashBatch];
        float rad[kHashBatch];
        Index idx[kHashBatch];
        uint32_t okey[kHashBatch];
#pragma unroll
        for (int u = 0; u < kHashBatch; ++u) {                        // the loads of a batch are in flight together
            idx[u] = (r0 + (Index)u) * stride + first_idx;
            const bool in = r0 + (Index)u < rounds && idx[u] < nv;
            p[u] = in ? pos[idx[u]] : make_float2(0.f, 0.f);
            if constexpr (UNIFORM) rad[u] = uniform_r;
            else rad[u] = in ? radius[idx[u]] : 0.f;
            okey[u] = (in && sorted_key) ? sorted_key[idx[u]] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kHashBatch; ++u) {
            if (r0 + (Index)u >= rounds) break;                        // wave-uniform
            const bool valid = idx[u] < n;
            uint32_t key = pad_key;
            if (valid && idx[u] >= nv) {
                if (keys) keys[idx[u]] = pad_key;
                codes[idx[u]] = 0u;
                if (GHOSTS && G.gkeys && (uint64_t)(idx[u] - n_own) < G.g_bound) { G.gkeys[idx[u] - n_own] = pad_key; G.gids[idx[u] - n_own] = 0u; }
            }
            const bool ghost = GHOSTS && idx[u] >= n_own;
            uint32_t gkey = 0;
            bool gvalid = false;
            if (idx[u] < nv) {
                // the particle's 8x8-cell block, row-major over the block box (0 for a particle outside it: flagged)
                int32_t cx, cy;
                bool out;
                key = block_key_of(p[u], cell_size, gx, gy, bx0, by0, blocks_x, blocks_y, cx, cy, out);
                oob |= out;
                if (GHOSTS && ghost && G.gkeys) {
                    // a ghost: grouped by the ghosts' own sort; in the owned particles' sort it is padding
                    const uint64_t j = (uint64_t)(idx[u] - n_own);
                    if (j < G.g_bound) { G.gkeys[j] = key; G.gids[j] = (uint32_t)idx[u]; gkey = key; gvalid = true; }
                    key = pad_key;
                }
                if (keys) keys[idx[u]] = key;                          // (kernel-uniform; NULL: nobody reads them unless the step sorts)
                // The particle's cell relative to the first cell of the block it was SORTED into: is it still within the
                // reach of the tiles that find it through that block?
                bool straggler = false;
                if (sorted_key && !(GHOSTS && ghost && G.gkeys)) {
                    // (sorted_key holds the block's coordinates in the block box, x | y << 16: the radix pass that
                    // copies the keys divides once per sort, k_onesweep.hip, instead of this kernel every step)
                    const uint32_t obx = okey[u] & 0xFFFFu, oby = okey[u] >> 16;
                    const int32_t relx = cx - (int32_t)((obx + (uint32_t)bx0) << 3);
                    const int32_t rely = cy - (int32_t)((oby + (uint32_t)by0) << 3);
                    // out of reach of its old block, or not in the kept grouping at all (an arrival of a sharded run,
                    // filed behind the particles the last sort covered): handed to the tiles directly
                    straggler = !out && ((relx < -kDriftLeft) | (relx > 7 + kDriftRight) | (rely < -kDriftDown) | (rely > 7 + kDriftUp) |
                                         (idx[u] >= sorted_cnt));
                }
                // what the tiles need to file the particle: its cell (mod 128) and its phantom cells.
                // Computed once here instead of by each of the ~2.25 tiles that stage the particle.
                codes[idx[u]] = ((uint32_t)cx & kCodeCellMask) | (((uint32_t)cy & kCodeCellMask) << kCodeYShift) |
                                (neighbour_overlap_mask(p[u], rad[u], cx, cy, cell_size) << kCodeOverlapShift) |
                                (straggler ? kCodeStraggler : 0u);
                // Stragglers are meant to be the few fast particles of a hot cloud.  When the whole cloud moves (free
                // fall) a large share of the particles runs out of reach within a step or two: handing millions of
                // them over, at up to four atomics each, costs more than the sort that makes them ordinary again.
                // Once the sort is known to run, handing stragglers over is wasted work (the tiles then ignore the lists):
                // a crushed scene makes a third of the particles stragglers, and their atomics -- one per wave on the
                // counter, up to four per particle on the lists -- took longer than the tiles (100 M soak, step 1000:
                // 22 ms/step with them, 16 without).  A wave learns it from the counter itself (its own add comes back
                // above the limit) or from its workgroup (an LDS word): no extra global round trip in calm scenes.
                const uint64_t ms = ballot64(straggler);
                bool route = false;
                if (ms != 0 && !sort_known) {                            // (wave-uniform)
                    sort_known = wave_lds_load(&s_sort_known) != 0u;     // (another wave of the workgroup has learnt it)
                    if (!sort_known) {
                        const int leader = (int)__builtin_ctzll(ms);
                        uint32_t before = 0;
                        if (lane_id() == leader)
                            before = atomicAdd(&tile_ctl[parity ? kCtlStragglers1 : kCtlStragglers0], (uint32_t)__popcll(ms));
                        before = (uint32_t)__builtin_amdgcn_readlane((int)before, leader);
                        if (before + (uint32_t)__popcll(ms) > straggler_limit) {
                            sort_known = true;
                            if (lane_id() == leader) { wave_lds_store(&s_sort_known, 1u); atomicOr(&tile_ctl[kCtlNeedSort + parity], 1u); }
                        } else route = true;
                    }
                }
                if (straggler && route) {
                    // every 32x32 tile whose window [32 tx - 5, 32 tx + 35] x [32 ty - 3, 32 ty + 33] holds the cell
                    // (sub-tiles of the over-capacity launch read their parent's list: their windows lie inside its)
                    const int tx0 = max(tb.x0, (cx - (kConeRight + 1)) >> 5), tx1 = min(tb.x0 + tb.nx - 1, (cx + kConeLeft + 1) >> 5);
                    const int ty0 = max(tb.y0, (cy - (kConeUp + 1)) >> 5), ty1 = min(tb.y0 + tb.ny - 1, (cy + kConeDown + 1) >> 5);
                    for (int ty = ty0; ty <= ty1; ++ty)
                        for (int tx = tx0; tx <= tx1; ++tx) {
                            const uint32_t t = tb.index(tx, ty);
                            const uint32_t slot = atomicAdd(&exc_count[t], 1u);
                            if (slot < kExcSlots) exc_entry[(uint64_t)t * kExcSlots + slot] = make_uint2((uint32_t)idx[u], (uint32_t)cx | ((uint32_t)cy << 16));
                            else { drifted = true; atomicOr(&tile_ctl[kCtlNeedSort + parity], 1u); }   // a list ran over: sort (and tell the others)
                        }
                }
            }
            if (fuse_hist) {                                           // (uniform)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < digits) hist_add(s_hist + q * 256, (key >> (8 * q)) & 255u, valid);
            }
            if (GHOSTS && G.gkeys) {                                   // (uniform)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < digits) hist_add(s_ghist + q * 256, (gkey >> (8 * q)) & 255u, gvalid);
            }
        }
    }
    if (GHOSTS && G.gl_count) {
        // The ghosts once more, for the tiles: every ghost is listed for each 32x32 tile whose window holds its cell (as
        // the stragglers above).  A loop of its own over the few thousand ghosts -- inside the particle loop the routing
        // pushed the kernel over its 64 registers.
        for (Index i = n_own + first_idx; i < nv; i += stride) {
            const float2 p = pos[i];
            const int32_t cx = cell_coord(p.x, cell_size), cy = cell_coord(p.y, cell_size);
            if ((cx < 0) | (cx >= gx) | (cy < 0) | (cy >= gy)) continue;
            const int tx0 = max(tb.x0, (cx - (kConeRight + 1)) >> 5), tx1 = min(tb.x0 + tb.nx - 1, (cx + kConeLeft + 1) >> 5);
            const int ty0 = max(tb.y0, (cy - (kConeUp + 1)) >> 5), ty1 = min(tb.y0 + tb.ny - 1, (cy + kConeDown + 1) >> 5);
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) {
                    const uint32_t t = tb.index(tx, ty);
                    const uint32_t slot = atomicAdd(&G.gl_count[t], 1u);
                    if (slot < kGhostSlots) G.gl_entry[(uint64_t)t * kGhostSlots + slot] = (uint32_t)i;
                    else atomicOr(G.ghost_sort, 1u);                   // a list ran over: the ghosts' sort runs this step
                }
        }
    }
    if (GHOSTS && G.gkeys && blockIdx.x == 0 && threadIdx.x < (uint32_t)digits) {
        // the ghost sort covers g_bound slots: those behind the ghosts hold the padding key
        const uint64_t ng = min((uint64_t)(nv - n_own), G.g_bound);
        atomicAdd(&s_ghist[threadIdx.x * 256 + ((pad_key >> (8 * threadIdx.x)) & 255u)], (uint32_t)(G.g_bound - ng));
    }
    if (oob) atomicOr(&tile_ctl[kCtlError], kErrOutOfBox);
    if (ballot64(drifted) != 0 && lane_id() == 0) atomicOr(&tile_ctl[kCtlNeedSort + parity], 1u);
    if (!fuse_hist && !ghost_hist) return;                             // (kernel-uniform) nothing was counted: nothing to flush
    __syncthreads();
    // Flush: fire-and-forget device-scope atomics (the kernel boundary makes them visible); the radix passes turn the
    // histograms into digit bases themselves (k_os_pass, hist_src), so no workgroup waits for the others here.
    if ((threadIdx.x & 1u) == 0) {
        // two neighbouring bins per 64-bit atomic (no bin reaches 2^32, so nothing carries into the upper one)
        if (fuse_hist) {
            const uint32_t lo = s_hist[threadIdx.x], hi = s_hist[threadIdx.x + 1];   // index = digit * 256 + bin
            if (lo | hi)
                __hip_atomic_fetch_add(
                    reinterpret_cast<unsigned long long *>(&hist4[(blockIdx.x % kHistCopies) * 1024 + threadIdx.x]),
                    (unsigned long long)lo | ((unsigned long long)hi << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (GHOSTS && G.ghist_now) {
            const uint32_t glo = s_ghist[threadIdx.x], ghi = s_ghist[threadIdx.x + 1];
            if (glo | ghi)
                __hip_atomic_fetch_add(
                    reinterpret_cast<unsigned long long *>(&G.ghist_now[(blockIdx.x % kHistCopies) * 1024 + threadIdx.x]),
                    (unsigned long long)glo | ((unsigned long long)ghi << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The digit histograms of the keys when the hash kernel has left them out (a run that keeps its block table): gated like
// the radix passes behind it -- every workgroup looks at need_sort first and returns at once when no sort is due.  Same
// layout as the hash's flush (kHistCopies copies of 4 x 256 bins, two bins per 64-bit atomic).
// K.pos != NULL: the hash stored no keys this step (nobody reads them on a step that does not sort); this kernel runs exactly
// when the radix passes behind it will (the same word gates both), so it forms the keys from the positions -- the hash's
// own expression, block_key_of -- stores them for the first pass and counts them.  K.pos == NULL: the hash stored them.
__global__ __launch_bounds__(kHistGatedBlock) void k_native_hist_gated(uint32_t *__restrict__ keys, uint64_t n, int digits,
                                                                       uint32_t *__restrict__ hist4,
                                                                       const uint32_t *__restrict__ need,
                                                                       unsigned long long *stamp, HistKeys K)
{
    // (a sampled step's boundary in front of this launch: scope_stamps.h)
    if (stamp && blockIdx.x == 0 && threadIdx.x == 0) *stamp = wall_clock64();
    if (*need == 0u) return;
    __shared__ uint32_t s_hist[4 * 256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t idx = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const bool valid = idx < n;
        uint32_t key = 0u;
        if (K.pos) {                                                   // (kernel-uniform)
            if (valid) {
                int32_t cx, cy;
                bool out;
                key = block_key_of(K.pos[idx], K.cell_size, K.gx, K.gy, K.bx0, K.by0, K.blocks_x, K.blocks_y, cx, cy, out);
                keys[idx] = key;
            }
        } else if (valid) key = keys[idx];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < digits) hist_add(s_hist + q * 256, (key >> (8 * q)) & 255u, valid);
    }
    __syncthreads();
    if ((threadIdx.x & 1u) == 0) {
        const uint32_t lo = s_hist[threadIdx.x], hi = s_hist[threadIdx.x + 1];
        if (lo | hi)
            __hip_atomic_fetch_add(
                reinterpret_cast<unsigned long long *>(&hist4[(blockIdx.x % kHistCopies) * 1024 + threadIdx.x]),
                (unsigned long long)lo | ((unsigned long long)hi << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Largest particle count of any 3x3-block (24x24-cell) window: what the smallest cell window must hold.
// Configuration-time check over the whole table (the step path gets the same number from the tiles).
__global__ __launch_bounds__(kStreamBlock) void k_native_window_max(const uint2 *__restrict__ table,
                                                                    uint32_t entries, int32_t blocks_x,
                                                                    int32_t blocks_y,
                                                                    uint32_t *__restrict__ out_max)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t best = 0;
    for (uint64_t mb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; mb < entries; mb += stride) {
        const int bx = (int)(mb % (uint32_t)blocks_x), by = (int)(mb / (uint32_t)blocks_x);
        uint32_t sum = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = bx + dx, y = by + dy;
                if (x < 0 || y < 0 || x >= blocks_x || y >= blocks_y) continue;
                const uint32_t m = (uint32_t)(y * blocks_x + x);
                if (m < entries) { const uint2 se = table[m]; sum += se.y > se.x ? se.y - se.x : 0u; }
            }
        best = max(best, sum);
    }
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d, 64));
    if (lane_id() == 0 && best) atomicMax(out_max, best);
}

// the asynchronous probe's last link: the measured maximum (+ 1, so that 0 means "no answer yet") goes to the host
__global__ void k_native_publish_probe(uint32_t *__restrict__ tile_ctl, uint32_t *__restrict__ host_stat)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        __hip_atomic_store(&host_stat[kStatProbe], tile_ctl[kCtlWindowMax] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        tile_ctl[kCtlWindowMax] = 0;
    }
}

// every particle inside the cell box?  (configuration-time check, not on the step path)
// radius != NULL: also the range of the radii's BIT PATTERNS, as maxima into radius_bits (cleared by the caller):
// [0] = ~(smallest pattern), [1] = largest pattern.  Equal patterns: every particle has that one radius (NativeState::uniform).
__global__ __launch_bounds__(kStreamBlock) void k_native_check_box(const float2 *__restrict__ pos, uint64_t n,
                                                                   const uint32_t *__restrict__ n_valid_ptr,
                                                                   float cell_size, int32_t gx, int32_t gy,
                                                                   uint32_t *__restrict__ flag,
                                                                   const float *__restrict__ radius,
                                                                   uint32_t *__restrict__ radius_bits)
{
    if (n_valid_ptr && *n_valid_ptr < n) n = *n_valid_ptr;           // sharded run: the count lives on the device
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool oob = false;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float2 p = pos[i];
        const int32_t cx = cell_coord(p.x, cell_size), cy = cell_coord(p.y, cell_size);
        oob |= (cx < 0) | (cx >= gx) | (cy < 0) | (cy >= gy);
        if (radius) {                                                  // (kernel-uniform)
            const uint32_t bits = __float_as_uint(radius[i]);
            lo = min(lo, bits);
            hi = max(hi, bits);
        }
    }
    if (oob) atomicOr(flag, kErrOutOfBox);
    if (radius) {
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
            hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
        }
        if (lane_id() == 0 && lo <= hi) { atomicMax(&radius_bits[0], ~lo); atomicMax(&radius_bits[1], hi); }
    }
}

// ---------------------------------------------------------------------------------------------------
// table: the sort key is the particle's 8x8-cell block (row-major index over the box).  table[b] = (first,
// one-past-last) position of the block's particles in the sorted order, (0xFFFFFFFF, 0) for an empty block.
// It is filled by the last radix pass (k_onesweep.hip, k_os_pass): no launch of its own.
// ---------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------
// collide
// ---------------------------------------------------------------------------------------------------
// (CollideArgs, what a collide launch is told, and kRosterCap: native_launch.h)
// The pack as the tiles do it: a particle whose new position lies inside the `safe` box (the rank's rectangle shrunk by
// one block and a cell on every side that has a neighbour) sits in a block this rank owns and no other rank borders --
// four compares say so, no table lookup; only the others go through pack_particle (a wave none of whose lanes holds one
// skips it: every tile away from the rank's border, whatever the speed of its particles).
__device__ __forceinline__ void pack_if_near_border(const PackArgs &P, const bool mine, const uint32_t id, const float2 o,
                                                    const float2 c, const float rad, const uint32_t key, const float cell_size)
{
    const bool near = mine && (o.x < P.safe_x0 || o.x >= P.safe_x1 || o.y < P.safe_y0 || o.y >= P.safe_y1);
    if (ballot64(near) == 0) return;
    if (P.on == 2u) {
        // an interior tile, resolved while the segments are already on their way: its particles lie more than a block
        // (+ a cell) inside the safe box at the start of the step, so only a particle that moved further than the
        // exchange's protocol allows (one block per step, k_shard.hip) gets here -- the run is in error, loudly
        if (near) atomicOr(P.err, kShardErrNoSlot);
        return;
    }
    pack_particle(P, near, id, o, c, rad, key, cell_size);
}

#ifdef GPE_TILE_CYCLES
// diagnostic builds only (scripts/tile_cycles.py): what every tile of the dense launch and every quarter of the
// over-capacity launch cost -- g_tile_cycles[tile of the tile box] = (cycles of the dense launch's workgroup, outcome:
// 0 done / 1 handed on, cycles of its quarters in the over-capacity launch, particles it looked up)
__device__ uint4 *g_tile_cycles;
__device__ uint32_t g_bail_reasons[8];         // why direct-slot tiles were handed on, counted since the last reset
#define GPE_BAIL(code) atomicAdd(&g_bail_reasons[code], threadIdx.x == 0 ? 1u : 0u)
#else
#define GPE_BAIL(code) ((void)0)
#endif
#ifdef GPE_DBG_RT
// diagnostic builds only (scripts/overflow_phases.py): parts of the counting-sort windows' colour passes switched off at
// run time (1 lane groups, 2 one-lane cells, 4 whole-wave cells, 8 everything behind P1) -- what a part costs in a scene
// that only exists after a thousand steps of the product's kernels.  Results are wrong while a bit is set.
__device__ uint32_t g_dbg_skip_rt;
#define GPE_RT_SKIP(bit) ((g_dbg_skip_rt & (bit)) != 0u)
#else
#define GPE_RT_SKIP(bit) false
#endif
#ifdef GPE_TILE_STAMPS
#define GPE_STAMP_BEGIN() long long _t_prev = clock64()
#define GPE_STAMP(i)                                                                  \
    do {                                                                              \
        if (A.stamps && threadIdx.x == 0 && (blockIdx.x & 127u) == 5u) {                  \
            const long long _t = clock64();                                           \
            atomicAdd(&A.stamps[i], (unsigned long long)(_t - _t_prev));              \
            atomicAdd(&A.stamps[16 + (i)], 1ull);                                      \
            _t_prev = _t;                                                             \
        }                                                                             \
    } while (0)
#else
#define GPE_STAMP_BEGIN() do {} while (0)
#define GPE_STAMP(i) do {} while (0)
#endif

// LID: a sharded run's windows also keep every particle's local index (4 bytes per slot): `id` then holds the order key
// the members are sorted by, and the write-back needs the local index again.
template <int T, int CAP, bool LID = false>
struct TileLds {
    static constexpr int TILE = T;
    static constexpr bool kGlobal = false;
    static constexpr bool kLid = LID;
    static constexpr int kSlots = CAP;                 // particles the window keeps
    uint32_t lid[LID ? CAP : 1];
    // The blocks of tile +- 8 cells are looked up (block granule), but only particles whose home cell lies in the
    // tile's dependency cone are kept -- 5 / 4 cells left / right of the tile, 3 / 2 below / above (see kConeLeft ...):
    // a third fewer particles in LDS at 32x32, and the window overflows that much later.
    static constexpr int HXL = kConeLeft + 1, HXR = kConeRight + 1, HYL = kConeDown + 1, HYR = kConeUp + 1;
    static constexpr int RWX = T + HXL + HXR, RWY = T + HYL + HYR;
    // The cell array carries a ring of one cell around the window: a kept particle's phantom cells then always have
    // a slot (home + a constant offset, no bounds tests).  Ring cells lie outside every colour's zone: never walked.
    static constexpr int PX = RWX + 2, PY = RWY + 2;
    static constexpr int NCELL = PX * PY;
    static constexpr int NB = (T + 2 * kHalo) / 8;
    static constexpr int NBLK = NB * NB;
    static constexpr int PER = (NCELL + kNatThreads - 1) / kNatThreads;   // cells per thread in the scan
    // Looked-up particles a window takes (P0 hands the tile on when its 3x3 / 4x4 / 6x6 blocks hold more, before any
    // gather): what the kept window holds at uniform density -- it keeps 66 % of what a 32x32 tile looks up, 51 % at
    // 16x16, 38 % at 8x8 -- plus a margin; a tile that passes this test and still keeps more than CAP is handed on
    // after the gather.  (Until the order-key windows kept their local indices this was bound to 1536 by an 11-bit
    // slot field: an 8x8 tile went to the spill arena at 590 kept particles.)  The 32x32 tile stays at 1536: in a
    // compressed scene its dense tiles are resolved faster as four quarters -- one crowded cell then holds up one
    // quarter's colour pass, not 512 threads' (100 M soak at step 1500: 22.9 ms with 1536, 22.2 with 1280, 24.3 /
    // 25.2 with 1700 / 1800 or 2048; profiles/r02/soak_1500_main_lookup_capacity.txt).
#ifndef GPE_QMAX_MAIN
#define GPE_QMAX_MAIN GPE_QMAX_MAIN_VALUE
#endif
    static constexpr int QMAX = T >= 32 ? GPE_QMAX_MAIN : (T >= 16 ? GPE_QMAX_MID : 8);
    static constexpr int RAWCAP = QMAX * kNatThreads;
    static_assert(NCELL < 2048, "hm packs home (11 bit) | overlap mask (8) | own (1)");
    static constexpr int QZ = (T + 8) * (T + 4) / 4;                      // cells of one colour inside its zone
    float px[CAP], py[CAP], rad[CAP];
    // (a radius per staged particle; TileDirect can do without: kUniform there)
    static constexpr bool kUniform = false;
    __device__ __forceinline__ float radius_of(const uint32_t s, const UniformRadii &) const { return rad[s]; }
    uint32_t id[CAP];
    uint32_t hm[CAP];          // bits 0-10 index of the home cell in the padded cell array; bits 11-18 overlap mask of
                               // the 8 neighbour cells (k_native_hash); bit 19 the home cell lies in the tile (the
                               // particle is the tile's own)
    __device__ __forceinline__ bool is_own(uint32_t s) const { return (hm[s] & (1u << 19)) != 0; }
    // cell[lc + 1]: members of cell lc (P1) -> first slot of its list (P2) -> one past its last slot (P3);
    // cell[0] = 0, so from P3 on the list of cell lc is mem[cell[lc] .. cell[lc + 1]).  Values stay below
    // 4 * CAP < 65536: two cells share a word (LDS atomics are 32 bit, so cell_inc adds 1 or 1 << 16 --
    // no carry can leave the low half), which buys 160 more particles per window than 32-bit cells.
    static_assert(4 * CAP < 65536, "cell offsets are 16 bit");
    union {
        uint32_t cellw[(NCELL + 2) / 2];
        uint16_t cellh[NCELL + 2];
    };
    __device__ __forceinline__ void cell_clear(int tid)
    {
        for (int i = tid; i < (NCELL + 2) / 2; i += kNatThreads) cellw[i] = 0;
    }
    __device__ __forceinline__ uint32_t cell_get(int i) const { return cellh[i]; }
    __device__ __forceinline__ void cell_set(int i, uint32_t v) { cellh[i] = (uint16_t)v; }
    __device__ __forceinline__ uint32_t cell_inc(int i)                // returns the value before the add
    {
        const uint32_t sh = (uint32_t)(i & 1) * 16u;
        return (atomicAdd(&cellw[i >> 1], 1u << sh) >> sh) & 0xFFFFu;
    }
    union {
        uint16_t mem[4 * CAP]; // member lists (local particle slots)
        uint8_t sblk[RAWCAP];  // P0-P1 only: region block a looked-up slot came from
        static_assert(RAWCAP <= 8 * CAP, "sblk fits under mem");
    };
    uint16_t list[4 * QZ];     // active cells, one segment per colour
    // cells of 9..64 members (piles): resolved by a whole wave each; WC per colour, the rest falls back to one lane
    static constexpr int WC = T >= 32 ? 16 : 64;
    uint16_t wlist[4 * WC];
    // cells of 9..16 members of the sub-tile windows: by the sixteen lanes of a DPP row (resolve_row), four per wave
    static constexpr bool kRows = T < 32;
    uint16_t rlist[kRows ? 4 * WC : 2];
    uint32_t lcnt[20];         // per colour: [c] cells resolved by one lane, [4 + c] by a lane group, [8 + c] by a wave, [12 + c] by a
                               // row; [16 + c] the ticket the waves draw whole-wave cells and quadruples of rows with
    // looked-up blocks; an order-key (sharded) window looks every block up twice: among the owned particles (the kept
    // table) and among the ghosts (their own table, rebuilt every step): virtual blocks [NBLK, 2 NBLK)
    static constexpr int VBMAX = (kLid || kGlobal) ? 2 * NBLK : NBLK;
    uint32_t bstart[VBMAX];
    uint32_t bcnt[VBMAX];
    uint32_t boff[VBMAX + 1];
    uint32_t s_w[16];
    uint32_t misc[4];
};

// Same window, but the per-particle arrays live in a slice of the global spill arena: for 8x8 tiles whose
// 24x24-cell region holds more particles than any LDS window stages (thousands of particles piled into a few
// cells).  Slow and rare; it exists so that the native path is exact for every input, not only for sparse ones.
template <int T>
struct TileGlobal {
    static constexpr int TILE = T;
    static constexpr bool kGlobal = true;
    static constexpr bool kLid = false;
    static constexpr int kSlots = 1;                   // (no per-lane own arrays: the write-back loops over the slots)
    // keeps every looked-up particle: slot == looked-up slot
    static constexpr int HXL = kHalo, HXR = kHalo, HYL = kHalo, HYR = kHalo;
    static constexpr int RWX = T + 2 * kHalo, RWY = T + 2 * kHalo;
    static constexpr int PX = RWX + 2, PY = RWY + 2;               // padded as in TileLds
    static constexpr int NCELL = PX * PY;
    static constexpr int NB = RWX / 8;
    static constexpr int NBLK = NB * NB;
    static constexpr int PER = (NCELL + kNatThreads - 1) / kNatThreads;
    static constexpr int QMAX = 1;
    static constexpr int QZ = (T + 8) * (T + 4) / 4;
    float *px, *py, *rad;
    static constexpr bool kUniform = false;
    __device__ __forceinline__ float radius_of(const uint32_t s, const UniformRadii &) const { return rad[s]; }
    uint32_t *id, *hm, *mem;
    uint8_t *sblk;
    uint32_t cell[NCELL + 1];      // 32-bit cells: the member count is not bounded by an LDS capacity here
    __device__ __forceinline__ void cell_clear(int tid)
    {
        for (int i = tid; i <= NCELL; i += kNatThreads) cell[i] = 0;
    }
    __device__ __forceinline__ uint32_t cell_get(int i) const { return cell[i]; }
    __device__ __forceinline__ void cell_set(int i, uint32_t v) { cell[i] = v; }
    __device__ __forceinline__ uint32_t cell_inc(int i) { return atomicAdd(&cell[i], 1u); }
    uint16_t list[4 * QZ];
    static constexpr int WC = 64;
    uint16_t wlist[4 * WC];
    static constexpr bool kRows = true;
    uint16_t rlist[4 * WC];
    uint32_t lcnt[20];         // per colour: [c] cells resolved by one lane, [4 + c] by a lane group, [8 + c] by a wave, [12 + c] by a
                               // row; [16 + c] the ticket the waves draw whole-wave cells and quadruples of rows with
    // looked-up blocks; an order-key (sharded) window looks every block up twice: among the owned particles (the kept
    // table) and among the ghosts (their own table, rebuilt every step): virtual blocks [NBLK, 2 NBLK)
    static constexpr int VBMAX = (kLid || kGlobal) ? 2 * NBLK : NBLK;
    uint32_t bstart[VBMAX];
    uint32_t bcnt[VBMAX];
    uint32_t boff[VBMAX + 1];
    uint32_t s_w[16];
    uint32_t misc[4];
};

// Members of one cell into ascending object index (the order the reference's stable sort gives them).
template <class L>
__device__ __forceinline__ void sort_members(L &S, const uint32_t b, const uint32_t e)
{
    const uint32_t n = e - b;
    if (n == 2) {
        const uint32_t m0 = S.mem[b], m1 = S.mem[b + 1];
        if (S.id[m0] > S.id[m1]) { S.mem[b] = m1; S.mem[b + 1] = m0; }
        return;
    }
    if (n == 3) {
        uint32_t m0 = S.mem[b], m1 = S.mem[b + 1], m2 = S.mem[b + 2];
        uint32_t i0 = S.id[m0], i1 = S.id[m1], i2 = S.id[m2];
        bool ch = false;
        if (i0 > i1) { uint32_t t = m0; m0 = m1; m1 = t; uint32_t u = i0; i0 = i1; i1 = u; ch = true; }
        if (i1 > i2) { uint32_t t = m1; m1 = m2; m2 = t; uint32_t u = i1; i1 = i2; i2 = u; ch = true; }
        if (i0 > i1) { uint32_t t = m0; m0 = m1; m1 = t; ch = true; }
        if (ch) { S.mem[b] = m0; S.mem[b + 1] = m1; S.mem[b + 2] = m2; }
        return;
    }
    if (n <= 8) {
        // 4..8 members: rank count (ids are distinct) -- two LDS round trips whatever the order, where an
        // insertion sort walks a dependent LDS chain per element; the colour pass waits for its slowest cell
        constexpr int M = 8;
        uint32_t slot[M], id[M];
#pragma unroll
        for (int k = 0; k < M; ++k) slot[k] = ((uint32_t)k < n) ? (uint32_t)S.mem[b + k] : 0u;
#pragma unroll
        for (int k = 0; k < M; ++k) id[k] = ((uint32_t)k < n) ? S.id[slot[k]] : 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            uint32_t rank = 0;
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (j != k) rank += (id[j] < id[k]) ? 1u : 0u;
            if ((uint32_t)k < n && rank != (uint32_t)k) S.mem[b + rank] = slot[k];
        }
        return;
    }
    for (uint32_t i = b + 1; i < e; ++i) {                             // insertion sort
        const uint32_t x = S.mem[i];
        const uint32_t kx = S.id[x];
        uint32_t j = i;
        while (j > b && S.id[S.mem[j - 1]] > kx) { S.mem[j] = S.mem[j - 1]; --j; }
        S.mem[j] = x;
    }
}

// One pair, in the form the window's layout L asks for: a layout without a radius array (L::kUniform, TileDirect) takes
// the uniform pair_response with the kernel's UniformRadii; every other layout the general one with the two radii its
// resolver read (S.radius_of) and the `plain` vote (plain_lanes).  The resolvers below are written once for both.
template <class L>
__device__ __forceinline__ uint64_t plain_lanes(const float r)
{
    if constexpr (L::kUniform) return 0ull; else return plain_radius_lanes(r);
}
template <class L, bool BOTH = true>
__device__ __forceinline__ uint64_t respond(const uint64_t active, f32x2 &p1, std::conditional_t<BOTH, f32x2 &, const f32x2 &> p2,
                                            const float r1, const float r2, const uint64_t plain, const UniformRadii &U,
                                            const float stiffness, const uint64_t lower = ~0ull, const uint64_t careful = 0)
{
    if constexpr (L::kUniform) return pair_response<BOTH>(active, p1, p2, U, stiffness, lower, careful);
    else return pair_response<BOTH>(active, p1, p2, r1, r2, plain, stiffness, lower, careful);
}

// The reference's pair resolution (collision_solver.wgsl:66-118), on LDS-resident positions: one lane walks the
// pairs (a, b), a < b, of its cell.  Bit-exact restatements that shorten the dependent chain:
//  * the next partner's position is fetched while the current pair is computed: within one `a` loop every pair
//    touches a different partner, so that position cannot change in between;
//  * see pair_response for the arithmetic.
// (Called under divergent control flow -- the lanes walk cells of different sizes: the votes cover the lanes that are
// in the same iteration.)
template <class L>
__device__ __forceinline__ void resolve_cell(L &S, const uint32_t b, const uint32_t e, const float stiffness, const UniformRadii &U)
{
    for (uint32_t ia = b; ia + 1 < e; ++ia) {                         // :68
        const uint32_t a = S.mem[ia];
        uint32_t nb = S.mem[ia + 1];
        f32x2 p1 = {S.px[a], S.py[a]};
        const float r1 = S.radius_of(a, U);
        f32x2 nxt = {S.px[nb], S.py[nb]};
        float nr = S.radius_of(nb, U);
        const uint64_t plain = plain_lanes<L>(r1);
        bool dirty = false;
        for (uint32_t ib = ia + 1; ib < e; ++ib) {                    // :77
            const uint32_t bb = nb;
            f32x2 p2 = nxt;                                           // :86 live position
            const float r2 = nr;
            if (ib + 1 < e) { nb = S.mem[ib + 1]; nxt = (f32x2){S.px[nb], S.py[nb]}; nr = S.radius_of(nb, U); }
            const uint64_t hit = respond<L>(ballot64(true), p1, p2, r1, r2, plain, U, stiffness);
            if (hit != 0) {
                if (lanes_of(hit)) { S.px[bb] = p2.x; S.py[bb] = p2.y; dirty = true; }
            }
        }
        if (dirty) { S.px[a] = p1.x; S.py[a] = p1.y; }
    }
}

// The one-lane cells of a wave -- 2 or 3 members, rarely a pile the wave list had no room for -- as straight-line
// code on registers: slots in one LDS round trip, ids / positions / radii in a second, a three-element sorting
// network (ascending object index, collision_solver.wgsl:66-118; a cell of two needs none: the response is symmetric
// under exchanging the particles -- v -> -v negates the correction exactly, sums and products commute), the pairs
// (0,1), (0,2), (1,2) back to back with pair_response's wave-uniform early-outs, the moved positions stored at the
// end.  The general loop (resolve_cell) walked the same pairs through two nested loops with an LDS round trip per
// partner: ~60 wave instructions and five dependent round trips more per pass.
// `on`, `n <= 3` ... must reach this function as comparisons (they are voted on one by one, see pair_response).
template <class L>
__device__ __forceinline__ void resolve_small_cells(L &S, const bool on, const uint32_t b, const uint32_t n,
                                                    const float stiffness, const UniformRadii &U)
{
    const uint64_t on_m = ballot64(on);
    const uint64_t small_m = on_m & ballot64(n <= 3u), three_m = on_m & ballot64(n == 3u);
    const bool small = lanes_of(small_m), three = lanes_of(three_m);
    uint32_t m0 = 0, m1 = 0, m2 = 0;
    if (small) { m0 = S.mem[b]; m1 = S.mem[b + 1]; m2 = three ? (uint32_t)S.mem[b + 2] : m1; }
    uint32_t i0 = 0, i1 = 1, i2 = 2;
    f32x2 p0 = {0.f, 0.f}, p1 = {3.f, 3.f}, p2 = {6.f, 6.f};
    float r0 = 1.f, r1 = 1.f, r2 = 1.f;
    const bool any3 = three_m != 0;                                    // wave-uniform
    // The three-element network on (object index, slot) only; positions and radii are loaded by the ordered slots
    // afterwards: 10 selects instead of the 28 that ordered positions and radii as well, for one more LDS round trip in a
    // wave that holds a cell of three (round 4: -27 VALU lane-slots per particle, -1.5 % at every size).
    if (any3) {
        if (three) { i0 = S.id[m0]; i1 = S.id[m1]; i2 = S.id[m2]; }
#define GPE_CSWAP(A, B)                                                                                       \
        {                                                                                                     \
            const bool sw = lanes_of(three_m & ballot64(i##A > i##B));                                        \
            const uint32_t ta = sw ? i##B : i##A, tb = sw ? i##A : i##B, ma = sw ? m##B : m##A, mb = sw ? m##A : m##B; \
            i##A = ta; i##B = tb; m##A = ma; m##B = mb;                                                       \
        }
        GPE_CSWAP(0, 1) GPE_CSWAP(1, 2) GPE_CSWAP(0, 1)
#undef GPE_CSWAP
    }
    if (small) {
        p0 = (f32x2){S.px[m0], S.py[m0]}; r0 = S.radius_of(m0, U);
        p1 = (f32x2){S.px[m1], S.py[m1]}; r1 = S.radius_of(m1, U);
    }
    if (any3) {
        if (three) { p2 = (f32x2){S.px[m2], S.py[m2]}; r2 = S.radius_of(m2, U); }
    }
    const uint64_t plain0 = plain_lanes<L>(r0);
    uint64_t h01 = 0, h02 = 0, h12 = 0;
    h01 = respond<L>(small_m, p0, p1, r0, r1, plain0, U, stiffness);
    if (any3) {
        h02 = respond<L>(three_m, p0, p2, r0, r2, plain0, U, stiffness);
        h12 = respond<L>(three_m, p1, p2, r1, r2, plain_lanes<L>(r1), U, stiffness);
    }
    if ((h01 | h02 | h12) != 0) {                                      // wave-uniform
        if (lanes_of(h01 | h02)) { S.px[m0] = p0.x; S.py[m0] = p0.y; }
        if (lanes_of(h01 | h12)) { S.px[m1] = p1.x; S.py[m1] = p1.y; }
        if (lanes_of(h02 | h12)) { S.px[m2] = p2.x; S.py[m2] = p2.y; }
    }
    if (on && n > 3u) {                                                // a pile in the one-lane list: the general walk
        sort_members(S, b, b + n);
        resolve_cell(S, b, b + n, stiffness, U);
    }
}

// A cell of 4..8 members resolved by kGroupLanes consecutive lanes of one wave.  The reference's pair sequence
// (a, b), a < b in ascending object index (:68-118) only orders pairs that share a particle; pair (a, b) can
// run as soon as (a, b-1) and (a-1, b) are done, i.e. at step s = a + b of a wavefront schedule (s = 1 .. 2n - 3)
// -- 2n - 3 steps instead of n (n-1) / 2, every particle still seeing its updates in the reference's order.
// Lane a of the group owns particle a (registers) for the whole walk.  At step s its partner is particle s - a: the
// two lanes of a pair each fetch the other's live position and radius through two DPP moves -- the reflection
// i <-> s - i of an 8-lane group is row_half_mirror (i <-> 7 - i) followed by a row shift by |7 - s|, both fixed at
// compile time because the steps are unrolled -- and EACH COMPUTES ITS OWN HALF of the response as "particle 1".
// That is exact: seen from the other side v is negated, and negation commutes with every operation of the chain
// (squares and the distance are the same; products, the fused refinement steps and the final addition are odd in v;
// r1 + r2 and inv1 + inv2 commute), so lane b's p_b + (-c) w_b is the reference's p_b - c w_b bit for bit -- the
// symmetry the two-member cells already rely on.  (Rounds 1-3 moved the visitors through the lanes instead: a pipe up,
// a feed pipe down and their bookkeeping -- seven DPP moves and as many selects per step, and both halves of every
// response in one lane.  The steps mostly stop at the candidate test, so their fixed cost is what a group costs.)
// No LDS access inside the walk.  A colour pass lasts as long as its slowest cell: this is what shortens it.
constexpr uint32_t kGroupLanes = 8, kGroupMin = 4;
template <int CTRL>
__device__ __forceinline__ float dpp_mov(const float v)
{
    // (bound_ctrl: a source lane outside the row, or switched off, reads as 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
constexpr int kDppHalfMirror = 0x141;
// the value lane (S - i) of the 8-lane group holds, given the group's half-mirrored values (lane i holds lane 7 - i's)
template <int S>
__device__ __forceinline__ float dpp_reflect_from_mirrored(const float m)
{
    if constexpr (S < 7) return dpp_mov<0x100 + (7 - S)>(m);          // row_shl: lane i reads lane i + (7 - S)
    else if constexpr (S > 7) return dpp_mov<0x110 + (S - 7)>(m);     // row_shr: lane i reads lane i - (S - 7)
    else return m;
}
// lanes whose partner at step S can exist at all: 0 <= S - a, S - a != a  (a = lane mod 8)
template <int S, bool LOWER = false>
constexpr uint64_t group_step_lanes()
{
    uint64_t m = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const int a = lane & 7;
        if (a <= S && 2 * a != S && (!LOWER || 2 * a < S)) m |= 1ull << lane;
    }
    return m;
}
template <int S, int SMAX, class F>
__device__ __forceinline__ void for_each_group_step(F &&f)
{
    f(std::integral_constant<int, S>{});
    if constexpr (S < SMAX) for_each_group_step<S + 1, SMAX>(f);
}
// NMAX: the most members a group cell of this window form can have
template <int NMAX, class L>
__device__ __forceinline__ void resolve_group(L &S, const uint32_t b, const uint32_t n, const int a,
                                              const float stiffness, const UniformRadii &U)
{
    static_assert(NMAX >= (int)kGroupMin && NMAX <= (int)kGroupLanes, "group cells: 4 .. 8 members");
    const int group_base = lane_id() & ~((int)kGroupLanes - 1);
    // order the members: rank = members with a smaller object index (they are distinct)
    const uint64_t has_m = ballot64((uint32_t)a < n);
    const bool has = lanes_of(has_m);
    const uint32_t my_slot = has ? (uint32_t)S.mem[b + a] : 0u;
    const uint32_t my_id = has ? S.id[my_slot] : 0xFFFFFFFFu;
    uint32_t rank = 0;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) rank += ((uint32_t)__shfl((int)my_id, i, kGroupLanes) < my_id) ? 1u : 0u;
    // forward permute: lane r receives the slot of the member of rank r
    const uint32_t a_slot = (uint32_t)__builtin_amdgcn_ds_permute((group_base + (int)(has ? rank : (uint32_t)a)) << 2,
                                                                  (int)my_slot);
    f32x2 o = {0.f, 0.f};                                             // step-start state of the lane's particle
    float r1 = 1.f;
    if (has) { o = (f32x2){S.px[a_slot], S.py[a_slot]}; r1 = S.radius_of(a_slot, U); }
    f32x2 p1 = o;
    const uint64_t plain = plain_lanes<L>(r1);
    const uint64_t careful = neg_zero_lanes(p1);                      // (see pair_response<false>)
    float r_mirrored = 0.f;                                           // (one radius for all: no partner's radius to fetch)
    if constexpr (!L::kUniform) r_mirrored = dpp_mov<kDppHalfMirror>(r1);
    const uint32_t n_plus_a = n + (uint32_t)a;                        // partner s - a exists while s - a < n
    // how long the longest schedule of the wave is (the cells of a wave differ): steps beyond 2 * 4 - 3 are skipped
    // by a scalar test unless some cell has the members for them
    const uint64_t any5 = has_m & ballot64(n >= 5u), any6 = has_m & ballot64(n >= 6u), any7 = has_m & ballot64(n >= 7u),
                   any8 = has_m & ballot64(n >= 8u);
    for_each_group_step<1, 2 * NMAX - 3>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int need = (s + 4) / 2;                              // smallest n with 2n - 3 >= s
        if constexpr (need >= 5) {
            const uint64_t any = need == 5 ? any5 : (need == 6 ? any6 : (need == 7 ? any7 : any8));
            if (any == 0) return;                                      // wave-uniform
        }
        const f32x2 ip = {dpp_reflect_from_mirrored<s>(dpp_mov<kDppHalfMirror>(p1.x)),
                          dpp_reflect_from_mirrored<s>(dpp_mov<kDppHalfMirror>(p1.y))};
        float ir = 0.f;
        if constexpr (!L::kUniform) ir = dpp_reflect_from_mirrored<s>(r_mirrored);
        constexpr uint64_t kStepLanes = group_step_lanes<s>();
        const uint64_t pairing = has_m & kStepLanes & ballot64((uint32_t)s < n_plus_a);
        constexpr uint64_t kLower = group_step_lanes<s, true>();      // (the lane with the smaller index of each pair)
        (void)respond<L, false>(pairing, p1, ip, r1, ir, plain, U, stiffness, kLower, careful);
    });
    if (has && (__float_as_uint(p1.x) != __float_as_uint(o.x) || __float_as_uint(p1.y) != __float_as_uint(o.y))) {
        S.px[a_slot] = p1.x;
        S.py[a_slot] = p1.y;
    }
}

// A cell of 9..16 members resolved by the sixteen lanes of one DPP row: the symmetric walk of resolve_group at twice the
// width -- the reflection i <-> s - i of a row is row_mirror (i <-> 15 - i) followed by a row shift by |15 - s| -- four
// cells per wave side by side, 2n - 3 steps of one half-response each.  (Until round 4 these cells went to resolve_wave,
// one cell per wave, 2n - 2 steps of a whole response and seven wave-wide shifts each: ~15 k cycles for eleven members,
// and a colour pass of a compressed region's window waits for its slowest wave; phase stamps in profiles/r04.)
constexpr uint32_t kRowLanes = 16;
constexpr int kDppRowMirror = 0x140;
template <int S>
__device__ __forceinline__ float dpp_reflect_from_row_mirrored(const float m)
{
    if constexpr (S < 15) return dpp_mov<0x100 + (15 - S)>(m);        // row_shl: lane i reads lane i + (15 - S)
    else if constexpr (S > 15) return dpp_mov<0x110 + (S - 15)>(m);   // row_shr: lane i reads lane i - (S - 15)
    else return m;
}
template <int S, bool LOWER = false>
constexpr uint64_t row_step_lanes()
{
    uint64_t m = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const int a = lane & 15;
        if (a <= S && 2 * a != S && (!LOWER || 2 * a < S)) m |= 1ull << lane;
    }
    return m;
}
template <int K>
__device__ __forceinline__ uint32_t row_rotated(const uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + K /* row_ror:K */, 0xF, 0xF, false);
}
template <int K, int KMAX>
__device__ __forceinline__ uint32_t row_rank(const uint32_t id)
{
    const uint32_t r = row_rotated<K>(id) < id ? 1u : 0u;
    if constexpr (K < KMAX) return r + row_rank<K + 1, KMAX>(id); else return r;
}
// every lane of the wave calls (n == 0: no cell in this row); a = lane & 15
template <class L>
__device__ __forceinline__ void resolve_row(L &S, const uint32_t b, const uint32_t n, const int a, const float stiffness,
                                            const UniformRadii &U)
{
    const int row_base = lane_id() & ~((int)kRowLanes - 1);
    const uint64_t has_m = ballot64((uint32_t)a < n);
    const bool has = lanes_of(has_m);
    const uint32_t my_slot = has ? (uint32_t)S.mem[b + a] : 0u;
    const uint32_t my_id = has ? S.id[my_slot] : 0xFFFFFFFFu;
    // rank = members of the row with a smaller object index (distinct; lanes without a member hold the largest value)
    const uint32_t rank = row_rank<1, (int)kRowLanes - 1>(my_id);
    const uint32_t a_slot = (uint32_t)__builtin_amdgcn_ds_permute((row_base + (int)(has ? rank : (uint32_t)a)) << 2, (int)my_slot);
    f32x2 o = {0.f, 0.f};
    float r1 = 1.f;
    if (has) { o = (f32x2){S.px[a_slot], S.py[a_slot]}; r1 = S.radius_of(a_slot, U); }
    f32x2 p1 = o;
    const uint64_t plain = plain_lanes<L>(r1);
    const uint64_t careful = neg_zero_lanes(p1);                      // (see pair_response<false>)
    float r_mirrored = 0.f;
    if constexpr (!L::kUniform) r_mirrored = dpp_mov<kDppRowMirror>(r1);
    const uint32_t n_plus_a = n + (uint32_t)a;                        // partner s - a exists while s - a < n
    for_each_group_step<1, 2 * (int)kRowLanes - 3>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int need = (s + 4) / 2;                              // smallest n with 2n - 3 >= s
        if constexpr (need >= 10) {
            if ((has_m & ballot64(n >= (uint32_t)need)) == 0) return;  // wave-uniform: no row of the wave is that long
        }
        const f32x2 ip = {dpp_reflect_from_row_mirrored<s>(dpp_mov<kDppRowMirror>(p1.x)),
                          dpp_reflect_from_row_mirrored<s>(dpp_mov<kDppRowMirror>(p1.y))};
        float ir = 0.f;
        if constexpr (!L::kUniform) ir = dpp_reflect_from_row_mirrored<s>(r_mirrored);
        constexpr uint64_t kStepLanes = row_step_lanes<s>();
        const uint64_t pairing = has_m & kStepLanes & ballot64((uint32_t)s < n_plus_a);
        constexpr uint64_t kLower = row_step_lanes<s, true>();
        (void)respond<L, false>(pairing, p1, ip, r1, ir, plain, U, stiffness, kLower, careful);
    });
    if (has && (__float_as_uint(p1.x) != __float_as_uint(o.x) || __float_as_uint(p1.y) != __float_as_uint(o.y))) {
        S.px[a_slot] = p1.x;
        S.py[a_slot] = p1.y;
    }
}

// A cell of 9..64 members (a pile: particles pressed into one cell) resolved by a whole wave: the systolic array
// of resolve_group over 64 lanes (wave-wide DPP shifts).  One lane would walk n (n - 1) / 2 pairs one after the
// other -- 1225 for 50 members, ~0.25 ms, which every colour pass of every tile near the pile would wait for; the
// wavefront schedule takes 2 n - 3 steps.  Same operations per particle in the same order, so the same bits.
__device__ __forceinline__ float wave_from_lane_below(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xF, 0xF, true));
}
__device__ __forceinline__ int wave_from_lane_below(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, true);
}
__device__ __forceinline__ float wave_from_lane_above(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xF, 0xF, true));
}
__device__ __forceinline__ f32x2 wave_from_lane_below(f32x2 v) { return (f32x2){wave_from_lane_below(v.x), wave_from_lane_below(v.y)}; }
__device__ __forceinline__ f32x2 wave_from_lane_above(f32x2 v) { return (f32x2){wave_from_lane_above(v.x), wave_from_lane_above(v.y)}; }
template <class L>
__device__ __forceinline__ void resolve_wave(L &S, const uint32_t b, const uint32_t n, const float stiffness, const UniformRadii &U)
{
    const int a = lane_id();
    const uint64_t has_m = ballot64((uint32_t)a < n);
    const bool has = lanes_of(has_m);
    const uint32_t my_slot = has ? (uint32_t)S.mem[b + a] : 0u;
    const uint32_t my_id = has ? S.id[my_slot] : 0xFFFFFFFFu;
    uint32_t rank = 0;
    for (int i = 0; i < (int)n; ++i)                                    // n is wave-uniform: v_readlane
        rank += ((uint32_t)__builtin_amdgcn_readlane((int)my_id, i) < my_id) ? 1u : 0u;
    const uint32_t a_slot = (uint32_t)__builtin_amdgcn_ds_permute((int)(has ? rank : (uint32_t)a) << 2, (int)my_slot);
    f32x2 o = {0.f, 0.f};
    float r1 = 1.f;
    if (has) { o = (f32x2){S.px[a_slot], S.py[a_slot]}; r1 = S.radius_of(a_slot, U); }
    f32x2 p1 = o;
    const uint64_t plain = plain_lanes<L>(r1);
    f32x2 qp = {0.f, 0.f};
    float qr = 1.f;
    int qb = -1;
    const int last = 2 * (int)n - 3;
    const bool first = a == 0;
    f32x2 fp = wave_from_lane_above(o);
    float fr = 1.f;                                                    // (the radii travel with the positions unless all are one)
    if constexpr (!L::kUniform) fr = wave_from_lane_above(r1);
    for (int t = 0; t <= last; ++t) {
        f32x2 ip = wave_from_lane_below(qp);
        float ir = 1.f;
        if constexpr (!L::kUniform) ir = wave_from_lane_below(qr);
        int ib = wave_from_lane_below(qb);
        if (first) { ip = fp; ir = fr; ib = (t + 1 < (int)n) ? t + 1 : -1; }
        fp = wave_from_lane_above(fp);
        if constexpr (!L::kUniform) fr = wave_from_lane_above(fr);
        if (ib == a) p1 = ip;                                          // the lane's own particle has arrived
        const uint64_t pairing_m = has_m & ballot64(ib > a);
        (void)respond<L>(pairing_m, p1, ip, r1, ir, plain, U, stiffness);
        // (what a lane without a pair passes on is marked "none" and never looked at)
        qp = ip; qr = ir; qb = lanes_of(pairing_m) ? ib : -1;
    }
    if (has && (__float_as_uint(p1.x) != __float_as_uint(o.x) || __float_as_uint(p1.y) != __float_as_uint(o.y))) {
        S.px[a_slot] = p1.x;
        S.py[a_slot] = p1.y;
    }
}

// Cells of 65..256 members (a crushed pile), sub-tile and spill windows only: one wave walks the pair matrix in
// 64 x 64 blocks, block row by block row.  The reference order -- pairs (a, b), a < b, ascending -- only constrains
// pairs that share a particle: (a, b) needs (a, b-1) and (a-1, b).  Diagonal block I: resolve_wave on chunk I.
// Block (I, J), J > I: the 64 owners of chunk I sit in the lanes (registers, for the whole block row), the members
// of chunk J enter at lane 0 one per step, meet one owner per step on their way up the lanes, and are stored back
// when they leave the last owner's lane: 64 + |J| - 1 steps.  Row-major block order gives every pair its two
// predecessors, so every particle sees its updates in the reference's order: same bits, ~n^2/64 steps instead
// of n (n - 1) / 2 pairs in one lane.
// (Up to 1024 members since round 4: by step 2000 of the 100 M gravity-on scene the two floor corners hold cells of 330,
// by step 2450 of 600 members; beyond this limit a cell falls to ONE lane -- 180 k pairs one after the other, each with
// the spill window's global round trips in its chain: one such tile took 107 M cycles, 2.7 x the over-capacity launch's
// whole balanced duration; profiles/r04/tile_cycles_tail.txt.)
constexpr uint32_t kWaveCellMax = 1024;
template <class L>
__device__ __forceinline__ void resolve_wave_blocked(L &S, const uint32_t b, const uint32_t n, const float stiffness,
                                                     const UniformRadii &U)
{
    const int a = lane_id();
    constexpr int K = (int)kWaveCellMax / 64;
    const uint32_t chunks = (n + 63u) / 64u;
    // members into ascending object index: rank count over the whole cell, up to sixteen members per lane; the rank
    // rides in the slot word's upper bits (slots stay below 2^22: P4 sends no cell of a larger window here)
    {
        constexpr uint32_t kRankOne = 1u << 22;
        uint32_t pk[K], id[K];
        // (branch-free: a lane without a member in chunk k re-reads the cell's first member and discards it -- behind
        // per-chunk branches hipcc kept sixteen copies of the two arrays alive and spilled them)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t m = (uint32_t)a + 64u * k;
            pk[k] = (uint32_t)S.mem[b + (m < n ? m : 0u)];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t m = (uint32_t)a + 64u * k;
            const uint32_t v = S.id[pk[k]];
            id[k] = m < n ? v : 0xFFFFFFFFu;
        }
#pragma unroll 1
        for (uint32_t kk = 0; kk < chunks; ++kk) {
            // (one copy of the loops: the chunk's ids by a chain of selects on the wave-uniform kk, not sixteen unrolled
            // bodies -- that form doubled the kernel's code and left its register arrays in scratch)
            uint32_t cur = id[0];
#pragma unroll
            for (int k = 1; k < K; ++k) cur = kk == (uint32_t)k ? id[k] : cur;
            const int lim = (int)min(64u, n - 64u * kk);                  // wave-uniform
#pragma unroll 1
            for (int i = 0; i < lim; ++i) {
                const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)cur, i);
#pragma unroll
                for (int k = 0; k < K; ++k) pk[k] += other < id[k] ? kRankOne : 0u;
            }
        }
        wave_lds_order();                                              // every read of mem above precedes the writes
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((uint32_t)a + 64u * k < n) S.mem[b + (pk[k] >> 22)] = pk[k] & (kRankOne - 1u);
        wave_lds_order();
    }
    for (uint32_t I = 0; I < chunks; ++I) {
        const uint32_t bI = b + 64u * I, cI = min(64u, n - 64u * I);
        resolve_wave(S, bI, cI, stiffness, U);                         // pairs inside chunk I (it re-ranks: already sorted)
        if (I + 1 == chunks) break;
        wave_lds_order();
        // the owners of this block row
        const uint64_t has_m = ballot64((uint32_t)a < cI);
        const bool has = lanes_of(has_m);
        const uint32_t o_slot = has ? (uint32_t)S.mem[bI + a] : 0u;
        f32x2 p1 = {0.f, 0.f};
        float r1 = 1.f;
        if (has) { p1 = (f32x2){S.px[o_slot], S.py[o_slot]}; r1 = S.radius_of(o_slot, U); }
        const f32x2 o = p1;
        const uint64_t plain = plain_lanes<L>(r1);
        const bool first = a == 0;
        for (uint32_t J = I + 1; J < chunks; ++J) {
            const uint32_t bJ = b + 64u * J, cJ = min(64u, n - 64u * J);
            // the visitors of chunk J: fetched by the 64 lanes at once, handed to lane 0 one per step with v_readlane
            // (a spill window keeps its arrays in global memory: fetched by lane 0 one step ahead, as until round 4,
            // every step waited for two dependent global round trips)
            int vs = 0;
            f32x2 vp = {0.f, 0.f};
            float vr = 1.f;
            if ((uint32_t)a < cJ) { vs = (int)S.mem[bJ + a]; vp = (f32x2){S.px[vs], S.py[vs]}; vr = S.radius_of((uint32_t)vs, U); }
            f32x2 qp = {0.f, 0.f};
            float qr = 1.f;
            int qb = -1, qs = 0;
            const int steps = (int)(cI + cJ) - 1;
            for (int t = 0; t < steps; ++t) {
                f32x2 ip = wave_from_lane_below(qp);
                float ir = wave_from_lane_below(qr);
                int ib = wave_from_lane_below(qb), is = wave_from_lane_below(qs);
                const int tv = t & 63;                                 // (t >= cJ: no visitor enters, the values are unused)
                const f32x2 np = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(vp.x), tv)),
                                  __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vp.y), tv))};
                const float nr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vr), tv));
                const int ns = __builtin_amdgcn_readlane(vs, tv);
                if (first) {
                    ip = np; ir = nr; is = ns;
                    ib = t < (int)cJ ? t : -1;
                }
                const uint64_t pairing_m = has_m & ballot64(ib >= 0);
                (void)respond<L>(pairing_m, p1, ip, r1, ir, plain, U, stiffness);
                const bool pairing = lanes_of(pairing_m);
                // the visitor leaves the block behind the last owner: store it (it may have been moved by lower
                // lanes; an unchanged store is harmless)
                if (pairing && (uint32_t)a + 1u == cI) { S.px[is] = ip.x; S.py[is] = ip.y; }
                qp = ip; qr = ir; qb = pairing ? ib : -1; qs = is;
            }
            wave_lds_order();
        }
        if (has && (__float_as_uint(p1.x) != __float_as_uint(o.x) || __float_as_uint(p1.y) != __float_as_uint(o.y))) {
            S.px[o_slot] = p1.x;
            S.py[o_slot] = p1.y;
        }
        wave_lds_order();
    }
}

// Offset of neighbour k (grid.wgsl:68-90 scan order: y outer, x inner, centre skipped) in a cell array of row
// stride PX, eight signed bytes packed into one constant.
template <int PX>
__device__ __forceinline__ int neighbour_offset(const int k)
{
    static_assert(PX + 1 < 128, "offsets fit a signed byte");
    constexpr unsigned long long packed =
        ((unsigned long long)(uint8_t)(int8_t)(-PX - 1)) | ((unsigned long long)(uint8_t)(int8_t)(-PX) << 8) |
        ((unsigned long long)(uint8_t)(int8_t)(-PX + 1) << 16) | ((unsigned long long)(uint8_t)(int8_t)(-1) << 24) |
        ((unsigned long long)(uint8_t)(int8_t)(1) << 32) | ((unsigned long long)(uint8_t)(int8_t)(PX - 1) << 40) |
        ((unsigned long long)(uint8_t)(int8_t)(PX) << 48) | ((unsigned long long)(uint8_t)(int8_t)(PX + 1) << 56);
    return (int)(int8_t)(uint8_t)(packed >> (8 * k));
}

// a * B + c for a, c < 2^24 and a small constant B, as the one full-rate v_mad_u32_u24.  (Written out: __umul24 does not
// survive where the compiler has proved its operands small -- it drops the 24-bit form for a plain multiply, and the
// instruction selector, which does not know the range any more, emits the quarter-rate v_mul_lo_u32.)
template <int B>
__device__ __forceinline__ uint32_t mad_u24(const uint32_t a, const uint32_t c)
{
    static_assert(B >= 0 && B <= 64, "an inline constant");
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(B), "v"(c));
    return r;
}

// The wave's first thread, as a scalar: what a wave compares to skip, by a scalar branch, a round in which none of its
// lanes has work -- an idle wave then issues nothing, where lane predicates alone leave it the whole straight-line body.
__device__ __forceinline__ uint32_t wave_first_thread(const int tid)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63);
}

// Consecutive slots for the particles a wave keeps (`mask`: the lanes that keep theirs, one mask per round of the gather):
// one atomic on the counter word per wave, by lane 0 -- the order of the slots is free.  A slot at or beyond `cap` is not
// kept; the counter then tells the tile that it ran over.  (Both tile forms, gather and list intake: the kernels this
// changed were timed against their parent, profiles/tile_phases/.)
template <int Q>
__device__ __forceinline__ void take_slots(uint32_t *counter, const int lane, const uint32_t cap, const uint64_t (&mask)[Q],
                                           uint32_t (&slot)[Q], bool (&keep)[Q])
{
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) cnt += (uint32_t)__popcll(mask[q]);
    uint32_t base = 0;
    if (lane == 0 && cnt) base = atomicAdd(counter, cnt);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        slot[q] = base + popc_below_lane(mask[q]);
        base += (uint32_t)__popcll(mask[q]);
        keep[q] = keep[q] && slot[q] < cap;
    }
}
__device__ __forceinline__ uint32_t take_slots(uint32_t *counter, const int lane, const uint32_t cap, const uint64_t mask, bool &keep)
{
    const uint64_t m[1] = {mask};
    uint32_t slot[1];
    bool k[1] = {keep};
    take_slots(counter, lane, cap, m, slot, k);
    keep = k[0];
    return slot[0];
}

// P1 of the counting-sort windows, one staged particle the window keeps: its arrays, the count of its home cell, and of
// up to three phantom cells.
template <class L>
__device__ __forceinline__ void file_kept(L &S, const uint32_t s, const float2 pp, const float pr, const uint32_t pid, const uint32_t lid,
                                          const int lx, const int ly, const uint32_t code)
{
    constexpr int T = L::TILE, HX = L::HXL, HY = L::HYL, PX = L::PX;
    S.px[s] = pp.x; S.py[s] = pp.y; S.rad[s] = pr; S.id[s] = pid;
    if constexpr (L::kLid) S.lid[s] = lid;
    const int home = (ly + 1) * PX + lx + 1;                          // index in the padded cell array
    S.cell_inc(home + 1);
    // phantom cells: the first three set bits of the overlap mask (grid.wgsl:68-90 keeps at most three)
    uint32_t over = (code >> kCodeOverlapShift) & 0xFFu;
    const uint32_t own = (lx >= HX && lx < HX + T && ly >= HY && ly < HY + T) ? (1u << 19) : 0u;
    S.hm[s] = (uint32_t)home | (over << 11) | own;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (over == 0) break;
        const int k = __ffs((int)over) - 1;
        over &= over - 1u;
        S.cell_inc(home + neighbour_offset<PX>(k) + 1);               // (always inside the padded array)
    }
}
// ... and one the spill window does not keep.  The spill window's slots are the looked-up slots (the stragglers and the
// listed ghosts sit behind them): a particle that has drifted out of the looked-up region (it is listed under its old
// block) still owns one.  Filed under ring cell 0 -- outside every colour's zone, never walked, never written back -- so
// that the loops over the slots find a valid entry.
template <class L>
__device__ __forceinline__ void file_dropped(L &S, const uint32_t s, const float2 pp, const float pr, const uint32_t pid)
{
    S.px[s] = pp.x; S.py[s] = pp.y; S.rad[s] = pr; S.id[s] = pid;
    S.cell_inc(0 + 1);
    S.hm[s] = 0u;
}

// The tile's own particles (S.is_own) and, when K12 is fused into the write-back, their previous positions, into one
// register per round of NT slots.  Branch-free like the gather of P1: every lane loads -- a lane without a particle of
// the tile reads element 0 -- and the loads of all rounds are issued before anything uses one of them, so they are in
// flight together and nothing waits for them before write_own_back.  Rounds from QSKIP on are skipped by a scalar test,
// wave by wave, when the window holds no slot for the wave in them (PS >= 1): a wave whose slots of the round all lie
// beyond PS issues nothing for it -- with ~575 kept particles on 512 threads the second round is wave 0's alone.
template <bool ORD, int NT, int QSKIP, class L, int QOWN>
__device__ __forceinline__ void fetch_own(const L &S, const CollideArgs &A, const int tid, const uint32_t PS, const uint32_t n_owned,
                                          uint32_t (&own_id)[QOWN], float2 (&own_prev)[QOWN])
{
    static_assert(!ORD || L::kLid, "order-key windows keep the local indices");
    uint32_t fetch[QOWN];
    const uint32_t wave_s = wave_first_thread(tid);
#pragma unroll
    for (int q = 0; q < QOWN; ++q) {
        const uint32_t s = (uint32_t)tid + (uint32_t)q * NT;
        own_id[q] = 0xFFFFFFFFu;
        fetch[q] = 0u;
        if (q >= QSKIP && PS <= wave_s + (uint32_t)q * NT) continue;   // (scalar)
        const uint32_t sc = min(s, PS - 1u);
        const bool own = s < PS && S.is_own(sc);
        uint32_t id = S.id[sc];
        asm volatile("" : "+v"(id));                                 // keep this an LDS read (no pointer select -> flat load)
        if constexpr (ORD) id = S.lid[sc];                             // S.id holds the order key; the local index was kept
        own_id[q] = own ? id : 0xFFFFFFFFu;
        fetch[q] = (own && id < n_owned) ? id : 0u;
    }
#pragma unroll
    for (int q = 0; q < QOWN; ++q) {
        own_prev[q] = make_float2(0.f, 0.f);
        if (q >= QSKIP && PS <= wave_s + (uint32_t)q * NT) continue;
#ifdef GPE_DBG_SKIP
        if (GPE_DBG_SKIP & 32) continue;                               // diagnostic builds: phase cost by omission (results wrong)
#endif
        if (A.fuse_verlet) own_prev[q] = A.prev[fetch[q]];
    }
}
// P6: what fetch_own found, written back with K12 applied -- the integrated position becomes the live one, the resolved
// position the previous one (particle_integration.wgsl:64,76).  A sharded step (`packs`, scalar) packs the tile's
// particles for the neighbours on the way (S.id holds the order key).
template <bool ORD, int NT, int QSKIP, class L, int QOWN>
__device__ __forceinline__ void write_own_back(const L &S, const CollideArgs &A, const int tid, const uint32_t PS, const uint32_t n_owned,
                                               const bool packs, const uint32_t (&own_id)[QOWN], const float2 (&own_prev)[QOWN],
                                               const UniformRadii &U)
{
    const uint32_t wave_s = wave_first_thread(tid);
#pragma unroll
    for (int q = 0; q < QOWN; ++q) {
#ifdef GPE_DBG_SKIP
        if (GPE_DBG_SKIP & 32) continue;
#endif
        if (q >= QSKIP && PS <= wave_s + (uint32_t)q * NT) continue;   // (scalar, the test that filled own_id)
        const uint32_t id = own_id[q];
        const bool have = id != 0xFFFFFFFFu;
        const uint32_t s = min((uint32_t)tid + (uint32_t)q * NT, (uint32_t)L::kSlots - 1u);
        const float2 c = make_float2(S.px[s], S.py[s]);
        const float rr = S.radius_of(s, U);
        float2 o = c;
        const bool mine = have && A.fuse_verlet && id < n_owned;
        if (mine) {
            verlet_one(c.x, c.y, own_prev[q].x, own_prev[q].y, rr, A.vp, o.x, o.y);
            A.prev[id] = c;
            A.pos_out[id] = o;
        } else if (have) {
            A.pos_out[id] = c;
        }
        if constexpr (ORD) {
            if (packs) pack_if_near_border(A.pack, mine, id, o, c, rr, S.id[s], A.cell_size);
        }
    }
}

// ---- P0 of both tile forms ---------------------------------------------------------------------------------------------
// The control words a tile reads at its entry, for its 32x32 parent tile (ptx, pty): the straggler and ghost lists are
// kept per parent.  Issued in front of P0, consumed behind it: a crowded scene runs tens of thousands of short-lived tiles
// and sub-tiles, and a global round trip exposed in each of them cost the dense launch a quarter of its time again (5.95
// -> 7.5 ms at step 1000 of the 100 M soak).
struct TileWords {
    bool in_tb;                // the parent has lists (always, for the tiles of the dense launch)
    uint32_t pt;               // ... at this index
    uint32_t fresh, owned, exc, gho, gsort;
};
template <bool ORD>
__device__ __forceinline__ TileWords read_tile_words(const CollideArgs &A, const int ptx, const int pty)
{
    TileWords w;
    w.fresh = *A.fresh;
    w.owned = A.counts ? A.counts[0] : (uint32_t)(A.n_owned < 0xFFFFFFFFull ? A.n_owned : 0xFFFFFFFFull);
    w.in_tb = A.tb.holds(ptx, pty);
    w.pt = w.in_tb ? A.tb.index(ptx, pty) : 0u;
    w.exc = (A.exc_count && w.in_tb) ? A.exc_count[w.pt] : 0u;
    w.gho = 0; w.gsort = 0;
    if constexpr (ORD) {
        if (A.ghost_sort) w.gsort = *A.ghost_sort;
        if (A.gho_count && w.in_tb) w.gho = A.gho_count[w.pt];
    }
    return w;
}
// The region's NBX x NBY blocks from (box, boy) on, looked up in the block table: S.bstart / S.bcnt.  GHOST_TABLE: an
// order-key counting-sort window looks every block up a second time, among the ghosts (virtual blocks [NBLK, 2 NBLK)) --
// through their block table only when a ghost list ran over this step (gsort), or there are no lists.
template <int NBX, int NBY, bool GHOST_TABLE, class L>
__device__ __forceinline__ void look_blocks_up(L &S, const CollideArgs &A, const int tid, const int box, const int boy, const uint32_t gsort)
{
    constexpr int NBLK = NBX * NBY, VB = GHOST_TABLE ? 2 * NBLK : NBLK;
    if (tid < VB) {
        const int rb = tid % NBLK;                                     // the block; tid >= NBLK: among the ghosts
        const int bi = rb % NBX, bj = rb / NBX;
        const int lbx = box + bi - A.bx0, lby = boy + bj - A.by0;
        uint32_t start = 0, count = 0;
        const uint2 *tab = A.table;
        if constexpr (GHOST_TABLE) {
            const bool ghosts_by_table = A.gho_count == nullptr || __builtin_amdgcn_readfirstlane((int)gsort) != 0;
            if (tid >= NBLK) tab = ghosts_by_table ? A.gtable : nullptr;
        }
        if (tab && lbx >= 0 && lby >= 0 && lbx < A.blocks_x && lby < A.blocks_y) {
            const uint32_t mb = (uint32_t)(lby * A.blocks_x + lbx);
            if (mb < A.entries) {
                const uint2 se = tab[mb];                            // empty blocks hold (0xFFFFFFFF, 0)
                if (se.y > se.x) { start = se.x; count = se.y - se.x; }
            }
        }
        S.bstart[tid] = start;
        S.bcnt[tid] = count;
    }
}
// Behind a barrier: wave 0 scans the block populations (S.boff; S.misc[0] all looked-up particles, S.misc[1] those of the
// tile's own blocks, the ones not on the region's rim); the threads behind it take the population of each 3x3-block
// window of the tile (what an 8x8-cell sub-tile would stage): the host reads the step's maximum (lagged) to leave the
// native path before windows overfill, `tile_max` (LDS, or null) keeps the tile's for its roster.  ZERO: the words of
// S.misc (bits 2..4) that the tile starts at 0.
template <int NBX, int NBY, int VB, uint32_t ZERO, class L>
__device__ __forceinline__ void scan_blocks(L &S, const CollideArgs &A, const int tid, uint32_t *tile_max)
{
    constexpr int NBLK = NBX * NBY;
    const int lane = tid & 63;
    if (tid < 64) {
        uint32_t carry = 0, own = 0;
        for (int base = 0; base < VB; base += 64) {
            const int b = base + lane;
            const uint32_t cb = (b < VB) ? S.bcnt[b] : 0u;
            const uint32_t inc = wave_inclusive_scan(cb);
            if (b < VB) {
                S.boff[b] = carry + inc - cb;
                const int bi = (b % NBLK) % NBX, bj = (b % NBLK) / NBX;
                if (bi >= 1 && bi < NBX - 1 && bj >= 1 && bj < NBY - 1) own += cb;
            }
            carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        own = wave_sum(own);
        if (lane == 0) {
            S.boff[VB] = carry; S.misc[0] = carry; S.misc[1] = own;
#pragma unroll
            for (int k = 2; k < 5; ++k)
                if (ZERO & (1u << k)) S.misc[k] = 0;
        }
    } else if (tid < 64 + (NBX - 2) * (NBY - 2)) {
        const int wi = (tid - 64) % (NBX - 2), wj = (tid - 64) / (NBX - 2);
        uint32_t w = 0;
#pragma unroll
        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
            for (int di = 0; di < 3; ++di) w += S.bcnt[(wj + dj) * NBX + wi + di];
        if (w > kWindowReport) atomicMax(&A.tile_ctl[kCtlWindowMax], w);
        if (tile_max && w > kWindowReport) atomicMax(tile_max, w);
    }
}
// Slot -> block map (S.sblk) of the looked-up slots: NT / VB threads share each block's slots.
template <int NT, int VB, class L>
__device__ __forceinline__ void map_slots_to_blocks(L &S, const int tid)
{
    constexpr int SHARE = (NT / VB) > 0 ? (NT / VB) : 1;
    for (int b = tid % VB, sub = tid / VB; sub < SHARE && b < VB; b += NT) {
        const uint32_t lo = S.boff[b], hi = S.boff[b + 1];
        for (uint32_t i = lo + sub; i < hi; i += SHARE) S.sblk[i] = (uint8_t)b;
    }
}

// A tile this launch has no room for, appended to the list of a launch behind it (thread 0; CollideArgs::overflow1 / 2).
__device__ __forceinline__ void hand_tile_on(const CollideArgs &A, const int counter, uint32_t *list, const uint32_t cap, const int tx, const int ty)
{
    const uint32_t slot = atomicAdd(&A.tile_ctl[counter], 1u);
    if (slot < cap) list[slot] = ((uint32_t)ty << 16) | (uint32_t)tx;
    else atomicOr(&A.tile_ctl[kCtlError], kErrTileOverflow);
}

// One tile: returns false when the region exceeds the window's capacity (nothing written).
// ORD: a sharded run -- the members of a cell are ordered by A.order_keys[local index] (the particle's index in the
// unsharded system) instead of by the local index.  A template parameter, not a run-time test: the instantiation
// of ordinary runs then contains no load of the order keys, and hipcc has no reason to wait for one
// (s_waitcnt vmcnt(0) in front of every prefetch of a previous position -- the rounds' loads ran one after the other).
template <bool ORD, class L>
__device__ __forceinline__ bool process_tile(L &S, const CollideArgs &A, const int tx, const int ty)
{
    const UniformRadii U = UniformRadii();                             // (not used: these windows keep a radius per particle)
    constexpr int T = L::TILE;
    constexpr int RWX = L::RWX, RWY = L::RWY, PX = L::PX, NCELL = L::NCELL, NB = L::NB, NBLK = L::NBLK, PER = L::PER, QMAX = L::QMAX;
    // virtual blocks: an order-key (sharded) window looks every block up among the owned particles AND among the ghosts
    constexpr int VB = ORD ? 2 * NBLK : NBLK;
    static_assert(VB <= 255 && VB <= L::VBMAX, "sblk is 8 bit; the lookup arrays hold the virtual blocks");
    int tid_ = (int)threadIdx.x;
    // (the windows of the over-capacity launch run in a loop over tickets: everything that depends on the thread index
    // alone -- P4's cell coordinates and zone tests, the scans' offsets -- is invariant in that loop, and hipcc hoisted
    // 37 registers of it in front of the loop, spilled them there and reloaded them inside, s_waitcnt vmcnt(0) behind
    // each reload; recomputing them per window costs a few VALU instructions)
    if constexpr (T < 32) asm volatile("" : "+v"(tid_));
    const int tid = tid_;
    const int lane = tid & 63;
    constexpr int HX = L::HXL, HY = L::HYL;                            // cells kept left of / below the tile
    constexpr bool kTrim = !L::kGlobal;
    const int ox = tx * T - HX, oy = ty * T - HY;                      // origin of the cell window
    const int box = (tx * T - kHalo) >> 3, boy = (ty * T - kHalo) >> 3;   // first looked-up block
    GPE_STAMP_BEGIN();
    const int ptx = (tx * T) >> 5, pty = (ty * T) >> 5;                // the 32x32 parent tile (lists are kept per parent)
    const TileWords W = read_tile_words<ORD>(A, ptx, pty);
    const uint32_t pt = W.pt;

    // ---- P0: clear, look the region's blocks up, slot -> block map ---------------------------------
    S.cell_clear(tid);
    if (tid < 20) S.lcnt[tid] = 0;
    look_blocks_up<NB, NB, ORD>(S, A, tid, box, boy, W.gsort);
    __syncthreads();
    // (misc[3], the kept particles, starts at 0; in a main tile misc[2] as well: "a cell of more than 64 members")
    scan_blocks<NB, NB, VB, L::kGlobal ? 8u : 12u>(S, A, tid, nullptr);
    __syncthreads();
    const uint32_t P = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.misc[0]);   // the same in every lane: keep it scalar
    const bool stale = __builtin_amdgcn_readfirstlane((int)W.fresh) == 0;
    const uint32_t n_owned_now = (uint32_t)__builtin_amdgcn_readfirstlane((int)W.owned);
    const uint32_t straggler_bit = stale ? kCodeStraggler : 0u;       // (listed under a block it is out of reach of: skipped)
    // stragglers handed to this tile's 32x32 parent by the hash kernel (P1 files them behind the looked-up particles)
    const uint32_t n_exc = stale ? min((uint32_t)__builtin_amdgcn_readfirstlane((int)W.exc), kExcSlots) : 0u;
    // ghosts listed for the tile's parent (sharded runs; none when the ghosts come through their block table this step)
    uint32_t n_gho = 0;
    if constexpr (ORD) {
        if (A.gho_count != nullptr && __builtin_amdgcn_readfirstlane((int)W.gsort) == 0)
            n_gho = min((uint32_t)__builtin_amdgcn_readfirstlane((int)W.gho), kGhostSlots);
    }
    // Nothing of its own to write?  With the table of this step: no particle in the tile's own blocks.  With a kept
    // table a particle may have drifted up to kDrift* cells out of the block that lists it, so only an empty lookup
    // region (own blocks + the ring around them) AND an empty straggler list tell -- a straggler that flew into empty
    // space exists for its tile through the list alone (test_stragglers_flying_into_empty_space_are_not_lost).
    if (stale ? (P == 0 && n_exc == 0) : S.misc[1] == 0) return true;
    if constexpr (L::kGlobal) {
        // take a slice of the global spill arena for this tile's particle arrays
        if (tid == 0) {
            const uint32_t extra = kExcSlots + (ORD ? kGhostSlots : 0u);                 // (+ the stragglers' and the listed ghosts' slots)
            const uint32_t base = atomicAdd(&A.tile_ctl[kCtlArena], P + extra);
            const bool ok = (uint64_t)base + P + extra <= (uint64_t)A.arena_cap;
            S.misc[2] = ok ? 1u : 0u;
            S.px = A.arena_px + base; S.py = A.arena_py + base; S.rad = A.arena_rad + base;
            S.id = A.arena_id + base; S.hm = A.arena_hm + base; S.sblk = A.arena_sblk + base;
            S.mem = A.arena_mem + 4ull * base;
        }
        __syncthreads();
        if (S.misc[2] == 0) return false;
    } else {
        if (P > (uint32_t)L::RAWCAP) return false;                     // more looked-up particles than slots
    }
    map_slots_to_blocks<kNatThreads, VB>(S, tid);
    __syncthreads();
    GPE_STAMP(0);

    // ---- P1: gather the region's particles (all loads of a thread in flight together), count the
    //          cell memberships -----------------------------------------------------------------------
    // Two rounds of 512 looked-up particles per pass of this loop: the window takes three (QMAX), but the mean tile
    // looks up 1.7 x 512, so the third round's instructions -- executed by every wave whether or not a lane has a
    // particle -- are left to a second pass that a scalar branch skips unless P > 1024.
    constexpr int QP = QMAX >= 2 ? 2 : 1;
    for (uint32_t s0 = 0; s0 < P; s0 += (uint32_t)QP * kNatThreads) {
        uint32_t pid[QP], blk[QP], cc[QP];
        float2 pp[QP];
        float pr[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            // Branch-free on purpose: behind `if (s < P)` hipcc merges the loaded value with the default through
            // register copies that wait for the load (s_waitcnt vmcnt(0) right behind it), so the rounds' loads ran one
            // after the other -- three dependent global round trips.  Slots beyond P re-read slot P - 1 (a cache hit)
            // and are discarded by `keep` below.  (P >= 1: see P0.)
            const uint32_t s = min(s0 + (uint32_t)tid + (uint32_t)q * kNatThreads, P - 1u);
            blk[q] = S.sblk[s];
            const uint32_t *ids = (ORD && blk[q] >= (uint32_t)NBLK) ? A.gsorted_ids : A.sorted_ids;
            pid[q] = ids[S.bstart[blk[q]] + (s - S.boff[blk[q]])];
        }
#ifdef GPE_TILE_STAMPS
        { uint32_t acc = 0; for (int q = 0; q < QP; ++q) acc += pid[q]; asm volatile("" :: "v"(acc)); }
        GPE_STAMP(7);
#endif
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            pp[q] = A.pos_in[pid[q]];
            pr[q] = A.radius[pid[q]];
            cc[q] = A.codes[pid[q]];
        }
        // sharded run: the member order is the particle's index in the unsharded system; the local index is looked
        // up again at write-back (P6)
        uint32_t lidq[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) lidq[q] = pid[q];
        if constexpr (ORD) {
#pragma unroll
            for (int q = 0; q < QP; ++q) pid[q] = A.order_keys[pid[q]];
        }
#ifdef GPE_TILE_STAMPS
        { float acc = 0; for (int q = 0; q < QP; ++q) acc += pp[q].x + pr[q]; asm volatile("" :: "v"(acc)); }
        GPE_STAMP(8);
#endif
        // home cell: the slot's block among the looked-up ones + the cell inside the block (k_native_hash),
        // relative to the cell window; particles whose home lies outside the window are dropped here
        int lxq[QP], lyq[QP];
        bool keep[QP];
        uint32_t slot[QP];
        uint64_t mq[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const uint32_t s = s0 + (uint32_t)tid + (uint32_t)q * kNatThreads;
            lxq[q] = code_window_x(cc[q], ox);
            lyq[q] = code_window_y(cc[q], oy);
            // (voted comparison by comparison, the masks combined by scalar ANDs: see pair_response)
            mq[q] = ballot64(s < P) & ballot64(lxq[q] < RWX) & ballot64(lyq[q] < RWY) & ballot64((cc[q] & straggler_bit) == 0u);
            // (an order-key window: the kept table may still list indices the owned range has shrunk below -- those
            // particles are ghosts now, or gone: they come through the ghosts' table, or not at all)
            if constexpr (ORD) {
                if (A.gtable != nullptr) mq[q] &= ballot64(blk[q] >= (uint32_t)NBLK) | ballot64(lidq[q] < n_owned_now);
            }
            keep[q] = lanes_of(mq[q]);
            slot[q] = s;
        }
        // kept particles get consecutive slots (over capacity: see below); the spill window's are the looked-up ones
        if constexpr (kTrim) take_slots(&S.misc[3], lane, (uint32_t)L::kSlots, mq, slot, keep);
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            if constexpr (!kTrim) {
                if (!keep[q] && s0 + (uint32_t)tid + (uint32_t)q * kNatThreads < P) file_dropped(S, slot[q], pp[q], pr[q], pid[q]);
            }
            if (!keep[q]) continue;
            file_kept(S, slot[q], pp[q], pr[q], pid[q], lidq[q], lxq[q], lyq[q], cc[q]);
        }
    }
    // One entry of a list the hash kernel handed to the tile's parent -- a straggler, a listed ghost: fetched, placed by its
    // cell (`cell_of`: the entry's or the code word's), given a slot (`spill_slot`: the spill window's, behind the
    // looked-up ones), filed.  (Called by whole waves: the slots use ballots.)
    auto take_listed = [&](const bool have, const uint32_t lidv, const uint32_t spill_slot, auto cell_of) {
        const float2 pp = A.pos_in[lidv];
        const float pr = A.radius[lidv];
        const uint32_t cc = A.codes[lidv];
        uint32_t pid = lidv;
        if constexpr (ORD) pid = A.order_keys[lidv];
        int lx, ly;
        cell_of(cc, lx, ly);
        bool keep = have && lx >= 0 && lx < RWX && ly >= 0 && ly < RWY;
        uint32_t sl = spill_slot;
        if constexpr (kTrim) sl = take_slots(&S.misc[3], lane, (uint32_t)L::kSlots, ballot64(keep), keep);
        if (keep) file_kept(S, sl, pp, pr, pid, lidv, lx, ly, cc);
        else if (!kTrim && have) file_dropped(S, sl, pp, pr, pid);
    };
    if (n_exc != 0 && tid < 64) {                                      // (scalar condition; one wave files them)
        // Stragglers: particles out of reach of the block the table lists them under, handed over with their cell.
        const bool have = (uint32_t)tid < n_exc;
        const uint2 en = A.exc_entry[(uint64_t)pt * kExcSlots + (have ? (uint32_t)tid : 0u)];
        take_listed(have, en.x, P + (uint32_t)tid,
                    [&](uint32_t, int &lx, int &ly) { lx = (int)(en.y & 0xFFFFu) - ox; ly = (int)(en.y >> 16) - oy; });
    }
    if constexpr (ORD) {
        // Ghosts listed for the tile's parent by the hash kernel: placed by the cell in their code word (a listed ghost
        // lies in the parent's window, so its cell mod 128 names one cell of this window or none); behind the stragglers.
        for (uint32_t g0 = 0; g0 < n_gho; g0 += kNatThreads) {         // (scalar bounds: whole waves)
            const uint32_t gi = g0 + (uint32_t)tid;
            const bool have = gi < n_gho;
            take_listed(have, A.gho_entry[(uint64_t)pt * kGhostSlots + (have ? gi : 0u)], P + n_exc + gi,
                        [&](uint32_t cc, int &lx, int &ly) { lx = code_window_x(cc, ox); ly = code_window_y(cc, oy); });
        }
    }
    __syncthreads();
    GPE_STAMP(1);
    // particles in the window from here on: the kept ones (the global window keeps every looked-up particle: its
    // cell window is the looked-up blocks; the stragglers and the listed ghosts sit behind them)
    uint32_t PS = P + (kTrim ? 0u : n_exc + n_gho);
    if constexpr (kTrim) {
        PS = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.misc[3]);
        if (PS > (uint32_t)(sizeof(S.px) / sizeof(float))) return false;    // more kept particles than the window stages
        if (PS == 0) return true;                                      // (looked up, none inside the window)
    }

    // ---- P2: exclusive scan of the per-cell counts -> list starts ----------------------------------
    {
        const int c0 = tid * PER;
        uint32_t cn[PER];
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { cn[k] = (c0 + k < NCELL) ? S.cell_get(c0 + k + 1) : 0u; sum += cn[k]; }
        uint32_t run = nat_block_exclusive_scan(sum, S.s_w, nullptr);
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (c0 + k < NCELL) { S.cell_set(c0 + k + 1, run); run += cn[k]; }
    }
    __syncthreads();
    GPE_STAMP(2);

    // ---- P3: fill the member lists (order fixed later by the per-cell sort) --------------------------
#ifdef GPE_DBG_SKIP
    if (!(GPE_DBG_SKIP & 4))
#endif
    for (uint32_t s = tid; s < PS; s += kNatThreads) {
        const uint32_t hm = S.hm[s];
        const int home = (int)(hm & 0x7FFu);
        uint32_t k = S.cell_inc(home + 1);
        S.mem[k] = s;
        uint32_t over = (hm >> 11) & 0xFFu;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (over == 0) break;
            const int kb = __ffs((int)over) - 1;
            over &= over - 1u;
            k = S.cell_inc(home + neighbour_offset<PX>(kb) + 1);
            S.mem[k] = s;
        }
    }
    __syncthreads();
    GPE_STAMP(3);

    // The tile's own particles and, when K12 is fused into the write-back, their previous positions: fetched
    // here so that the global round trip runs under the colour passes instead of at the end of the tile.
    // (a scalar, so that comparing against it waits for no load: the count of a sharded run is read here, once)
    const uint32_t n_owned = n_owned_now;
    constexpr int QOWN = (L::kSlots + kNatThreads - 1) / kNatThreads;  // ceil(kept capacity / threads)
    // (The windows of the over-capacity launch fetch at P6 instead: their kernel holds three window forms and the
    // blocked whole-wave walk, and twelve registers kept across the colour passes were spilled there -- each previous
    // position right behind its load, s_waitcnt vmcnt(0) in between: P4 took 18.6 k cycles per window instead of 4 k.)
    constexpr bool kFetchEarly = T >= 32;
    uint32_t own_id[QOWN];
    float2 own_prev[QOWN];
    constexpr int QSKIP = kFetchEarly ? 2 : 1;                         // (the third round of a 32x32 tile is nearly always empty)
    if constexpr (kTrim && kFetchEarly) fetch_own<ORD, kNatThreads, QSKIP>(S, A, tid, PS, n_owned, own_id, own_prev);

#ifdef GPE_DBG_SKIP
    if (!(GPE_DBG_SKIP & 2))
#endif
    // ---- P4: active cells per colour.  Colour-major walk: every wave round looks at 64 cells of EACH colour
    //          (the four colours' reads are in flight together), so one ballot and one LDS atomic per colour,
    //          class and round compact them -------------------------------------------------------------
    {
        // only cells inside the widest exactness zone (colour 1: [x0-4, x1+3] x [y0-2, y1+1]) can be active:
        // (T + 8) (T + 4) / 4 per colour
        constexpr int ZW = (T + 8) / 2, ZH = (T + 4) / 2, QC = ZW * ZH, QZ = L::QZ;
        static_assert(QC == QZ, "one list slot per zone cell of a colour");
        // the walk starts at the even cell (x0 - 4, y0 - 2) and visits 2 x 2 groups: colour = position in the group
        static_assert(kConeLeft % 2 == 0 && kConeDown % 2 == 0 && T % 2 == 0, "groups start at even cells");
        static_assert(HX > kConeLeft && HY > kConeDown && L::HXR > kConeRight && L::HYR > kConeUp, "zones inside the window");
        for (int base = 0; base < QC; base += kNatThreads) {
            if (base + (int)wave_first_thread(tid) >= QC) continue;    // (scalar) no colour group for this wave: see process_tile_direct
            const int i = base + tid;
            const int hx = 2 * (i % ZW) + (HX - kConeLeft), hy = 2 * (i / ZW) + (HY - kConeDown);
            int lc[4];
            uint32_t cnt[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // colour - 1 = (gx & 1) + 2 * (gy & 1) (collision_solver.wgsl:55-58); ox + hx, oy + hy are even
                lc[c] = (hy + (c >> 1) + 1) * PX + hx + (c & 1) + 1;
                cnt[c] = 0;
                if (i < QC) cnt[c] = S.cell_get(lc[c] + 1) - S.cell_get(lc[c]);
            }
            // (the classes as lane masks, voted comparison by comparison: see pair_response)
            uint64_t ms[4], mg[4];
            bool single[4], group[4];
            constexpr int WC = L::WC;
            const uint64_t in_m = ballot64(i < QC);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int lx = hx + (c & 1), ly = hy + (c >> 1);
                const int gxx = ox + lx, gyy = oy + ly;
                // cells beyond the tile's edges on each side; the colour's zone (kCone*): colour c + 1 reaches
                // 4 - c cells left, 3 - c right, 2 - (c >> 1) down, 1 - (c >> 1) up
                const int exl = HX - lx, exr = lx - (HX + T - 1), eyl = HY - ly, eyr = ly - (HY + T - 1);
                const uint64_t zone_m = ballot64(exl <= kConeLeft - c) & ballot64(exr <= kConeRight - c) &
                                        ballot64(eyl <= kConeDown - (c >> 1)) & ballot64(eyr <= kConeUp - (c >> 1));
                // morton(-1,-1) == 0xFFFFFFFF == UNUSED_CELL_ID: never a collision cell
                // (collision_cell_builder.wgsl:56); cells outside the colour's exactness zone are skipped
                const uint64_t alias_m = ballot64((gxx & 0xFFFF) == 0xFFFF) & ballot64((gyy & 0xFFFF) == 0xFFFF);
                const uint64_t act_m = in_m & ballot64(cnt[c] >= 2u) & zone_m & ~alias_m;
                // cells of 4..8 members go to the BACK of the colour's segment: they are resolved by a group
                // of 8 lanes (resolve_group); the others fill the segment from the front (one lane each)
                mg[c] = act_m & ballot64(cnt[c] >= kGroupMin) & ballot64(cnt[c] <= kGroupLanes);
                // cells of 9..64 members go to a whole wave each (resolve_wave), as far as the colour's list takes
                // (65..256 members: blocked, in the sub-tile and spill windows only; a main tile that meets such a
                // cell hands itself over to them)
                // (the blocked form packs a member's rank above its 22-bit slot: a spill window of 4 M particles and more
                // -- the whole system in 24 x 24 cells -- leaves its piles to one lane)
                const uint32_t kWaveMax = (T >= 32 || PS >= (1u << 22)) ? 64u : kWaveCellMax;
                const uint64_t big_m = act_m & ballot64(cnt[c] > kGroupLanes);
                uint64_t wave_m = big_m & ballot64(cnt[c] <= kWaveMax);
                if (big_m != 0) {                                      // (scalar: no such cell in most rounds)
                    if (T >= 32 && lanes_of(big_m) && cnt[c] > 64u) S.misc[2] = 1u;
                    bool wavec = lanes_of(wave_m);
                    bool rowc = false;
                    if constexpr (L::kRows) {
                        rowc = wavec && cnt[c] <= kRowLanes;
                        if (rowc) {
                            const uint32_t k = atomicAdd(&S.lcnt[12 + c], 1u);
                            if (k < (uint32_t)WC) { S.rlist[c * WC + k] = (uint16_t)lc[c]; wavec = false; } else rowc = false;
                        }
                    }
                    if (wavec) {
                        const uint32_t k = atomicAdd(&S.lcnt[8 + c], 1u);
                        if (k < (uint32_t)WC) S.wlist[c * WC + k] = (uint16_t)lc[c]; else wavec = false;
                    }
                    wave_m = ballot64(wavec || rowc);                  // (cells the lists had no room for: one lane)
                }
                ms[c] = act_m & ~mg[c] & ~wave_m;
                group[c] = lanes_of(mg[c]);
                single[c] = lanes_of(ms[c]);
            }
            // the eight list counters (colour x class) are bumped by eight lanes at once: one LDS round trip for
            // the wave instead of eight dependent ones
            uint32_t mine = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                mine = (lane == c) ? (uint32_t)__popcll(ms[c]) : mine;
                mine = (lane == 4 + c) ? (uint32_t)__popcll(mg[c]) : mine;
            }
            uint32_t mybase = 0;
            if (lane < 8 && mine) mybase = atomicAdd(&S.lcnt[lane], mine);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t bs = (uint32_t)__builtin_amdgcn_readlane((int)mybase, c);
                const uint32_t bg = (uint32_t)__builtin_amdgcn_readlane((int)mybase, 4 + c);
                if (single[c]) S.list[c * QZ + bs + popc_below_lane(ms[c])] = (uint16_t)lc[c];
                if (group[c]) S.list[c * QZ + (QZ - 1) - (bg + popc_below_lane(mg[c]))] = (uint16_t)lc[c];
            }
        }
    }
    __syncthreads();
    GPE_STAMP(4);
    if constexpr (T >= 32) {
        // a cell of more than 64 members: the sub-tile windows resolve those with a wave per cell
        if (S.misc[2]) return false;
    }

    // ---- P5: the four colour passes (collision_solver.rs:224), one lane per collision cell ----------
#ifdef GPE_DBG_SKIP
    if (!(GPE_DBG_SKIP & 1))                                           // diagnostic builds: phase cost by omission
#endif
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
#ifdef GPE_TILE_STAMPS
        const long long _tw0 = clock64();
#endif
        const uint32_t ns = S.lcnt[k], group_lanes = S.lcnt[4 + k] * kGroupLanes;
        const uint32_t nw = min(S.lcnt[8 + k], (uint32_t)L::WC);
        const uint32_t single_base = (group_lanes + 63u) & ~63u;      // waves are all-group or all-single
        const uint32_t work = single_base + ns;
        for (uint32_t i0 = 0; i0 < work; i0 += kNatThreads) {
            const uint32_t i = i0 + (uint32_t)tid;
            if (i < group_lanes) {
                const int lc = S.list[k * L::QZ + (L::QZ - 1) - (i / kGroupLanes)];
                const uint32_t b = S.cell_get(lc), e = S.cell_get(lc + 1);
#ifdef GPE_DBG_SKIP
                if (!(GPE_DBG_SKIP & 8))
#endif
                if (!GPE_RT_SKIP(1u))
                resolve_group<(int)kGroupLanes>(S, b, e - b, (int)(i % kGroupLanes), A.stiffness, U);
            } else if (i >= single_base && (i & ~63u) < work) {         // (whole waves: the walk uses ballots)
                const bool on = i < work;
                uint32_t b = 0, e = 0;
                if (on) {
                    const int lc = S.list[k * L::QZ + (i - single_base)];
                    b = S.cell_get(lc); e = S.cell_get(lc + 1);
                }
#ifdef GPE_DBG_SKIP
                if (!(GPE_DBG_SKIP & 16))
#endif
                if (!GPE_RT_SKIP(2u)) {
                    resolve_small_cells(S, on, b, e - b, A.stiffness, U);
                }
            }
        }
#ifdef GPE_TILE_STAMPS
        const long long _tw_cells = clock64();
#endif
        // Whole-wave cells and rows: drawn with a ticket, the whole-wave cells (the longest items) first -- the waves that
        // hold the colour's lane groups or one-lane cells come for them when they are through, the idle ones at once.
        // (Fixed shares were measured: with the items dealt out from the first wave up the group waves carried them on
        // top of their groups; from the last wave down the one-lane waves did, and step 2000 of the 100 M soak lost 3 %.)
        if constexpr (L::kRows) {
            const uint32_t nr = min(S.lcnt[12 + k], (uint32_t)L::WC);
            const uint32_t items = nw + (nr + 3u) / 4u;
            while (items != 0u) {                                         // (wave-uniform)
                uint32_t t = 0;
                if (lane == 0) t = atomicAdd(&S.lcnt[16 + k], 1u);
                t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
                if (t >= items || GPE_RT_SKIP(4u)) break;
                if (t < nw) {
                    const int lc = S.wlist[k * L::WC + t];
                    const uint32_t b = S.cell_get(lc), e = S.cell_get(lc + 1);
                    if (e - b <= 64u) resolve_wave(S, b, e - b, A.stiffness, U);
                    else resolve_wave_blocked(S, b, e - b, A.stiffness, U);
                } else {
                    const uint32_t ci = 4u * (t - nw) + (uint32_t)(lane >> 4);
                    uint32_t b = 0, e = 0;
                    if (ci < nr) {
                        const int lc = S.rlist[k * L::WC + ci];
                        b = S.cell_get(lc); e = S.cell_get(lc + 1);
                    }
                    resolve_row(S, b, e - b, lane & 15, A.stiffness, U);
                }
            }
        } else
        for (uint32_t i = (uint32_t)(tid >> 6); i < nw; i += kNatWaves) {     // wave-uniform
            if (GPE_RT_SKIP(4u)) break;
            const int lc = S.wlist[k * L::WC + i];
            const uint32_t b = S.cell_get(lc), e = S.cell_get(lc + 1);
            if (e - b <= 64u) resolve_wave(S, b, e - b, A.stiffness, U);
        }
#ifdef GPE_TILE_STAMPS
        GPE_STAMP(9 + k);
        {
            const long long _tw1 = clock64();
            __syncthreads();
            const long long _tw2 = clock64();
            if (A.stamps && lane == 0 && (blockIdx.x & 127u) == 5u) {
                const int w = tid >> 6;
                const int cls = ((uint32_t)(w * 64) < group_lanes) ? 0 : ((uint32_t)(w * 64) < work ? 1 : 2);   // groups / singles / idle
                atomicAdd(&A.stamps[32 + cls], (unsigned long long)(_tw1 - _tw0));
                atomicAdd(&A.stamps[36 + cls], (unsigned long long)(_tw2 - _tw1));
                atomicAdd(&A.stamps[40 + cls], 1ull);
                // the colour pass by class of cell: cells, and this wave's cycles in the whole-wave cells
                atomicAdd(&A.stamps[48], (unsigned long long)(_tw1 - _tw_cells));
                if (w == 0) {
                    atomicAdd(&A.stamps[44], (unsigned long long)ns);
                    atomicAdd(&A.stamps[45], (unsigned long long)(group_lanes / kGroupLanes));
                    atomicAdd(&A.stamps[46], (unsigned long long)nw);
                    atomicAdd(&A.stamps[47], 1ull);
                    uint32_t members = 0, largest = 0;
                    for (uint32_t i = 0; i < nw; ++i) {
                        const int lc = S.wlist[k * L::WC + i];
                        const uint32_t m = S.cell_get(lc + 1) - S.cell_get(lc);
                        members += m; largest = max(largest, m);
                        atomicAdd(&A.stamps[52 + (m <= 16u ? 0 : m <= 32u ? 1 : m <= 64u ? 2 : 3)], 1ull);
                    }
                    atomicAdd(&A.stamps[51], (unsigned long long)min(S.lcnt[12 + k], (uint32_t)L::WC));
                    atomicAdd(&A.stamps[49], (unsigned long long)members);
                    atomicAdd(&A.stamps[50], (unsigned long long)largest);
                }
            }
        }
#else
        __syncthreads();
#endif
    }
    GPE_STAMP(5);

    // ---- P6: write the tile's own particles back ------------------------------------------------------
    const bool packs = ORD && A.pack.on != 0u;                         // (scalar) a sharded step: the tiles pack
    if constexpr (kTrim && !kFetchEarly) fetch_own<ORD, kNatThreads, QSKIP>(S, A, tid, PS, n_owned, own_id, own_prev);
    if constexpr (kTrim) write_own_back<ORD, kNatThreads, QSKIP>(S, A, tid, PS, n_owned, packs, own_id, own_prev, U);
    else
    for (uint32_t s0 = 0; s0 < PS; s0 += kNatThreads) {                // (whole waves: the pack uses ballots)
        const uint32_t s = s0 + (uint32_t)tid;
        const bool own = s < PS && (S.hm[min(s, PS - 1u)] & (1u << 19)) != 0;
        bool mine = false;
        uint32_t pk_id = 0, pk_key = 0;
        float2 pk_o = make_float2(0.f, 0.f), pk_c = pk_o;
        float pk_r = 0.f;
        if (own) {                                                     // the tile's own particle
            uint32_t id = S.id[s];
            pk_key = id;
            asm volatile("" : "+v"(id));                             // keep this an LDS read (no pointer select -> flat load)
            if constexpr (ORD) {                                       // S.id holds the order key: find the block of
                const uint32_t raw = s;                                // the looked-up slot, re-read the local index
                if (raw >= P + n_exc) {
                    id = A.gho_entry[(uint64_t)pt * kGhostSlots + (raw - P - n_exc)];   // a listed ghost
                } else if (raw >= P) {
                    // a straggler (filed behind the looked-up slots by P1): no block lists it -- its local index is
                    // the entry of the tile's straggler list it came from
                    id = A.exc_entry[(uint64_t)pt * kExcSlots + (raw - P)].x;
                } else {
                    int lo = 0, hi = VB;
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (S.boff[mid] <= raw) lo = mid; else hi = mid;
                    }
                    id = (lo >= NBLK ? A.gsorted_ids : A.sorted_ids)[S.bstart[lo] + (raw - S.boff[lo])];
                }
            }
            const float2 c = make_float2(S.px[s], S.py[s]);
            if (A.fuse_verlet && id < n_owned) {
                const float2 q = A.prev[id];
                float2 o;
                verlet_one(c.x, c.y, q.x, q.y, S.rad[s], A.vp, o.x, o.y);
                A.prev[id] = c;
                A.pos_out[id] = o;
                mine = true; pk_id = id; pk_o = o; pk_c = c; pk_r = S.rad[s];
            } else {
                A.pos_out[id] = c;
            }
        }
        if constexpr (ORD) {
            if (packs) pack_if_near_border(A.pack, mine, pk_id, pk_o, pk_c, pk_r, pk_key, A.cell_size);
        }
    }
    __syncthreads();
    GPE_STAMP(6);
    return true;
}


// One 16x16 quarter (tx, ty in 16-cell units) of an over-capacity 32x32 tile: as a 16x16 tile, else as four 8x8
// tiles, and an 8x8 tile whose 24x24-cell window exceeds even that LDS capacity gets its particle arrays from the
// global spill arena.
template <bool ORD>
struct OverflowLds {
    using Mid = TileLds<kTileMid, ORD ? kCapOrd : kCapMid, ORD>;
    using Small = TileLds<kTileSmall, ORD ? kCapOrd : kCapSmall, ORD>;
    using Spill = TileGlobal<kTileSmall>;
    union { Mid mid; Small small; Spill spill; };
};
template <bool ORD>
__device__ __forceinline__ void resolve_quarter(OverflowLds<ORD> &u, const CollideArgs &A, const int tx, const int ty)
{
    using Spill = typename OverflowLds<ORD>::Spill;
    const bool done = process_tile<ORD>(u.mid, A, tx, ty);
    __syncthreads();                                                   // the union's views alias each other
    if (done) return;
    if (threadIdx.x == 0) atomicAdd(&A.tile_ctl[kCtlSubTiles], 1u);
    for (int sub = 0; sub < 4; ++sub) {
        const int sx = tx * 2 + (sub & 1), sy = ty * 2 + (sub >> 1);
        bool ok = process_tile<ORD>(u.small, A, sx, sy);
        __syncthreads();
        if (ok) continue;
        if (threadIdx.x == 0) atomicAdd(&A.tile_ctl[kCtlSpills], 1u);
        ok = process_tile<ORD>(u.spill, A, sx, sy);
        __syncthreads();
        if (ok) continue;
        // The spill arena is exhausted: flag it (sticky; gpe_sync / gpe_download report the error and the state of
        // this step is NOT a result) and pass the tile's own particles through unresolved and unintegrated, so that
        // what a host reads back stays finite.  "Own" as P1 decides it -- by the home cell in the code word, not by
        // block membership: with a kept table a block still lists particles that have drifted into a neighbouring
        // tile (that tile writes them) and misses those that drifted in; stragglers come through the tile's list.
        if (threadIdx.x == 0) atomicOr(&A.tile_ctl[kCtlError], kErrTileOverflow);
        {
            constexpr int VBS = ORD ? 2 * Spill::NBLK : Spill::NBLK;
            const int wx = sx * kTileSmall - Spill::HXL, wy = sy * kTileSmall - Spill::HYL;
            const bool stale = *A.fresh == 0u;
            const uint32_t owned_now = A.counts ? A.counts[0] : (uint32_t)(A.n_owned < 0xFFFFFFFFull ? A.n_owned : 0xFFFFFFFFull);
            for (int b = threadIdx.x; b < VBS; b += kNatThreads) {
                const uint32_t *ids = (ORD && b >= Spill::NBLK) ? A.gsorted_ids : A.sorted_ids;
                for (uint32_t q = 0; q < u.spill.bcnt[b]; ++q) {
                    const uint32_t id = ids[u.spill.bstart[b] + q];
                    const uint32_t code = A.codes[id];
                    const int lx = code_window_x(code, wx) - Spill::HXL, ly = code_window_y(code, wy) - Spill::HYL;
                    bool own = lx >= 0 && lx < kTileSmall && ly >= 0 && ly < kTileSmall && !(stale && (code & kCodeStraggler));
                    if (ORD) own = own && (A.gtable == nullptr || b >= Spill::NBLK || id < owned_now);
                    if (own) A.pos_out[id] = A.pos_in[id];
                }
            }
            const int qtx = (sx * kTileSmall) >> 5, qty = (sy * kTileSmall) >> 5;
            if (stale && A.exc_count && A.tb.holds(qtx, qty)) {
                const uint32_t pt = A.tb.index(qtx, qty);
                const uint32_t ne = min(A.exc_count[pt], kExcSlots);
                for (uint32_t e = threadIdx.x; e < ne; e += kNatThreads) {
                    const uint2 en = A.exc_entry[(uint64_t)pt * kExcSlots + e];
                    const int lx = (int)(en.y & 0xFFFFu) - sx * kTileSmall, ly = (int)(en.y >> 16) - sy * kTileSmall;
                    if (lx >= 0 && lx < kTileSmall && ly >= 0 && ly < kTileSmall) A.pos_out[en.x] = A.pos_in[en.x];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The 32x32 tile of the dense launch, second form: DIRECT cell slots.
//
// process_tile builds the member lists of a window by a counting sort -- count the memberships per cell (P1), scan the
// counts (P2), fill the lists (P3): three barrier-separated phases whose LDS round trips every wave of the tile waits
// for, and the tile is bound by exactly that, the latency of its chain of phases (profiles/r03/
// ab_p5_candidate_cull_rejected.txt).  At the densities the dense launch is for, cells are small (25 % packing: 0.2 % of
// the cells hold more than six members), so here every cell of the tile's zone owns six member slots outright: the
// atomic that counts a membership hands out the slot, and P2 / P3 are gone.  The colour passes read a cell's members
// with one LDS access instead of list -> cell offsets -> members.  A seventh member goes to a short side list; cells of
// 7..64 members are gathered from it by the wave that resolves them.  A window with more than kBigCap such entries (a
// compressed scene) is left to process_tile's windows in the over-capacity launch, as is anything else this form has
// no room for.  Same operations per particle pair in the same order: same bits.
// ---------------------------------------------------------------------------------------------------
// The phantom cells of a particle, decoded once: entry[overlap mask] = count (2 bits) | for each of the first three set
// bits k of the mask (grid.wgsl:68-90 keeps at most three, in scan order: y outer, x inner, centre skipped) dx + 1 (2 bits)
// and dy + 1 (2 bits).  512 bytes that stay in the vector L1: one load per staged particle instead of find-first-set,
// clear, the centre skip and a division by three per membership (~7 VALU instructions x 3 memberships x 2 rounds per wave).
struct PhantomTable { uint16_t v[256]; };
constexpr PhantomTable make_phantom_table()
{
    PhantomTable t{};
    for (int m = 0; m < 256; ++m) {
        int cnt = 0, e = 0;
        for (int k = 0; k < 8 && cnt < 3; ++k) {
            if (!((m >> k) & 1)) continue;
            const int kk = k + (k >= 4 ? 1 : 0);
            e |= ((kk % 3) | ((kk / 3) << 2)) << (2 + 4 * cnt);
            ++cnt;
        }
        t.v[m] = (uint16_t)(e | cnt);
    }
    return t;
}
__device__ const PhantomTable kPhantomTable = make_phantom_table();
constexpr int kDirectSlots = 6;                // member slots a zone cell owns
constexpr int kBigCap = 96;                    // memberships beyond that, per tile
template <int TX_, int TY_, int CAP, bool LID, int NT_, bool UNI = false>
struct TileDirect {
    static_assert(!(UNI && LID), "order-key windows keep the general path");
    static constexpr int TX = TX_, TY = TY_, NT = NT_, NW = NT_ / 64;   // tile (cells), threads, waves
    static constexpr bool kGlobal = false;
    static constexpr bool kLid = LID;
    static constexpr int kSlots = CAP;
    static constexpr int HXL = kConeLeft + 1, HXR = kConeRight + 1, HYL = kConeDown + 1, HYR = kConeUp + 1;
    static constexpr int RWX = TX + HXL + HXR, RWY = TY + HYL + HYR;   // cell window: where a kept particle's home may lie
    // zone cells: the 2 x 2 colour groups from the even cell (x0 - 4, y0 - 2) on, (T + 8) x (T + 4) cells; the colour
    // zones (kCone*) lie inside.  Only memberships of zone cells are filed.
    static constexpr int ZX = TX + 8, ZY = TY + 4, NZ = ZX * ZY, QZ = NZ / 4;
    static constexpr int ZOX = HXL - kConeLeft, ZOY = HYL - kConeDown;   // window coordinate of zone cell (0, 0)
    static constexpr int NBX = (TX + 2 * kHalo) / 8, NBY = (TY + 2 * kHalo) / 8;
    static constexpr int NBLK = NBX * NBY;
    // (a 32x16 half looks up 6 x 4 blocks, 3/4 of what a 32x32 tile does, for half the cells: it exists for tiles of up to
    // ~4 x the benchmark density, so it stages more looked-up particles, side-list entries and whole-wave cells)
    static constexpr int QMAX = TY >= 32 ? GPE_QMAX_MAIN : 7;
    static constexpr int RAWCAP = QMAX * NT;
    static constexpr int WC = TY >= 32 ? 16 : 32;
    static constexpr int kBig = TY >= 32 ? kBigCap : 2 * kBigCap;
    uint32_t lid[LID ? CAP : 1];
    float px[CAP], py[CAP];
    // UNI: every particle has the kernel's one radius (CollideArgs::uniform_r, NativeState::uniform): no radius array --
    // 4 B per slot less to gather, store and read back -- and the resolvers take the uniform pair_response (respond)
    static constexpr bool kUniform = UNI;
    float rad[UNI ? 1 : CAP];
    __device__ __forceinline__ float radius_of(const uint32_t s, const UniformRadii &U) const
    {
        if constexpr (UNI) return U.r; else return rad[s];
    }
    uint32_t id[CAP];
    uint8_t own[CAP];          // the particle's home cell lies in the tile
    __device__ __forceinline__ bool is_own(uint32_t s) const { return own[s] != 0; }
    // member slots a zone cell owns: six; an order-key (sharded) window keeps a local index per particle as well and
    // pays for it with the sixth slot (its cells of six members go to the side list and a wave, like cells of seven)
    static constexpr int kMemSlots = LID ? kDirectSlots - 1 : kDirectSlots;
    // members per zone cell.  Two 16-bit counters per word (LDS atomics are 32 bit) cost every membership a shift by the
    // cell's parity on the way in and a shift and a mask on the way out; the uniform windows have no radius array and
    // spend 2 NZ of the bytes that frees on a word per cell -- the general and the order-key windows have no such room
    // (the general 32x32 window is 40 928 B of the 40 960 that four workgroups per CU leave each)
    static constexpr bool kWordCounters = UNI;
    static constexpr int kCntWords = kWordCounters ? NZ : (NZ + 1) / 2;
    static_assert(!kWordCounters || NZ % 4 == 0, "cleared four words at a time");
    alignas(kWordCounters ? 16 : 4) uint32_t cntw[kCntWords];
    __device__ __forceinline__ uint32_t cnt_inc(int i)                // returns the value before the add
    {
        if constexpr (kWordCounters) return atomicAdd(&cntw[i], 1u);
        else {
            const uint32_t sh = (uint32_t)(i & 1) * 16u;
            return (atomicAdd(&cntw[i >> 1], 1u << sh) >> sh) & 0xFFFFu;
        }
    }
    __device__ __forceinline__ uint32_t cnt_get(int i) const
    {
        if constexpr (kWordCounters) return cntw[i];
        else return (cntw[i >> 1] >> ((uint32_t)(i & 1) * 16u)) & 0xFFFFu;
    }
    // members: kDirectSlots per zone cell, then 64 per wave for the cells gathered from the side list.  (Named like
    // TileLds' member array: the resolvers index S.mem[b + k].)
    uint16_t mem[kMemSlots * NZ + NW * 64];
    union {
        uint16_t list[4 * QZ]; // active cells, one segment per colour (P4 on)
        uint8_t sblk[RAWCAP];  // P0-P1 only: region block a looked-up slot came from
    };
    uint16_t wlist[4 * WC];    // cells of more than kDirectSlots members, per colour
    uint32_t big[kBig];        // memberships that found their cell's slots taken: zone cell << 16 | particle slot
    uint32_t lcnt[12];
    static constexpr int VBMAX = NBLK;                    // (an order-key window gets its ghosts from the tile's ghost list)
    uint32_t bstart[VBMAX];
    uint32_t bcnt[VBMAX];
    uint32_t boff[VBMAX + 1];
    uint32_t s_w[16];
    uint32_t misc[6];          // [0] looked up, [2] hand the tile on, [3] kept, [4] side-list entries
};

template <bool ORD, class L, bool HINTS = false>
__device__ __forceinline__ bool process_tile_direct(L &S, const CollideArgs &A, const int tx, const int ty)
{
    constexpr int TX = L::TX, TY = L::TY, NT = L::NT, NW = L::NW;
    constexpr int RWX = L::RWX, RWY = L::RWY, NBX = L::NBX, NBY = L::NBY, NBLK = L::NBLK, QMAX = L::QMAX;
    constexpr int VB = NBLK;                                           // (the ghosts of an order-key window: from the ghost list)
    static_assert(VB <= 255 && VB <= L::VBMAX, "sblk is 8 bit; the lookup arrays hold the blocks");
    constexpr int ZX = L::ZX, ZY = L::ZY, NZ = L::NZ, QZ = L::QZ;
    constexpr int MS = L::kMemSlots;
    constexpr int HX = L::HXL, HY = L::HYL;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int ox = tx * TX - HX, oy = ty * TY - HY;                    // origin of the cell window
    const int box = (tx * TX - kHalo) >> 3, boy = (ty * TY - kHalo) >> 3;   // first looked-up block
    // the one radius, its double, that squared and the prefilter's bound: formed here, once, as pair_response forms them
    UniformRadii U = UniformRadii();
    if constexpr (L::kUniform) U = uniform_radii(A.uniform_r);
    GPE_STAMP_BEGIN();
    // stragglers handed to this tile by the hash kernel (the lists are kept per 32x32 tile: a half reads its parent's)
    static_assert(TX == 32 && (TY == 32 || TY == 16), "straggler lists, ghost lists and rosters are kept per 32x32 tile");
    const TileWords W = read_tile_words<ORD>(A, tx, (ty * TY) >> 5);
    const bool in_tb = W.in_tb;
    const uint32_t pt = W.pt;
    // the tile's roster (CollideArgs): header, and the first ids on the chance that it is valid
    constexpr bool kRoster = TX == 32 && TY == 32 && NT == 512;
    constexpr int QP = QMAX >= 2 ? 2 : 1;
    static_assert(!kRoster || L::RAWCAP == kRosterCap, "roster stride");
    const bool rosters = kRoster && A.roster_hdr != nullptr && in_tb;
    const uint64_t roster_base = (uint64_t)pt * (uint64_t)kRosterCap;
    uint4 hdr = make_uint4(0u, 0u, 0u, 0u);
    uint32_t sorts_word = 0;
    uint32_t first_ids[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) first_ids[q] = 0u;
    if (rosters) {
        hdr = A.roster_hdr[pt];
        sorts_word = *A.sorts_seen;
#pragma unroll
        for (int q = 0; q < QP; ++q) first_ids[q] = A.roster_ids[roster_base + (uint32_t)tid + (uint32_t)q * NT];
    }

    // ---- P0: clear the counters, look the region's blocks up, slot -> block map ------------------------------------
    if constexpr (L::kWordCounters) {
        for (int i = tid; i < NZ / 4; i += NT) reinterpret_cast<uint4 *>(S.cntw)[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int i = tid; i < L::kCntWords; i += NT) S.cntw[i] = 0;
    }
    if (tid < 12) S.lcnt[tid] = 0;
    const bool stale = __builtin_amdgcn_readfirstlane((int)W.fresh) == 0;
    if constexpr (kRoster && HINTS) {
        // A hinted tile (kCtlHints): two of the launch's first workgroups redo it as halves.  (In front of every other way
        // out: a sharded tile must not be taken twice -- it would pack its particles twice.)
        const uint32_t hinted_for = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr.w);
        if (rosters && A.front_wgs != 0u && (hinted_for == A.step_stamp || hinted_for == A.step_stamp + 1u)) return true;
    }
    if constexpr (ORD) {
        // a ghost list ran over this step: the ghosts come through their block table, which only the counting-sort
        // windows of the over-capacity launch look up -- hand the tile on (a crowded border; the host's `crowded` policy
        // moves such scenes to those windows altogether)
        if (A.gho_count == nullptr || __builtin_amdgcn_readfirstlane((int)W.gsort) != 0) return false;
    }
    const uint32_t stamp_now = (uint32_t)__builtin_amdgcn_readfirstlane((int)sorts_word) + 1u;
    // (scalar) the roster is of the table in use: no lookup
    const bool listed = rosters && stale && (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr.y) == stamp_now;
    const bool record = rosters && !listed && A.roster_write != 0u;
    if (listed) {
        const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr.x);
        if (count == 0xFFFFFFFFu) { GPE_BAIL(1); return false; }       // more looked-up particles than the tile stages
        const uint32_t wmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr.z);
        if (tid == 0) {
            S.misc[0] = count; S.misc[2] = 0; S.misc[3] = 0; S.misc[4] = 0;
            if (wmax > kWindowReport) atomicMax(&A.tile_ctl[kCtlWindowMax], wmax);
        }
    } else {
        if (tid == 0) S.misc[5] = 0;
        look_blocks_up<NBX, NBY, false>(S, A, tid, box, boy, 0u);
        __syncthreads();
        scan_blocks<NBX, NBY, VB, 4u | 8u | 16u>(S, A, tid, record ? &S.misc[5] : nullptr);
        __syncthreads();
    }
    const uint32_t P = listed ? (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr.x)
                              : (uint32_t)__builtin_amdgcn_readfirstlane((int)S.misc[0]);
    const uint32_t n_owned = (uint32_t)__builtin_amdgcn_readfirstlane((int)W.owned);
    const uint32_t straggler_bit = stale ? kCodeStraggler : 0u;
    const uint32_t n_exc = stale ? min((uint32_t)__builtin_amdgcn_readfirstlane((int)W.exc), kExcSlots) : 0u;
    const uint32_t n_gho = ORD ? min((uint32_t)__builtin_amdgcn_readfirstlane((int)W.gho), kGhostSlots) : 0u;   // listed ghosts
    if (record && tid == 0) {
        // the header of the roster the gather below writes (an empty lookup is a valid, empty roster)
        const uint32_t count = P > (uint32_t)L::RAWCAP ? 0xFFFFFFFFu : P;
        A.roster_hdr[pt] = make_uint4(count, stamp_now, S.misc[5], 0u);   // (w: no hint)
    }
    {
        // nothing of its own to write?  (see process_tile: own blocks with the table of this step; the whole lookup
        // region and the straggler lists with a kept table)
        const uint32_t any_exc = n_exc;
        // (A tile that writes a roster goes through the gather for it even when nothing of this step's is its own.)
        if (stale ? (P == 0 && any_exc == 0) : (S.misc[1] == 0 && !(record && P != 0))) return true;
    }
    if (P > (uint32_t)L::RAWCAP) { GPE_BAIL(1); return false; }        // more looked-up particles than slots
    if (!listed) map_slots_to_blocks<NT, VB>(S, tid);
    __syncthreads();
    GPE_STAMP(0);

    // ---- P1: gather, keep, and file every membership straight into its cell's slots ---------------------------------
    // one membership: the counter's old value is the slot; the seventh member of a cell goes to the side list
    auto file = [&](const int zx, const int zy, const uint32_t s) {
#ifdef GPE_DBG_SKIP
        if (GPE_DBG_SKIP & 4) return;
#endif
        if ((unsigned)zx < (unsigned)ZX && (unsigned)zy < (unsigned)ZY) {
            // (zc < 4096: 24-bit multiply-adds, full rate, where the 32-bit multiply takes four issue slots)
            const uint32_t zc = mad_u24<ZX>((uint32_t)zy, (uint32_t)zx);
            const uint32_t k = S.cnt_inc((int)zc);
            if (k < (uint32_t)MS) S.mem[mad_u24<MS>(zc, k)] = (uint16_t)s;
            else {
                const uint32_t e = atomicAdd(&S.misc[4], 1u);
                if (e < (uint32_t)L::kBig) S.big[e] = (zc << 16) | s;
            }
        }
    };
    auto insert = [&](const uint32_t s, const float2 pp, const float pr, const uint32_t pid, const uint32_t lidv,
                      const int lx, const int ly, uint32_t over) {
        S.px[s] = pp.x; S.py[s] = pp.y; S.id[s] = pid;
        if constexpr (!L::kUniform) S.rad[s] = pr;
        if constexpr (L::kLid) S.lid[s] = lidv;
        S.own[s] = (lx >= HX && lx < HX + TX && ly >= HY && ly < HY + TY) ? 1 : 0;
        const int zx = lx - L::ZOX, zy = ly - L::ZOY;
        file(zx, zy, s);
        // phantom cells: the first three set bits of the overlap mask (grid.wgsl:68-90 keeps at most three); neighbour
        // k of the scan (y outer, x inner, centre skipped): dx = {-1,0,1,-1,1,-1,0,1}[k], dy = {-1,-1,-1,0,0,1,1,1}[k]
        // (`over` is the particle's entry of kPhantomTable: the gather looked it up)
        const int cnt = (int)(over & 3u);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j >= cnt) break;
            file(zx - 1 + (int)((over >> (2 + 4 * j)) & 3u), zy - 1 + (int)((over >> (4 + 4 * j)) & 3u), s);
        }
    };
    // what insert() takes as `over`: the table entry of the particle's overlap mask
    auto phantoms_of = [&](const uint32_t code) -> uint32_t { return kPhantomTable.v[(code >> kCodeOverlapShift) & 0xFFu]; };
#ifdef GPE_DBG_SKIP
    if (!(GPE_DBG_SKIP & 64))                                          // diagnostic builds: phase cost by omission (results wrong)
#endif
    for (uint32_t s0 = 0; s0 < P; s0 += (uint32_t)QP * NT) {
        uint32_t pid[QP], blk[QP], cc[QP];
        float2 pp[QP];
        float pr[QP];
        uint32_t lidq[QP], ph[QP];
        int lxq[QP], lyq[QP];
        bool keep[QP];
        uint32_t slot[QP];
        uint64_t mq[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            pid[q] = 0u; blk[q] = 0u; cc[q] = 0u; pr[q] = 0.f; lidq[q] = 0u; ph[q] = 0u;
            pp[q] = make_float2(0.f, 0.f);
            lxq[q] = 0; lyq[q] = 0; mq[q] = 0; keep[q] = false;
        }
        // the first NQ slots of the batch, from the ids to the keep votes: branch-free, each stage's loads issued together
        auto stage = [&](auto nq) {
            constexpr int NQ = decltype(nq)::value;
            if (listed) {                                              // (scalar)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint32_t sr = s0 + (uint32_t)tid + (uint32_t)q * NT;
                    uint32_t v = first_ids[q];
                    if (s0 != 0) v = A.roster_ids[roster_base + min(sr, P - 1u)];
                    pid[q] = sr < P ? v : 0u;                          // (what lies behind the roster's end is not an id)
                }
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {                         // branch-free, all loads in flight: see process_tile
                    const uint32_t s = min(s0 + (uint32_t)tid + (uint32_t)q * NT, P - 1u);
                    blk[q] = S.sblk[s];
                    pid[q] = A.sorted_ids[S.bstart[blk[q]] + (s - S.boff[blk[q]])];
                }
                if (record) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const uint32_t sr = s0 + (uint32_t)tid + (uint32_t)q * NT;
                        if (sr < P) A.roster_ids[roster_base + sr] = pid[q];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                pp[q] = A.pos_in[pid[q]];
                if constexpr (L::kUniform) pr[q] = 0.f; else pr[q] = A.radius[pid[q]];
                cc[q] = A.codes[pid[q]];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) lidq[q] = pid[q];
            if constexpr (ORD) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) pid[q] = A.order_keys[pid[q]];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) ph[q] = phantoms_of(cc[q]);   // (issued here: in flight under the keep votes)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const uint32_t s = s0 + (uint32_t)tid + (uint32_t)q * NT;
                lxq[q] = code_window_x(cc[q], ox);
                lyq[q] = code_window_y(cc[q], oy);
                // (voted comparison by comparison: see pair_response)
                mq[q] = ballot64(s < P) & ballot64(lxq[q] < RWX) & ballot64(lyq[q] < RWY) & ballot64((cc[q] & straggler_bit) == 0u);
                // (an order-key window: the kept table -- or the roster written from it -- may still list indices the owned
                // range has shrunk below: those particles are ghosts now, or gone; they come through the ghost list, or not at all)
                if constexpr (ORD) mq[q] &= ballot64(lidq[q] < n_owned);
                keep[q] = lanes_of(mq[q]);
            }
        };
        // (scalar) the slots of the batch that lie wholly beyond P for this wave -- ~873 looked-up ids on 512 threads: the
        // second slot of waves 6 and 7 -- are not loaded, decoded or voted on: nothing of them is kept (mq = 0).  One
        // copy of the stages per number of slots, so that the slots that run still issue each stage's loads together.
        const uint32_t wave_s0 = s0 + wave_first_thread(tid);
        if constexpr (QP == 2) {
            if (wave_s0 + (uint32_t)NT < P) stage(std::integral_constant<int, 2>());
            else if (wave_s0 < P) stage(std::integral_constant<int, 1>());
        } else {
            if (wave_s0 < P) stage(std::integral_constant<int, QP>());
        }
        take_slots(&S.misc[3], lane, (uint32_t)L::kSlots, mq, slot, keep);   // (over capacity: handed on below)
#pragma unroll
        for (int q = 0; q < QP; ++q)
            if (keep[q]) insert(slot[q], pp[q], pr[q], pid[q], lidq[q], lxq[q], lyq[q], ph[q]);
    }
    // One entry of a list the hash kernel handed to the tile -- a straggler, a listed ghost: fetched, placed by its cell
    // (`cell_of`: the entry's or the code word's), given a slot, filed.  (Called by whole waves: the slots use ballots.)
    auto take_listed = [&](const bool have, const uint32_t lidv, auto cell_of) {
        const float2 pp = A.pos_in[lidv];
        float pr = 0.f;
        if constexpr (!L::kUniform) pr = A.radius[lidv];
        const uint32_t cc = A.codes[lidv];
        uint32_t pid = lidv;
        if constexpr (ORD) pid = A.order_keys[lidv];
        int lx, ly;
        cell_of(cc, lx, ly);
        const uint64_t mk = ballot64(have) & ballot64((uint32_t)lx < (uint32_t)RWX) & ballot64((uint32_t)ly < (uint32_t)RWY);
        bool keep = lanes_of(mk);
        const uint32_t sl = take_slots(&S.misc[3], lane, (uint32_t)L::kSlots, mk, keep);
        if (keep) insert(sl, pp, pr, pid, lidv, lx, ly, phantoms_of(cc));
    };
    if (n_exc != 0 && tid < 64) {                                      // stragglers: out of reach of the block that lists them
        const bool have = (uint32_t)tid < n_exc;
        const uint2 en = A.exc_entry[(uint64_t)pt * kExcSlots + (have ? (uint32_t)tid : 0u)];
        take_listed(have, en.x, [&](uint32_t, int &lx, int &ly) { lx = (int)(en.y & 0xFFFFu) - ox; ly = (int)(en.y >> 16) - oy; });
    }
    if constexpr (ORD) {
        // the ghosts listed for the tile: placed by the cell in their code word
        for (uint32_t g0 = 0; g0 < n_gho; g0 += (uint32_t)NT) {        // (scalar bounds: whole waves)
            const uint32_t gi = g0 + (uint32_t)tid;
            const bool have = gi < n_gho;
            take_listed(have, A.gho_entry[(uint64_t)pt * kGhostSlots + (have ? gi : 0u)],
                        [&](uint32_t cc, int &lx, int &ly) { lx = code_window_x(cc, ox); ly = code_window_y(cc, oy); });
        }
    }
    __syncthreads();
    GPE_STAMP(1);
    const uint32_t PS = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.misc[3]);
    if (PS > (uint32_t)L::kSlots) { GPE_BAIL(2); return false; }       // more kept particles than the window stages
    if (PS == 0) return true;
    const uint32_t n_big = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.misc[4]);
    if (n_big > (uint32_t)L::kBig) { GPE_BAIL(3); return false; }      // crowded cells: process_tile's windows take it

    // the tile's own particles and their previous positions: fetched here, used in P6
    constexpr int QOWN = (L::kSlots + NT - 1) / NT;
    uint32_t own_id[QOWN];
    float2 own_prev[QOWN];
    fetch_own<ORD, NT, 1>(S, A, tid, PS, n_owned, own_id, own_prev);

    // ---- P4: active cells per colour (the walk of process_tile over the 2 x 2 colour groups; a cell's member count is
    //          its counter).  List entry: zone cell | class data << 12: cells of 2-3 members (one lane each; bit 12: three)
    //          from the front, cells of 4-6 (a lane group; members - 4) from the back; cells of 7-64 in the wave list.
#ifdef GPE_DBG_SKIP
    if (!(GPE_DBG_SKIP & 2))
#endif
    {
        constexpr int ZW = ZX / 2, ZH = ZY / 2, QC = ZW * ZH;
        static_assert(QC == QZ && NZ < 4096, "list entries: 12 bits of cell");
        for (int base = 0; base < QC; base += NT) {
            // (scalar) a wave without a colour group in this round -- QC = 360 groups on 512 threads: waves 6 and 7 -- goes
            // on to the barrier: its masks and their eight counts would all be 0, it adds to no counter and stores nothing
            if (base + (int)wave_first_thread(tid) >= QC) continue;
            const int i = base + tid;
            const int gx2 = 2 * (i % ZW), gy2 = 2 * (i / ZW);          // zone coordinates of the group's first cell
            int zc[4];
            uint32_t cnt[4];
            static_assert(ZX % 2 == 0, "the two cells of a group's row share a counter word");
            {
                const int z0 = gy2 * ZX + gx2;                         // even
                zc[0] = z0; zc[1] = z0 + 1; zc[2] = z0 + ZX; zc[3] = z0 + ZX + 1;
                if constexpr (L::kWordCounters) {
                    // a row's two counters are one aligned 64-bit read
                    uint2 r0 = make_uint2(0u, 0u), r1 = make_uint2(0u, 0u);
                    if (i < QC) {
                        r0 = *reinterpret_cast<const uint2 *>(&S.cntw[z0]);
                        r1 = *reinterpret_cast<const uint2 *>(&S.cntw[z0 + ZX]);
                    }
                    cnt[0] = r0.x; cnt[1] = r0.y; cnt[2] = r1.x; cnt[3] = r1.y;
                } else {
                    const uint32_t w0 = (i < QC) ? S.cntw[z0 >> 1] : 0u, w1 = (i < QC) ? S.cntw[(z0 + ZX) >> 1] : 0u;
                    cnt[0] = w0 & 0xFFFFu; cnt[1] = w0 >> 16; cnt[2] = w1 & 0xFFFFu; cnt[3] = w1 >> 16;
                }
            }
            // (the classes as lane masks, voted comparison by comparison: see pair_response)
            uint64_t ms[4], mg[4];
            bool single[4], group[4];
            const uint64_t in_m = ballot64(i < QC);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int lx = gx2 + (c & 1) + L::ZOX, ly = gy2 + (c >> 1) + L::ZOY;   // window coordinates
                const int gxx = ox + lx, gyy = oy + ly;
                const int exl = HX - lx, exr = lx - (HX + TX - 1), eyl = HY - ly, eyr = ly - (HY + TY - 1);
                const uint64_t zone_m = ballot64(exl <= kConeLeft - c) & ballot64(exr <= kConeRight - c) &
                                        ballot64(eyl <= kConeDown - (c >> 1)) & ballot64(eyr <= kConeUp - (c >> 1));
                // morton(-1,-1) == 0xFFFFFFFF == UNUSED_CELL_ID: never a collision cell (collision_cell_builder.wgsl:56).
                // Cell (-1, -1) lies in the zone of tile (0, 0) alone (the box has at most 65000 cells per axis, so no
                // other coordinate ends in 0xFFFF): a scalar test spares every other tile the comparisons.
                uint64_t alias_m = 0;
                if (tx == 0 && ty == 0) alias_m = ballot64((gxx & 0xFFFF) == 0xFFFF) & ballot64((gyy & 0xFFFF) == 0xFFFF);
                const uint64_t act_m = in_m & ballot64(cnt[c] >= 2u) & zone_m & ~alias_m;
                const uint64_t wave_m = act_m & ballot64(cnt[c] > (uint32_t)MS);
                mg[c] = act_m & ballot64(cnt[c] >= kGroupMin) & ~wave_m;
                ms[c] = act_m & ~mg[c] & ~wave_m;
                group[c] = lanes_of(mg[c]);
                single[c] = lanes_of(ms[c]);
                if (wave_m != 0) {                                     // (scalar: rare)
                    if (lanes_of(wave_m)) {
                        if (cnt[c] > 64u) { S.misc[2] = 1u; GPE_BAIL(4); }   // a pile: the sub-tile windows resolve those
                        const uint32_t k = atomicAdd(&S.lcnt[8 + c], 1u);
                        if (k < (uint32_t)L::WC) S.wlist[c * L::WC + k] = (uint16_t)zc[c]; else { S.misc[2] = 1u; GPE_BAIL(5); }
                    }
                }
            }
            // the eight list counters (colour x class) are bumped by eight lanes at once: the counts are scalars, each
            // written into its lane by one v_writelane
            int mine = 0;
            write_lane<0>(mine, (int)__popcll(ms[0])); write_lane<1>(mine, (int)__popcll(ms[1]));
            write_lane<2>(mine, (int)__popcll(ms[2])); write_lane<3>(mine, (int)__popcll(ms[3]));
            write_lane<4>(mine, (int)__popcll(mg[0])); write_lane<5>(mine, (int)__popcll(mg[1]));
            write_lane<6>(mine, (int)__popcll(mg[2])); write_lane<7>(mine, (int)__popcll(mg[3]));
            uint32_t mybase = 0;
            if (lane < 8 && mine) mybase = atomicAdd(&S.lcnt[lane], (uint32_t)mine);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t bs = (uint32_t)__builtin_amdgcn_readlane((int)mybase, c);
                const uint32_t bg = (uint32_t)__builtin_amdgcn_readlane((int)mybase, 4 + c);
                if (single[c]) S.list[c * QZ + bs + popc_below_lane(ms[c])] = (uint16_t)(zc[c] | ((cnt[c] == 3u) ? 0x1000 : 0));
                if (group[c]) S.list[c * QZ + (QZ - 1) - (bg + popc_below_lane(mg[c]))] = (uint16_t)(zc[c] | ((cnt[c] - kGroupMin) << 12));
            }
        }
    }
    __syncthreads();
    GPE_STAMP(4);
    if (S.misc[2]) return false;

    // ---- P5: the four colour passes (collision_solver.rs:224) ----------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t ns = S.lcnt[k], group_lanes = S.lcnt[4 + k] * kGroupLanes;
        const uint32_t nw = min(S.lcnt[8 + k], (uint32_t)L::WC);
        const uint32_t single_base = (group_lanes + 63u) & ~63u;      // waves are all-group or all-single
        const uint32_t work = single_base + ns;
        for (uint32_t i0 = 0; i0 < work; i0 += NT) {
            const uint32_t i = i0 + (uint32_t)tid;
#ifdef GPE_DBG_SKIP
            if (GPE_DBG_SKIP & 1) continue;
            if ((GPE_DBG_SKIP & 8) && i < group_lanes) continue;
            if ((GPE_DBG_SKIP & 16) && i >= group_lanes) continue;
#endif
            if (i < group_lanes) {
                const uint32_t en = S.list[k * QZ + (QZ - 1) - (i / kGroupLanes)];
                resolve_group<MS>(S, __umul24(en & 0xFFFu, (uint32_t)MS), (en >> 12) + kGroupMin, (int)(i % kGroupLanes), A.stiffness, U);
            } else if (i >= single_base && (i & ~63u) < work) {         // (whole waves: the walk uses ballots)
                const bool on = i < work;
                uint32_t b = 0, n = 0;
                if (on) {
                    const uint32_t en = S.list[k * QZ + (i - single_base)];
                    b = __umul24(en & 0xFFFu, (uint32_t)MS); n = 2u + (en >> 12);
                }
                resolve_small_cells(S, on, b, n, A.stiffness, U);
            }
        }
        for (uint32_t i = (uint32_t)(NW - 1 - (tid >> 6)); i < nw; i += NW) {     // wave-uniform
            // a cell of 7..64 members: its first six from its own slots, the others from the side list, into the wave's
            // scratch run of the member array; then the whole-wave walk
            const uint32_t zc = S.wlist[k * L::WC + i];
            const uint32_t n = S.cnt_get((int)zc);
            const uint32_t wb = (uint32_t)(MS * NZ) + (uint32_t)(tid >> 6) * 64u;
            if (lane < MS) S.mem[wb + lane] = S.mem[__umul24(zc, (uint32_t)MS) + (uint32_t)lane];
            uint32_t filled = MS;
            for (uint32_t e0 = 0; e0 < n_big; e0 += 64u) {
                const uint32_t e = e0 + (uint32_t)lane;
                const uint32_t v = e < n_big ? S.big[e] : 0xFFFFFFFFu;
                const bool hit = e < n_big && (v >> 16) == zc;
                const uint64_t mh = ballot64(hit);
                if (hit) S.mem[wb + filled + popc_below_lane(mh)] = (uint16_t)(v & 0xFFFFu);
                filled += (uint32_t)__popcll(mh);
            }
            wave_lds_order();
            resolve_wave(S, wb, n, A.stiffness, U);                    // (filled == n: every membership is in one of the two)
            wave_lds_order();
        }
        __syncthreads();
        GPE_STAMP(9 + k);
    }

    // ---- P6: write the tile's own particles back, K12 applied ----------------------------------------------------------
    write_own_back<ORD, NT, 1>(S, A, tid, PS, n_owned, ORD && A.pack.on != 0u, own_id, own_prev, U);
    __syncthreads();
    GPE_STAMP(6);
    return true;
}

#ifndef GPE_CAP_DIRECT
#define GPE_CAP_DIRECT 928
#endif
#ifndef GPE_CAP_DIRECT_ORD
#define GPE_CAP_DIRECT_ORD 880                 // order-key windows: 21 B per particle instead of 17, five member slots per cell
#endif
// 32 x 32-cell tiles on 512 threads, four workgroups per CU.  A tile the window has no room for is listed for
// k_collide_overflow.  (64 x 32-cell tiles on 1024 threads -- two per CU, the window 1.32 x the tile's own cells instead of
// 1.48 x -- were built, are exact and 5-6.5 % slower: profiles/r03/ab_wide_tiles_64x32_1024_threads_rejected.txt, the
// code in profiles/r04/wide_tiles_64x32_removed.patch.)
// Which tile does workgroup `wg` of the dense launch take?  Workgroups go round the eight XCDs (wg mod 8), and the tiles an
// XCD works through should be neighbours -- they share halo particles in that XCD's L2 -- so every XCD walks BANDS of
// A.band_tiles consecutive tiles (row-major: about two tile rows), band b belonging to XCD b mod 8, from the bottom of the
// box to its top.  (Rounds 1-3 gave each XCD one contiguous eighth of the rows.  A scene stratified in y -- anything
// under gravity: a crushed pile at the bottom, free fall above, nothing at the top -- then loads the XCDs so unevenly that
// the launch took twice the time its work amounts to: 6.4 ms for 3.3 ms of workgroup time at step 1250 of the 100 M
// soak, profiles/r04/tile_cycles_*.txt.)  Returns false when the workgroup has no tile.
__device__ __forceinline__ bool dense_launch_tile(const CollideArgs &A, const uint32_t wg, int *tx, int *ty)
{
    const uint32_t xcd = wg & 7u, j = wg >> 3;
    const uint32_t band = (j / A.band_tiles) * 8u + xcd;               // the j-th tile of this XCD lies in this band
    const uint32_t t = band * A.band_tiles + j % A.band_tiles;
    if (t >= (uint32_t)A.tiles_x * (uint32_t)A.tiles_y) return false;
    *tx = A.tile_x0 + (int)(t % (uint32_t)A.tiles_x);
    *ty = A.tile_y0 + (int)(t / (uint32_t)A.tiles_x);
    return true;
}
// The band size for a tile grid: bands a multiple of eight (every XCD the same number, so the busiest XCD has at most a
// band's remainder more than its share: 30 tile rows of 87 in whole rows give six XCDs 348 tiles and two 261 -- +6.7 % on
// the busiest against the 326 of an even deal; bands of 82 tiles give 328), about two tile rows each, at least four per XCD.
uint32_t dense_launch_band(uint32_t tiles_x, uint32_t tiles_y, bool eighths)
{
    const uint64_t total = (uint64_t)tiles_x * tiles_y;
    const uint64_t per_xcd = eighths ? 1u : std::max<uint64_t>(4u, (total + 8u * tiles_x) / (16ull * tiles_x));
    return (uint32_t)std::max<uint64_t>(1u, (total + 8u * per_xcd - 1u) / (8u * per_xcd));
}
// ... and the grid that covers every tile
uint32_t dense_launch_grid(uint32_t tiles_x, uint32_t tiles_y, uint32_t band_tiles)
{
    const uint64_t total = (uint64_t)tiles_x * tiles_y;
    const uint64_t bands = (total + band_tiles - 1) / band_tiles;
    return (uint32_t)(((bands + 7u) / 8u) * band_tiles * 8u);
}

// (three workgroups per CU: 80 VGPRs and 53 KB of LDS each -- room for 2000 particles, what a half of a tile at ~6 x the
// benchmark density keeps; an order-key window pays 4 more bytes per particle)
#ifndef GPE_CAP_HALF
#define GPE_CAP_HALF 2000
#endif
#ifndef GPE_CAP_HALF_ORD
#define GPE_CAP_HALF_ORD 1680
#endif
#ifndef GPE_CAP_HALF_FRONT
#define GPE_CAP_HALF_FRONT 1392                 // a half redone by the dense launch's front workgroups (kCtlHints): the tile's LDS
#endif
#ifndef GPE_CAP_HALF_FRONT_ORD
#define GPE_CAP_HALF_FRONT_ORD 1192             // ... of an order-key (sharded) run: 21 bytes per particle in 40 748
#endif
// The uniform windows carry a word per zone-cell counter (TileDirect::kWordCounters): the tile still leaves four workgroups
// a CU their LDS, the half of the half-tile launch three, as before.
static_assert(sizeof(TileDirect<32, 32, GPE_CAP_DIRECT, false, 512, true>) <= 40960, "uniform tile: four workgroups per CU");
static_assert(sizeof(TileDirect<32, 16, GPE_CAP_HALF, false, 512, true>) <= 163840 / 3, "uniform half: three workgroups per CU");
static_assert(sizeof(TileDirect<32, 16, GPE_CAP_HALF_FRONT, false, 512, true>) <= 40960, "uniform half of a hinted tile: in the tile's LDS");
// Registers a tile that ran over for the front workgroups of the next step's dense launch (kCtlHints).
__device__ __forceinline__ void hint_tile(const CollideArgs &A, const int tx, const int ty, const uint32_t age = 0u)
{
    if (A.hints_on == 0u || !A.tb.holds(tx, ty) || (uint32_t)tx >= 2048u || (uint32_t)ty >= 2048u) return;
    const uint32_t next = A.hint_parity ^ 1u;
    const uint32_t k = atomicAdd(&A.tile_ctl[kCtlHints + next], 1u);
    if (k >= kHintMax) return;
    A.hints[next * kHintMax + k] = (age << 22) | ((uint32_t)ty << 11) | (uint32_t)tx;
    A.roster_hdr[A.tb.index(tx, ty)].w = A.step_stamp + 1u;
}

// HINTS: the launch carries front workgroups for the registered tiles (kCtlHints) -- a kernel of its own, launched only
// while such tiles exist: the plain kernel is 3 % faster without the code (48.0 against 49.5 us at 1 M).
// UNI: the windows without a radius array (TileDirect), the hinted halves included: launched while the context's radii are
// one ordinary number (CollideArgs::uniform).
template <int TX, int CAP, bool ORD, int NT, bool HINTS = false, bool UNI = false>
__global__ __launch_bounds__(NT, 8) void k_collide_direct(CollideArgs A)
{
    // (The half-tile form of the hinted tiles lives in the tile's own LDS: 40 928 bytes, four workgroups per CU, hold a
    // half of 1392 particles -- 59 % of a tile's window at 1.5 x its capacity; the half-tile launch's 2000 would make it
    // 51 KB and three per CU: 54.2 instead of 47.8 us at 1 M, profiles/r04/ab_hints_bisect.txt.)
    struct NoHalf { char unused; };
    using Half = typename std::conditional<HINTS, TileDirect<32, 16, ORD ? GPE_CAP_HALF_FRONT_ORD : GPE_CAP_HALF_FRONT, ORD, 512, UNI>, NoHalf>::type;
    using Tile = TileDirect<TX, 32, CAP, ORD, NT, UNI>;
    // (the uniform window has no radius array and is 3.7 KB smaller; the half form was sized for the general tile's LDS,
    // which four workgroups per CU have room for either way)
    __shared__ union { Tile tile; Half half; } u;
    Tile &S = u.tile;
    static_assert(UNI || (sizeof(Half) <= sizeof(Tile) && alignof(Half) <= alignof(Tile)), "the half form fits the tile's LDS");
    static_assert(sizeof(u) <= 40960, "four workgroups per CU");
    uint32_t wg = blockIdx.x;
    if constexpr (HINTS) {
        if (wg < A.front_wgs) {
            // half (wg & 1) of hinted tile wg >> 1
            const uint32_t count = min(A.tile_ctl[kCtlHints + A.hint_parity], kHintMax);
            if ((wg >> 1) >= count) return;
            const uint32_t tile = A.hints[A.hint_parity * kHintMax + (wg >> 1)];
            const int htx = (int)(tile & 0x7FFu), hty = (int)((tile >> 11) & 0x7FFu);
            const uint32_t age = tile >> 22;
            if (!A.tb.holds(htx, hty)) return;
            const uint32_t hinted_for = A.roster_hdr[A.tb.index(htx, hty)].w;   // (not registered for this launch: its own workgroup takes it)
            if (hinted_for != A.step_stamp && hinted_for != A.step_stamp + 1u) return;
            const int hy = hty * 2 + (int)(wg & 1u);
            const bool done = process_tile_direct<ORD>(u.half, A, htx, hy);
            if (threadIdx.x == 0) {
                if (!done) hand_tile_on(A, kCtlOverflow2, A.overflow2, 2u * A.overflow1_cap, htx, hy);
                // again in the next launch, kHintAge launches long
                if ((wg & 1u) == 0u && age + 1u < kHintAge) hint_tile(A, htx, hty, age + 1u);
            }
            return;
        }
        wg -= A.front_wgs;                                             // (a multiple of 8: the XCD of a tile stays)
    }
    int tx, ty;
    if (!dense_launch_tile(A, wg, &tx, &ty)) return;
#ifdef GPE_TILE_CYCLES
    const long long tc0 = clock64();
#endif
    const bool done = process_tile_direct<ORD, Tile, HINTS>(S, A, tx, ty);
#ifdef GPE_TILE_CYCLES
    if (g_tile_cycles && threadIdx.x == 0 && A.tb.holds(tx, ty)) {
        uint4 *e = &g_tile_cycles[A.tb.index(tx, ty)];
        e->x = (uint32_t)(clock64() - tc0); e->y = done ? 0u : 1u; e->z = 0u; e->w = S.misc[0];
    }
#endif
    if (!done) {
        // (the launch that takes the tile off list 1 -- half tiles or over-capacity windows -- registers it: kCtlHints)
        if (threadIdx.x == 0) hand_tile_on(A, kCtlOverflow1, A.overflow1, A.overflow1_cap, tx, ty);
    }
}

// The frame of a sharded rank's tile grid (CollideArgs::frame_*), one workgroup per tile: the tiles whose particles may
// have to be packed for the neighbours.  Launched BEFORE the interior tiles so that the exchange can start while those
// are resolved; everything such a tile needs happens in this launch -- a tile the direct-slot form has no room for is
// redone on the spot as four 16x16 quarters (the over-capacity launch would pack its particles after the segments left).
template <bool ORD>
__global__ __launch_bounds__(512, 6) void k_collide_border(CollideArgs A)
{
    __shared__ union { TileDirect<32, 32, ORD ? GPE_CAP_DIRECT_ORD : GPE_CAP_DIRECT, ORD, 512> tile; OverflowLds<ORD> windows; } u;
    // frame tile t: the bottom rows, the top rows, then the left and right columns of the rows between
    const uint32_t nx = (uint32_t)A.tiles_x, ny = (uint32_t)A.tiles_y;
    const uint32_t fb = (uint32_t)A.frame_b, ft = (uint32_t)A.frame_t, fl = (uint32_t)A.frame_l, fr = (uint32_t)A.frame_r;
    uint32_t t = blockIdx.x, x, y;
    if (t < fb * nx) { x = t % nx; y = t / nx; }
    else if (t < (fb + ft) * nx) { t -= fb * nx; x = t % nx; y = ny - ft + t / nx; }
    else {
        t -= (fb + ft) * nx;
        const uint32_t w = fl + fr;
        if (w == 0 || t / w >= ny - fb - ft) return;
        const uint32_t col = t % w;
        x = col < fl ? col : nx - fr + (col - fl);
        y = fb + t / w;
    }
    const int tx = A.tile_x0 + (int)x, ty = A.tile_y0 + (int)y;
    if (process_tile_direct<ORD>(u.tile, A, tx, ty)) return;
    __syncthreads();
    for (int q = 0; q < 4; ++q) resolve_quarter<ORD>(u.windows, A, tx * 2 + (q & 1), ty * 2 + (q >> 1));
}

// Level 0: one workgroup per 32x32 tile, tiles dealt so that each XCD (blockIdx % 8) works through a
// contiguous run of tile rows (neighbouring tiles share halo particles in that XCD's L2).
template <int T, int CAP, bool ORD>
__global__ __launch_bounds__(kNatThreads, 2048 / kNatThreads * 2) void k_collide_dense(CollideArgs A)
{
    __shared__ TileLds<T, CAP, ORD> S;
    int tx, ty;
    if (!dense_launch_tile(A, blockIdx.x, &tx, &ty)) return;
    // A tile whose window exceeds the capacity returns early and is listed for k_collide_overflow.  (Redoing it
    // here, quarter by quarter, on steps whose statistics let the host skip that launch: the extra code costs this
    // kernel 3 % at 1 M and 5 % at 100 M, more than the 4.5 us launch: profiles/r02/ab_inline_fallback_rejected.txt.)
    if (!process_tile<ORD>(S, A, tx, ty)) {
        if (threadIdx.x == 0) hand_tile_on(A, kCtlOverflow1, A.overflow1, A.overflow1_cap, tx, ty);
    }
}

// The 32x32 tiles the dense launch handed on, each redone as two 32x16 halves in the direct-slot form (CollideArgs::
// overflow2): a ticketed grid like the over-capacity launch's, only launched while the host's lagged statistic reports
// such tiles.  A half that does not fit either is listed for the over-capacity launch's 16x16 / 8x8 windows.
// (Why: one tile a little over 928 particles used to cost the step a whole over-capacity launch -- a counting-sort 16x16
// window takes ~30 us whatever it holds, behind the dense launch: +40 % on the 1 M step once the undamped benchmark cloud
// has clumped, from step ~1000 on.  A half costs what a dense-launch tile costs, ~10 us.)
template <bool ORD, bool UNI = false>
__global__ __launch_bounds__(512, 6) void k_collide_halves(CollideArgs A)
{
    __shared__ TileDirect<32, 16, ORD ? GPE_CAP_HALF_ORD : GPE_CAP_HALF, ORD, 512, UNI> S;
    __shared__ uint32_t s_item;
    uint32_t count = A.tile_ctl[kCtlOverflow1];
    if (count > A.overflow1_cap) count = A.overflow1_cap;
    const uint32_t work = count * 2u;
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&A.tile_ctl[kCtlHalfTicket], 1u);
        __syncthreads();
        const uint32_t i = s_item;
        __syncthreads();
        if (i >= work) break;
        const uint32_t parent = A.overflow1[i >> 1];
        const int tx = (int)(parent & 0xFFFFu), ty = (int)((parent >> 16) * 2u + (i & 1u));
        if ((i & 1u) == 0u && threadIdx.x == 0) hint_tile(A, tx, (int)(parent >> 16));   // (for the next dense launch: kCtlHints)
        const bool done = process_tile_direct<ORD>(S, A, tx, ty);
        __syncthreads();
        if (!done && threadIdx.x == 0) hand_tile_on(A, kCtlOverflow2, A.overflow2, 2u * A.overflow1_cap, tx, ty);
    }
}

// Over-capacity 32x32 tiles are redone by a fixed grid that takes work items off the device-side list (HIP has no
// indirect dispatch): one work item per 16x16 quarter.  One launch, nothing to wait for.
// (Eight waves per SIMD = 64 VGPRs: the kernel spills -- the item loop keeps the arguments of three inlined tile
// walks live -- and is still faster than with 85 or 128 VGPRs and three or two workgroups per CU: 12.1 against 13.1 /
// 15.2 ms in the compressed 100 M scene, profiles/r02/soak_1500_overflow_kernel_register_budget.txt.)
template <bool ORD>
__global__ __launch_bounds__(kNatThreads, GPE_OVF_WAVES) void k_collide_overflow(CollideArgs A)
{
    __shared__ OverflowLds<ORD> u;
    __shared__ uint32_t s_item;
    // work items: the four quarters of every tile of list 1 (unless the half-tile launch took that list), then the two
    // of every half of list 2 (CollideArgs)
    const uint32_t count1 = A.quarters_of_halves != 0u ? 0u : min(A.tile_ctl[kCtlOverflow1], A.overflow1_cap);
    const uint32_t count2 = min(A.tile_ctl[kCtlOverflow2], 2u * A.overflow1_cap);
    const uint32_t work1 = count1 * 4u, work = work1 + count2 * 2u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the hints this collide launch has used: counted for the statistics, the list free for the launch after the next
        const uint32_t used = min(A.tile_ctl[kCtlHints + A.hint_parity], kHintMax);
        A.tile_ctl[kCtlHintsSeen] = A.front_wgs != 0u ? used : 0u;
        A.tile_ctl[kCtlHints + A.hint_parity] = 0u;
    }
    if (work == 0) return;
    // Work items are taken from a ticket counter: their durations differ by orders of magnitude (in a compressed scene
    // the lower quarters of a tile hold several times the particles of the upper ones), and a fixed stride of 1024
    // gives a workgroup the same quarter of every tile it meets.
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&A.tile_ctl[kCtlOverflowTicket], 1u);
        __syncthreads();
        const uint32_t i = s_item;
        __syncthreads();
        if (i >= work) break;
        // the quarter, in 16-cell units, and its 32x32 tile
        uint32_t qx, qy;
        if (i >= work1) { const uint32_t h = A.overflow2[(i - work1) >> 1]; qx = (h & 0xFFFFu) * 2u + (i & 1u); qy = h >> 16; }
        else {
            const uint32_t parent = A.overflow1[i >> 2]; qx = (parent & 0xFFFFu) * 2u + (i & 1u); qy = (parent >> 16) * 2u + ((i >> 1) & 1u);
            if ((i & 3u) == 0u && threadIdx.x == 0) hint_tile(A, (int)(parent & 0xFFFFu), (int)(parent >> 16));   // (kCtlHints)
        }
#ifdef GPE_TILE_CYCLES
        const long long tq0 = clock64();
#endif
        resolve_quarter<ORD>(u, A, (int)qx, (int)qy);
#ifdef GPE_TILE_CYCLES
        if (g_tile_cycles && threadIdx.x == 0 && A.tb.holds((int)(qx >> 1), (int)(qy >> 1)))
            atomicAdd(&g_tile_cycles[A.tb.index((int)(qx >> 1), (int)(qy >> 1))].z, (uint32_t)(clock64() - tq0));
#endif
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (native_launch.h): the host side of the native step (gpe_native.hip) starts the kernels through these
// ---------------------------------------------------------------------------------------------------
void launch_native_hash(gpe_ctx *c, bool ghosts, int grid, const float2 *pos, const float *radius, bool uniform,
                        float uniform_r, uint64_t n, const uint32_t *n_valid_ptr, float cell_size, int32_t gx, int32_t gy, int32_t bx0, int32_t by0,
                        int32_t blocks_x, int32_t blocks_y, uint32_t pad_key, uint32_t *keys, uint32_t *codes, int digits,
                        uint32_t *hist4, uint32_t *hist_next, uint32_t *os_ctl, uint32_t *tile_ctl, uint4 *table2,
                        uint64_t table_pairs, uint32_t *host_stat, const uint32_t *sorted_key, uint32_t parity,
                        uint64_t div_magic, uint32_t *exc_count, uint2 *exc_entry, uint32_t *exc_count_next, TileBox tb,
                        uint32_t straggler_limit, uint32_t fuse_always, const HashGhosts &G, bool index64)
{
    unsigned long long *stamp = scope_stamp_for_next_launch(c);
    note_enqueue(c);
    // 32-bit indices while every index the kernel's loop forms -- up to kHashBatch strides past n -- stays below 2^31
    // (index64: GPE_FLAG_HASH_INDEX64 asks for the 64-bit form regardless; the two give the same bits)
    const bool narrow = !index64 && n + (uint64_t)grid * kHashBlock * kHashBatch < (1ull << 31);
    // (uniform: the ordinary instantiation's only; a sharded run keeps the general kernels)
    const auto hash_kernel = ghosts ? (narrow ? k_native_hash<true, uint32_t> : k_native_hash<true, uint64_t>)
                             : uniform ? (narrow ? k_native_hash<false, uint32_t, true> : k_native_hash<false, uint64_t, true>)
                                       : (narrow ? k_native_hash<false, uint32_t> : k_native_hash<false, uint64_t>);
    (void)div_magic;                                                   // (the kernel has not divided since the radix pass does)
    hipLaunchKernelGGL(hash_kernel, dim3(grid), dim3(kHashBlock), 0, c->stream, pos, radius, n, n_valid_ptr, cell_size, gx,
                       gy, bx0, by0, blocks_x, blocks_y, pad_key, keys, codes, digits, hist4, hist_next, os_ctl, tile_ctl,
                       table2, table_pairs, host_stat, sorted_key, parity, uniform_r, exc_count, exc_entry, exc_count_next,
                       tb, straggler_limit, fuse_always, G, stamp);
}

void launch_native_hist_gated(gpe_ctx *c, int grid, uint32_t *keys, uint64_t n, int digits, uint32_t *hist4,
                              const uint32_t *need, const HistKeys &K)
{
    unsigned long long *stamp = scope_stamp_for_next_launch(c);
    note_enqueue(c);
    hipLaunchKernelGGL(k_native_hist_gated, dim3(grid), dim3(kHistGatedBlock), 0, c->stream, keys, n, digits, hist4, need,
                       stamp, K);
}

void launch_native_check_box(gpe_ctx *c, const float2 *pos, uint64_t n, const uint32_t *n_valid_ptr, float cell_size,
                             int32_t gx, int32_t gy, uint32_t *flag, const float *radius, uint32_t *radius_bits)
{
    note_enqueue(c);
    hipLaunchKernelGGL(k_native_check_box, dim3(stream_grid(n)), dim3(kStreamBlock), 0, c->stream, pos, n, n_valid_ptr,
                       cell_size, gx, gy, flag, radius, radius_bits);
}

void launch_native_window_max(gpe_ctx *c, const uint2 *table, uint32_t entries, int32_t blocks_x, int32_t blocks_y,
                              uint32_t *out_max)
{
    note_enqueue(c);
    hipLaunchKernelGGL(k_native_window_max, dim3(stream_grid(entries)), dim3(kStreamBlock), 0, c->stream, table, entries,
                       blocks_x, blocks_y, out_max);
}

void launch_native_publish_probe(gpe_ctx *c, uint32_t *tile_ctl, uint32_t *host_stat)
{
    note_enqueue(c);
    hipLaunchKernelGGL(k_native_publish_probe, dim3(1), dim3(64), 0, c->stream, tile_ctl, host_stat);
}

// (The cases stand in the order native_collide meets the forms: the kernels are instantiated, and the assembler's local
// labels numbered, in that order, and scripts/kernel_isa_diff.sh compares the labels too.)
void launch_collide(gpe_ctx *c, CollideForm form, uint32_t grid, const CollideArgs &A)
{
    note_enqueue(c);
    switch (form) {
    case CollideForm::DenseOrd:
        hipLaunchKernelGGL((k_collide_dense<kTileMain, kCapOrd, true>), dim3(grid), dim3(kNatThreads), 0, c->stream, A);
        break;
    case CollideForm::Dense:
        hipLaunchKernelGGL((k_collide_dense<kTileMain, kCapMain, false>), dim3(grid), dim3(kNatThreads), 0, c->stream, A);
        break;
    case CollideForm::BorderOrd:
        hipLaunchKernelGGL(k_collide_border<true>, dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::DirectOrd:
        hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT_ORD, true, 512>), dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::DirectOrdFront:
        hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT_ORD, true, 512, true>), dim3(grid), dim3(512), 0, c->stream, A);
        break;
    // (A.uniform: the windows without a radius array; the forms that have no such variant gather radii as ever -- a step may
    // mix the two, every pair's arithmetic is the same)
    case CollideForm::DirectFront:
        if (A.uniform)
            hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT, false, 512, true, true>), dim3(grid), dim3(512), 0, c->stream, A);
        else
            hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT, false, 512, true>), dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::Direct:
        if (A.uniform)
            hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT, false, 512, false, true>), dim3(grid), dim3(512), 0, c->stream, A);
        else
            hipLaunchKernelGGL((k_collide_direct<32, GPE_CAP_DIRECT, false, 512>), dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::HalvesOrd:
        hipLaunchKernelGGL(k_collide_halves<true>, dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::Halves:
        if (A.uniform) hipLaunchKernelGGL((k_collide_halves<false, true>), dim3(grid), dim3(512), 0, c->stream, A);
        else hipLaunchKernelGGL(k_collide_halves<false>, dim3(grid), dim3(512), 0, c->stream, A);
        break;
    case CollideForm::OverflowOrd:
        hipLaunchKernelGGL(k_collide_overflow<true>, dim3(grid), dim3(kNatThreads), 0, c->stream, A);
        break;
    case CollideForm::Overflow:
        hipLaunchKernelGGL(k_collide_overflow<false>, dim3(grid), dim3(kNatThreads), 0, c->stream, A);
        break;
    }
}

}  // namespace gpe

#ifdef GPE_TILE_CYCLES
// diagnostic builds only: start recording (out == NULL: a buffer of one uint4 per tile of the tile box is attached) or
// download what the last step recorded (out: tiles x 4 words; *tiles_x / *tiles_y the tile box)
extern "C" gpe_status gpe_debug_tile_cycles(gpe_ctx *c, uint32_t *out, uint64_t words, uint32_t *tiles_x, uint32_t *tiles_y)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    gpe::NativeState &N = c->native;
    uint4 *&buf = N.dbg_cycles;
    uint64_t &cap = N.dbg_cycles_cap;
    (void)hipStreamSynchronize(c->stream);
    const uint64_t tiles = N.exc_tiles;
    if (tiles_x) *tiles_x = (uint32_t)N.tb.nx;
    if (tiles_y) *tiles_y = (uint32_t)N.tb.ny;
    if (!out) {
        if (cap < tiles) { cap = 0; if (gpe::dev_release(c, buf) != hipSuccess || gpe::dev_reserve(c, &buf, tiles * sizeof(uint4), 0, "native.dbg_cycles") != hipSuccess) return GPE_ERR_HIP; cap = tiles; }
        (void)hipMemset(buf, 0, tiles * sizeof(uint4));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_tile_cycles), &buf, sizeof(buf));
        return GPE_OK;
    }
    if (!buf || words < tiles * 4) return GPE_ERR_INVALID_ARG;
    (void)hipMemcpy(out, buf, tiles * sizeof(uint4), hipMemcpyDeviceToHost);
    return GPE_OK;
}
#endif

#ifdef GPE_TILE_CYCLES
// diagnostic builds only: how often each reason handed a direct-slot tile on since the last call (1 looked up > 1536,
// 2 kept > capacity, 3 more than kBigCap memberships beyond a cell's slots, 4 a cell of more than 64 (lanes counted),
// 5 more than 16 cells of 7+ members in a colour (lanes counted))
extern "C" gpe_status gpe_debug_bail_reasons(gpe_ctx *c, uint32_t *out8)
{
    if (!c || !out8) return GPE_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(gpe::g_bail_reasons), 8 * sizeof(uint32_t));
    uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_bail_reasons), z, sizeof(z));
    return GPE_OK;
}
#endif

#ifdef GPE_DBG_RT
extern "C" gpe_status gpe_debug_skip(gpe_ctx *c, uint32_t mask)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_dbg_skip_rt), &mask, sizeof(mask));
    return GPE_OK;
}
#endif

#ifdef GPE_COUNT_PAIRS
// diagnostic builds only: (pairs walked, pairs resolved) since the last reset
extern "C" gpe_status gpe_debug_pair_counts(gpe_ctx *c, uint64_t *out2, int32_t reset)
{
    // out2 = (pairs walked, pairs resolved) since the last reset; reset != 0 also switches the counting on, reset < 0 off
    if (!c || !out2) return GPE_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(c->stream);
    static unsigned long long w[gpe::kPairCounters * 8], h[gpe::kPairCounters * 8];
    (void)hipMemcpyFromSymbol(w, HIP_SYMBOL(gpe::g_pairs_walked), sizeof(w));
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(gpe::g_pairs_hit), sizeof(h));
    out2[0] = out2[1] = 0;
    for (int i = 0; i < gpe::kPairCounters; ++i) { out2[0] += w[i * 8]; out2[1] += h[i * 8]; }
    if (reset) {
        memset(w, 0, sizeof(w));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_pairs_walked), w, sizeof(w));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_pairs_hit), w, sizeof(w));
        const uint32_t on = reset > 0 ? 1u : 0u;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(gpe::g_pairs_on), &on, sizeof(on));
    }
    return GPE_OK;
}
#endif
