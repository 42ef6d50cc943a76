// k_spawn.hip -- overlap-checked adds (gpe_add_particles_free): which of K candidate particles have room, decided on the
// device (gfx950, wave64) without downloading the N particles of the context.  The K candidates of a brush are few, so
// THEY are binned and the N particles stream past them once.
//
// Not on the per-step path, so the plain form:
//   (1) k_spawn_keys: key[i] = candidate i's clamped cell under the SEARCH cell size (2.2 x the larger of |max radius|
//       and the candidates' largest |radius|; contacts_axis of k_contacts.h, so positions at 1e30, +-inf and NaN have a
//       cell), val[i] = i, state[i] = OUTSIDE_WORLD or undecided, and the cell box of the candidates that passed the
//       world test (four atomicMin per wave into ctl[0..3]).
//   (2) sort_pairs (stable) on (key, val) and k_contacts_records over the candidate arrays: one 16-byte record (x, y,
//       radius, input index) per sorted slot -- the table of the contact query, built of the candidates.
//   (3) k_spawn_pass, the one pass over the N particles: a grid-stride loop with coalesced pos loads.  A particle takes
//       its clamped cell and leaves at once when that cell is outside the candidates' box grown by one; only the others
//       load their radius, find the three row runs of the candidate table (contacts_row_run) and store blocked[index] = 1
//       for every candidate they touch (in_contact).  Many lanes may store the same 1: a relaxed atomic store.
//       Bytes: R 8 B per particle, + 4 B and the table walk (L2) per particle inside the box.
//   (4) k_spawn_resolve: undecided -> BLOCKED_BY_PARTICLE where blocked, else ADDED (or stays undecided: SEPARATE).
//   (5) k_spawn_round, SEPARATE only: one launch is one round over the undecided candidates.  Candidate i looks at the
//       candidates of LOWER input index it touches: an ADDED one blocks it; if none of them is still undecided it is
//       ADDED; otherwise it waits.  A state only ever goes from undecided to its final value, and whenever a candidate
//       decides it decides what the sequential greedy rule (ascending index) gives it -- so the order in which lanes,
//       waves and launches see each other's states changes the number of rounds, never a verdict.  The lowest undecided
//       index always decides, so the rounds end.  A workgroup owns kSpawnBlock consecutive input indices and repeats
//       the round over them in LDS until none of them changes (it waits for nobody: it leaves as soon as an iteration
//       decides nothing).  The host reads the undecided counters every kSpawnRoundsPerLook rounds.
//       The number of rounds: a candidate depends on lower indices only, which lie in its own or a lower block, and a
//       block settles everything whose dependencies outside it are settled.  So the rounds are bounded by the number of
//       distinct blocks the longest chain of index-descending contacts (i touches j < i touches l < j ...) passes
//       through, at most ceil(K / kSpawnBlock).  The slow case is a long chain in ASCENDING index that spans many blocks
//       (a line or lattice finer than a diameter, painted in order): one block per round.  A random spray settles in a
//       handful.
//   (6) k_spawn_flags (the verdicts as bytes for the host, and the ADDED flags), inclusive_scan (k_scan.hip),
//       k_spawn_scatter: the ADDED candidates go to old_n + rank, in input order: pos, prev = pos and radius.
// Candidates the world test rejected stay in the sorted table on purpose: taking them out would need a compaction
// before the sort, and they cost only table length -- the pass may set their `blocked` flag, which k_spawn_resolve
// ignores, the cell box leaves them out, and a round never sees them as ADDED or undecided.
// The predicate and the row-run search are those of gpe_query_contacts (k_contacts.h), not restated here.
#include "k_contacts.h"

namespace gpe {

constexpr int kSpawnBlock = 256;                // consecutive input indices one workgroup of a round owns

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t spawn_key(float2 p, float cell_size)
{
    return (contacts_axis(p.y, cell_size) << 16) | contacts_axis(p.x, cell_size);
}

// (1)  The world test: a = |r|; x >= a && x <= W - a && y >= a && y <= H - a, binary32, one rounding per operation; a
// NaN anywhere fails it.
__global__ __launch_bounds__(kStreamBlock) void k_spawn_keys(const float2 *__restrict__ cpos,
                                                             const float *__restrict__ crad, uint32_t k, float cell_size,
                                                             float world_w, float world_h, uint32_t inside_world,
                                                             uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                             uint32_t *__restrict__ state, uint32_t *__restrict__ ctl)
{
#pragma clang fp contract(off)
    uint32_t lo_x = 0xFFFFFFFFu, lo_y = 0xFFFFFFFFu, hi_x = 0xFFFFFFFFu, hi_y = 0xFFFFFFFFu;   // hi_*: 65535 - max
    const uint32_t stride = gridDim.x * kStreamBlock;
    for (uint32_t i = blockIdx.x * kStreamBlock + threadIdx.x; i < k; i += stride) {
        const float2 p = cpos[i];
        const float a = fabsf(crad[i]);
        const float wx = world_w - a, wy = world_h - a;
        const bool inside = p.x >= a && p.x <= wx && p.y >= a && p.y <= wy;
        const bool out = inside_world != 0u && !inside;
        const uint32_t cx = contacts_axis(p.x, cell_size), cy = contacts_axis(p.y, cell_size);
        keys[i] = (cy << 16) | cx;
        vals[i] = i;
        state[i] = out ? (uint32_t)GPE_SPAWN_OUTSIDE_WORLD : kSpawnUndecided;
        if (!out) {
            lo_x = min(lo_x, cx); lo_y = min(lo_y, cy);
            hi_x = min(hi_x, (uint32_t)kContactsAxisMax - cx); hi_y = min(hi_y, (uint32_t)kContactsAxisMax - cy);
        }
    }
    lo_x = wave_min_u32(lo_x); lo_y = wave_min_u32(lo_y); hi_x = wave_min_u32(hi_x); hi_y = wave_min_u32(hi_y);
    if (lane_id() == 0 && lo_x != 0xFFFFFFFFu) {
        atomicMin(&ctl[0], lo_x); atomicMin(&ctl[1], lo_y); atomicMin(&ctl[2], hi_x); atomicMin(&ctl[3], hi_y);
    }
}

// (3)
__global__ __launch_bounds__(kStreamBlock) void k_spawn_pass(const float2 *__restrict__ pos,
                                                             const float *__restrict__ radius, uint64_t n,
                                                             float cell_size, const uint32_t *__restrict__ ckeys,
                                                             const uint4 *__restrict__ crec, uint32_t k,
                                                             const uint32_t *__restrict__ ctl,
                                                             uint32_t *__restrict__ blocked)
{
    if (ctl[0] == 0xFFFFFFFFu) return;                          // no candidate passed the world test
    // the candidates' cell box grown by one (clamped cells: 0 .. 65535)
    const uint32_t bx0 = ctl[0], by0 = ctl[1];
    const uint32_t bx1 = (uint32_t)kContactsAxisMax - ctl[2], by1 = (uint32_t)kContactsAxisMax - ctl[3];
    const uint32_t x0 = bx0 > 0u ? bx0 - 1u : 0u, y0 = by0 > 0u ? by0 - 1u : 0u;
    const uint32_t x1 = bx1 < (uint32_t)kContactsAxisMax ? bx1 + 1u : bx1, y1 = by1 < (uint32_t)kContactsAxisMax ? by1 + 1u : by1;
    const uint64_t stride = (uint64_t)gridDim.x * kStreamBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kStreamBlock + threadIdx.x; i < n; i += stride) {
        const float2 p = pos[i];
        const uint32_t cx = contacts_axis(p.x, cell_size), cy = contacts_axis(p.y, cell_size);
        if (cx < x0 || cx > x1 || cy < y0 || cy > y1) continue;
        const float r = radius[i];
        const uint32_t key = (cy << 16) | cx;
        for (int dy = -1; dy <= 1; ++dy) {
            uint32_t s, e, k_mid;
            if (!contacts_row_run(ckeys, k, key, dy, &s, &e, &k_mid)) continue;
            for (uint32_t j = s; j < e; ++j) {
                const uint4 o = crec[j];
                float q, rs;
                if (in_contact(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z), p.x, p.y, r, &q, &rs))
                    __hip_atomic_store(&blocked[o.w], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// (4)
__global__ __launch_bounds__(kStreamBlock) void k_spawn_resolve(uint32_t *__restrict__ state,
                                                                const uint32_t *__restrict__ blocked, uint32_t k,
                                                                uint32_t separate)
{
    const uint32_t stride = gridDim.x * kStreamBlock;
    for (uint32_t i = blockIdx.x * kStreamBlock + threadIdx.x; i < k; i += stride) {
        if (state[i] != kSpawnUndecided) continue;
        state[i] = blocked[i] ? (uint32_t)GPE_SPAWN_BLOCKED_BY_PARTICLE
                              : (separate ? kSpawnUndecided : (uint32_t)GPE_SPAWN_ADDED);
    }
}

// (5) one round; workgroup b owns the input indices [b * kSpawnBlock, (b + 1) * kSpawnBlock)
__global__ __launch_bounds__(kSpawnBlock) void k_spawn_round(const float2 *__restrict__ cpos,
                                                             const float *__restrict__ crad,
                                                             const uint32_t *__restrict__ ckeys,
                                                             const uint4 *__restrict__ crec, uint32_t k, float cell_size,
                                                             uint32_t *state, uint32_t *__restrict__ left)
{
    __shared__ uint32_t s_state[kSpawnBlock];
    const uint32_t base = blockIdx.x * kSpawnBlock, i = base + threadIdx.x;
    const uint32_t before = i < k ? state[i] : (uint32_t)GPE_SPAWN_ADDED;   // (only its own thread ever writes state[i])
    uint32_t mine = before;
    s_state[threadIdx.x] = mine;
    if (!__syncthreads_or(mine == kSpawnUndecided)) return;     // block-uniform: nothing of this block is open
    float x = 0.f, y = 0.f, r = 0.f;
    uint32_t run_s[3] = {0, 0, 0}, run_e[3] = {0, 0, 0};        // (an absent row: an empty run)
    if (mine == kSpawnUndecided) {
        const float2 p = cpos[i];
        x = p.x; y = p.y; r = crad[i];
        const uint32_t key = spawn_key(p, cell_size);
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            uint32_t s, e, k_mid;
            if (contacts_row_run(ckeys, k, key, row - 1, &s, &e, &k_mid)) { run_s[row] = s; run_e[row] = e; }
        }
    }
    for (;;) {
        bool changed = false;
        if (mine == kSpawnUndecided) {
            bool blocked = false, wait = false;
#pragma unroll
            for (int row = 0; row < 3; ++row) {
                for (uint32_t j = run_s[row]; j < run_e[row]; ++j) {
                    const uint4 o = crec[j];
                    float q, rs;
                    if (o.w >= i || !in_contact(x, y, r, __uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z), &q, &rs))
                        continue;
                    const uint32_t st = o.w >= base ? s_state[o.w - base]
                                                    : __hip_atomic_load(&state[o.w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    blocked |= st == (uint32_t)GPE_SPAWN_ADDED;
                    wait |= st == kSpawnUndecided;
                }
            }
            if (blocked) mine = GPE_SPAWN_BLOCKED_BY_CANDIDATE;
            else if (!wait) mine = GPE_SPAWN_ADDED;
            changed = mine != kSpawnUndecided;
        }
        __syncthreads();                                        // every read of s_state of this iteration is done
        if (changed) s_state[threadIdx.x] = mine;
        if (!__syncthreads_or(changed)) break;
    }
    if (mine != before) __hip_atomic_store(&state[i], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t open = (uint32_t)__popcll(ballot64(mine == kSpawnUndecided));
    if (lane_id() == 0 && open) atomicAdd(left, open);
}

// (6)
__global__ __launch_bounds__(kStreamBlock) void k_spawn_flags(const uint32_t *__restrict__ state, uint32_t k,
                                                              uint32_t *__restrict__ rank, uint8_t *__restrict__ verdict)
{
    const uint32_t stride = gridDim.x * kStreamBlock;
    for (uint32_t i = blockIdx.x * kStreamBlock + threadIdx.x; i < k; i += stride) {
        const uint32_t st = state[i];
        rank[i] = st == (uint32_t)GPE_SPAWN_ADDED ? 1u : 0u;
        verdict[i] = (uint8_t)st;
    }
}

// rank: the inclusive scan of the flags
__global__ __launch_bounds__(kStreamBlock) void k_spawn_scatter(const uint32_t *__restrict__ state,
                                                                const uint32_t *__restrict__ rank,
                                                                const float2 *__restrict__ cpos,
                                                                const float *__restrict__ crad, uint32_t k, uint64_t old_n,
                                                                float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                                float *__restrict__ radius)
{
    const uint32_t stride = gridDim.x * kStreamBlock;
    for (uint32_t i = blockIdx.x * kStreamBlock + threadIdx.x; i < k; i += stride) {
        if (state[i] != (uint32_t)GPE_SPAWN_ADDED) continue;
        const uint64_t d = old_n + rank[i] - 1u;
        const float2 p = cpos[i];
        pos[d] = p;
        prev[d] = p;
        radius[d] = crad[i];
    }
}

gpe_status launch_spawn_keys(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, bool inside_world)
{
    GPE_HIP(c, hipMemsetAsync(ws.ctl, 0xFF, kSpawnCtlRounds * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_spawn_keys, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, ws.pos, ws.radius, k, cell_size,
                       c->cfg.world_width, c->cfg.world_height, inside_world ? 1u : 0u, ws.keys, ws.vals, ws.state, ws.ctl);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_spawn_pass(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, bool search)
{
    GPE_HIP(c, hipMemsetAsync(ws.blocked, 0, (uint64_t)k * sizeof(uint32_t), c->stream));
    if (!search) return GPE_OK;
    hipLaunchKernelGGL(k_spawn_pass, dim3(stream_grid(c->n)), dim3(kStreamBlock), 0, c->stream, c->pos, c->radius, c->n,
                       cell_size, ws.keys, ws.rec, k, ws.ctl, ws.blocked);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_spawn_resolve(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, bool separate)
{
    hipLaunchKernelGGL(k_spawn_resolve, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, ws.state, ws.blocked, k,
                       separate ? 1u : 0u);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_spawn_round(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, float cell_size, uint32_t *left)
{
    const uint32_t blocks = (k + kSpawnBlock - 1) / kSpawnBlock;
    hipLaunchKernelGGL(k_spawn_round, dim3(blocks), dim3(kSpawnBlock), 0, c->stream, ws.pos, ws.radius, ws.keys, ws.rec, k,
                       cell_size, ws.state, left);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_spawn_flags(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k)
{
    hipLaunchKernelGGL(k_spawn_flags, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, ws.state, k, ws.rank,
                       ws.verdict);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_spawn_scatter(gpe_ctx *c, const SpawnWorkspace &ws, uint32_t k, uint64_t old_n)
{
    hipLaunchKernelGGL(k_spawn_scatter, dim3(stream_grid(k)), dim3(kStreamBlock), 0, c->stream, ws.state, ws.rank, ws.pos,
                       ws.radius, k, old_n, c->pos, c->prev, c->radius);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
