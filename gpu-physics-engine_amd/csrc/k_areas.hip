// k_areas.hip -- the area constraints' pass (gfx950, wave64): `iterations` relaxations of the set, each a loop phase
// (one launch per non-empty width class) and a node phase (k_area.h says what a loop's corrections are; area_table.h
// builds the tables on the host).
//
// One relaxation must not read a position it has written itself (Jacobi), and a uid may be a member of several loops,
// so it is two phases on the context's in-order stream:
//   - k_areas_loop<G>.  A wave serves 64 / G loops of class G at once, one sub-group of G lanes each; lane l of a
//     sub-group is lane l of the canonical sum (k_body.h).  The reductions are xor butterflies (offsets below G: they
//     never leave the sub-group); binary32 addition commutes, so every lane ends with the bits the halving tree leaves
//     in partial[0].  Every lane of the wave runs every shuffle and every ballot: there is no early return, a
//     sub-group past the class's end or with nothing to do only stops loading and storing.
//       count <= 64 (every class): a lane reads its member's slot (4 B) and pos (8 B) once and keeps them in registers
//       through both sums; member 0 and the two neighbours n and m come from lanes of the same sub-group by an indexed
//       shuffle whose wrap-around is computed per lane.  The lane writes corr[first + l] (8 B).
//       count > 64 (class 64 only, one loop per wave): the lanes loop over the members lane-strided, at most 64 rounds,
//       the gathers of kAreaBatch rounds issued together.  Inside a batch a member's neighbours across a lane or round
//       boundary (j = 63 <-> 64) come from lane 0 of the next round and lane 63 of the round before, by shuffle; across
//       a batch boundary from a second gather (the member before the batch's first and the one behind its last: every
//       lane loads the same two addresses); member count - 1's n is member 0, which every lane holds.  Both sums are
//       taken in that one sweep; each lane leaves its g_j in corr[first + j] and, once lambda is known, reads its own
//       8 bytes back and scales them (the same lane, the same address: program order).
//     Lane 0 of a sub-group writes value[loop] = (area, lambda), two NaNs for an inert loop, and the state byte when
//     it changes: 0 acted, 2 inert in this relaxation.  A loop's lanes are the only writers of its members' corr, of
//     its value and of its state byte.
//   - the node phase, one lane per node v (a distinct uid the loops name): k_uid_nodes.h's kernel, which asks
//     AreaPassArgs::share.  Per membership, in ascending member index, that reads inc (8 B: member, loop), state (1 B)
//     and for an acting loop corr (8 B).  One lane walks a node's whole row (at most GPE_AREA_MAX_DEGREE).
// corr cannot carry the "did not act" mark itself (a correction of zero still counts: its particle is clamped), so the
// mark is the state byte.  No LDS, no float atomics.  Every slot is checked against n, every index against the count of
// its array, before it indexes anything.
#include "gpe_internal.h"
#include "area_table.h"
#include "k_area.h"
#include "k_uid_nodes.h"

namespace gpe {

static_assert(sizeof(AreaRecord) == sizeof(uint4), "the device reads an AreaRecord as one 16-byte word");
static_assert(sizeof(AreaIncidence) == sizeof(uint2), "the device reads an AreaIncidence as one 8-byte word");

struct AreaPassArgs {
    const uint4 *rec = nullptr;
    const uint32_t *order = nullptr;             // this class's loop indices
    const uint32_t *member_slot = nullptr;
    const uint32_t *node_slot = nullptr, *row_start = nullptr;
    const uint2 *inc = nullptr;
    float2 *corr = nullptr;
    uint8_t *state = nullptr;
    float2 *value = nullptr;
    uint32_t loops = 0;                          // in this class
    uint32_t k = 0, members = 0, m = 0, n = 0;
    float world_w = 0.f, world_h = 0.f;
    // the node phase's shares (k_uid_nodes.h): every member is one incidence
    __device__ __forceinline__ uint32_t incidences() const { return members; }
    template <class Add>
    __device__ __forceinline__ void share(uint32_t e, Add add) const
    {
        const uint2 w = inc[e];                                         // (member, loop)
        if (w.x >= members || w.y >= k || state[w.y] != kAreaActs) return;
        const float2 c = corr[w.x];
        add(c.x, c.y);
    }
};

// S over the G lanes of a sub-group: every lane receives the sum.
template <int G>
__device__ __forceinline__ float area_group_sum(float partial)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int off = G / 2; off >= 1; off /= 2) partial = body_add(partial, __shfl_xor(partial, off));
    return partial;
}

// The position of member j of the loop at `first`, (0, 0) for a member without a particle.  j < count.
__device__ __forceinline__ float2 area_member_pos(const AreaPassArgs &P, const float2 *__restrict__ pos, uint32_t first,
                                                  uint32_t j)
{
    const uint32_t slot = P.member_slot[first + j];
    return slot < P.n ? pos[slot] : make_float2(0.f, 0.f);
}

constexpr uint32_t kAreaBatch = 8;

template <int G>
__global__ __launch_bounds__(kStreamBlock) void k_areas_loop(const float2 *__restrict__ pos, AreaPassArgs P)
{
#pragma clang fp contract(off)
    constexpr uint32_t kPerWave = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = lane / G, l = lane % G;
    const uint64_t group_mask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << (sub * G);
    const uint64_t at = (uint64_t)wave * kPerWave + sub;
    const bool served = at < P.loops;
    const uint32_t loop = served ? P.order[at] : 0u;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    uint32_t was = kAreaInert;
    const bool known = served && loop < P.k;
    if (known) {
        r = P.rec[loop];
        was = P.state[loop];
    }
    const uint32_t first = r.x, count = r.y;
    const float rest_area = __uint_as_float(r.z), stiffness = __uint_as_float(r.w);
    // (a range the host did not check would be a bug of gpe_set_areas: it is refused here, never followed)
    const bool runs = known && count >= 3u && count <= GPE_AREA_MAX_MEMBERS && (uint64_t)first + count <= P.members;
    const float nanf_ = __uint_as_float(0x7fc00000u);
    uint32_t now = kAreaInert;
    float2 value = make_float2(nanf_, nanf_);

    if (G < 64 || __all(!runs || count <= 64u)) {
        // ---- one member per lane, kept in registers -----------------------------------------------------------------
        const bool mine = runs && l < count;
        uint32_t slot = 0xffffffffu;
        float2 p = make_float2(0.f, 0.f);
        if (mine) slot = P.member_slot[first + l];
        const bool live = mine && slot < P.n;
        if (live) p = pos[slot];
        const bool whole = (__ballot(mine && !live) & group_mask) == 0ull;   // every member has a particle
        const float p0x = __shfl(p.x, 0, G), p0y = __shfl(p.y, 0, G);
        const float qx = area_rel(p.x, p0x), qy = area_rel(p.y, p0y);
        // (a lane past the loop's end asks lane 0: its values are not used)
        const uint32_t ln = mine ? (l + 1u == count ? 0u : l + 1u) : 0u;
        const uint32_t lm = mine ? (l == 0u ? count - 1u : l - 1u) : 0u;
        const float nx = __shfl(qx, (int)ln, G), ny = __shfl(qy, (int)ln, G);
        const float mx = __shfl(qx, (int)lm, G), my = __shfl(qy, (int)lm, G);
        float gx = 0.f, gy = 0.f;
        const float t = area_term(qx, qy, nx, ny);
        const float d = area_gradient(nx, ny, mx, my, &gx, &gy);
        const float A2 = area_group_sum<G>(mine ? body_add(0.0f, t) : 0.0f);
        const float D = area_group_sum<G>(mine ? body_add(0.0f, d) : 0.0f);
        float area = 0.f, lambda = 0.f;
        if (runs && whole && area_lambda(A2, D, rest_area, stiffness, &area, &lambda)) {
            now = kAreaActs;
            value = make_float2(area, lambda);
            if (mine) P.corr[first + l] = make_float2(area_scale(lambda, gx), area_scale(lambda, gy));
        }
    } else if constexpr (G == 64) {
        // ---- one loop per wave, its members lane-strided (runs and count are wave-uniform here) ----------------------
        // A round past the loop's last adds +0.0f (x + +0.0f == x for every x a sum from +0.0f holds).
        const uint32_t rounds = runs ? (count + 63u) / 64u : 0u;
        float2 p0 = make_float2(0.f, 0.f);
        if (runs) p0 = area_member_pos(P, pos, first, 0u);
        bool absent = false;
        float sA = 0.0f, sD = 0.0f;
        for (uint32_t t0 = 0; t0 < rounds; t0 += kAreaBatch) {
            uint32_t slot[kAreaBatch];
            float2 p[kAreaBatch];
#pragma unroll
            for (uint32_t u = 0; u < kAreaBatch; ++u) {
                const uint32_t j = (t0 + u) * 64u + l;
                slot[u] = j < count ? P.member_slot[first + j] : 0xffffffffu;
            }
            // the member before the batch's first (member 0's m is member count - 1) and the one behind its last
            const uint32_t jb = t0 * 64u, je = (t0 + kAreaBatch) * 64u;
            const uint32_t jprev = jb == 0u ? count - 1u : jb - 1u;
            const uint32_t sprev = P.member_slot[first + jprev];
            const uint32_t snext = je < count ? P.member_slot[first + je] : 0xffffffffu;
#pragma unroll
            for (uint32_t u = 0; u < kAreaBatch; ++u) {
                const uint32_t j = (t0 + u) * 64u + l;
                p[u] = slot[u] < P.n ? pos[slot[u]] : make_float2(0.f, 0.f);
                absent |= j < count && slot[u] >= P.n;
            }
            const float2 eprev = sprev < P.n ? pos[sprev] : make_float2(0.f, 0.f);
            const float2 enext = snext < P.n ? pos[snext] : make_float2(0.f, 0.f);
#pragma unroll
            for (uint32_t u = 0; u < kAreaBatch; ++u) {
                const uint32_t j = (t0 + u) * 64u + l;
                const bool mine = j < count;
                // n: lane l + 1 of this round, for lane 63 lane 0 of the next, for the loop's last member member 0
                // (u is a constant once unrolled; the array indices below are written so that none leaves the batch)
                float pnx = __shfl(p[u].x, (int)((l + 1u) & 63u)), pny = __shfl(p[u].y, (int)((l + 1u) & 63u));
                float fx = enext.x, fy = enext.y;
                if (u + 1u < kAreaBatch) {
                    fx = __shfl(p[u + 1u < kAreaBatch ? u + 1u : u].x, 0);
                    fy = __shfl(p[u + 1u < kAreaBatch ? u + 1u : u].y, 0);
                }
                if (l == 63u) { pnx = fx; pny = fy; }
                if (j + 1u == count) { pnx = p0.x; pny = p0.y; }
                // m: lane l - 1 of this round, for lane 0 lane 63 of the round before
                float pmx = __shfl(p[u].x, (int)((l + 63u) & 63u)), pmy = __shfl(p[u].y, (int)((l + 63u) & 63u));
                float bx = eprev.x, by = eprev.y;
                if (u > 0u) {
                    bx = __shfl(p[u > 0u ? u - 1u : u].x, 63);
                    by = __shfl(p[u > 0u ? u - 1u : u].y, 63);
                }
                if (l == 0u) { pmx = bx; pmy = by; }
                const float qx = area_rel(p[u].x, p0.x), qy = area_rel(p[u].y, p0.y);
                const float nx = area_rel(pnx, p0.x), ny = area_rel(pny, p0.y);
                const float mx = area_rel(pmx, p0.x), my = area_rel(pmy, p0.y);
                float gx = 0.f, gy = 0.f;
                const float t = area_term(qx, qy, nx, ny);
                const float d = area_gradient(nx, ny, mx, my, &gx, &gy);
                sA = body_add(sA, mine ? t : 0.0f);
                sD = body_add(sD, mine ? d : 0.0f);
                if (mine) P.corr[first + j] = make_float2(gx, gy);
            }
        }
        const bool whole = __ballot(absent) == 0ull;
        const float A2 = area_group_sum<64>(sA);
        const float D = area_group_sum<64>(sD);
        float area = 0.f, lambda = 0.f;
        if (runs && whole && area_lambda(A2, D, rest_area, stiffness, &area, &lambda)) {
            now = kAreaActs;
            value = make_float2(area, lambda);
            for (uint32_t t0 = 0; t0 < rounds; t0 += kAreaBatch) {
                float2 g[kAreaBatch];
#pragma unroll
                for (uint32_t u = 0; u < kAreaBatch; ++u) {
                    const uint32_t j = (t0 + u) * 64u + l;
                    g[u] = j < count ? P.corr[first + j] : make_float2(0.f, 0.f);
                }
#pragma unroll
                for (uint32_t u = 0; u < kAreaBatch; ++u) {
                    const uint32_t j = (t0 + u) * 64u + l;
                    if (j < count) P.corr[first + j] = make_float2(area_scale(lambda, g[u].x), area_scale(lambda, g[u].y));
                }
            }
        }
    }

    if (runs && l == 0u) {
        P.value[loop] = value;
        if (now != was) P.state[loop] = (uint8_t)now;
    }
}

// member_slot[i] = node_slot[member_node[i]]: the loop phase gathers through one table
__global__ __launch_bounds__(kStreamBlock) void k_areas_expand(const uint32_t *__restrict__ member_node,
                                                               const uint32_t *__restrict__ node_slot,
                                                               uint32_t *__restrict__ member_slot, uint32_t members,
                                                               uint32_t m)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < members; i += stride) {
        const uint32_t v = member_node[i];
        member_slot[i] = v < m ? node_slot[v] : 0xffffffffu;
    }
}

gpe_status launch_areas_expand(gpe_ctx *c, const AreaState &A)
{
    if (A.members == 0 || A.nt.nodes == 0) return GPE_OK;
    hipLaunchKernelGGL(k_areas_expand, dim3(stream_grid(A.members)), dim3(kStreamBlock), 0, c->stream, A.member_node,
                       A.nt.node_slot, A.member_slot, (uint32_t)A.members, (uint32_t)A.nt.nodes);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

template <int G>
static gpe_status launch_class(gpe_ctx *c, const float2 *pos, AreaPassArgs P)
{
    const uint64_t waves = ((uint64_t)P.loops + (64 / G) - 1) / (64 / G);
    const uint64_t blocks = (waves * 64 + kStreamBlock - 1) / kStreamBlock;
    Scope s(c, "areas/loop");
    hipLaunchKernelGGL(k_areas_loop<G>, dim3((uint32_t)blocks), dim3(kStreamBlock), 0, c->stream, pos, P);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

// A's tables as gpe_set_areas uploaded them for k loops and m nodes (every order entry < k, every member range inside
// A.members, every inc entry below (A.members, k)), node_slot and member_slot resolved for the particles as they are.
gpe_status launch_areas_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const AreaState &A, uint32_t k,
                             uint32_t m, uint32_t iterations)
{
    if (n == 0 || k == 0 || m == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "areas");
    AreaPassArgs P;
    P.rec = A.rec; P.member_slot = A.member_slot;
    P.node_slot = A.nt.node_slot; P.row_start = A.nt.row_start; P.inc = A.inc;
    P.corr = A.corr; P.state = A.state; P.value = A.value;
    P.k = k; P.members = (uint32_t)A.members; P.m = m; P.n = (uint32_t)n;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    for (uint32_t it = 0; it < iterations; ++it) {
        for (uint32_t q = 0; q < kAreaClasses; ++q) {
            const uint32_t lo = A.class_start[q], hi = A.class_start[q + 1];
            if (hi <= lo || hi > k) continue;
            P.order = A.order + lo;
            P.loops = hi - lo;
            switch (q) {
            case 0: GPE_TRY(launch_class<4>(c, pos, P)); break;
            case 1: GPE_TRY(launch_class<8>(c, pos, P)); break;
            case 2: GPE_TRY(launch_class<16>(c, pos, P)); break;
            case 3: GPE_TRY(launch_class<32>(c, pos, P)); break;
            default: GPE_TRY(launch_class<64>(c, pos, P)); break;
            }
        }
        GPE_TRY(launch_uid_nodes(c, "areas/node", pos, radius, P));
    }
    return GPE_OK;
}

}  // namespace gpe
