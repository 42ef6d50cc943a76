// k_bodies.hip -- the rigid and soft bodies' pass (gfx950, wave64): shape matching of every body of the set, one launch
// per non-empty width class (k_body.h says what the pass computes; body_table.h builds the tables on the host).
//
// A wave serves 64 / G bodies of class G at once, one sub-group of G lanes each; lane l of a sub-group is lane l of
// the canonical sum.  The reductions are xor butterflies (__shfl_xor, offsets below G, so they never leave the
// sub-group): binary32 addition commutes, so every lane ends with the bits the halving tree leaves in partial[0].
// Every lane of the wave runs every shuffle and every ballot: there is no early return, a sub-group past the class's
// end or with nothing to do only stops loading and storing.  Break and inert decisions are taken per sub-group from
// ballot masks.
//   - count <= 64 (every class): a lane reads its member's slot (4 B), rest (8 B), pos (8 B) once and keeps them in
//     registers through the four phases (centroids, moments, errors, move); it reads radius (4 B) and writes pos (8 B)
//     only when the body acts.
//   - count > 64 (class 64 only, one body per wave): the lanes loop over the members lane-strided, at most 64 rounds
//     per phase, and gather slot, rest and pos again in the later phases (from L2: the body's lanes are the only
//     writers of those positions, and they write in the last phase only).  The gathers of eight rounds are issued
//     together (244 bodies of 4096 are 244 waves: latency, not bandwidth, is their cost); the additions keep their
//     order.
// Lane 0 of a sub-group writes the body's pose (16 B) and its state byte when it changes, and counts a break
// (atomicAdd on an integer: order-free).  A body's lanes are the only writers of its members' pos (a uid is in one body
// at most and names one particle at most), of its pose and of its state byte.  No LDS, no float atomics.  Slots are
// checked against n before they index anything.
#include "gpe_internal.h"
#include "body_table.h"
#include "k_body.h"

namespace gpe {

static_assert(sizeof(BodyRecord) == sizeof(uint4), "the device reads a BodyRecord as one 16-byte word");

struct BodyPassArgs {
    const uint4 *rec = nullptr;
    const uint32_t *order = nullptr;             // this class's body indices
    const uint32_t *member_slot = nullptr;
    const float2 *member_rest = nullptr;
    float4 *pose = nullptr;
    uint8_t *state = nullptr;
    unsigned long long *broken = nullptr;
    uint32_t bodies = 0;                         // in this class
    uint32_t members = 0, n = 0;
    float world_w = 0.f, world_h = 0.f;
};

// S over the G lanes of a sub-group: every lane receives the sum.
template <int G>
__device__ __forceinline__ float group_sum(float partial)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int off = G / 2; off >= 1; off /= 2) partial = body_add(partial, __shfl_xor(partial, off));
    return partial;
}

template <int G>
__device__ __forceinline__ uint32_t group_count(uint32_t v)
{
#pragma unroll
    for (int off = G / 2; off >= 1; off /= 2) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

// kBodyBatch rounds of a looping body: lane l's members t0 * 64 + l, (t0 + 1) * 64 + l, ...  A member past the body's
// count, without a particle or with a slot >= n has slot 0xffffffff (or its stale value >= n), rest and p zero.
constexpr uint32_t kBodyBatch = 8;
struct BodyBatch {
    uint32_t slot[kBodyBatch];
    float2 rest[kBodyBatch], p[kBodyBatch];
    __device__ __forceinline__ void gather(const BodyPassArgs &P, const float2 *__restrict__ pos, uint32_t first,
                                           uint32_t count, uint32_t t0, uint32_t l)
    {
#pragma unroll
        for (uint32_t u = 0; u < kBodyBatch; ++u) {
            const uint32_t j = (t0 + u) * 64u + l;
            slot[u] = j < count ? P.member_slot[first + j] : 0xffffffffu;
        }
#pragma unroll
        for (uint32_t u = 0; u < kBodyBatch; ++u) {
            const uint32_t j = (t0 + u) * 64u + l;
            const bool live = slot[u] < P.n;
            rest[u] = live ? P.member_rest[first + j] : make_float2(0.f, 0.f);
            p[u] = live ? pos[slot[u]] : make_float2(0.f, 0.f);
        }
    }
};

template <int G>
__global__ __launch_bounds__(kStreamBlock) void k_bodies_pass(float2 *__restrict__ pos, const float *__restrict__ radius,
                                                              BodyPassArgs P)
{
#pragma clang fp contract(off)
    constexpr uint32_t kPerWave = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = lane / G, l = lane % G;
    const uint64_t group_mask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << (sub * G);
    const uint64_t at = (uint64_t)wave * kPerWave + sub;
    const bool served = at < P.bodies;
    const uint32_t body = served ? P.order[at] : 0u;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    uint32_t was = kBodyBroken;
    if (served) {
        r = P.rec[body];
        was = P.state[body];
    }
    const uint32_t first = r.x, count = r.y;
    const float stiffness = __uint_as_float(r.z), bd2 = __uint_as_float(r.w);
    // (a range the host did not check would be a bug of gpe_set_bodies: it is refused here, never followed)
    const bool runs = served && was != kBodyBroken && count >= 2 && (uint64_t)first + count <= P.members;
    const float nanf_ = __uint_as_float(0x7fc00000u);
    uint32_t now = kBodyInert;
    float4 pose = make_float4(nanf_, nanf_, nanf_, nanf_);

    if (G < 64 || __all(!runs || count <= 64u)) {
        // ---- one member per lane, kept in registers -----------------------------------------------------------------
        const bool mine = runs && l < count;
        uint32_t slot = 0xffffffffu;
        float2 rest = make_float2(0.f, 0.f), p = make_float2(0.f, 0.f);
        if (mine) slot = P.member_slot[first + l];
        const bool live = mine && slot < P.n;
        if (live) {
            rest = P.member_rest[first + l];
            p = pos[slot];
        }
        const uint32_t L = (uint32_t)__popcll(__ballot(live) & group_mask);
        const float fL = (float)L;
        const float rbx = group_sum<G>(body_add(0.0f, live ? rest.x : 0.0f)) / fL;
        const float rby = group_sum<G>(body_add(0.0f, live ? rest.y : 0.0f)) / fL;
        const float cx = group_sum<G>(body_add(0.0f, live ? p.x : 0.0f)) / fL;
        const float cy = group_sum<G>(body_add(0.0f, live ? p.y : 0.0f)) / fL;
        float qx = 0.f, qy = 0.f, a = 0.f, b = 0.f;
        if (live) body_moment(rest.x, rest.y, rbx, rby, p.x, p.y, cx, cy, &qx, &qy, &a, &b);
        const float A = group_sum<G>(body_add(0.0f, live ? a : 0.0f));
        const float B = group_sum<G>(body_add(0.0f, live ? b : 0.0f));
        float co = 0.f, si = 0.f;
        const bool fits = runs && L >= 2u && body_rotation(A, B, &co, &si);
        float ex = 0.f, ey = 0.f;
        bool far = false;
        if (fits && live) far = body_breaks(body_error(qx, qy, p.x, p.y, cx, cy, co, si, &ex, &ey), bd2);
        const bool breaks = (__ballot(far) & group_mask) != 0ull;
        if (runs) now = !fits ? kBodyInert : breaks ? kBodyBroken : kBodyActs;
        if (now == kBodyActs) {
            pose = make_float4(cx, cy, co, si);
            if (live) {
                float2 o;
                body_move(p.x, p.y, radius[slot], stiffness, ex, ey, P.world_w, P.world_h, &o.x, &o.y);
                pos[slot] = o;
            }
        }
    } else if constexpr (G == 64) {
        // ---- one body per wave, its members lane-strided (runs and count are wave-uniform here) ----------------------
        // kBodyBatch rounds' gathers are issued before the first of their values is added: the additions keep the
        // canonical order, the loads overlap.  A round past the body's last adds +0.0f (x + +0.0f == x for every x a
        // sum from +0.0f holds)
        const uint32_t rounds = runs ? (count + 63u) / 64u : 0u;
        BodyBatch m;
        uint32_t mineL = 0;
        float srx = 0.0f, sry = 0.0f, spx = 0.0f, spy = 0.0f;
        for (uint32_t t0 = 0; t0 < rounds; t0 += kBodyBatch) {
            m.gather(P, pos, first, count, t0, l);
#pragma unroll
            for (uint32_t u = 0; u < kBodyBatch; ++u) {
                srx = body_add(srx, m.rest[u].x); sry = body_add(sry, m.rest[u].y);
                spx = body_add(spx, m.p[u].x); spy = body_add(spy, m.p[u].y);
                mineL += m.slot[u] < P.n ? 1u : 0u;
            }
        }
        const uint32_t L = group_count<64>(mineL);
        const float fL = (float)L;
        const float rbx = group_sum<64>(srx) / fL, rby = group_sum<64>(sry) / fL;
        const float cx = group_sum<64>(spx) / fL, cy = group_sum<64>(spy) / fL;
        float sa = 0.0f, sb = 0.0f;
        for (uint32_t t0 = 0; t0 < rounds; t0 += kBodyBatch) {
            m.gather(P, pos, first, count, t0, l);
#pragma unroll
            for (uint32_t u = 0; u < kBodyBatch; ++u) {
                float a = 0.f, b = 0.f, qx = 0.f, qy = 0.f;
                if (m.slot[u] < P.n)
                    body_moment(m.rest[u].x, m.rest[u].y, rbx, rby, m.p[u].x, m.p[u].y, cx, cy, &qx, &qy, &a, &b);
                sa = body_add(sa, a); sb = body_add(sb, b);
            }
        }
        const float A = group_sum<64>(sa), B = group_sum<64>(sb);
        float co = 0.f, si = 0.f;
        const bool fits = runs && L >= 2u && body_rotation(A, B, &co, &si);
        bool far = false;
        if (fits && bd2 >= 0.0f) {
            for (uint32_t t0 = 0; t0 < rounds; t0 += kBodyBatch) {
                m.gather(P, pos, first, count, t0, l);
#pragma unroll
                for (uint32_t u = 0; u < kBodyBatch; ++u) {
                    if (m.slot[u] >= P.n) continue;
                    float qx, qy, a, b, ex, ey;
                    body_moment(m.rest[u].x, m.rest[u].y, rbx, rby, m.p[u].x, m.p[u].y, cx, cy, &qx, &qy, &a, &b);
                    far |= body_breaks(body_error(qx, qy, m.p[u].x, m.p[u].y, cx, cy, co, si, &ex, &ey), bd2);
                }
            }
        }
        const bool breaks = __ballot(far) != 0ull;
        if (runs) now = !fits ? kBodyInert : breaks ? kBodyBroken : kBodyActs;
        if (now == kBodyActs) {
            pose = make_float4(cx, cy, co, si);
            for (uint32_t t0 = 0; t0 < rounds; t0 += kBodyBatch) {
                m.gather(P, pos, first, count, t0, l);
                float r[kBodyBatch];
#pragma unroll
                for (uint32_t u = 0; u < kBodyBatch; ++u) r[u] = m.slot[u] < P.n ? radius[m.slot[u]] : 0.f;
#pragma unroll
                for (uint32_t u = 0; u < kBodyBatch; ++u) {
                    if (m.slot[u] >= P.n) continue;
                    float qx, qy, a, b, ex, ey;
                    body_moment(m.rest[u].x, m.rest[u].y, rbx, rby, m.p[u].x, m.p[u].y, cx, cy, &qx, &qy, &a, &b);
                    (void)body_error(qx, qy, m.p[u].x, m.p[u].y, cx, cy, co, si, &ex, &ey);
                    float2 o;
                    body_move(m.p[u].x, m.p[u].y, r[u], stiffness, ex, ey, P.world_w, P.world_h, &o.x, &o.y);
                    pos[m.slot[u]] = o;
                }
            }
        }
    }

    if (runs && l == 0u) {
        P.pose[body] = pose;
        if (now != was) P.state[body] = (uint8_t)now;
        if (now == kBodyBroken) atomicAdd(P.broken, 1ull);
    }
}

template <int G>
static gpe_status launch_class(gpe_ctx *c, float2 *pos, const float *radius, BodyPassArgs P)
{
    const uint64_t waves = ((uint64_t)P.bodies + (64 / G) - 1) / (64 / G);
    const uint64_t blocks = (waves * 64 + kStreamBlock - 1) / kStreamBlock;
    Scope s(c, "bodies/match");
    hipLaunchKernelGGL(k_bodies_pass<G>, dim3((uint32_t)blocks), dim3(kStreamBlock), 0, c->stream, pos, radius, P);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

// B's tables as gpe_set_bodies uploaded them for k bodies (every order entry < k, every member range inside
// B.members), member_slot resolved for the particles as they are.
gpe_status launch_bodies_pass(gpe_ctx *c, float2 *pos, const float *radius, uint64_t n, const BodyState &B, uint32_t k)
{
    if (n == 0 || k == 0) return GPE_OK;
    if (n > 0xFFFFFFFFull) return refuse_too_many(c, "bodies");
    BodyPassArgs P;
    P.rec = B.rec; P.member_slot = B.member_slot; P.member_rest = B.member_rest;
    P.pose = B.pose; P.state = B.state; P.broken = B.broken;
    P.members = (uint32_t)B.members; P.n = (uint32_t)n;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    for (uint32_t q = 0; q < kBodyClasses; ++q) {
        const uint32_t lo = B.class_start[q], hi = B.class_start[q + 1];
        if (hi <= lo || hi > k) continue;
        P.order = B.order + lo;
        P.bodies = hi - lo;
        switch (q) {
        case 0: GPE_TRY(launch_class<2>(c, pos, radius, P)); break;
        case 1: GPE_TRY(launch_class<4>(c, pos, radius, P)); break;
        case 2: GPE_TRY(launch_class<8>(c, pos, radius, P)); break;
        case 3: GPE_TRY(launch_class<16>(c, pos, radius, P)); break;
        case 4: GPE_TRY(launch_class<32>(c, pos, radius, P)); break;
        default: GPE_TRY(launch_class<64>(c, pos, radius, P)); break;
        }
    }
    return GPE_OK;
}

}  // namespace gpe
