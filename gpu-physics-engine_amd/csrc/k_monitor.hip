// k_monitor.hip -- the run monitor's device side (gpe_measure / gpe_monitor_*, include/gpe.h; gfx950, wave64).
//
// One gpe_measures record = a full-pass reduction over pos and prev (16 B per particle; radii play no part), in two
// launches.  Nothing here runs on a context that is neither armed nor asked by gpe_measure.
//   - k_monitor_partial: a lane reads 16 bytes of pos and 16 bytes of prev per load -- one float4 holds two particles --
//     kMonitorUnroll groups of each in flight, and grid-strides; the n % 2 last particle is read by one lane of
//     workgroup 0 with 8-byte loads, so nothing is read past pos[n) or prev[n).  Every lane keeps a MonitorAcc in
//     registers: five double sums, three counters, four ordered-key extents, the 64-bit key of the fastest particle and
//     the lowest irregular index.  A fixed wave64 butterfly (xor 1, 2, 4, 8, 16, 32) reduces each wave, the four waves
//     combine through LDS in wave order, and thread 0 writes the workgroup's partial record with plain stores.
//   - k_monitor_final: one workgroup; lane t folds partials t, t + 256, ... in ascending order, the same butterfly and
//     wave-order combine follow, and thread 0 decodes the keys, reads uids[index] for the two uid fields and writes the
//     finished record straight into its place (a ring slot or the one-shot's device record).
// The grid is a function of n alone and there is no atomic anywhere, so the order of every addition is a function of n
// alone: two measurements of the same arrays give the same bytes.  IEEE addition is commutative, so both lanes of a
// butterfly exchange compute the same bits and every lane of a wave ends with the wave's result.
// The counters are 32-bit: a record is refused above 2^32 - 1 particles and no count can pass n.
// Arithmetic on particle data is IEEE binary32, one rounding per operation, left to right, no FMA (fp contract off
// here, and the build compiles with -ffp-contract=off), like dist2 of k_region.h.
#include <algorithm>

#include "gpe_internal.h"

namespace gpe {

constexpr int kMonitorBlock = 256;
constexpr int kMonitorWaves = kMonitorBlock / kWave;
constexpr int kMonitorUnroll = 4;                                      // 16-byte groups of pos (and of prev) per lane and trip
constexpr uint64_t kMonitorGroupsPerTrip = (uint64_t)kMonitorBlock * kMonitorUnroll;   // 1024 groups = 2048 particles

struct MonitorAcc {                                                    // a lane's accumulators = a workgroup's partial record
    double sx, sy, svx, svy, sv2;
    unsigned long long max_key;                                        // bits(v2) << 32 | (0xFFFFFFFF - index); 0: none
    uint32_t irregular, moving, outside;
    uint32_t first_irregular;                                          // 0xFFFFFFFF: none
    uint32_t min_x, min_y, max_x, max_y;                               // ordered keys (monitor_key)
};
static_assert(sizeof(MonitorAcc) == kMonitorPartialBytes, "MonitorState sizes its scratch by kMonitorPartialBytes");

// The sign-magnitude total order of binary32 as an unsigned order: -0 < +0, and the bits come back unchanged.
__device__ __forceinline__ uint32_t monitor_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float monitor_unkey(uint32_t k)
{
    return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}
constexpr uint32_t kMonitorKeyPosInf = 0xFF800000u;                    // monitor_key(+inf): above every finite key
constexpr uint32_t kMonitorKeyNegInf = 0x007FFFFFu;                    // monitor_key(-inf): below every finite key

__device__ __forceinline__ void monitor_clear(MonitorAcc &a)
{
    a.sx = a.sy = a.svx = a.svy = a.sv2 = 0.0;
    a.max_key = 0ull;
    a.irregular = a.moving = a.outside = 0u;
    a.first_irregular = 0xFFFFFFFFu;
    a.min_x = a.min_y = kMonitorKeyPosInf;
    a.max_x = a.max_y = kMonitorKeyNegInf;
}

// a = a (+) b, a on the left: the one combine of the butterfly, of the waves and of the partials
__device__ __forceinline__ void monitor_merge(MonitorAcc &a, const MonitorAcc &b)
{
    a.sx += b.sx; a.sy += b.sy; a.svx += b.svx; a.svy += b.svy; a.sv2 += b.sv2;
    a.max_key = b.max_key > a.max_key ? b.max_key : a.max_key;
    a.irregular += b.irregular; a.moving += b.moving; a.outside += b.outside;
    a.first_irregular = min(a.first_irregular, b.first_irregular);
    a.min_x = min(a.min_x, b.min_x); a.min_y = min(a.min_y, b.min_y);
    a.max_x = max(a.max_x, b.max_x); a.max_y = max(a.max_y, b.max_y);
}

// Particle i = (px, py) now, (qx, qy) before.  v2 is finite exactly when the particle is regular: a non-finite
// coordinate makes its difference, the square of that and the sum non-finite, and so does an overflowing difference or
// square.  `live` = false: a lane past the end, which adds +0.0 to sums that are never -0.0 and changes nothing.
__device__ __forceinline__ void monitor_take(MonitorAcc &a, float px, float py, float qx, float qy, uint32_t i, bool live,
                                             float rs2, float W, float H)
{
#pragma clang fp contract(off)
    const float vx = px - qx;
    const float vy = py - qy;
    const float vxx = vx * vx;
    const float vyy = vy * vy;
    const float v2 = vxx + vyy;
    const bool finite = (__float_as_uint(v2) & 0x7FFFFFFFu) < 0x7F800000u;
    const bool reg = live && finite, irr = live && !finite;
    a.sx += reg ? (double)px : 0.0;
    a.sy += reg ? (double)py : 0.0;
    a.svx += reg ? (double)vx : 0.0;
    a.svy += reg ? (double)vy : 0.0;
    a.sv2 += reg ? (double)v2 : 0.0;
    const unsigned long long key = ((unsigned long long)__float_as_uint(v2) << 32) | (0xFFFFFFFFu - i);
    a.max_key = (reg && key > a.max_key) ? key : a.max_key;
    a.irregular += irr ? 1u : 0u;
    a.moving += (reg && v2 > rs2) ? 1u : 0u;
    a.outside += (reg && !(px >= 0.f && px <= W && py >= 0.f && py <= H)) ? 1u : 0u;
    a.first_irregular = irr ? min(a.first_irregular, i) : a.first_irregular;
    const uint32_t kx = monitor_key(px), ky = monitor_key(py);
    a.min_x = reg ? min(a.min_x, kx) : a.min_x;
    a.min_y = reg ? min(a.min_y, ky) : a.min_y;
    a.max_x = reg ? max(a.max_x, kx) : a.max_x;
    a.max_y = reg ? max(a.max_y, ky) : a.max_y;
}

// The workgroup's record, valid in thread 0.  s: kMonitorWaves records of LDS.  Contains __syncthreads.
__device__ __forceinline__ void monitor_block_reduce(MonitorAcc &a, MonitorAcc *s)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        MonitorAcc o;
        o.sx = __shfl_xor(a.sx, d, kWave); o.sy = __shfl_xor(a.sy, d, kWave);
        o.svx = __shfl_xor(a.svx, d, kWave); o.svy = __shfl_xor(a.svy, d, kWave);
        o.sv2 = __shfl_xor(a.sv2, d, kWave);
        o.max_key = __shfl_xor(a.max_key, d, kWave);
        o.irregular = __shfl_xor(a.irregular, d, kWave); o.moving = __shfl_xor(a.moving, d, kWave);
        o.outside = __shfl_xor(a.outside, d, kWave);
        o.first_irregular = __shfl_xor(a.first_irregular, d, kWave);
        o.min_x = __shfl_xor(a.min_x, d, kWave); o.min_y = __shfl_xor(a.min_y, d, kWave);
        o.max_x = __shfl_xor(a.max_x, d, kWave); o.max_y = __shfl_xor(a.max_y, d, kWave);
        monitor_merge(a, o);
    }
    if (lane_id() == 0) s[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kMonitorWaves; ++w) monitor_merge(a, s[w]);
    }
}

__global__ __launch_bounds__(kMonitorBlock) void k_monitor_partial(const float2 *__restrict__ pos,
                                                                   const float2 *__restrict__ prev, const uint32_t n,
                                                                   const float rs2, const float W, const float H,
                                                                   MonitorAcc *__restrict__ partials)
{
    __shared__ MonitorAcc s_part[kMonitorWaves];
    MonitorAcc a;
    monitor_clear(a);
    const uint32_t groups = n >> 1;                                    // whole groups of two particles: 16-byte loads
    const float4 *__restrict__ pos4 = reinterpret_cast<const float4 *>(pos);
    const float4 *__restrict__ prev4 = reinterpret_cast<const float4 *>(prev);
    for (uint64_t base = (uint64_t)blockIdx.x * kMonitorGroupsPerTrip; base < groups;
         base += (uint64_t)gridDim.x * kMonitorGroupsPerTrip) {
        float4 p[kMonitorUnroll], q[kMonitorUnroll];
#pragma unroll
        for (int u = 0; u < kMonitorUnroll; ++u) {
            const uint64_t g = base + (uint64_t)u * kMonitorBlock + threadIdx.x;
            p[u] = g < groups ? pos4[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            q[u] = g < groups ? prev4[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kMonitorUnroll; ++u) {
            const uint64_t g = base + (uint64_t)u * kMonitorBlock + threadIdx.x;
            const bool live = g < groups;
            const uint32_t i = 2u * (uint32_t)g;
            monitor_take(a, p[u].x, p[u].y, q[u].x, q[u].y, i, live, rs2, W, H);
            monitor_take(a, p[u].z, p[u].w, q[u].z, q[u].w, i + 1u, live, rs2, W, H);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1u)) {             // the odd last particle
        const float2 p = pos[n - 1u], q = prev[n - 1u];
        monitor_take(a, p.x, p.y, q.x, q.y, n - 1u, true, rs2, W, H);
    }
    monitor_block_reduce(a, s_part);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

__global__ __launch_bounds__(kMonitorBlock) void k_monitor_final(const MonitorAcc *__restrict__ partials,
                                                                 const uint32_t nblocks, const uint64_t step,
                                                                 const uint32_t n, const uint32_t *__restrict__ uids,
                                                                 gpe_measures *__restrict__ out)
{
    __shared__ MonitorAcc s_part[kMonitorWaves];
    MonitorAcc a;
    monitor_clear(a);
    for (uint32_t j = threadIdx.x; j < nblocks; j += kMonitorBlock) monitor_merge(a, partials[j]);
    monitor_block_reduce(a, s_part);
    if (threadIdx.x == 0) {
        gpe_measures r;
        r.step = step;
        r.n = n;
        r.irregular = a.irregular;
        r.moving = a.moving;
        r.outside = a.outside;
        r.sum_x = a.sx; r.sum_y = a.sy; r.sum_vx = a.svx; r.sum_vy = a.svy; r.sum_v2 = a.sv2;
        r.min_x = monitor_unkey(a.min_x); r.min_y = monitor_unkey(a.min_y);
        r.max_x = monitor_unkey(a.max_x); r.max_y = monitor_unkey(a.max_y);
        r.max_v2 = __uint_as_float((uint32_t)(a.max_key >> 32));
        r.max_v2_index = 0xFFFFFFFFu - (uint32_t)a.max_key;            // key 0 (none): +0 and 0xFFFFFFFF
        r.max_v2_uid = (uids && r.max_v2_index != 0xFFFFFFFFu) ? uids[r.max_v2_index] : GPE_UID_ABSENT;
        r.first_irregular = a.first_irregular;
        r.first_irregular_uid = (uids && a.first_irregular != 0xFFFFFFFFu) ? uids[a.first_irregular] : GPE_UID_ABSENT;
        r.reserved = 0u;
        *out = r;
    }
}

uint32_t monitor_grid(uint64_t n)
{
    const uint64_t g = ((n >> 1) + kMonitorGroupsPerTrip - 1) / kMonitorGroupsPerTrip;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g, 1), kMonitorMaxBlocks);
}

gpe_status launch_monitor_partial(gpe_ctx *c, const float2 *pos, const float2 *prev, uint64_t n, float rs2, float W,
                                  float H, void *partials)
{
    if (n == 0 || n > 0xFFFFFFFFull) return fail(c, GPE_ERR_STATE, "monitor: bad particle count");
    hipLaunchKernelGGL(k_monitor_partial, dim3(monitor_grid(n)), dim3(kMonitorBlock), 0, c->stream, pos, prev, (uint32_t)n,
                       rs2, W, H, (MonitorAcc *)partials);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_monitor_final(gpe_ctx *c, const void *partials, uint64_t n, uint64_t step, const uint32_t *uids,
                                gpe_measures *out)
{
    if (n > 0xFFFFFFFFull) return fail(c, GPE_ERR_STATE, "monitor: bad particle count");
    hipLaunchKernelGGL(k_monitor_final, dim3(1), dim3(kMonitorBlock), 0, c->stream, (const MonitorAcc *)partials,
                       n ? monitor_grid(n) : 0u, step, (uint32_t)n, uids, out);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
