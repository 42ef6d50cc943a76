// k_raycast.hip -- ray casts (gpe_cast_rays): the first particle each of k segments touches.  A walk on the device
// (gfx950, wave64) of the contact query's sorted cell records (k_contacts.hip stages (1) and (2)) along each segment;
// it reads the particles and writes only scratch of its own.
//
// Not on the per-step path, so the plain form:
//   (1) k_ray_row_start: row_start[y] = the first sorted slot whose key is at or past row y (y = 0 .. 65536, one binary
//       search each), so that every later search stays inside one row of the table.
//   (2) k_ray_cast: one wave per ray.  The rows the ray's clamped rows span, plus one row on either side, are dealt to
//       the lanes 64 at a time, starting at the origin's side.  Each lane derives the clamped column interval of its row -- the columns of the piece of
//       the segment that passes through the rows Y-1 .. Y+1, plus one column on either side -- and finds its run of the
//       sorted keys by two binary searches inside the row.  The wave then consumes the 64 runs laid end to end, 64
//       records at a time: an inclusive scan of the run lengths, and each lane finds the (row, offset) of its record by
//       a six-step search of the scanned lengths through lane shuffles.  So a horizontal ray (one long run) and a
//       vertical one (thousands of short runs) both keep the lanes busy.  Each lane keeps the least
//       bits(t) << 32 | index of the records ray_touches accepts; t >= +0, so its bits order as its values, and the
//       lowest index wins a tie.  One wave reduction, then lane 0 writes the ray's row of every requested output.
// Completeness: a touched centre lies less than one cell from a point of the segment, in x and in y;
// contacts_axis is monotone, so its clamped cell is within one row and one column of that point's clamped cell.  The
// windows below are padded by half a cell before they are turned into cells, which covers the rounding of the window
// arithmetic itself (a few 2^-6 of a cell while |coordinate| <= 131072 cells, the bound gpe_cast_rays checks).
// The rows are visited in the order the ray meets them, and after each round of 64 rows the walk stops if no later row
// can hold a hit at a t below the best one so far; that cannot change a result.
#include "k_contacts.h"
#include "k_ray.h"

namespace gpe {

constexpr int kRayBlock = 256;                             // threads per workgroup of the cast: one wave per ray
constexpr int kRayWaves = kRayBlock / kWave;
constexpr uint32_t kRayRows = (uint32_t)kContactsAxisMax + 1;     // rows of the clamped key: 65536
static_assert(kRayRowWords == kRayRows + 1u, "row_start holds one word per row and the end of the last row");
constexpr unsigned long long kRayNone = ~0ull;

// (1)
__global__ __launch_bounds__(kStreamBlock) void k_ray_row_start(const uint32_t *__restrict__ keys, uint32_t n,
                                                                uint32_t *__restrict__ row_start)
{
    const uint32_t y = blockIdx.x * kStreamBlock + threadIdx.x;
    if (y <= kRayRows) row_start[y] = contacts_lower_bound(keys, 0, n, (uint64_t)y << 16);
}

// Where the cast writes: one row per ray; NULL = not requested.
struct RayOut {
    uint32_t *index;
    uint32_t *uid;
    float *t;
    float2 *pos;
    float *radius;
};

__device__ __forceinline__ unsigned long long ray_wave_min(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

// The run [*s, *s + *len) of row Y's sorted slots that holds every particle of that row the segment can touch.
__device__ __forceinline__ void ray_row_run(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ row_start,
                                            uint32_t Y, float2 o, float dx, float dy, float cs, uint32_t *s, uint32_t *len)
{
    // the piece of the segment inside the rows Y-1 .. Y+1: those rows hold the cells Y-2 .. Y, that is
    // (Y-2) cs <= y < (Y+1) cs, open-ended where a clamped row takes part; half a cell of padding
    float t_lo = 0.0f, t_hi = 1.0f;
    if (dy != 0.0f) {
        const float w_lo = Y <= 1u ? -INFINITY : ((float)((int32_t)Y - 2) - 0.5f) * cs;
        const float w_hi = Y >= (uint32_t)kContactsAxisMax - 1u ? INFINITY : ((float)(Y + 1u) + 0.5f) * cs;
        const float t1 = (w_lo - o.y) / dy, t2 = (w_hi - o.y) / dy;
        t_lo = fmaxf(fminf(t1, t2), 0.0f);
        t_hi = fminf(fmaxf(t1, t2), 1.0f);
    }
    const float xa = o.x + t_lo * dx, xb = o.x + t_hi * dx;
    const float half = 0.5f * cs;
    uint32_t c0 = contacts_axis(fminf(xa, xb) - half, cs), c1 = contacts_axis(fmaxf(xa, xb) + half, cs);
    c0 = c0 > 0u ? c0 - 1u : 0u;
    c1 = c1 < (uint32_t)kContactsAxisMax ? c1 + 1u : (uint32_t)kContactsAxisMax;
    const uint32_t lo = row_start[Y], hi = row_start[Y + 1u];
    const uint32_t row = Y << 16;
    const uint32_t b = contacts_lower_bound(keys, lo, hi, row | c0);
    const uint32_t e = contacts_lower_bound(keys, b, hi, (uint64_t)(row | c1) + 1u);
    *s = b;
    *len = e - b;
}

// (2) k rays, endpoints finite and within 131072 cells of 0 (checked on the host); cs > 0; n > 0 sorted slots
__global__ __launch_bounds__(kRayBlock) void k_ray_cast(const float2 *__restrict__ from, const float2 *__restrict__ to,
                                                        uint32_t k, float cs, const uint32_t *__restrict__ keys,
                                                        const uint4 *__restrict__ rec,
                                                        const uint32_t *__restrict__ row_start,
                                                        const float2 *__restrict__ pos,
                                                        const float *__restrict__ radius,
                                                        const uint32_t *__restrict__ uids, RayOut O)
{
    const uint32_t ray = blockIdx.x * kRayWaves + (threadIdx.x >> 6);
    if (ray >= k) return;                                      // wave-uniform; the kernel has no barrier
    const uint32_t lane = (uint32_t)lane_id();
    const float2 o = from[ray], e = to[ray];
    const float dx = e.x - o.x, dy = e.y - o.y;
    const uint32_t ya = contacts_axis(o.y, cs), yb = contacts_axis(e.y, cs);
    // the rows in the order the ray meets them: from one row before the origin's to one row past the end's
    const uint32_t top = (uint32_t)kContactsAxisMax;
    const bool up = yb >= ya;
    const uint32_t first = up ? (ya > 0u ? ya - 1u : 0u) : (ya < top ? ya + 1u : top);
    const uint32_t last = up ? (yb < top ? yb + 1u : top) : (yb > 0u ? yb - 1u : 0u);
    const uint32_t rows = (up ? last - first : first - last) + 1u;
    unsigned long long best = kRayNone;
    for (uint32_t r0 = 0; r0 < rows; r0 += kWave) {            // wave-uniform trip count
        const uint32_t r = r0 + lane;
        const uint32_t Y = up ? first + r : first - r;         // meaningful while r < rows
        uint32_t s = 0, len = 0;
        if (r < rows) ray_row_run(keys, row_start, Y, o, dx, dy, cs, &s, &len);
        const uint32_t incl = wave_inclusive_scan(len);        // the runs are disjoint: their sum is at most n < 2^32
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        for (uint64_t off = 0; off < total; off += kWave) {
            const uint64_t item64 = off + lane;
            const uint32_t item = (uint32_t)item64;
            // j = the lane whose run holds record `item` of the concatenation: the number of lanes with incl <= item
            uint32_t j = 0;
#pragma unroll
            for (uint32_t step = kWave / 2; step; step >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)incl, (int)(j + step - 1u), kWave);
                j += v <= item ? step : 0u;
            }
            const uint32_t incl_j = (uint32_t)__shfl((int)incl, (int)j, kWave);
            const uint32_t len_j = (uint32_t)__shfl((int)len, (int)j, kWave);
            const uint32_t s_j = (uint32_t)__shfl((int)s, (int)j, kWave);
            if (item64 < total) {
                const uint4 p = rec[s_j + (item - (incl_j - len_j))];
                float t;
                if (ray_touches(o.x, o.y, e.x, e.y, __uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), &t)) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | p.w;
                    best = key < best ? key : best;
                }
            }
        }
        if (r0 + kWave >= rows) break;
        // Stop once no later row can beat the best hit.  A particle of a later row is touched, if at all, at a point of
        // the segment whose clamped row is at or past Yn -+ 1 (less than one cell from its centre), so at a t past the
        // segment's crossing of that row's near edge -- taken half a cell early, as the windows of ray_row_run are.
        best = ray_wave_min(best);                             // wave-uniform from here on
        if (best != kRayNone) {
            const uint32_t Yn = up ? first + (r0 + kWave) : first - (r0 + kWave);    // the next row; dy != 0 here
            const bool open = up ? Yn <= 1u : Yn >= top - 1u;  // a clamped row takes part: no near edge
            const float edge = up ? ((float)((int32_t)Yn - 2) - 0.5f) * cs : ((float)(Yn + 1u) + 0.5f) * cs;
            if (!open && __uint_as_float((uint32_t)(best >> 32)) < (edge - o.y) / dy) break;
        }
    }
    best = ray_wave_min(best);
    if (lane != 0u) return;
    const bool hit = best != kRayNone;
    const uint32_t i = (uint32_t)(best & 0xFFFFFFFFull);
    const float nan = __uint_as_float(0x7FC00000u);
    if (O.index) O.index[ray] = hit ? i : GPE_RAY_MISS;
    if (O.uid) O.uid[ray] = hit ? uids[i] : GPE_UID_ABSENT;
    if (O.t) O.t[ray] = hit ? __uint_as_float((uint32_t)(best >> 32)) : nan;
    if (O.pos) O.pos[ray] = hit ? pos[i] : make_float2(nan, nan);
    if (O.radius) O.radius[ray] = hit ? radius[i] : nan;
}

gpe_status launch_ray_row_start(gpe_ctx *c, const uint32_t *keys, uint32_t *row_start)
{
    if (c->n == 0 || c->n > 0xFFFFFFFFull) return fail(c, GPE_ERR_INVALID_ARG, "ray cast: bad particle count");
    const uint32_t g = (kRayRows + 1u + kStreamBlock - 1u) / kStreamBlock;
    hipLaunchKernelGGL(k_ray_row_start, dim3(g), dim3(kStreamBlock), 0, c->stream, keys, (uint32_t)c->n, row_start);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

gpe_status launch_ray_cast(gpe_ctx *c, const float2 *from, const float2 *to, uint32_t k, float cell_size,
                           const uint32_t *keys, const uint4 *rec, const uint32_t *row_start, uint32_t *index_out,
                           uint32_t *uid_out, float *t_out, float2 *pos_out, float *radius_out)
{
    if (k == 0 || k > kRayMaxBatch || c->n == 0 || c->n > 0xFFFFFFFFull)
        return fail(c, GPE_ERR_INVALID_ARG, "ray cast: bad batch or particle count");
    const RayOut O{index_out, uid_out, t_out, pos_out, radius_out};
    const uint32_t g = (k + kRayWaves - 1u) / kRayWaves;
    hipLaunchKernelGGL(k_ray_cast, dim3(g), dim3(kRayBlock), 0, c->stream, from, to, k, cell_size, keys, rec, row_start,
                       (const float2 *)c->pos, (const float *)c->radius, (const uint32_t *)c->uid.uids, O);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
