// k_fields.hip -- the force fields' pass: every particle against the fields of its lookup cell, their accelerations
// summed and their drags multiplied in ascending field index, then prev rewritten (k_field.h says what a field
// contributes and how the sum is applied).  pos is only read.
//
// A streaming pass shaped like k_colliders_pass: two particles per lane, so pos is read 16 B per lane.  The common lane
// finds an empty list: it has read its pos and two words of cell_start per particle and is done -- no prev load, no
// store.  prev is loaded only under a non-empty list and stored only for a particle some field matched.  The fields
// are 48-byte records (three float4: region | pole, uniform | strength, reach, rr, code): 4096 of them are 192 KB and
// stay in an XCD's L2; cell_start is read at the particles' own locality (they are kept in Morton order).  A particle
// outside the grid or with a NaN coordinate walks all k fields: no result rests on the grid.
#include "gpe_internal.h"
#include "k_field.h"

namespace gpe {

struct FieldPassArgs {
    const uint32_t *cell_start = nullptr;        // view.gx * view.gy + 1
    const uint32_t *items = nullptr;
    const float4 *rec = nullptr;                 // 3 per field
    uint32_t k = 0;
    ColliderGridView view;
    float dt2 = 0.f;
    unsigned long long *touched = nullptr;
};

__device__ __forceinline__ void field_try(const FieldPassArgs &P, uint32_t j, float cx, float cy, FieldSum &sum)
{
    const float4 a = P.rec[3 * j];
    const float4 m = P.rec[3 * j + 2];
    const uint32_t code = __float_as_uint(m.w);
    if (!field_matches(field_shape(code), a.x, a.y, a.z, a.w, m.z, cx, cy)) return;
    FieldRecord f;
    f.x0 = a.x; f.y0 = a.y; f.x1 = a.z; f.y1 = a.w;
    f.px = f.py = f.fx = f.fy = 0.f;
    if (field_kind(code) != kFieldDrag) {
        const float4 b = P.rec[3 * j + 1];
        f.px = b.x; f.py = b.y; f.fx = b.z; f.fy = b.w;
    }
    f.strength = m.x; f.reach = m.y; f.rr = m.z; f.code = code;
    field_contribute(f, cx, cy, sum);
}

// particle i at (cx, cy).  true: some field matched, q is its new prev
__device__ __forceinline__ bool field_resolve(const FieldPassArgs &P, const float2 *__restrict__ prev, uint64_t i, float cx,
                                              float cy, float2 &q)
{
#pragma clang fp contract(off)
    uint32_t cell = 0, lo = 0, hi = 0;
    const bool in_grid = collider_cell_of(P.view, cx, cy, &cell);
    if (in_grid) {
        lo = P.cell_start[cell];
        hi = P.cell_start[cell + 1];
        if (lo == hi) return false;
    }
    q = prev[i];                                               // in flight while the list is walked
    FieldSum sum;
    if (!in_grid) {
        for (uint32_t j = 0; j < P.k; ++j) field_try(P, j, cx, cy, sum);
    } else {
        for (uint32_t e = lo; e < hi; ++e) field_try(P, P.items[e], cx, cy, sum);
    }
    return field_finish(sum, P.dt2, cx, cy, &q.x, &q.y);
}

__global__ __launch_bounds__(kStreamBlock) void k_fields_pass(const float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                              uint64_t n, FieldPassArgs P)
{
    const uint64_t pairs = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float4 *pos4 = reinterpret_cast<const float4 *>(pos);
    // particles this wave touched: wave-uniform among the lanes still in the loop.  Lane 0 holds the wave's lowest
    // index, leaves the loop last and so has seen every vote
    uint32_t touched = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const float4 c = pos4[i];
        float2 q0, q1;
        const bool t0 = field_resolve(P, prev, 2 * i, c.x, c.y, q0);
        const bool t1 = field_resolve(P, prev, 2 * i + 1, c.z, c.w, q1);
        if (t0) prev[2 * i] = q0;
        if (t1) prev[2 * i + 1] = q1;
        touched += (uint32_t)__popcll(ballot64(t0)) + (uint32_t)__popcll(ballot64(t1));
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t i = n - 1;
        const float2 c = pos[i];
        float2 q;
        if (field_resolve(P, prev, i, c.x, c.y, q)) {
            prev[i] = q;
            touched += 1;
        }
    }
    // the waves' totals folded through LDS: one integer atomic per workgroup that touched anything (as k_kick counts;
    // one per wave, all on one word, cost more than the pass itself where every wave touches something)
    __shared__ uint32_t s_touched[kStreamBlock / kWave];
    if (lane_id() == 0) s_touched[threadIdx.x >> 6] = touched;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int v = 0; v < kStreamBlock / kWave; ++v) total += s_touched[v];
        if (total) atomicAdd(P.touched, (unsigned long long)total);
    }
}

// One pass over prev[0, n) in place, pos read only.  cell_start / items / rec: device memory of view.gx * view.gy + 1
// words, the entries cell_start's last word counts (each < k) and 3 k float4.  *touched += the particles written
gpe_status launch_fields_pass(gpe_ctx *c, const float2 *pos, float2 *prev, uint64_t n, const uint32_t *cell_start,
                              const uint32_t *items, const float4 *rec, uint32_t k, const ColliderGridView &view, float dt2,
                              unsigned long long *touched)
{
    if (n == 0 || k == 0) return GPE_OK;
    FieldPassArgs P;
    P.cell_start = cell_start; P.items = items; P.rec = rec; P.k = k;
    P.view = view;
    P.dt2 = dt2;
    P.touched = touched;
    hipLaunchKernelGGL(k_fields_pass, dim3(stream_grid((n + 1) >> 1)), dim3(kStreamBlock), 0, c->stream, pos, prev, n, P);
    GPE_HIP(c, hipGetLastError());
    return GPE_OK;
}

}  // namespace gpe
