// k_fields.hip -- the force fields' pass: every particle against the fields of its lookup cell, their accelerations
// summed and their drags multiplied in ascending field index, then prev rewritten (k_field.h says what a field
// contributes and how the sum is applied).  pos is only read.
//
// A streaming pass over the pair loop of k_stream_pairs.h, called from the kernel function itself.  The common lane
// finds an empty list: it has read its pos and two words of cell_start per particle and is done -- no prev load, no
// store.  prev is loaded only under a non-empty list and stored only for a particle some field matched.  The fields
// are 48-byte records (three float4: region | pole, uniform | strength, reach, rr, code): 4096 of them are 192 KB and
// stay in an XCD's L2; cell_start is read at the particles' own locality (they are kept in Morton order).  A particle
// outside the grid or with a NaN coordinate walks all k fields: no result rests on the grid.
#include "gpe_internal.h"
#include "k_capsule_pass.h"
#include "k_field.h"
#include "k_stream_pairs.h"

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
    const CsrCellLookup L{P.cell_start, P.items};
    if (in_grid) {
        if (L.empty(cell, lo, hi)) return false;
    }
    q = prev[i];                                               // in flight while the list is walked
    FieldSum sum;
    auto attempt = [&](uint32_t j) { field_try(P, j, cx, cy, sum); };
    if (!in_grid) {
        for (uint32_t j = 0; j < P.k; ++j) attempt(j);
    } else {
        L.each(cell, lo, hi, attempt);
    }
    return field_finish(sum, P.dt2, cx, cy, &q.x, &q.y);
}

__global__ __launch_bounds__(kStreamBlock) void k_fields_pass(const float2 *__restrict__ pos, float2 *__restrict__ prev,
                                                              uint64_t n, FieldPassArgs P)
{
    const PairCounts<1> count = stream_pairs<1, false>(
        pos, nullptr, n,
        [&](uint64_t i, float cx, float cy, float, float, float4 &o) -> bool {
            float2 q;
            const bool hit = field_resolve(P, prev, i, cx, cy, q);
            o.x = q.x;
            o.y = q.y;
            return hit;
        },
        [&](uint64_t i, bool, const float4 &o, float, float, float, float) { prev[i] = make_float2(o.x, o.y); });
    const uint32_t touched = count.of[0];
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
