// k_cells.h -- the NATIVE pipeline's cell membership: which neighbour cells a particle overlaps (k_native_hash).
// A header of its own so that tests/hip/cell_probe.hip runs the very function the hash kernel runs, beside the compat
// form (cell_coord / is_obj_in_cell, gpe_internal.h); tests/test_gpu_cell_math.py pins both to an IEEE binary32
// restatement of the oracle's.
#pragma once

#include "gpe_internal.h"

namespace gpe {

// Which of the 8 neighbour cells does the particle overlap?  Bit k = the k-th neighbour of the reference's scan
// (grid.wgsl:68-90: y outer, x inner, centre skipped).  is_obj_in_cell (grid.wgsl:117-129) per axis: the
// clamped offset of neighbour column i / row j does not depend on the other axis, so the 8 tests share 3 + 3
// squared offsets (same operations and order as dot(d, d) = d.x*d.x + d.y*d.y).
__device__ __forceinline__ uint32_t neighbour_overlap_mask(float2 p, float r, int32_t cx, int32_t cy, float cell_size)
{
    const float sq = r * r;
    float sx[3], sy[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lo_x = (float)(cx + i - 1) * cell_size, lo_y = (float)(cy + i - 1) * cell_size;
        // clamp as one v_med3_f32: equal to clamp_f for every non-NaN p (a zero of either sign squares
        // to +0 below), and for a NaN p the difference is NaN whatever the clamp returns
        const float dx = p.x - __builtin_amdgcn_fmed3f(p.x, lo_x, lo_x + cell_size);
        const float dy = p.y - __builtin_amdgcn_fmed3f(p.y, lo_y, lo_y + cell_size);
        sx[i] = dx * dx;
        sy[i] = dy * dy;
    }
    uint32_t over = 0;
    int k = 0;
#pragma unroll
    for (int y = -1; y <= 1; ++y) {
#pragma unroll
        for (int x = -1; x <= 1; ++x) {
            if (x == 0 && y == 0) continue;
            over |= (sx[x + 1] + sy[y + 1] < sq) ? (1u << k) : 0u;
            ++k;
        }
    }
    return over;
}

}  // namespace gpe
