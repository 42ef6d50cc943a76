// k_region.h -- the region predicate and the tile shape shared by the full passes over the live set that select
// particles by a circle or a box: the region queries (k_query.hip) and the velocity kicks (k_edit.hip).  One
// definition, so that a kick touches exactly the set the query with the same arguments returns.  The queries have a
// third kind, the segment (gpe_query_segment), whose predicate is ray_touches of k_ray.h and reads the radius too.
#pragma once

#include "gpe_internal.h"
#include "k_ray.h"
#include "k_region_pred.h"

namespace gpe {

constexpr int kQueryBlock = 256;
constexpr int kQueryWaves = kQueryBlock / kWave;
constexpr int kQueryRounds = 8;                            // K: rounds per tile
constexpr uint64_t kQueryTile = (uint64_t)kQueryBlock * kQueryRounds;

enum QueryKind { kQueryCircle = 0, kQueryBox = 1, kQuerySegment = 2 };

// The region: the closed disc around (x0, y0) with rr = radius * radius, the closed box [x0, x1] x [y0, y1], or the
// segment from (x0, y0) to (x1, y1).
struct QueryRegion {
    float x0, y0, x1, y1, rr;
};

// The disc test of k_remove.hip (in_disc), restated: IEEE binary32, one rounding per operation, left to right, no FMA
// (the build also compiles with -ffp-contract=off).  The circle query returns what the eraser removes.  The arithmetic
// itself is k_region_pred.h's, which the force fields share.
__device__ __forceinline__ float dist2(const float2 p, float x, float y)
{
    return region_dist2(p.x, p.y, x, y);
}

template <int KIND>
__device__ __forceinline__ bool in_region(const float2 p, const QueryRegion &Q)
{
    if constexpr (KIND == kQueryCircle)
        return region_in_disc(p.x, p.y, Q.x0, Q.y0, Q.rr);
    else
        return region_in_box(p.x, p.y, Q.x0, Q.y0, Q.x1, Q.y1);
}

// hit[r] for the rounds of this thread's tile (false past n); the positions of all rounds are loaded first, so that
// kQueryRounds loads per lane are in flight together.  p[] keeps them for the caller.  `radius` is read by the segment
// kind alone (the circle and the box never load it).
template <int KIND>
__device__ __forceinline__ void matches_of_tile(const QueryRegion &Q, const float2 *__restrict__ pos, uint64_t n,
                                                uint64_t first, float2 (&p)[kQueryRounds], bool (&hit)[kQueryRounds],
                                                const float *__restrict__ radius = nullptr)
{
#pragma unroll
    for (int r = 0; r < kQueryRounds; ++r) {
        const uint64_t i = first + (uint64_t)r * kQueryBlock;
        p[r] = i < n ? pos[i] : make_float2(0.f, 0.f);
    }
    if constexpr (KIND == kQuerySegment) {
        float rad[kQueryRounds];
#pragma unroll
        for (int r = 0; r < kQueryRounds; ++r) {
            const uint64_t i = first + (uint64_t)r * kQueryBlock;
            rad[r] = i < n ? radius[i] : 0.f;                  // radius 0 is never touched
        }
#pragma unroll
        for (int r = 0; r < kQueryRounds; ++r) {
            float t;
            hit[r] = first + (uint64_t)r * kQueryBlock < n && ray_touches(Q.x0, Q.y0, Q.x1, Q.y1, p[r].x, p[r].y, rad[r], &t);
        }
    } else {
#pragma unroll
        for (int r = 0; r < kQueryRounds; ++r) hit[r] = first + (uint64_t)r * kQueryBlock < n && in_region<KIND>(p[r], Q);
    }
}

}  // namespace gpe
