// k_capsule_pass.h -- what the passes against capsules share beside the pair loop (k_stream_pairs.h): the two walks
// over a lookup grid's candidates, the plain rule of one particle (k_collider.h, k_surface.h) and the swept rule of one
// particle (k_sweep.h), each written once over what a pass supplies.  The static colliders find their candidates in CSR
// lists, the movers in bit masks; the fields' pass (k_fields.hip) uses the CSR cell lookup and walk alone.
//
// The walks.  Both call f(j) once per candidate in ASCENDING index order (the fields sum in it) and read nothing when
// there is nothing to walk.
//     csr_each   every item 0 .. k - 1, or the entries of the ranges range(y) names for y0 <= y <= y1: the list of one
//                cell (already in registers) or, per row of a box, the lists of that row's cells, contiguous in items[]
//     mask_each  the set bits of word(w) for every bit w of summary, ascending words, ascending bits; word(w) is one
//                mask word of a cell, or the OR of that word over the cells of a box (no array, no scratch)
//
// capsule_resolve<SURF>: the plain rule.  The pass supplies its tables P (rec, k, view, world_w, world_h and, for SURF,
// surf and prev, by these names), a lookup L and a wall-move hook.
//     L.empty(cell)   reads what says whether the cell has candidates (two words of cell_start, or the summary word)
//                     and keeps it for L.each(f), the walk of that cell
//     wall(j, s, u, &wx, &wy)   the displacement of winner j's wall at the contact: 0 for a static collider,
//                     surface_wall_move of the old and the new capsule for a mover
// It guarantees: a particle whose cell is empty returns in front of the radius load, having read its cell's words
// alone; a particle with no cell or with a radius the table was not built for is tried against every item; the winner
// is measured again (the same bits) and pushed or, for SURF, handed to surface_apply, which also rewrites prev[i].
//
// swept_resolve<SURF>: the swept rule over a policy S.
//     S.cands(x0, x1, C)       the candidates of the box of the path x0 -> x1; false: in the grid and none.  C.all:
//                              every item
//     S.each(C, f)             their walk
//     S.judge(j, from, to, r, &c)   the contact of item j on the path from -> to (the policy orders the arguments as its
//                              own arithmetic takes them)
//     S.respond(who, win, p, q, r, res)   res = (pos', prev') of the winner's response
//     S.P                      the tables: view.rb, world_w, world_h
// It guarantees: the path's box is read in front of the radius load; a radius the table was not built for walks every
// item, in the verification too; the winner by sweep_better; one verification over the box from prev to the result, the
// winner included; sweep_stop for a particle still over the slop.
#pragma once

#include "gpe_internal.h"
#include "k_sweep.h"

namespace gpe {

constexpr uint32_t kSweepMoved = 1u, kSweepSwept = 2u, kSweepStopped = 4u;   // what a resolve returns: k_stream_pairs.h's flags

template <class Range, class F>
__device__ __forceinline__ void csr_each(const uint32_t *items, uint32_t k, bool all, uint32_t y0, uint32_t y1, Range range, F f)
{
    if (all) {
        for (uint32_t j = 0; j < k; ++j) f(j);
    } else {
        for (uint32_t y = y0; y <= y1; ++y) {
            uint32_t lo, hi;
            range(y, lo, hi);
            for (uint32_t e = lo; e < hi; ++e) f(items[e]);
        }
    }
}

template <class Word, class F>
__device__ __forceinline__ void mask_each(uint32_t summary, Word word, F f)
{
    while (summary) {
        const uint32_t w = (uint32_t)__builtin_ctz(summary);   // < words: the build sets no other bit
        summary &= summary - 1;
        unsigned long long bits = word(w);
        while (bits) {
            const uint32_t b = (uint32_t)__builtin_ctzll(bits);
            bits &= bits - 1;
            f(w * 64u + b);                                     // < k: the build sets bits of its items only
        }
    }
}

// the list of one cell: the two words are its bounds
struct CsrCellLookup {
    const uint32_t *cell_start, *items;
    __device__ __forceinline__ bool empty(uint32_t cell, uint32_t &lo, uint32_t &hi) const
    {
        lo = cell_start[cell];
        hi = cell_start[cell + 1];
        return lo == hi;
    }
    template <class F>
    __device__ __forceinline__ void each(uint32_t, uint32_t lo, uint32_t hi, F f) const
    {
        csr_each(items, 0, false, 0, 0, [&](uint32_t, uint32_t &a, uint32_t &b) { a = lo; b = hi; }, f);
    }
};

// the masks of one cell: the first word is the cell's summary
struct MaskCellLookup {
    const unsigned long long *masks;
    const uint32_t *summary;
    uint32_t words;
    __device__ __forceinline__ bool empty(uint32_t cell, uint32_t &s, uint32_t &) const
    {
        s = summary[cell];
        return s == 0;
    }
    template <class F>
    __device__ __forceinline__ void each(uint32_t cell, uint32_t s, uint32_t, F f) const
    {
        const unsigned long long *mask = masks + (uint64_t)cell * words;
        mask_each(s, [&](uint32_t w) { return mask[w]; }, f);
    }
};

// touch, key, max: item j of rec against the particle at p
__device__ __forceinline__ void capsule_try(const float4 *rec, uint32_t j, float px, float py, float r, unsigned long long &best)
{
    const float4 s = rec[2 * j];
    const float R = rec[2 * j + 1].x;
    ColliderTouch t;
    if (!collider_touch(px, py, r, s.x, s.y, s.z, s.w, R, &t)) return;
    const unsigned long long key = collider_key(t.depth, j);
    best = key > best ? key : best;
}

// particle i at (px, py).  true: it moved, (ox, oy) is its new position.  SURF: the winner's surface is applied against
// the wall's displacement at the contact, and prev[i] written here, unless the row is PLAIN or p - prev is not finite
template <bool SURF, class Args, class Lookup, class Wall>
__device__ __forceinline__ bool capsule_resolve(const Args &P, const Lookup &L, Wall wall, const float *__restrict__ radius, uint64_t i,
                                                float px, float py, float &ox, float &oy)
{
#pragma clang fp contract(off)
    uint32_t cell = 0, w0 = 0, w1 = 0;                         // the cell and what L read of it
    const bool in_grid = collider_cell_of(P.view, px, py, &cell);
    if (in_grid) {
        if (L.empty(cell, w0, w1)) return false;
    }
    const float r = radius[i];
    unsigned long long best = 0;
    auto attempt = [&](uint32_t j) { capsule_try(P.rec, j, px, py, r, best); };
    // no cell (outside the grid, NaN) or a radius the table was not built for: every item.  Exactness never rests on
    // the grid
    if (!in_grid || !(fabsf(r) <= P.view.rb)) {
        for (uint32_t j = 0; j < P.k; ++j) attempt(j);
    } else {
        L.each(cell, w0, w1, attempt);
    }
    if (best == 0) return false;
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
    const float4 s = P.rec[2 * j];
    ColliderTouch t;
    (void)collider_touch(px, py, r, s.x, s.y, s.z, s.w, P.rec[2 * j + 1].x, &t);   // the winner again: the same bits
    float nx, ny;
    collider_normal(t, &nx, &ny);
    if constexpr (SURF) {
        const float4 row = P.surf[j];
        if (!(__float_as_uint(row.z) & kSurfacePlain)) {
            const float2 pv = P.prev[i];
            if (surface_velocity_finite(px, py, pv.x, pv.y)) {
                float wx, wy;
                wall(j, s, t.u, &wx, &wy);
                float o[4];
                surface_apply(px, py, pv.x, pv.y, r, nx, ny, t.depth, wx, wy, row.x, row.y, P.world_w, P.world_h, o);
                ox = o[0];
                oy = o[1];
                P.prev[i] = make_float2(o[2], o[3]);
                return true;
            }
        }
    }
    const float mx = nx * t.depth;
    const float my = ny * t.depth;
    const float qx = px + mx;
    const float qy = py + my;
    ox = clamp_f(qx, r, P.world_w - r);                        // particle_integration.wgsl:70-71, as verlet_one
    oy = clamp_f(qy, r, P.world_h - r);
    return true;
}

// particle i at p with the previous position q.  -> kSweep* flags; moved: o = (pos', prev')
template <bool SURF, class Policy>
__device__ __forceinline__ uint32_t swept_resolve(const Policy &S, const float *__restrict__ radius, uint64_t i, float px,
                                                  float py, float qx, float qy, float4 &o)
{
#pragma clang fp contract(off)
    typename Policy::Cands C;
    if (!S.cands(qx, qy, px, py, C)) return 0;
    const float r = radius[i];
    // a radius the table was not built for: every item.  Exactness never rests on the grid
    const bool wide = !(fabsf(r) <= S.P.view.rb);
    if (wide) C.all = true;
    SweepContact win;
    uint32_t who = 0;
    bool have = false;
    S.each(C, [&](uint32_t j) {
        SweepContact c;
        if (!S.judge(j, qx, qy, px, py, r, &c)) return;
        if (!have || sweep_better(c, j, win, who)) {
            win = c;
            who = j;
            have = true;
        }
    });
    if (!have) return 0;
    const uint32_t flags = kSweepMoved | ((win.t > 0.0f && win.t < 1.0f) ? kSweepSwept : 0u);
    float res[4];
    S.respond(who, win, px, py, qx, qy, r, res);
    // verify once: every item on the path prev -> result, the winner included
    typename Policy::Cands V;
    bool over = false;
    if (S.cands(qx, qy, res[0], res[1], V) || wide) {
        if (wide) V.all = true;
        S.each(V, [&](uint32_t j) {
            SweepContact c;
            if (S.judge(j, qx, qy, res[0], res[1], r, &c) && sweep_over_slop(c)) over = true;
        });
    }
    if (over) {
        float sx, sy;
        sweep_stop(r, win, S.P.world_w, S.P.world_h, &sx, &sy);
        o = make_float4(sx, sy, qx, qy);
        return flags | kSweepStopped;
    }
    o = make_float4(res[0], res[1], res[2], res[3]);
    return flags;
}

}  // namespace gpe
