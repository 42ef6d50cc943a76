// gpe_colliders.hip -- the static colliders of a context (gpe_set_colliders and the rest): the set, its lookup grid
// (collider_grid.h, rebuilt lazily) and the pass behind every step (k_colliders.hip).  gpe_api.hip calls
// colliders_after_step from after_step and colliders_release from gpe_destroy.  Also the cell-list grid holder the
// fields share (CellListGrid: its release and its upload).
#include <math.h>
#include <string.h>

#include "collider_grid.h"
#include "gpe_internal.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

void gpe::cell_grid_release(gpe_ctx *c, CellListGrid &G)
{
    dev_free(c, G.cell_start); dev_free(c, G.items);
    G.valid = false;
    G.entries = 0;
    G.view = ColliderGridView();
}

gpe_status gpe::cell_grid_upload(gpe_ctx *c, const char *who, CellListGrid &G, const ColliderGridView &view,
                                 const std::vector<uint32_t> &cell_start, const std::vector<uint32_t> &items,
                                 const char *cell_start_tag, const char *items_tag)
{
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old tables)
    cell_grid_release(c, G);
    // read by index: cell_start below gx * gy + 1 (the pass reads the words of a cell collider_cell_of names and the
    // one behind it), items below cell_start's last word.  no slack
    HipSetUpload up({c}, who, "grid upload");
    up.reserve(&G.cell_start, cell_start.size(), cell_start_tag);
    up.reserve(&G.items, std::max<uint64_t>(items.size(), 1), items_tag);
    up.copy(G.cell_start, cell_start.data(), cell_start.size());
    up.copy(G.items, items.data(), items.size());
    GPE_TRY(up.finish());                                              // (the host's vectors go away on return)
    G.view = view;
    G.entries = items.size();
    G.w = c->cfg.world_width; G.h = c->cfg.world_height;
    G.valid = true;
    return GPE_OK;
}

void gpe::colliders_release(gpe_ctx *c)
{
    ColliderState &S = c->colliders;
    cell_grid_release(c, S.grid);
    surfaces_drop(c, GPE_SURFACES_OF_COLLIDERS);
    dev_free(c, S.rec); dev_free(c, S.pushed);
    S = ColliderState();
}

gpe_status gpe::refuse_colliders(gpe_ctx *c, const char *who)
{
    return refuse_holds(c, who, "colliders", "gpe_set_colliders");
}

// The grid for the radius bound and the world as they are now.  Builds only when one of them has changed since the last
// build; that synchronises.
static gpe_status colliders_grid_ready(gpe_ctx *c, const char *who)
{
    ColliderState &S = c->colliders;
    CellListGrid &G = S.grid;
    const float rb = c->max_radius, W = c->cfg.world_width, H = c->cfg.world_height;
    if (G.valid && bits_of(rb) == bits_of(G.rb) && bits_of(W) == bits_of(G.w) && bits_of(H) == bits_of(G.h)) return GPE_OK;
    const uint32_t k = (uint32_t)S.set.size();
    std::vector<ColliderCapsule> caps(k);
    for (uint32_t j = 0; j < k; ++j) caps[j] = {S.set[j].ax, S.set[j].ay, S.set[j].bx, S.set[j].by, S.set[j].radius};
    const ColliderGrid g = collider_grid_build(caps.data(), k, rb, W, H);
    GPE_TRY(cell_grid_upload(c, who, G, g.view, g.cell_start, g.items, "grid.collider_cell_start", "grid.collider_items"));
    G.rb = rb;
    return GPE_OK;
}

// One pass over the particles as they are now.  Enqueues only, unless the grid has to be rebuilt first.
static gpe_status colliders_pass(gpe_ctx *c, const char *who)
{
    ColliderState &S = c->colliders;
    if (S.set.empty() || c->n == 0 || !c->pos) return GPE_OK;
    GPE_TRY(colliders_grid_ready(c, who));
    Scope s(c, "Colliders");
    if (c->sweep.mode == GPE_SWEEP_ON) {
        GPE_TRY(sweep_pass(c));
        S.passes += 1;
        return GPE_OK;
    }
    GPE_TRY(launch_colliders_pass(c, c->pos, c->radius, c->n, S.grid.cell_start, S.grid.items, S.rec, (uint32_t)S.set.size(), S.grid.view,
                                  S.pushed, S.surf, c->prev));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::colliders_after_step(gpe_ctx *c)
{
    return colliders_pass(c, "gpe_step");                             // (after_step has looked: the set is not empty)
}

gpe_status gpe_set_colliders(gpe_ctx *c, const gpe_collider *colliders, uint64_t k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (k > 0 && !colliders) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_colliders: NULL colliders");
    if (k > GPE_COLLIDERS_MAX) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_colliders: k must be at most GPE_COLLIDERS_MAX");
    for (uint64_t j = 0; j < k; ++j) {
        const gpe_collider &q = colliders[j];
        if (!isfinite(q.ax) || !isfinite(q.ay) || !isfinite(q.bx) || !isfinite(q.by))
            return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_colliders: a coordinate is not finite");
        if (!isfinite(q.radius) || !(q.radius >= 0.0f))                // (-0.0 >= 0: accepted, stored as +0)
            return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_colliders: a radius is NaN, infinite or negative");
        if (q.flags) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_colliders: flags must be 0");
    }
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_colliders");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    ColliderState &S = c->colliders;
    if (k == 0) {
        colliders_release(c);
        return GPE_OK;
    }
    std::vector<gpe_collider> set(colliders, colliders + k);
    std::vector<float4> rec(2 * k);
    for (uint64_t j = 0; j < k; ++j) {
        if (set[j].radius == 0.0f) set[j].radius = 0.0f;               // -0.0 -> +0
        rec[2 * j] = make_float4(set[j].ax, set[j].ay, set[j].bx, set[j].by);
        rec[2 * j + 1] = make_float4(set[j].radius, 0.f, 0.f, 0.f);
    }
    // the new records and a counter word at 0 beside the old ones (set_upload.h).  Read by index below 2 k.  no slack
    float4 *d_rec = nullptr;
    unsigned long long *d_pushed = nullptr;
    HipSetUpload up({c}, "gpe_set_colliders");
    up.reserve(&d_rec, 2 * k, "grid.collider_rec");
    up.reserve(&d_pushed, 1, "grid.collider_pushed");
    up.copy(d_rec, rec.data(), rec.size());
    up.fill(d_pushed, 0, sizeof(unsigned long long));
    GPE_TRY(up.finish());
    dev_free(c, S.rec); dev_free(c, S.pushed);
    cell_grid_release(c, S.grid);                                      // built before the next pass
    surfaces_drop(c, GPE_SURFACES_OF_COLLIDERS);                       // a new set gets new surfaces
    S.pushed = d_pushed;
    S.rec = d_rec;
    S.set.swap(set);
    S.passes = 0;
    return GPE_OK;
}

gpe_status gpe_get_colliders(const gpe_ctx *c, gpe_collider *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k || (capacity > 0 && !out)) return GPE_ERR_INVALID_ARG;
    return rows_out(c->colliders.set, out, capacity, k);
}

gpe_status gpe_apply_colliders(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has_colliders(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return colliders_pass(c, "gpe_apply_colliders");
}

gpe_status gpe_get_colliders_info(gpe_ctx *c, gpe_colliders_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_colliders_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_colliders_info: NULL info or bad struct_size");
    ColliderState &S = c->colliders;
    gpe_colliders_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    out.k = (uint32_t)S.set.size();
    out.passes = S.passes;
    if (has_colliders(c)) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long pushed = 0;
        GPE_TRY(read_back(c, S.pushed, &pushed, sizeof(pushed)));
        out.pushed = pushed;
        if (S.grid.valid) {                                            // (none yet: no pass has needed it)
            out.grid_x = S.grid.view.gx; out.grid_y = S.grid.view.gy;
            out.list_entries = S.grid.entries;
        }
    }
    *info = out;
    return GPE_OK;
}
