// gpe_colliders.hip -- the static colliders of a context (gpe_set_colliders and the rest): the set, its lookup grid
// (collider_grid.h, rebuilt lazily) and the pass behind every step (k_colliders.hip).  gpe_api.hip calls
// colliders_after_step from gpe_step / gpe_run, before the observers, and colliders_release from gpe_destroy.
#include <math.h>
#include <string.h>

#include "collider_grid.h"
#include "gpe_internal.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}

static void colliders_grid_release(gpe_ctx *c)
{
    ColliderState &S = c->colliders;
    dev_free(c, S.cell_start); dev_free(c, S.items);
    S.grid_valid = false;
    S.entries = 0;
    S.view = ColliderGridView();
}

void gpe::colliders_release(gpe_ctx *c)
{
    ColliderState &S = c->colliders;
    colliders_grid_release(c);
    surfaces_drop(c, GPE_SURFACES_OF_COLLIDERS);
    dev_free(c, S.rec); dev_free(c, S.pushed);
    S = ColliderState();
}

gpe_status gpe::refuse_colliders(gpe_ctx *c, const char *who)
{
    return fail(c, GPE_ERR_UNSUPPORTED, std::string(who) + ": not supported while the context holds colliders "
                                                            "(gpe_set_colliders with k = 0 clears them)");
}

// The grid for the radius bound and the world as they are now.  Builds only when one of them has changed since the last
// build; that synchronises (a pass in flight reads the old tables, the host's vectors go away on return).
static gpe_status colliders_grid_ready(gpe_ctx *c, const char *who)
{
    ColliderState &S = c->colliders;
    const float rb = c->max_radius, W = c->cfg.world_width, H = c->cfg.world_height;
    if (S.grid_valid && bits_of(rb) == bits_of(S.grid_rb) && bits_of(W) == bits_of(S.grid_w) && bits_of(H) == bits_of(S.grid_h))
        return GPE_OK;
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    colliders_grid_release(c);
    const uint32_t k = (uint32_t)S.set.size();
    std::vector<ColliderCapsule> caps(k);
    for (uint32_t j = 0; j < k; ++j) caps[j] = {S.set[j].ax, S.set[j].ay, S.set[j].bx, S.set[j].by, S.set[j].radius};
    const ColliderGrid g = collider_grid_build(caps.data(), k, rb, W, H);
    // read by index: cell_start below gx * gy + 1 (the pass reads the words of a cell collider_cell_of names and the
    // one behind it), items below cell_start's last word.  no slack
    gpe_status st = ws_alloc(c, who, &S.cell_start, g.cell_start.size(), 0, "grid.collider_cell_start");
    if (st == GPE_OK) st = ws_alloc(c, who, &S.items, std::max<uint64_t>(g.items.size(), 1), 0, "grid.collider_items");
    if (st == GPE_OK) {
        hipError_t e = hipMemcpyAsync(S.cell_start, g.cell_start.data(), g.cell_start.size() * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && !g.items.empty())
            e = hipMemcpyAsync(S.items, g.items.data(), g.items.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st = fail(c, GPE_ERR_HIP, std::string(who) + ": grid upload: " + hipGetErrorName(e));
        }
    }
    if (st != GPE_OK) {
        const std::string why = c->last_error;
        colliders_grid_release(c);                                     // no grid: the next pass tries again
        c->last_error = why;
        return st;
    }
    S.view = g.view;
    S.entries = g.items.size();
    S.grid_rb = rb; S.grid_w = W; S.grid_h = H;
    S.grid_valid = true;
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
    GPE_TRY(launch_colliders_pass(c, c->pos, c->radius, c->n, S.cell_start, S.items, S.rec, (uint32_t)S.set.size(), S.view,
                                  S.pushed, S.surf, c->prev));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::colliders_after_step(gpe_ctx *c)
{
    return has_colliders(c) ? colliders_pass(c, "gpe_step") : GPE_OK;
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
    // the new records beside the old ones: a failure leaves the previous set as it was.  Read by index below 2 k.  no slack
    float4 *d_rec = nullptr;
    gpe_status st = ws_alloc(c, "gpe_set_colliders", &d_rec, 2 * k, 0, "grid.collider_rec");
    if (st == GPE_OK && !S.pushed) st = ws_alloc(c, "gpe_set_colliders", &S.pushed, 1, 0, "grid.collider_pushed");
    if (st == GPE_OK) {
        hipError_t e = hipMemcpyAsync(d_rec, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(S.pushed, 0, sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // the host vector goes away on return
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st = fail(c, GPE_ERR_HIP, std::string("gpe_set_colliders: upload: ") + hipGetErrorName(e));
        }
    }
    if (st != GPE_OK) {
        const std::string why = c->last_error;
        dev_free(c, d_rec);
        c->last_error = why;
        return st;
    }
    dev_free(c, S.rec);
    colliders_grid_release(c);                                         // built before the next pass
    surfaces_drop(c, GPE_SURFACES_OF_COLLIDERS);                       // a new set gets new surfaces
    S.rec = d_rec;
    S.set.swap(set);
    S.passes = 0;
    return GPE_OK;
}

gpe_status gpe_get_colliders(const gpe_ctx *c, gpe_collider *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k || (capacity > 0 && !out)) return GPE_ERR_INVALID_ARG;
    const std::vector<gpe_collider> &set = c->colliders.set;
    *k = set.size();
    const uint64_t m = std::min<uint64_t>(set.size(), capacity);
    if (m) memcpy(out, set.data(), m * sizeof(gpe_collider));
    return GPE_OK;
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
        GPE_HIP(c, hipMemcpyAsync(&pushed, S.pushed, sizeof(pushed), hipMemcpyDeviceToHost, c->stream));
        GPE_TRY(check_device_errors(c));                               // (synchronises the stream)
        out.pushed = pushed;
        if (S.grid_valid) {                                            // (none yet: no pass has needed it)
            out.grid_x = S.view.gx; out.grid_y = S.view.gy;
            out.list_entries = S.entries;
        }
    }
    *info = out;
    return GPE_OK;
}
