// gpe_surfaces.hip -- the surface materials of the static colliders and the movers (gpe_set_surfaces, gpe_get_surfaces):
// one row per obstacle of the set held at the call, bounce and friction (k_surface.h is the one definition of what a
// row does).  The rows live beside their set (ColliderState, MoverState); gpe_colliders.hip and gpe_movers.hip launch the
// surface form of their pass only while their set holds rows, and call surfaces_drop when the set is replaced.
#include <string.h>

#include "gpe_internal.h"
#include "k_surface.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static_assert(sizeof(gpe_surface) == 16 && sizeof(gpe_surface) == sizeof(float4), "a surface row is one float4");
static_assert(sizeof(SurfaceRow) == sizeof(gpe_surface), "k_surface.h restates gpe_surface");
static_assert(kSurfacePlain == GPE_SURFACE_PLAIN, "k_surface.h restates the constants of include/gpe.h");

void gpe::surfaces_drop(gpe_ctx *c, uint32_t target)
{
    if (target == GPE_SURFACES_OF_COLLIDERS) {
        dev_free(c, c->colliders.surf);
        c->colliders.surfaces.clear();
    } else {
        dev_free(c, c->movers.surf); dev_free(c, c->movers.old);
        c->movers.surfaces.clear();
    }
}

gpe_status gpe_set_surfaces(gpe_ctx *c, uint32_t target, const gpe_surface *rows, uint64_t k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (target != GPE_SURFACES_OF_COLLIDERS && target != GPE_SURFACES_OF_MOVERS)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_surfaces: unknown target");
    if (k > 0 && !rows) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_surfaces: NULL rows");
    if (k > 0 && is_sharded(c)) return refuse_sharded(c, "gpe_set_surfaces");   // (such a context holds no set either)
    const bool of_movers = target == GPE_SURFACES_OF_MOVERS;
    const uint64_t held = of_movers ? c->movers.set.size() : c->colliders.set.size();
    if (k != 0 && k != held) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_surfaces: k must be 0 or the size of the target's set");
    std::vector<gpe_surface> set(rows, rows + k);
    for (uint64_t j = 0; j < k; ++j) {
        const char *why = surface_refusal(set[j].restitution, set[j].friction, set[j].flags, set[j].reserved);
        if (why) return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_surfaces: ") + why);
        if (set[j].restitution == 0.0f) set[j].restitution = 0.0f;     // -0.0 -> +0
        if (set[j].friction == 0.0f) set[j].friction = 0.0f;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old rows)
    if (k == 0) {
        surfaces_drop(c, target);
        return GPE_OK;
    }
    // the new rows beside the old ones (set_upload.h).  Read by index below k (the winner's index, always a member of
    // the set).  no slack
    float4 *d_surf = nullptr, *d_old = nullptr;
    HipSetUpload up({c}, "gpe_set_surfaces");
    up.reserve(&d_surf, k, of_movers ? "grid.mover_surf" : "grid.collider_surf");
    up.reserve(&d_old, of_movers ? k : 0, "grid.mover_old");
    up.copy(d_surf, set.data(), k);
    if (d_old) up.fill(d_old, 0, k * sizeof(float4));                  // (the build writes it before a pass reads it)
    GPE_TRY(up.finish());
    surfaces_drop(c, target);
    if (of_movers) {
        c->movers.surf = d_surf; c->movers.old = d_old;
        c->movers.surfaces.swap(set);
    } else {
        c->colliders.surf = d_surf;
        c->colliders.surfaces.swap(set);
    }
    return GPE_OK;
}

gpe_status gpe_get_surfaces(const gpe_ctx *c, uint32_t target, gpe_surface *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k || (capacity > 0 && !out)) return GPE_ERR_INVALID_ARG;
    if (target != GPE_SURFACES_OF_COLLIDERS && target != GPE_SURFACES_OF_MOVERS) return GPE_ERR_INVALID_ARG;
    return rows_out(target == GPE_SURFACES_OF_MOVERS ? c->movers.surfaces : c->colliders.surfaces, out, capacity, k);
}
