// gpe_fields.hip -- the force fields of a context (gpe_set_fields and the rest): the set, its lookup grid (field_grid.h,
// rebuilt lazily) and the pass behind every step (k_fields.hip).  gpe_api.hip calls fields_after_step from after_step,
// fields_world_changed from gpe_set_world and fields_release from gpe_destroy.
#include <math.h>
#include <string.h>

#include "field_grid.h"
#include "gpe_internal.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static_assert(sizeof(gpe_field) == 56, "gpe_field is 56 bytes");
static_assert(sizeof(FieldRecord) == 3 * sizeof(float4), "a field record is three float4");
static_assert(kFieldEverywhere == GPE_FIELD_EVERYWHERE && kFieldCircle == GPE_FIELD_CIRCLE && kFieldBox == GPE_FIELD_BOX &&
              kFieldUniform == GPE_FIELD_UNIFORM && kFieldRadial == GPE_FIELD_RADIAL && kFieldVortex == GPE_FIELD_VORTEX &&
              kFieldDrag == GPE_FIELD_DRAG && kFalloffNone == GPE_FALLOFF_NONE && kFalloffLinear == GPE_FALLOFF_LINEAR,
              "k_field.h restates the enums of include/gpe.h");

void gpe::fields_release(gpe_ctx *c)
{
    FieldState &S = c->fields;
    cell_grid_release(c, S.grid);
    dev_free(c, S.rec); dev_free(c, S.touched);
    S = FieldState();
}

void gpe::fields_world_changed(gpe_ctx *c)
{
    c->fields.grid.valid = false;                                      // (the tables stay until the next pass replaces them)
}

gpe_status gpe::refuse_fields(gpe_ctx *c, const char *who)
{
    return refuse_holds(c, who, "force fields", "gpe_set_fields");
}

// The grid for the world as it is now.  Builds only when the world has changed since the last build; that synchronises.
static gpe_status fields_grid_ready(gpe_ctx *c, const char *who)
{
    FieldState &S = c->fields;
    CellListGrid &G = S.grid;
    const float W = c->cfg.world_width, H = c->cfg.world_height;
    if (G.cell_start && bits_of(W) == bits_of(G.w) && bits_of(H) == bits_of(G.h)) {
        G.valid = true;                                                // (gpe_set_world with the world it had)
        return GPE_OK;
    }
    const uint32_t k = (uint32_t)S.set.size();
    std::vector<FieldRegion> regions(k);
    for (uint32_t j = 0; j < k; ++j) regions[j] = {S.set[j].shape, S.set[j].x0, S.set[j].y0, S.set[j].x1, S.set[j].y1};
    const FieldGrid g = field_grid_build(regions.data(), k, W, H);
    return cell_grid_upload(c, who, G, g.view, g.cell_start, g.items, "grid.field_cell_start", "grid.field_items");
}

// One pass over the particles as they are now.  Enqueues only, unless the grid has to be rebuilt first.
static gpe_status fields_pass(gpe_ctx *c, float dt, const char *who)
{
    FieldState &S = c->fields;
    if (S.set.empty() || c->n == 0 || !c->pos) return GPE_OK;
    if (!S.grid.valid) GPE_TRY(fields_grid_ready(c, who));
    const float dt2 = dt * dt;                                         // as verlet_params forms it
    Scope s(c, "Fields");
    GPE_TRY(launch_fields_pass(c, c->pos, c->prev, c->n, S.grid.cell_start, S.grid.items, S.rec, (uint32_t)S.set.size(), S.grid.view, dt2,
                               S.touched));
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::fields_after_step(gpe_ctx *c, float dt)
{
    return fields_pass(c, dt, "gpe_step");                            // (after_step has looked: the set is not empty)
}

static const char *field_fault(const gpe_field &f)
{
    if (f.shape > GPE_FIELD_BOX) return "an unknown shape";
    if (f.kind > GPE_FIELD_DRAG) return "an unknown kind";
    if (f.falloff > GPE_FALLOFF_LINEAR) return "an unknown falloff";
    if (f.flags) return "flags must be 0";
    const float v[10] = {f.x0, f.y0, f.x1, f.y1, f.px, f.py, f.fx, f.fy, f.strength, f.reach};
    for (float x : v)
        if (!isfinite(x)) return "a value is not finite";
    if (f.shape == GPE_FIELD_CIRCLE && !(f.x1 >= 0.0f)) return "a circle's radius is negative";   // (-0.0 >= 0: accepted)
    if (f.falloff != GPE_FALLOFF_NONE && (f.kind == GPE_FIELD_UNIFORM || f.kind == GPE_FIELD_DRAG))
        return "a falloff on a UNIFORM or DRAG field";
    if (f.falloff == GPE_FALLOFF_LINEAR && !(f.reach > 0.0f)) return "LINEAR falloff needs a reach > 0";
    if (f.kind == GPE_FIELD_DRAG && !(f.strength >= 0.0f && f.strength <= 1.0f)) return "a DRAG strength outside [0, 1]";
    return nullptr;
}

gpe_status gpe_set_fields(gpe_ctx *c, const gpe_field *fields, uint64_t k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (k > 0 && !fields) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_fields: NULL fields");
    if (k > GPE_FIELDS_MAX) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_fields: k must be at most GPE_FIELDS_MAX");
    for (uint64_t j = 0; j < k; ++j)
        if (const char *why = field_fault(fields[j]))
            return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_fields: field " + std::to_string(j) + ": " + why);
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_fields");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    FieldState &S = c->fields;
    if (k == 0) {
        fields_release(c);
        return GPE_OK;
    }
    std::vector<gpe_field> set(fields, fields + k);
    std::vector<FieldRecord> rec(k);
    for (uint64_t j = 0; j < k; ++j) {
        gpe_field &f = set[j];
        if (f.shape == GPE_FIELD_CIRCLE && f.x1 == 0.0f) f.x1 = 0.0f;  // -0.0 -> +0
        FieldRecord &r = rec[j];
        r.x0 = f.x0; r.y0 = f.y0; r.x1 = f.x1; r.y1 = f.y1;
        r.px = f.px; r.py = f.py; r.fx = f.fx; r.fy = f.fy;
        r.strength = f.strength; r.reach = f.reach;
        r.rr = field_rr(f.x1);
        r.code = field_code(f.shape, f.kind, f.falloff);
    }
    // the new records and a counter word at 0 beside the old ones (set_upload.h).  Read by index below 3 k.  no slack
    float4 *d_rec = nullptr;
    unsigned long long *d_touched = nullptr;
    HipSetUpload up({c}, "gpe_set_fields");
    up.reserve(&d_rec, 3 * k, "grid.field_rec");
    up.reserve(&d_touched, 1, "grid.field_touched");
    up.copy(d_rec, rec.data(), rec.size());
    up.fill(d_touched, 0, sizeof(unsigned long long));
    GPE_TRY(up.finish());
    dev_free(c, S.rec); dev_free(c, S.touched);
    cell_grid_release(c, S.grid);                                      // built before the next pass
    S.touched = d_touched;
    S.rec = d_rec;
    S.set.swap(set);
    S.passes = 0;
    return GPE_OK;
}

gpe_status gpe_get_fields(const gpe_ctx *c, gpe_field *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k || (capacity > 0 && !out)) return GPE_ERR_INVALID_ARG;
    return rows_out(c->fields.set, out, capacity, k);
}

gpe_status gpe_apply_fields(gpe_ctx *c, float dt)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!isfinite(dt)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_apply_fields: dt is not finite");
    if (!has_fields(c) || c->n == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return fields_pass(c, dt, "gpe_apply_fields");
}

gpe_status gpe_get_fields_info(gpe_ctx *c, gpe_fields_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_fields_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_fields_info: NULL info or bad struct_size");
    FieldState &S = c->fields;
    gpe_fields_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    out.k = (uint32_t)S.set.size();
    out.passes = S.passes;
    if (has_fields(c)) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long touched = 0;
        GPE_TRY(read_back(c, S.touched, &touched, sizeof(touched)));
        out.touched = touched;
        if (S.grid.cell_start) {                                       // (none yet: no pass has needed it)
            out.grid_x = S.grid.view.gx; out.grid_y = S.grid.view.gy;
            out.list_entries = S.grid.entries;
        }
    }
    *info = out;
    return GPE_OK;
}
