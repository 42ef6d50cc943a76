// gpe_sweep.hip -- the sweep of the static colliders (gpe_set_collider_sweep and the rest): a mode of their pass and its
// two counters.  gpe_colliders.hip's colliders_pass calls sweep_pass while the mode is on (k_sweep.hip is the pass,
// k_sweep.h the rule); gpe_api.hip calls sweep_release from gpe_destroy.  Also the mode setter and the info getter
// this mode shares with the movers' sweep (sweep_mode_set, sweep_mode_info).
#include <string.h>

#include "gpe_internal.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

void gpe::sweep_release(gpe_ctx *c)
{
    dev_free(c, c->sweep.counts);
    c->sweep = SweepState();
}

// One swept pass over the particles as they are now: the colliders' grid is ready.  Enqueues only.
gpe_status gpe::sweep_pass(gpe_ctx *c)
{
    ColliderState &S = c->colliders;
    SweepState &W = c->sweep;
    if (!c->prev || !W.counts) return fail(c, GPE_ERR_STATE, "the swept colliders' pass: no previous positions or no counters");
    GPE_TRY(launch_colliders_sweep(c, c->pos, c->prev, c->radius, c->n, S.grid.cell_start, S.grid.items, S.rec,
                                   (uint32_t)S.set.size(), S.grid.view, S.pushed, W.counts, S.surf));
    W.passes += 1;
    return GPE_OK;
}

// Both sweep modes (this one and the movers', gpe_movers.hip): counts is two words, written by index 0 and 1 alone; the
// buffers are reserved when the mode is first switched on, all or none, and kept until gpe_destroy.  no slack
gpe_status gpe::sweep_mode_set(gpe_ctx *c, const char *who, SweepState &W, uint32_t mode, const char *tag,
                               std::initializer_list<SweepTable> more)
{
    if (mode != GPE_SWEEP_OFF && mode != GPE_SWEEP_ON)
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": mode must be GPE_SWEEP_OFF or GPE_SWEEP_ON");
    if (is_sharded(c)) return refuse_sharded(c, who);
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight counts into the old words)
    HipSetUpload up({c}, who, nullptr);
    if (mode == GPE_SWEEP_ON && !W.counts) {
        up.reserve(&W.counts, 2, tag);
        for (const SweepTable &t : more) up.reserve((uint8_t **)t.p, t.bytes, t.tag);
    }
    if (W.counts) up.fill(W.counts, 0, 2 * sizeof(unsigned long long));
    GPE_TRY(up.finish());
    W.mode = mode;
    W.passes = 0;
    return GPE_OK;
}

gpe_status gpe::sweep_mode_info(gpe_ctx *c, const char *who, const SweepState &W, gpe_sweep_info *info)
{
    if (!info || info->struct_size < sizeof(gpe_sweep_info))
        return fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": NULL info or bad struct_size");
    gpe_sweep_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    out.mode = W.mode;
    out.passes = W.passes;
    if (W.counts) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long counts[2] = {0, 0};
        GPE_TRY(read_back(c, W.counts, counts, sizeof(counts)));
        out.swept = counts[0];
        out.stopped = counts[1];
    }
    *info = out;
    return GPE_OK;
}

gpe_status gpe_set_collider_sweep(gpe_ctx *c, uint32_t mode)
{
    return c ? sweep_mode_set(c, "gpe_set_collider_sweep", c->sweep, mode, "grid.sweep_counts") : GPE_ERR_INVALID_ARG;
}

gpe_status gpe_get_collider_sweep(const gpe_ctx *c, uint32_t *mode)
{
    if (!c || !mode) return GPE_ERR_INVALID_ARG;
    *mode = c->sweep.mode;
    return GPE_OK;
}

gpe_status gpe_get_sweep_info(gpe_ctx *c, gpe_sweep_info *info)
{
    return c ? sweep_mode_info(c, "gpe_get_sweep_info", c->sweep, info) : GPE_ERR_INVALID_ARG;
}
