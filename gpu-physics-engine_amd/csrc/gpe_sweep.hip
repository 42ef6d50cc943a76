// gpe_sweep.hip -- the sweep of the static colliders (gpe_set_collider_sweep and the rest): a mode of their pass and its
// two counters.  gpe_colliders.hip's colliders_pass calls sweep_pass while the mode is on (k_sweep.hip is the pass,
// k_sweep.h the rule); gpe_api.hip calls sweep_release from gpe_destroy.
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
    GPE_TRY(launch_colliders_sweep(c, c->pos, c->prev, c->radius, c->n, S.cell_start, S.items, S.rec, (uint32_t)S.set.size(),
                                   S.view, S.pushed, W.counts, S.surf));
    W.passes += 1;
    return GPE_OK;
}

gpe_status gpe_set_collider_sweep(gpe_ctx *c, uint32_t mode)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (mode != GPE_SWEEP_OFF && mode != GPE_SWEEP_ON)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_collider_sweep: mode must be GPE_SWEEP_OFF or GPE_SWEEP_ON");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_collider_sweep");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight counts into the old words)
    SweepState &W = c->sweep;
    // two words, written by index 0 and 1 alone.  no slack.  Kept until gpe_destroy once the mode has been on
    if (mode == GPE_SWEEP_ON && !W.counts) GPE_TRY(ws_alloc(c, "gpe_set_collider_sweep", &W.counts, 2, 0, "grid.sweep_counts"));
    if (W.counts) {
        hipError_t e = hipMemsetAsync(W.counts, 0, 2 * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, GPE_ERR_HIP, std::string("gpe_set_collider_sweep: ") + hipGetErrorName(e));
        }
    }
    W.mode = mode;
    W.passes = 0;
    return GPE_OK;
}

gpe_status gpe_get_collider_sweep(const gpe_ctx *c, uint32_t *mode)
{
    if (!c || !mode) return GPE_ERR_INVALID_ARG;
    *mode = c->sweep.mode;
    return GPE_OK;
}

gpe_status gpe_get_sweep_info(gpe_ctx *c, gpe_sweep_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_sweep_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_sweep_info: NULL info or bad struct_size");
    const SweepState &W = c->sweep;
    gpe_sweep_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    out.mode = W.mode;
    out.passes = W.passes;
    if (W.counts) {
        GPE_HIP(c, hipSetDevice(c->device));
        unsigned long long counts[2] = {0, 0};
        GPE_HIP(c, hipMemcpyAsync(counts, W.counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
        GPE_TRY(check_device_errors(c));                               // (synchronises the stream)
        out.swept = counts[0];
        out.stopped = counts[1];
    }
    *info = out;
    return GPE_OK;
}
