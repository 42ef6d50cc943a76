// gpe_observe.hip -- what watches a run without changing it: the tracer recorder (gpe_tracers_*) and the run monitor
// (gpe_measure, gpe_monitor_*).  gpe_api.hip calls observers_after_step from gpe_step / gpe_run and observers_release
// from gpe_destroy.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "gpe_internal.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

// ---- tracers (k_tracers.hip) ---------------------------------------------------------------------------------
static void tracers_release(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    dev_free(c, t.keys); dev_free(c, t.perm); dev_free(c, t.slot_index);
    dev_free(c, t.ring_pos); dev_free(c, t.ring_prev); dev_free(c, t.ring_index);
    t = TracerState();
}

// One frame at the current steps_seen into ring slot recorded % frames.  Enqueues only: a memset and the resolve pass
// when the slot table is stale, then the sample.  The step numbers stay on the host, which issues every frame.
static gpe_status tracers_take_frame(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    const uint32_t k = (uint32_t)t.k;
    if (t.stale) {
        Scope s(c, "tracers/resolve");
        GPE_HIP(c, hipMemsetAsync(t.slot_index, 0xff, k * sizeof(uint32_t), c->stream));
        if (c->uid.on && c->uid.uids)                                  // uids off: nothing to read, every tracer is absent
            GPE_TRY(launch_tracers_resolve(c, c->uid.uids, c->n, t.keys, t.perm, k, t.lo, t.hi, t.slot_index));
        t.stale = false;
    }
    const uint64_t slot = t.recorded % t.frames, row = slot * t.k;
    {
        Scope s(c, "tracers/sample");
        GPE_TRY(launch_tracers_sample(c, t.slot_index, k, c->pos, c->prev, c->n, t.ring_pos ? t.ring_pos + row : nullptr,
                                      t.ring_prev ? t.ring_prev + row : nullptr,
                                      t.ring_index ? t.ring_index + row : nullptr));
    }
    t.step_of[slot] = t.steps_seen;
    t.recorded += 1;
    t.held = std::min(t.held + 1, t.frames);
    return GPE_OK;
}

gpe_status gpe_tracers_begin(gpe_ctx *c, const gpe_tracer_config *cfg)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!cfg || cfg->struct_size < sizeof(gpe_tracer_config))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: NULL cfg or bad struct_size");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_tracers_begin");
    constexpr uint32_t kFields = GPE_TRACER_POS | GPE_TRACER_PREV | GPE_TRACER_INDEX;
    if (!cfg->uids) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: NULL uids");
    if (cfg->k == 0 || cfg->k > GPE_TRACERS_MAX)
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: k must be 1 .. GPE_TRACERS_MAX");
    if (cfg->every == 0 || cfg->frames == 0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: every and frames must be >= 1");
    if (cfg->fields == 0 || (cfg->fields & ~kFields))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: fields must be GPE_TRACER_* bits, at least one");
    const uint32_t k = (uint32_t)cfg->k;
    // the tracked uids ascending with the tracer each one is: what the resolve pass searches
    std::vector<uint32_t> perm(k), keys(k);
    for (uint32_t j = 0; j < k; ++j) perm[j] = j;
    std::sort(perm.begin(), perm.end(), [cfg](uint32_t a, uint32_t b) { return cfg->uids[a] < cfg->uids[b]; });
    for (uint32_t j = 0; j < k; ++j) keys[j] = cfg->uids[perm[j]];
    for (uint32_t j = 1; j < k; ++j)
        if (keys[j] == keys[j - 1]) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_begin: two tracers share a uid");
    if (c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_begin: already armed (gpe_tracers_end first)");
    if (!c->uid.on) return fail(c, GPE_ERR_STATE, "gpe_tracers_begin: uids are off (gpe_enable_uids)");
    GPE_TRY(need_particles(c));
    if (cfg->frames > (1ull << 40) / k)                                // (frames * k * 8 bytes is far past any device)
        return fail(c, GPE_ERR_OOM, "gpe_tracers_begin: the ring does not fit in device memory");
    GPE_HIP(c, hipSetDevice(c->device));
    TracerState &t = c->tracers;
    const uint64_t rows = cfg->frames * cfg->k;
    // every array is read and written by index below k or frames * k (the resolve pass reads keys by single words
    // below k, the uids by 16-byte groups below n / 4 and single words below n).  no slack
    HipSetUpload up({c}, "gpe_tracers_begin");                         // (a failure leaves the recorder unarmed, as before)
    up.reserve(&t.keys, k, "tracers.keys");
    up.reserve(&t.perm, k, "tracers.perm");
    up.reserve(&t.slot_index, k, "tracers.slot_index");
    up.reserve(&t.ring_pos, (cfg->fields & GPE_TRACER_POS) ? rows : 0, "tracers.ring_pos");
    up.reserve(&t.ring_prev, (cfg->fields & GPE_TRACER_PREV) ? rows : 0, "tracers.ring_prev");
    up.reserve(&t.ring_index, (cfg->fields & GPE_TRACER_INDEX) ? rows : 0, "tracers.ring_index");
    up.copy(t.keys, keys.data(), k);
    up.copy(t.perm, perm.data(), k);
    GPE_TRY(up.finish());
    t.armed = true;
    t.stale = true;
    t.fields = cfg->fields;
    t.k = cfg->k; t.every = cfg->every; t.frames = cfg->frames;
    t.steps_seen = t.recorded = t.held = 0;
    t.lo = keys.front(); t.hi = keys.back();
    t.step_of.assign((size_t)cfg->frames, 0);
    return GPE_OK;
}

gpe_status gpe_tracers_sample(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_sample: not armed (gpe_tracers_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    return tracers_take_frame(c);
}

gpe_status gpe_tracers_read(gpe_ctx *c, gpe_tracer_frames *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out || out->struct_size < sizeof(gpe_tracer_frames))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: NULL out or bad struct_size");
    out->count = out->recorded = 0;
    TracerState &t = c->tracers;
    if (!t.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_read: not armed (gpe_tracers_begin)");
    if (out->flags & ~(uint32_t)GPE_TRACERS_CONSUME) return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: unknown flag");
    if ((out->pos_xy && !t.ring_pos) || (out->prev_xy && !t.ring_prev) || (out->index && !t.ring_index))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_tracers_read: an array for a field the recorder was not configured with");
    GPE_HIP(c, hipSetDevice(c->device));
    const uint64_t m = std::min(t.held, out->capacity), first = t.recorded - m;   // frames first .. recorded - 1
    // the frames lie in at most two runs of ring slots
    for (uint64_t done = 0; done < m;) {
        const uint64_t slot = (first + done) % t.frames, run = std::min(m - done, t.frames - slot);
        const uint64_t src = slot * t.k, dst = done * t.k, rows = run * t.k;
        if (out->pos_xy)
            GPE_HIP(c, hipMemcpyAsync(out->pos_xy + 2 * dst, t.ring_pos + src, rows * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        if (out->prev_xy)
            GPE_HIP(c, hipMemcpyAsync(out->prev_xy + 2 * dst, t.ring_prev + src, rows * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        if (out->index)
            GPE_HIP(c, hipMemcpyAsync(out->index + dst, t.ring_index + src, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->step)
            for (uint64_t f = 0; f < run; ++f) out->step[done + f] = t.step_of[slot + f];
        done += run;
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    out->count = t.held;
    out->recorded = t.recorded;
    if (out->flags & GPE_TRACERS_CONSUME) t.held = 0;
    return check_device_errors(c);
}

gpe_status gpe_tracers_end(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->tracers.armed) return fail(c, GPE_ERR_STATE, "gpe_tracers_end: not armed (gpe_tracers_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (frames in flight still write the ring)
    tracers_release(c);
    return GPE_OK;
}

// ---- run monitor (k_monitor.hip) -------------------------------------------------------------------------------
static void monitor_release(gpe_ctx *c)
{
    dev_free(c, c->monitor.ring); dev_free(c, c->monitor.partials);
    c->monitor = MonitorState();
}

// The scratch of every record: the partial records, then the device record of gpe_measure.  Written by index below
// monitor_grid(n) <= kMonitorMaxBlocks and whole records.  no slack
static gpe_status monitor_reserve(gpe_ctx *c, const char *who)
{
    if (c->monitor.partials) return GPE_OK;
    return ws_alloc(c, who, &c->monitor.partials, kMonitorMaxBlocks * kMonitorPartialBytes + sizeof(gpe_measures), 0,
                    "monitor.partials", "does not fit in device memory");
}

// One record of the particles as they are now into *out (device memory).  Enqueues only.  Reads whichever pos / prev /
// uids are live (the native step swaps pos with its copy partner), gpe_len and the world at this moment.
static gpe_status monitor_record(gpe_ctx *c, const char *who, float rest_speed, uint64_t step, gpe_measures *out)
{
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, who);
    const float rs2 = rest_speed * rest_speed;                         // binary32 (-0.0 -> +0, +inf -> +inf)
    if (c->n) {
        Scope s(c, "monitor/partial");
        GPE_TRY(launch_monitor_partial(c, c->pos, c->prev, c->n, rs2, c->cfg.world_width, c->cfg.world_height,
                                       c->monitor.partials));
    }
    Scope s(c, "monitor/final");
    return launch_monitor_final(c, c->monitor.partials, c->n, step, c->uid.on ? c->uid.uids : nullptr, out);
}

// One frame at the current steps_seen into ring slot recorded % frames.
static gpe_status monitor_take_frame(gpe_ctx *c)
{
    MonitorState &m = c->monitor;
    GPE_TRY(monitor_record(c, "gpe_monitor", m.rest_speed, m.steps_seen, m.ring + m.recorded % m.frames));
    m.recorded += 1;
    m.held = std::min(m.held + 1, m.frames);
    return GPE_OK;
}

static bool monitor_rest_speed_ok(float r) { return r >= 0.0f; }      // NaN and negatives fail; -0.0 and +inf pass

gpe_status gpe_measure(gpe_ctx *c, float rest_speed, gpe_measures *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out) return fail(c, GPE_ERR_INVALID_ARG, "gpe_measure: NULL out");
    if (!monitor_rest_speed_ok(rest_speed)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_measure: rest_speed is NaN or negative");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_measure");
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, "gpe_measure");
    gpe_measures r;
    if (c->n == 0) {                                                   // nothing to read: the "none" values
        memset(&r, 0, sizeof(r));
        r.min_x = r.min_y = INFINITY;
        r.max_x = r.max_y = -INFINITY;
        r.max_v2_index = r.first_irregular = 0xFFFFFFFFu;
        r.max_v2_uid = r.first_irregular_uid = GPE_UID_ABSENT;
        *out = r;
        return GPE_OK;
    }
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(monitor_reserve(c, "gpe_measure"));
    gpe_measures *dev = (gpe_measures *)(c->monitor.partials + kMonitorMaxBlocks * kMonitorPartialBytes);
    GPE_TRY(monitor_record(c, "gpe_measure", rest_speed, 0, dev));
    GPE_HIP(c, hipMemcpyAsync(&r, dev, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    GPE_TRY(check_device_errors(c));                                   // (synchronises the stream)
    *out = r;
    return GPE_OK;
}

gpe_status gpe_monitor_begin(gpe_ctx *c, const gpe_monitor_config *cfg)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!cfg || cfg->struct_size < sizeof(gpe_monitor_config))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: NULL cfg or bad struct_size");
    if (cfg->flags) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: flags must be 0");
    if (cfg->every == 0 || cfg->frames == 0) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: every and frames must be >= 1");
    if (!monitor_rest_speed_ok(cfg->rest_speed))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_begin: rest_speed is NaN or negative");
    if (is_sharded(c)) return refuse_sharded(c, "gpe_monitor_begin");
    if (c->n > 0xFFFFFFFFull) return refuse_too_many(c, "gpe_monitor_begin");
    MonitorState &m = c->monitor;
    if (m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_begin: already armed (gpe_monitor_end first)");
    GPE_TRY(need_particles(c));
    if (cfg->frames > (1ull << 40) / sizeof(gpe_measures))             // (far past any device)
        return fail(c, GPE_ERR_OOM, "gpe_monitor_begin: the ring does not fit in device memory");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_TRY(monitor_reserve(c, "gpe_monitor_begin"));
    // written one whole record at a time, at slot recorded % frames.  no slack
    GPE_TRY(ws_alloc(c, "gpe_monitor_begin: the ring", &m.ring, cfg->frames, 0, "monitor.ring", "does not fit in device memory"));
    m.armed = true;
    m.every = cfg->every; m.frames = cfg->frames; m.rest_speed = cfg->rest_speed;
    m.steps_seen = m.recorded = m.held = 0;
    return GPE_OK;
}

gpe_status gpe_monitor_sample(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!c->monitor.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_sample: not armed (gpe_monitor_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    return monitor_take_frame(c);
}

gpe_status gpe_monitor_read(gpe_ctx *c, gpe_monitor_frames *out)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!out || out->struct_size < sizeof(gpe_monitor_frames))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_read: NULL out or bad struct_size");
    MonitorState &m = c->monitor;
    if (!m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_read: not armed (gpe_monitor_begin)");
    if (out->flags & ~(uint32_t)GPE_MONITOR_CONSUME) return fail(c, GPE_ERR_INVALID_ARG, "gpe_monitor_read: unknown flag");
    GPE_HIP(c, hipSetDevice(c->device));
    const uint64_t want = out->frames ? std::min(m.held, out->capacity) : 0, first = m.recorded - want;
    // records first .. recorded - 1 lie in at most two runs of ring slots
    for (uint64_t done = 0; done < want;) {
        const uint64_t slot = (first + done) % m.frames, run = std::min(want - done, m.frames - slot);
        GPE_HIP(c, hipMemcpyAsync(out->frames + done, m.ring + slot, run * sizeof(gpe_measures), hipMemcpyDeviceToHost, c->stream));
        done += run;
    }
    GPE_HIP(c, hipStreamSynchronize(c->stream));
    out->count = m.held;
    out->recorded = m.recorded;
    if (out->flags & GPE_MONITOR_CONSUME) m.held = 0;
    return check_device_errors(c);
}

gpe_status gpe_monitor_end(gpe_ctx *c)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    MonitorState &m = c->monitor;
    if (!m.armed) return fail(c, GPE_ERR_STATE, "gpe_monitor_end: not armed (gpe_monitor_begin)");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (frames in flight still write the ring)
    dev_free(c, m.ring);
    uint8_t *keep = m.partials;                                        // gpe_measure goes on using the scratch
    m = MonitorState();
    m.partials = keep;
    return GPE_OK;
}

// ---- both, as gpe_api.hip sees them ----------------------------------------------------------------------------
// After every step of gpe_step / gpe_run: an armed recorder counts the step and takes a frame after every every-th.
gpe_status gpe::observers_after_step(gpe_ctx *c)
{
    TracerState &t = c->tracers;
    MonitorState &m = c->monitor;
    if (t.armed && ++t.steps_seen % t.every == 0) GPE_TRY(tracers_take_frame(c));
    return m.armed && ++m.steps_seen % m.every == 0 ? monitor_take_frame(c) : GPE_OK;
}

void gpe::observers_release(gpe_ctx *c)
{
    tracers_release(c);
    monitor_release(c);
}
