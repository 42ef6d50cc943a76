// gpe_movers.hip -- the moving colliders of a context (gpe_set_movers and the rest): the set, the poses on the device
// and the three enqueues behind every step -- a memset of the lookup grid, k_movers_build (advance, pose, list) and
// k_movers_pass (k_movers.hip).  Nothing in a step synchronises or asks the host for more than the grid's view
// (mover_grid.h: host arithmetic on the world and the radius bound).  gpe_api.hip calls movers_check_dt before a step
// launches anything, movers_after_step from after_step, and movers_release from gpe_destroy.  The movers' sweep
// (gpe_set_mover_sweep, at the end of this file) is a mode of the same three enqueues: while it is on, the build and the
// pass are k_mover_sweep.hip's.
#include <math.h>
#include <string.h>

#include "gpe_internal.h"
#include "mover_grid.h"

using namespace gpe;               // (the entry points take their C linkage from their declarations in include/gpe.h)

static_assert(sizeof(gpe_mover) == 56, "gpe_mover is 56 bytes");
static_assert(sizeof(gpe_mover_pose) == 24, "gpe_mover_pose is 24 bytes");
static_assert(sizeof(gpe_movers_info) == 48, "gpe_movers_info is 48 bytes");
static_assert(sizeof(MoverDef) == 3 * sizeof(float4), "a mover's definition is three float4");
static_assert(kMoverLinear == GPE_MOVER_LINEAR && kMoverRotate == GPE_MOVER_ROTATE && kMoversMax == GPE_MOVERS_MAX,
              "k_mover.h restates the constants of include/gpe.h");

constexpr uint64_t kMoverGridMaxCells = (uint64_t)kMoverGridMaxDim * kMoverGridMaxDim;

// the grid buffer for `cells` cells of `words` mask words: the masks, the summary, then `listed` on an 8-byte boundary
static uint64_t grid_listed_offset(uint64_t cells, uint32_t words)
{
    return (cells * (8ull * words + 4ull) + 7ull) & ~7ull;
}

static void movers_buffers_free(gpe_ctx *c, MoverState &S)
{
    dev_free(c, S.def); dev_free(c, S.pose); dev_free(c, S.rec); dev_free(c, S.pushed); dev_free(c, S.grid);
    dev_free(c, S.surf); dev_free(c, S.old);                           // (a new set gets new surfaces)
    S.surfaces.clear();
}

void gpe::movers_release(gpe_ctx *c)
{
    movers_buffers_free(c, c->movers);
    c->movers = MoverState();
}

gpe_status gpe::refuse_movers(gpe_ctx *c, const char *who)
{
    return refuse_holds(c, who, "moving colliders", "gpe_set_movers");
}

gpe_status gpe::movers_check_dt(gpe_ctx *c, float dt, const char *who)
{
    if (!has_movers(c)) return GPE_OK;
    const char *why = mover_dt_refusal(c->movers.limits, dt);
    return why ? fail(c, GPE_ERR_INVALID_ARG, std::string(who) + ": " + why) : GPE_OK;
}

// memset, build, pass: enqueues only.  The view is chosen now, for the world and the radius bound as they are
static gpe_status movers_pass(gpe_ctx *c, float dt)
{
    MoverState &S = c->movers;
    if (S.set.empty() || c->n == 0 || !c->pos) return GPE_OK;
    MoverSweepState &M = c->mover_sweep;
    const bool swept = M.mode == GPE_SWEEP_ON;                         // the swept build and pass (k_mover_sweep.hip)
    if (swept && (!c->prev || !M.counts || !M.carry || !M.old))
        return fail(c, GPE_ERR_STATE, "the swept movers' pass: no previous positions, counters or records");
    const uint32_t k = (uint32_t)S.set.size();
    const MoverGridView g = mover_grid_choose(c->max_radius, c->cfg.world_width, c->cfg.world_height);
    const uint64_t cells = (uint64_t)g.view.gx * g.view.gy;            // <= kMoverGridMaxCells: what S.grid was sized for
    const uint64_t at_listed = grid_listed_offset(cells, S.words);
    Scope s(c, "Movers");
    GPE_HIP(c, hipMemsetAsync(S.grid, 0, at_listed + 8, c->stream));
    MoverBuildArgs B;
    B.def = S.def; B.pose = S.pose; B.rec = S.rec;
    B.old = S.surf ? S.old : nullptr;
    B.k = k; B.words = S.words;
    B.g = g;
    B.rb = g.view.rb; B.dt = dt;
    B.masks = reinterpret_cast<unsigned long long *>(S.grid);
    B.summary = reinterpret_cast<uint32_t *>(S.grid + cells * 8ull * S.words);
    B.listed = reinterpret_cast<unsigned long long *>(S.grid + at_listed);
    MoverSweepArgs W;
    if (swept) {                                                       // old also without surfaces, the carry records, the motion's cells
        B.old = M.old;
        W.carry = M.carry; W.prev = c->prev; W.counts = M.counts;
        GPE_TRY(launch_movers_sweep_build(c, B, W));
    } else {
        GPE_TRY(launch_movers_build(c, B));
    }
    S.view = g;
    S.built = true;
    MoverPassArgs P;
    P.masks = B.masks; P.summary = B.summary; P.rec = S.rec;
    P.k = k; P.words = S.words;
    P.view = g.view;
    P.world_w = c->cfg.world_width; P.world_h = c->cfg.world_height;
    P.pushed = S.pushed;
    if (S.surf) {
        P.surf = S.surf; P.old = S.old; P.prev = c->prev;
    }
    if (swept) {
        P.old = M.old;
        P.prev = nullptr;
        GPE_TRY(launch_movers_sweep(c, c->pos, c->radius, c->n, P, W));
        M.passes += 1;
    } else {
        GPE_TRY(launch_movers_pass(c, c->pos, c->radius, c->n, P));
    }
    S.passes += 1;
    return GPE_OK;
}

gpe_status gpe::movers_after_step(gpe_ctx *c, float dt)
{
    return movers_pass(c, dt);                                        // (after_step has looked: the set is not empty)
}

// the poses of the states q (2 per mover) as the device holds them: 6 floats per mover, and the pass's records
static void movers_pose_all(const std::vector<MoverDef> &def, const float *q, size_t q_stride, std::vector<float> &pose,
                            std::vector<float4> &rec)
{
    const size_t k = def.size();
    pose.resize(6 * k);
    rec.resize(2 * k);
    for (size_t j = 0; j < k; ++j) {
        const float q0 = q[j * q_stride], q1 = q[j * q_stride + 1];
        mover_pose(def[j], q0, q1, &pose[6 * j]);
        pose[6 * j + 4] = q0; pose[6 * j + 5] = q1;
        rec[2 * j] = make_float4(pose[6 * j], pose[6 * j + 1], pose[6 * j + 2], pose[6 * j + 3]);
        rec[2 * j + 1] = make_float4(def[j].radius, 0.f, 0.f, 0.f);
    }
}

gpe_status gpe_set_movers(gpe_ctx *c, const gpe_mover *movers, uint64_t k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (k > 0 && !movers) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_movers: NULL movers");
    if (k > GPE_MOVERS_MAX) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_movers: k must be at most GPE_MOVERS_MAX");
    std::vector<gpe_mover> set(movers, movers + k);
    std::vector<MoverDef> def(k);
    MoverState N;                                                      // the new set, beside the old one until it is whole
    for (uint64_t j = 0; j < k; ++j) {
        const char *why = mover_refusal(set[j]);
        if (why) return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_movers: ") + why);
        def[j] = mover_define(set[j]);
        set[j].radius = def[j].radius;                                 // -0.0 -> +0
        mover_limits_add(N.limits, def[j]);
    }
    if (is_sharded(c)) return refuse_sharded(c, "gpe_set_movers");
    GPE_HIP(c, hipSetDevice(c->device));
    GPE_HIP(c, hipStreamSynchronize(c->stream));                       // (a pass in flight reads the old set)
    MoverState &S = c->movers;
    if (k == 0) {
        movers_release(c);
        return GPE_OK;
    }
    std::vector<float> fresh(2 * k), pose;
    std::vector<float4> rec;
    for (uint64_t j = 0; j < k; ++j) {
        const bool lin = set[j].kind == GPE_MOVER_LINEAR;
        fresh[2 * j] = lin ? 0.0f : 1.0f;
        fresh[2 * j + 1] = lin ? 1.0f : 0.0f;
    }
    movers_pose_all(def, fresh.data(), 2, pose, rec);
    N.words = mover_mask_words((uint32_t)k);
    // the new tables beside the old ones (set_upload.h).  Read by index: def below k, pose below 6 k, rec below 2 k; the
    // grid below the bytes of the largest view (every view mover_grid_choose returns has at most kMoverGridMaxDim cells
    // per axis).  no slack
    HipSetUpload up({c}, "gpe_set_movers");
    up.reserve(&N.def, k, "grid.mover_def");
    up.reserve(&N.pose, 6 * k, "grid.mover_pose");
    up.reserve(&N.rec, 2 * k, "grid.mover_rec");
    up.reserve(&N.pushed, 1, "grid.mover_pushed");
    up.reserve(&N.grid, grid_listed_offset(kMoverGridMaxCells, N.words) + 8, "grid.mover_masks");
    up.copy(N.def, def.data(), k);
    up.copy(N.pose, pose.data(), pose.size());
    up.copy(N.rec, rec.data(), rec.size());
    up.fill(N.pushed, 0, sizeof(unsigned long long));
    GPE_TRY(up.finish());
    movers_buffers_free(c, S);
    N.set.swap(set);
    S = N;
    return GPE_OK;
}

gpe_status gpe_get_movers(const gpe_ctx *c, gpe_mover *out, uint64_t capacity, uint64_t *k)
{
    if (!c || !k || (capacity > 0 && !out)) return GPE_ERR_INVALID_ARG;
    return rows_out(c->movers.set, out, capacity, k);
}

gpe_status gpe_get_mover_poses(gpe_ctx *c, gpe_mover_pose *out, uint64_t capacity, uint64_t *k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!k || (capacity > 0 && !out)) return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_mover_poses: NULL k, or NULL out with a capacity");
    MoverState &S = c->movers;
    *k = S.set.size();
    const uint64_t m = std::min<uint64_t>(S.set.size(), capacity);
    if (m == 0) return GPE_OK;
    GPE_HIP(c, hipSetDevice(c->device));
    return read_back(c, S.pose, out, m * sizeof(gpe_mover_pose));
}

gpe_status gpe_set_mover_poses(gpe_ctx *c, const gpe_mover_pose *poses, uint64_t k)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    MoverState &S = c->movers;
    if (k != S.set.size()) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_mover_poses: k must be the number of movers set");
    if (k == 0) return GPE_OK;
    if (!poses) return fail(c, GPE_ERR_INVALID_ARG, "gpe_set_mover_poses: NULL poses");
    std::vector<MoverDef> def(k);
    for (uint64_t j = 0; j < k; ++j) {
        const char *why = mover_state_refusal(S.set[j], poses[j].q0, poses[j].q1);
        if (why) return fail(c, GPE_ERR_INVALID_ARG, std::string("gpe_set_mover_poses: ") + why);
        def[j] = mover_define(S.set[j]);
    }
    std::vector<float> pose;
    std::vector<float4> rec;
    movers_pose_all(def, &poses[0].q0, sizeof(gpe_mover_pose) / sizeof(float), pose, rec);
    GPE_HIP(c, hipSetDevice(c->device));
    hipError_t e = hipMemcpyAsync(S.pose, pose.data(), pose.size() * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(S.rec, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    const hipError_t waited = hipStreamSynchronize(c->stream);         // always: the host vectors go away on return
    GPE_HIP(c, e);
    GPE_HIP(c, waited);
    return GPE_OK;
}

gpe_status gpe_apply_movers(gpe_ctx *c, float dt)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!has_movers(c) || c->n == 0) return GPE_OK;
    GPE_TRY(movers_check_dt(c, dt, "gpe_apply_movers"));
    GPE_HIP(c, hipSetDevice(c->device));
    return movers_pass(c, dt);
}

gpe_status gpe_get_movers_info(gpe_ctx *c, gpe_movers_info *info)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    if (!info || info->struct_size < sizeof(gpe_movers_info))
        return fail(c, GPE_ERR_INVALID_ARG, "gpe_get_movers_info: NULL info or bad struct_size");
    MoverState &S = c->movers;
    gpe_movers_info out;
    memset(&out, 0, sizeof(out));
    out.struct_size = info->struct_size;
    out.k = (uint32_t)S.set.size();
    out.passes = S.passes;
    if (has_movers(c)) {
        GPE_HIP(c, hipSetDevice(c->device));
        out.mask_words = S.words;
        unsigned long long pushed = 0, listed = 0;
        if (S.built) {                                                 // (no grid yet: no pass has built one)
            const uint64_t at = grid_listed_offset((uint64_t)S.view.view.gx * S.view.view.gy, S.words);
            GPE_HIP(c, hipMemcpyAsync(&listed, S.grid + at, sizeof(listed), hipMemcpyDeviceToHost, c->stream));
            out.grid_x = S.view.view.gx; out.grid_y = S.view.view.gy;
        }
        GPE_TRY(read_back(c, S.pushed, &pushed, sizeof(pushed)));
        out.pushed = pushed;
        out.listed = listed;
    }
    *info = out;
    return GPE_OK;
}

// ---- the sweep of the movers: a mode of the pass above and its two counters ---------------------------------------------
void gpe::mover_sweep_release(gpe_ctx *c)
{
    MoverSweepState &M = c->mover_sweep;
    dev_free(c, M.counts); dev_free(c, M.carry); dev_free(c, M.old);
    M = MoverSweepState();
}

gpe_status gpe_set_mover_sweep(gpe_ctx *c, uint32_t mode)
{
    if (!c) return GPE_ERR_INVALID_ARG;
    // carry and old: one row per mover, written and read below the set's size <= kMoversMax.  no slack.  A new set needs
    // no new ones
    MoverSweepState &M = c->mover_sweep;
    return sweep_mode_set(c, "gpe_set_mover_sweep", M, mode, "grid.msweep_counts",
                          {{(void **)&M.carry, kMoversMax * sizeof(MoverCarry), "grid.msweep_carry"},
                           {(void **)&M.old, kMoversMax * sizeof(float4), "grid.msweep_old"}});
}

gpe_status gpe_get_mover_sweep(const gpe_ctx *c, uint32_t *mode)
{
    if (!c || !mode) return GPE_ERR_INVALID_ARG;
    *mode = c->mover_sweep.mode;
    return GPE_OK;
}

gpe_status gpe_get_mover_sweep_info(gpe_ctx *c, gpe_sweep_info *info)
{
    return c ? sweep_mode_info(c, "gpe_get_mover_sweep_info", c->mover_sweep, info) : GPE_ERR_INVALID_ARG;
}
