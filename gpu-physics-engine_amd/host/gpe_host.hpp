// gpe_host.hpp -- C++ host side above the C-ABI (include/gpe.h), mirroring the reference's Rust module API.
//
// The reference's host is Rust (no toolchain in this image), so the compiled-language mirror is C++: same type and
// method names, same argument meaning and the same error behaviour (the reference unwrap()s / panics -- here every
// failing gpe_status throws gpe::Error with gpe_last_error()).  tests/cpp/reference_tests.cpp restates the reference's
// five integration test files on top of it.  Citations: /root/reference/src.
//
//   WgpuContext::new_for_test  -> gpe::Context          renderer/wgpu_context.rs:73-101 (device + queue == HIP stream)
//   GpuBuffer<T>               -> gpe::GpuBuffer<T>     utils/gpu_buffer.rs:7-29   (device buffer + host mirror)
//   ParticleSystem             -> gpe::ParticleSystem   particles/particle_system.rs:16-24
//   Grid                       -> gpe::Grid             grid/grid.rs:24-33
//   CollisionSystem            -> gpe::CollisionSystem  physics/collision_system.rs:9-12
//   GPUSorter / PushConstants  -> gpe::GPUSorter        utils/radix_sort/radix_sort.rs:44-58
//   PrefixSum                  -> gpe::PrefixSum        utils/prefix_sum/prefix_sum.rs:11-18
//   State                      -> gpe::State            state.rs:21-31 (update() == gpe_step)
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gpe.h"

namespace gpe {

struct Vec2 { float x, y; };                       // glam::Vec2
inline bool operator==(const Vec2 &a, const Vec2 &b) { return a.x == b.x && a.y == b.y; }

constexpr uint32_t UNUSED_CELL_ID = GPE_UNUSED_CELL_ID;            // grid.rs:22
constexpr uint32_t MAX_CELLS_PER_OBJECT = GPE_MAX_CELLS_PER_OBJECT;  // grid.rs:18
constexpr uint32_t NUM_BLOCKS_PER_WORKGROUP = 45;                   // radix_sort.rs:40
constexpr uint32_t RADIX_SORT_BUCKETS = 256;                        // radix_sort.rs:30
constexpr uint32_t WORKGROUP_SIZE = 256;                            // radix_sort.rs:21

class Error : public std::runtime_error {
   public:
    Error(gpe_status s, const std::string &m) : std::runtime_error("gpe status " + std::to_string(s) + ": " + m), status(s) {}
    gpe_status status;
};

class Context {
   public:
    explicit Context(Vec2 world = {1920.0f, 1080.0f}, uint32_t mode = GPE_MODE_COMPAT)
    {
        gpe_config cfg;
        check(gpe_config_default(&cfg), nullptr);
        cfg.world_width = world.x;
        cfg.world_height = world.y;
        cfg.mode = mode;
        check(gpe_create(&cfg, &ctx_), nullptr);
    }
    ~Context() { if (ctx_) gpe_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    gpe_ctx *raw() const { return ctx_; }
    void call(gpe_status s) const { check(s, ctx_); }
    // the step constants the context holds, however they were set
    Vec2 world() const { Vec2 w{}; call(gpe_world(ctx_, &w.x, &w.y)); return w; }
    Vec2 gravity() const { Vec2 g{}; call(gpe_gravity(ctx_, &g.x, &g.y)); return g; }
    bool mouse(Vec2 *at) const
    {
        int32_t pressed = 0;
        Vec2 p{};
        call(gpe_mouse(ctx_, &pressed, &p.x, &p.y));
        if (at) *at = p;
        return pressed != 0;
    }
    static void check(gpe_status s, const gpe_ctx *c)
    {
        if (s != GPE_OK) throw Error(s, gpe_last_error(c));
    }
    template <typename T>
    std::vector<T> download(gpe_array what) const
    {
        uint64_t bytes = 0;
        call(gpe_array_bytes(ctx_, what, &bytes));
        std::vector<T> out(bytes / sizeof(T));
        call(gpe_download(ctx_, what, out.data(), bytes));
        return out;
    }

   private:
    gpe_ctx *ctx_ = nullptr;
};

// utils/gpu_buffer.rs:7-29 : a device buffer plus its host mirror (`data()`); download() refreshes the mirror.  Like the
// reference's, the device buffer grows by doubling (gpu_buffer.rs:54-76) and keeps its DEVICE contents when it does.
template <typename T>
class GpuBuffer {
   public:
    GpuBuffer(const Context &ctx, std::vector<T> data) : ctx_(&ctx), data_(std::move(data))
    {
        cap_bytes_ = std::max<size_t>(1, data_.size() * sizeof(T));
        ctx_->call(gpe_buffer_alloc(ctx_->raw(), cap_bytes_, &dptr_));
        ctx_->call(gpe_buffer_upload(ctx_->raw(), dptr_, data_.data(), data_.size() * sizeof(T)));
    }
    ~GpuBuffer() { if (dptr_) gpe_buffer_free(ctx_->raw(), dptr_); }
    GpuBuffer(const GpuBuffer &) = delete;
    GpuBuffer &operator=(const GpuBuffer &) = delete;
    GpuBuffer(GpuBuffer &&o) noexcept : ctx_(o.ctx_), data_(std::move(o.data_)), dptr_(o.dptr_), cap_bytes_(o.cap_bytes_) { o.dptr_ = nullptr; }
    size_t len() const { return data_.size(); }
    const std::vector<T> &data() const { return data_; }
    size_t capacity_bytes() const { return cap_bytes_; }
    T *device() const { return static_cast<T *>(dptr_); }
    const std::vector<T> &download()                                   // gpu_buffer.rs:96-175
    {
        ctx_->call(gpe_buffer_download(ctx_->raw(), dptr_, data_.data(), data_.size() * sizeof(T)));
        return data_;
    }
    // gpu_buffer.rs:177-262: the last element as the DEVICE holds it; false for an empty buffer.  The mirror stays.
    bool download_last(T *out) const
    {
        if (data_.empty()) return false;
        ctx_->call(gpe_buffer_download(ctx_->raw(), device() + (data_.size() - 1), out, sizeof(T)));
        return true;
    }
    void push(const T &value) { append(&value, 1); }                   // gpu_buffer.rs:30-33
    void push_all(const std::vector<T> &values) { append(values.data(), values.size()); }   // gpu_buffer.rs:35-38
    void replace_elem(const T &new_data, size_t index)                 // gpu_buffer.rs:264-275 (the reference panics)
    {
        if (index >= data_.size()) throw std::out_of_range("Index out of bounds");
        data_[index] = new_data;
        ctx_->call(gpe_buffer_upload(ctx_->raw(), device() + index, &new_data, sizeof(T)));
    }

   private:
    // gpu_buffer.rs:49-87 (`upload`): a buffer that is too small is replaced by one of twice the needed size, the old
    // device contents are carried over (buffer-to-buffer copy there; through the host here: the C-ABI has no
    // device-to-device copy and this is off the step path), then only the new tail is written
    void append(const T *values, size_t count)
    {
        const size_t old_n = data_.size(), need = (old_n + count) * sizeof(T);
        if (need > cap_bytes_) {
            std::vector<T> kept(old_n);
            ctx_->call(gpe_buffer_download(ctx_->raw(), dptr_, kept.data(), old_n * sizeof(T)));
            void *fresh = nullptr;
            const size_t cap = 2 * std::max<size_t>(need, 1);
            ctx_->call(gpe_buffer_alloc(ctx_->raw(), cap, &fresh));
            ctx_->call(gpe_buffer_upload(ctx_->raw(), fresh, kept.data(), old_n * sizeof(T)));
            ctx_->call(gpe_buffer_free(ctx_->raw(), dptr_));
            dptr_ = fresh;
            cap_bytes_ = cap;
        }
        data_.insert(data_.end(), values, values + count);
        ctx_->call(gpe_buffer_upload(ctx_->raw(), device() + old_n, values, count * sizeof(T)));
    }
    const Context *ctx_;
    std::vector<T> data_;
    void *dptr_ = nullptr;
    size_t cap_bytes_ = 0;
};

// particles/particle_buffers.rs:4-10 (host copies as downloaded)
struct ParticleBuffers {
    std::vector<Vec2> current_positions, previous_positions;
    std::vector<float> radii;
    std::vector<uint32_t> home_cell_ids;
};

class ParticleSystem {
   public:
    // particle_system.rs:49-99 (previous = current; max_radius = the radius of largest magnitude)
    static ParticleSystem new_from_buffers(const Context &ctx, const std::vector<Vec2> &positions,
                                           const std::vector<float> &radii)
    {
        if (positions.size() != radii.size()) throw std::invalid_argument("positions and radii differ in length");
        ctx.call(gpe_set_particles(ctx.raw(), &positions[0].x, nullptr, radii.data(), positions.size()));
        return ParticleSystem(ctx);
    }
    void add_particles(const std::vector<Vec2> &positions, const std::vector<float> &radii)   // :163-220
    {
        ctx_->call(gpe_add_particles(ctx_->raw(), &positions[0].x, radii.data(), positions.size()));
    }
    // not in the reference: of the candidates, append those that have room (include/gpe.h, gpe_add_particles_free) --
    // not touching a particle; with GPE_SPAWN_INSIDE_WORLD inside the world by their radius; with GPE_SPAWN_SEPARATE not
    // touching an earlier accepted candidate either.  GPE_SPAWN_DRY_RUN decides without appending.  Returns the number
    // accepted; verdict (may be NULL) receives one GPE_SPAWN_* per candidate, in input order.
    uint64_t add_particles_free(const std::vector<Vec2> &positions, const std::vector<float> &radii, uint32_t flags = 0,
                                std::vector<uint8_t> *verdict = nullptr)
    {
        if (positions.size() != radii.size()) throw std::invalid_argument("positions and radii differ in length");
        if (verdict) verdict->assign(radii.size(), 0);
        gpe_particle_spawn sp{};
        sp.struct_size = sizeof(gpe_particle_spawn);
        sp.flags = flags;
        sp.k = radii.size();
        if (sp.k) {                                                          // (k == 0: the arrays are not read)
            sp.pos_xy = &positions[0].x;
            sp.radius = radii.data();
            sp.verdict = verdict ? verdict->data() : nullptr;
        }
        ctx_->call(gpe_add_particles_free(ctx_->raw(), &sp));
        return sp.added;
    }
    // not in the reference: remove every particle i with remove[i] != 0 (storage order, len() entries) / every particle
    // whose centre lies in the disc around `center`; the survivors keep their order.  Returns the number removed.
    uint64_t remove_particles(const std::vector<uint8_t> &remove)
    {
        uint64_t removed = 0;
        ctx_->call(gpe_remove_particles(ctx_->raw(), remove.data(), remove.size(), &removed));
        return removed;
    }
    uint64_t remove_particles_in_circle(Vec2 center, float radius)
    {
        uint64_t removed = 0;
        ctx_->call(gpe_remove_particles_in_circle(ctx_->raw(), center.x, center.y, radius, &removed));
        return removed;
    }
    // not in the reference: opt-in particle uids that survive re-sorts, removal and growth (include/gpe.h)
    void enable_uids(bool on = true) { ctx_->call(gpe_enable_uids(ctx_->raw(), on ? 1 : 0)); }
    std::vector<uint32_t> uids() const { return ctx_->download<uint32_t>(GPE_UIDS); }        // storage order
    void set_uids(const std::vector<uint32_t> &uids)
    {
        ctx_->call(gpe_set_uids(ctx_->raw(), uids.data(), uids.size()));
    }
    uint64_t next_uid() const { uint64_t n = 0; ctx_->call(gpe_next_uid(ctx_->raw(), &n)); return n; }
    void set_next_uid(uint64_t next) { ctx_->call(gpe_set_next_uid(ctx_->raw(), next)); }
    // index[i] = storage index of uids[i] or GPE_UID_ABSENT; pos / prev / radius its bits (NaN when absent)
    struct UidLookup {
        std::vector<uint32_t> index;
        std::vector<Vec2> pos, prev;
        std::vector<float> radius;
    };
    UidLookup find_uids(const std::vector<uint32_t> &uids) const
    {
        UidLookup r;
        r.index.resize(uids.size());
        r.pos.resize(uids.size());
        r.prev.resize(uids.size());
        r.radius.resize(uids.size());
        const uint32_t none = 0;
        ctx_->call(gpe_find_uids(ctx_->raw(), uids.empty() ? &none : uids.data(), uids.size(), r.index.data(),
                                 reinterpret_cast<float *>(r.pos.data()), reinterpret_cast<float *>(r.prev.data()),
                                 r.radius.data()));
        return r;
    }
    uint64_t remove_particles_by_uid(const std::vector<uint32_t> &uids)
    {
        uint64_t removed = 0;
        const uint32_t none = 0;
        ctx_->call(gpe_remove_particles_by_uid(ctx_->raw(), uids.empty() ? &none : uids.data(), uids.size(), &removed));
        return removed;
    }
    // not in the reference: the path of k particles named by uid, recorded on the device while the steps go on
    // (include/gpe.h): a frame after every every-th step into a ring of `frames` frames, no synchronisation until
    // tracers_read.  Row j of a frame belongs to uids[j]; NaN / GPE_UID_ABSENT while no such particle exists.
    struct TracerFrames {
        uint64_t k = 0;                          // rows per frame
        std::vector<uint64_t> step;              // per frame: steps since tracers_begin
        std::vector<Vec2> pos, prev;             // count * k rows, oldest frame first; prev / index empty unless recorded
        std::vector<uint32_t> index;
        uint64_t recorded = 0;                   // frames taken since tracers_begin
    };
    void tracers_begin(const std::vector<uint32_t> &uids, uint64_t every = 1, uint64_t frames = 1024, bool prev = false,
                       bool index = false)
    {
        gpe_tracer_config cfg{};
        cfg.struct_size = sizeof(cfg);
        cfg.fields = GPE_TRACER_POS | (prev ? GPE_TRACER_PREV : 0u) | (index ? GPE_TRACER_INDEX : 0u);
        cfg.k = uids.size();
        cfg.uids = uids.data();
        cfg.every = every;
        cfg.frames = frames;
        ctx_->call(gpe_tracers_begin(ctx_->raw(), &cfg));
        tracers_k_ = uids.size();
        tracers_fields_ = cfg.fields;
    }
    void tracers_sample() { ctx_->call(gpe_tracers_sample(ctx_->raw())); }
    TracerFrames tracers_read(bool consume = false)
    {
        gpe_tracer_frames f{};
        f.struct_size = sizeof(f);
        ctx_->call(gpe_tracers_read(ctx_->raw(), &f));          // every array NULL: the count
        TracerFrames r;
        r.k = tracers_k_;
        const size_t rows = f.count * tracers_k_;
        r.step.resize(f.count);
        r.pos.resize(rows);
        r.prev.resize(tracers_fields_ & GPE_TRACER_PREV ? rows : 0);
        r.index.resize(tracers_fields_ & GPE_TRACER_INDEX ? rows : 0);
        f.flags = consume ? GPE_TRACERS_CONSUME : 0u;
        f.capacity = f.count;
        f.step = r.step.data();
        f.pos_xy = rows ? &r.pos[0].x : nullptr;
        f.prev_xy = r.prev.empty() ? nullptr : &r.prev[0].x;
        f.index = r.index.empty() ? nullptr : r.index.data();
        ctx_->call(gpe_tracers_read(ctx_->raw(), &f));
        r.recorded = f.recorded;
        return r;
    }
    void tracers_end() { ctx_->call(gpe_tracers_end(ctx_->raw())); tracers_k_ = 0; tracers_fields_ = 0; }
    // not in the reference: scalars of the whole system -- motion, extent, health -- from a full-pass reduction on the
    // device (include/gpe.h): one gpe_measures record now, or one per frame into a ring while the steps go on, with no
    // synchronisation until monitor_read.
    struct MonitorFrames {
        std::vector<gpe_measures> records;       // the records the ring holds, oldest first
        uint64_t recorded = 0;                   // records taken since monitor_begin
    };
    gpe_measures measure(float rest_speed = 0.f) const
    {
        gpe_measures m{};
        ctx_->call(gpe_measure(ctx_->raw(), rest_speed, &m));
        return m;
    }
    void monitor_begin(uint64_t every = 1, uint64_t frames = 1024, float rest_speed = 0.f)
    {
        gpe_monitor_config cfg{};
        cfg.struct_size = sizeof(cfg);
        cfg.every = every;
        cfg.frames = frames;
        cfg.rest_speed = rest_speed;
        ctx_->call(gpe_monitor_begin(ctx_->raw(), &cfg));
    }
    void monitor_sample() { ctx_->call(gpe_monitor_sample(ctx_->raw())); }
    MonitorFrames monitor_read(bool consume = false)
    {
        gpe_monitor_frames f{};
        f.struct_size = sizeof(f);
        ctx_->call(gpe_monitor_read(ctx_->raw(), &f));          // frames NULL: the count
        MonitorFrames r;
        r.records.resize(f.count);
        f.flags = consume ? GPE_MONITOR_CONSUME : 0u;
        f.capacity = f.count;
        f.frames = r.records.empty() ? nullptr : r.records.data();
        ctx_->call(gpe_monitor_read(ctx_->raw(), &f));
        r.recorded = f.recorded;
        return r;
    }
    void monitor_end() { ctx_->call(gpe_monitor_end(ctx_->raw())); }
    // not in the reference: static capsules the particles cannot enter (include/gpe.h), applied on the device after
    // every step of gpe_step / gpe_run, before the tracers and the monitor.  Step state: a snapshot keeps them.
    void set_colliders(const std::vector<gpe_collider> &capsules)
    {
        ctx_->call(gpe_set_colliders(ctx_->raw(), capsules.empty() ? nullptr : capsules.data(), capsules.size()));
    }
    std::vector<gpe_collider> colliders() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_colliders(ctx_->raw(), nullptr, 0, &k));
        std::vector<gpe_collider> out(k);
        ctx_->call(gpe_get_colliders(ctx_->raw(), out.empty() ? nullptr : out.data(), k, &k));
        return out;
    }
    void clear_colliders() { ctx_->call(gpe_set_colliders(ctx_->raw(), nullptr, 0)); }
    void apply_colliders() { ctx_->call(gpe_apply_colliders(ctx_->raw())); }   // one pass now: the hook of the per-module calls
    gpe_colliders_info colliders_info() const
    {
        gpe_colliders_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_colliders_info(ctx_->raw(), &info));
        return info;
    }
    // the sweep: the static colliders' pass judges the path prev -> pos of the step, so a thin wall is not tunnelled
    // through (csrc/k_sweep.h).  A mode of the pass: it outlives set_colliders / set_surfaces; a snapshot keeps it.
    void set_collider_sweep(bool on) { ctx_->call(gpe_set_collider_sweep(ctx_->raw(), on ? GPE_SWEEP_ON : GPE_SWEEP_OFF)); }
    bool collider_sweep() const
    {
        uint32_t mode = GPE_SWEEP_OFF;
        ctx_->call(gpe_get_collider_sweep(ctx_->raw(), &mode));
        return mode == GPE_SWEEP_ON;
    }
    gpe_sweep_info sweep_info() const
    {
        gpe_sweep_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_sweep_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: distance bonds between particles named by uid, or from a particle to a fixed point
    // (include/gpe.h), relaxed on the device after every step of gpe_step / gpe_run, before the static colliders.
    // Step state: a snapshot keeps the set and the broken flags (a broken bond is given back with GPE_BOND_BROKEN).
    void set_bonds(const std::vector<gpe_bond> &bonds, uint32_t iterations = 1)
    {
        ctx_->call(gpe_set_bonds(ctx_->raw(), bonds.empty() ? nullptr : bonds.data(), bonds.size(), iterations));
    }
    struct Bonds {
        std::vector<gpe_bond> records;
        std::vector<uint8_t> broken;
    };
    Bonds bonds() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_bonds(ctx_->raw(), nullptr, nullptr, 0, &k));
        Bonds out;
        out.records.resize(k);
        out.broken.resize(k);
        ctx_->call(gpe_get_bonds(ctx_->raw(), k ? out.records.data() : nullptr, k ? out.broken.data() : nullptr, k, &k));
        return out;
    }
    void clear_bonds() { ctx_->call(gpe_set_bonds(ctx_->raw(), nullptr, 0, 1)); }
    void apply_bonds() { ctx_->call(gpe_apply_bonds(ctx_->raw())); }   // one pass now: the hook of the per-module calls
    gpe_bonds_info bonds_info() const
    {
        gpe_bonds_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_bonds_info(ctx_->raw(), &info));
        return info;
    }
    // the bonds' solver: Jacobi (the default) or graph-coloured Gauss-Seidel, which holds stiff ropes and cloth at
    // stiffness 1.  Step state, independent of set_bonds: it outlives it.
    void set_bond_solver(bool coloured)
    {
        ctx_->call(gpe_set_bond_solver(ctx_->raw(), coloured ? GPE_BOND_SOLVER_COLOURED : GPE_BOND_SOLVER_JACOBI));
    }
    bool bond_solver_coloured() const
    {
        uint32_t mode = GPE_BOND_SOLVER_JACOBI;
        ctx_->call(gpe_get_bond_solver(ctx_->raw(), &mode));
        return mode == GPE_BOND_SOLVER_COLOURED;
    }
    gpe_bond_solver_info bond_solver_info() const
    {
        gpe_bond_solver_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_bond_solver_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: bend constraints (include/gpe.h): the angle at a hinge particle between two others, all named
    // by uid, held at a rest angle given as (rest_cos, rest_sin); relaxed on the device after every step of gpe_step /
    // gpe_run, in front of the bonds.  Step state: a snapshot keeps the set and its relaxation count.
    void set_bends(const std::vector<gpe_bend> &bends, uint32_t iterations = 1)
    {
        ctx_->call(gpe_set_bends(ctx_->raw(), bends.empty() ? nullptr : bends.data(), bends.size(), iterations));
    }
    std::vector<gpe_bend> bends() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_bends(ctx_->raw(), nullptr, 0, &k));
        std::vector<gpe_bend> out(k);
        ctx_->call(gpe_get_bends(ctx_->raw(), k ? out.data() : nullptr, k, &k));
        return out;
    }
    void clear_bends() { ctx_->call(gpe_set_bends(ctx_->raw(), nullptr, 0, 1)); }
    void apply_bends() { ctx_->call(gpe_apply_bends(ctx_->raw())); }   // one pass now: before apply_bonds
    gpe_bends_info bends_info() const
    {
        gpe_bends_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_bends_info(ctx_->raw(), &info));
        return info;
    }
    // the bends' solver: Jacobi (the default) or graph-coloured Gauss-Seidel, which holds short stiff pieces (grass,
    // hinges, folds) at stiffness 1; no gain on long chains.  Step state, independent of set_bends: it outlives it.
    void set_bend_solver(bool coloured)
    {
        ctx_->call(gpe_set_bend_solver(ctx_->raw(), coloured ? GPE_BEND_SOLVER_COLOURED : GPE_BEND_SOLVER_JACOBI));
    }
    bool bend_solver_coloured() const
    {
        uint32_t mode = GPE_BEND_SOLVER_JACOBI;
        ctx_->call(gpe_get_bend_solver(ctx_->raw(), &mode));
        return mode == GPE_BEND_SOLVER_COLOURED;
    }
    gpe_bend_solver_info bend_solver_info() const
    {
        gpe_bend_solver_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_bend_solver_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: area constraints (include/gpe.h): closed loops of particles named by uid, in order around a
    // polygon, that keep a signed rest area; relaxed on the device after every step of gpe_step / gpe_run, behind the
    // bends and in front of the bonds.  Step state: a snapshot keeps the set, its members and its relaxation count.
    void set_areas(const std::vector<gpe_area> &areas, const std::vector<uint32_t> &member_uid, uint32_t iterations = 1)
    {
        ctx_->call(gpe_set_areas(ctx_->raw(), areas.empty() ? nullptr : areas.data(), areas.size(),
                                 member_uid.empty() ? nullptr : member_uid.data(), member_uid.size(), iterations));
    }
    std::pair<std::vector<gpe_area>, std::vector<uint32_t>> areas() const
    {
        uint64_t k = 0, m = 0;
        ctx_->call(gpe_get_areas(ctx_->raw(), nullptr, 0, &k, nullptr, 0, &m));
        std::vector<gpe_area> out(k);
        std::vector<uint32_t> uid(m);
        ctx_->call(gpe_get_areas(ctx_->raw(), k ? out.data() : nullptr, k, &k, m ? uid.data() : nullptr, m, &m));
        return {out, uid};
    }
    void clear_areas() { ctx_->call(gpe_set_areas(ctx_->raw(), nullptr, 0, nullptr, 0, 1)); }
    void apply_areas() { ctx_->call(gpe_apply_areas(ctx_->raw())); }   // one pass now: behind apply_bends, before apply_bonds
    gpe_areas_info areas_info() const
    {
        gpe_areas_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_areas_info(ctx_->raw(), &info));
        return info;
    }
    std::vector<float> area_values() const                              // (area, lambda) per loop; blocks like a download
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_area_values(ctx_->raw(), nullptr, 0, &k));
        std::vector<float> out(2 * k);
        ctx_->call(gpe_get_area_values(ctx_->raw(), k ? out.data() : nullptr, k, &k));
        return out;
    }
    void set_area_targets(uint64_t first, const std::vector<float> &rest_area)   // the pump
    {
        ctx_->call(gpe_set_area_targets(ctx_->raw(), first, rest_area.size(), rest_area.empty() ? nullptr : rest_area.data()));
    }
    // not in the reference: rigid and soft bodies (include/gpe.h): groups of particles named by uid that keep their rest
    // shape, matched on the device after every step of gpe_step / gpe_run, behind the bonds and before the static
    // colliders.  Step state: a snapshot keeps the set, its members and the broken flags (a broken body is given back
    // with GPE_BODY_BROKEN).
    void set_bodies(const std::vector<gpe_body> &bodies, const std::vector<uint32_t> &member_uid,
                    const std::vector<float> &member_rest_xy)
    {
        if (member_rest_xy.size() != 2 * member_uid.size())
            throw std::invalid_argument("set_bodies: member_rest_xy must hold two coordinates per member uid");
        ctx_->call(gpe_set_bodies(ctx_->raw(), bodies.empty() ? nullptr : bodies.data(), bodies.size(),
                                  member_uid.empty() ? nullptr : member_uid.data(),
                                  member_rest_xy.empty() ? nullptr : member_rest_xy.data(), member_uid.size()));
    }
    struct Bodies {
        std::vector<gpe_body> records;
        std::vector<uint8_t> broken;
        std::vector<uint32_t> member_uid;
        std::vector<float> member_rest_xy;
    };
    Bodies bodies() const
    {
        uint64_t k = 0, m = 0;
        ctx_->call(gpe_get_bodies(ctx_->raw(), nullptr, nullptr, 0, &k, nullptr, nullptr, 0, &m));
        Bodies out;
        out.records.resize(k);
        out.broken.resize(k);
        out.member_uid.resize(m);
        out.member_rest_xy.resize(2 * m);
        ctx_->call(gpe_get_bodies(ctx_->raw(), k ? out.records.data() : nullptr, k ? out.broken.data() : nullptr, k, &k,
                                  m ? out.member_uid.data() : nullptr, m ? out.member_rest_xy.data() : nullptr, m, &m));
        return out;
    }
    // one body per group of uids, the particles' current positions captured as the rest shape
    Bodies bodies_from_groups(const std::vector<std::vector<uint32_t>> &uid_groups, float stiffness = 1.0f,
                              float break_distance = 0.0f)
    {
        Bodies out;
        for (const std::vector<uint32_t> &g : uid_groups) {
            gpe_body b{};
            b.first = (uint32_t)out.member_uid.size();
            b.count = (uint32_t)g.size();
            b.stiffness = stiffness;
            b.break_distance = break_distance;
            out.records.push_back(b);
            out.member_uid.insert(out.member_uid.end(), g.begin(), g.end());
        }
        out.broken.assign(out.records.size(), 0);
        out.member_rest_xy.resize(2 * out.member_uid.size());
        std::vector<uint32_t> index(out.member_uid.size());
        if (!out.member_uid.empty())
            ctx_->call(gpe_find_uids(ctx_->raw(), out.member_uid.data(), out.member_uid.size(), index.data(),
                                     out.member_rest_xy.data(), nullptr, nullptr));
        for (uint32_t i : index)
            if (i == GPE_UID_ABSENT) throw std::invalid_argument("bodies_from_groups: a uid names no live particle");
        return out;
    }
    void clear_bodies() { ctx_->call(gpe_set_bodies(ctx_->raw(), nullptr, 0, nullptr, nullptr, 0)); }
    void apply_bodies() { ctx_->call(gpe_apply_bodies(ctx_->raw())); }   // one pass now: the hook of the per-module calls
    std::vector<float> body_poses() const                                 // (cx, cy, cos, sin) per body, as of the last pass
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_body_poses(ctx_->raw(), nullptr, 0, &k));
        std::vector<float> out(4 * k);
        if (k) ctx_->call(gpe_get_body_poses(ctx_->raw(), out.data(), k, &k));
        return out;
    }
    gpe_bodies_info bodies_info() const
    {
        gpe_bodies_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_bodies_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: force fields (include/gpe.h) -- regions that push the particles whose centre lies in them: a
    // uniform acceleration, a pull toward a pole, a swirl around one, a drag.  Applied to prev on the device after every
    // step of update() / run(), behind the colliders and before the tracers and the monitor.  Step state: a snapshot
    // keeps the set.
    void set_fields(const std::vector<gpe_field> &fields)
    {
        ctx_->call(gpe_set_fields(ctx_->raw(), fields.empty() ? nullptr : fields.data(), fields.size()));
    }
    std::vector<gpe_field> fields() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_fields(ctx_->raw(), nullptr, 0, &k));
        std::vector<gpe_field> out(k);
        ctx_->call(gpe_get_fields(ctx_->raw(), out.empty() ? nullptr : out.data(), k, &k));
        return out;
    }
    void clear_fields() { ctx_->call(gpe_set_fields(ctx_->raw(), nullptr, 0)); }
    void apply_fields(float dt) { ctx_->call(gpe_apply_fields(ctx_->raw(), dt)); }   // one pass now: the hook of the per-module calls
    gpe_fields_info fields_info() const
    {
        gpe_fields_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_fields_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: moving colliders (include/gpe.h) -- capsules with a motion: a piston slides (back and forth
    // or for ever), a rotor turns about a pivot.  Advanced, listed and applied on the device after every step of
    // update() / run(), behind the bodies and before the static colliders.  Step state: a snapshot keeps the set and
    // the poses (movers(), mover_poses() -> set_movers, set_mover_poses).
    void set_movers(const std::vector<gpe_mover> &movers)
    {
        ctx_->call(gpe_set_movers(ctx_->raw(), movers.empty() ? nullptr : movers.data(), movers.size()));
    }
    std::vector<gpe_mover> movers() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_movers(ctx_->raw(), nullptr, 0, &k));
        std::vector<gpe_mover> out(k);
        ctx_->call(gpe_get_movers(ctx_->raw(), out.empty() ? nullptr : out.data(), k, &k));
        return out;
    }
    void clear_movers() { ctx_->call(gpe_set_movers(ctx_->raw(), nullptr, 0)); }
    void apply_movers(float dt) { ctx_->call(gpe_apply_movers(ctx_->raw(), dt)); }   // advance + one pass now: the hook of the per-module calls
    std::vector<gpe_mover_pose> mover_poses() const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_mover_poses(ctx_->raw(), nullptr, 0, &k));
        std::vector<gpe_mover_pose> out(k);
        ctx_->call(gpe_get_mover_poses(ctx_->raw(), out.empty() ? nullptr : out.data(), k, &k));
        return out;
    }
    void set_mover_poses(const std::vector<gpe_mover_pose> &poses)
    {
        ctx_->call(gpe_set_mover_poses(ctx_->raw(), poses.empty() ? nullptr : poses.data(), poses.size()));
    }
    gpe_movers_info movers_info() const
    {
        gpe_movers_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_movers_info(ctx_->raw(), &info));
        return info;
    }
    // the movers' sweep: the pass judges every particle by its path relative to each mover over the step, so a thin
    // piston or an R = 0 blade does not jump across particles (csrc/k_mover_sweep.h).  A mode of the pass, independent
    // of set_collider_sweep: it outlives set_movers / set_surfaces / set_mover_poses.
    void set_mover_sweep(bool on) { ctx_->call(gpe_set_mover_sweep(ctx_->raw(), on ? GPE_SWEEP_ON : GPE_SWEEP_OFF)); }
    bool mover_sweep() const
    {
        uint32_t mode = GPE_SWEEP_OFF;
        ctx_->call(gpe_get_mover_sweep(ctx_->raw(), &mode));
        return mode == GPE_SWEEP_ON;
    }
    gpe_sweep_info mover_sweep_info() const
    {
        gpe_sweep_info info{};
        info.struct_size = sizeof(info);
        ctx_->call(gpe_get_mover_sweep_info(ctx_->raw(), &info));
        return info;
    }
    // not in the reference: surface materials (include/gpe.h) -- bounce and friction, one row per static collider
    // (GPE_SURFACES_OF_COLLIDERS) or per mover (GPE_SURFACES_OF_MOVERS) of the set held now.  While a set holds surfaces
    // its pass also rewrites prev for the particles an obstacle touches.  set_colliders / set_movers drop their
    // target's surfaces.  Step state: a snapshot keeps surfaces(target) and restores it after the set and the poses.
    void set_surfaces(uint32_t target, const std::vector<gpe_surface> &rows)
    {
        ctx_->call(gpe_set_surfaces(ctx_->raw(), target, rows.empty() ? nullptr : rows.data(), rows.size()));
    }
    std::vector<gpe_surface> surfaces(uint32_t target) const
    {
        uint64_t k = 0;
        ctx_->call(gpe_get_surfaces(ctx_->raw(), target, nullptr, 0, &k));
        std::vector<gpe_surface> out(k);
        ctx_->call(gpe_get_surfaces(ctx_->raw(), target, out.empty() ? nullptr : out.data(), k, &k));
        return out;
    }
    void clear_surfaces(uint32_t target) { ctx_->call(gpe_set_surfaces(ctx_->raw(), target, nullptr, 0)); }
    // not in the reference: every particle in a circle / box, or the one under a point (include/gpe.h), ascending
    // storage index; uid stays empty while uids are off.  pick() returns no rows when no disc contains the point.
    struct QueryResult {
        std::vector<uint32_t> index, uid;
        std::vector<Vec2> pos, prev;
        std::vector<float> radius;
    };
    QueryResult query_circle(Vec2 center, float radius) const
    {
        return query([&](gpe_query_result *r) { return gpe_query_circle(ctx_->raw(), center.x, center.y, radius, r); });
    }
    QueryResult query_box(Vec2 lo, Vec2 hi) const
    {
        return query([&](gpe_query_result *r) { return gpe_query_box(ctx_->raw(), lo.x, lo.y, hi.x, hi.y, r); });
    }
    QueryResult pick(Vec2 point) const
    {
        return query([&](gpe_query_result *r) { return gpe_pick(ctx_->raw(), point.x, point.y, r); }, 1);
    }
    uint64_t count_circle(Vec2 center, float radius) const
    {
        gpe_query_result r = empty_query();
        ctx_->call(gpe_query_circle(ctx_->raw(), center.x, center.y, radius, &r));
        return r.count;
    }
    uint64_t count_box(Vec2 lo, Vec2 hi) const
    {
        gpe_query_result r = empty_query();
        ctx_->call(gpe_query_box(ctx_->raw(), lo.x, lo.y, hi.x, hi.y, &r));
        return r.count;
    }
    // not in the reference: which particles touch -- dx*dx + dy*dy < (ri + rj)^2 in binary32 -- and how many neighbours
    // each one has (include/gpe.h), searched on the device.  contacts(): the pairs (a < b), ascending by a then b, at most
    // `capacity` of them (0: all, after one counting call); uid_a / uid_b stay empty while uids are off.
    struct ContactResult {
        std::vector<uint32_t> a, b, uid_a, uid_b;
        std::vector<float> overlap;
    };
    ContactResult contacts(uint64_t capacity = 0) const
    {
        uint64_t next = 0;
        const bool with_uids = gpe_next_uid(ctx_->raw(), &next) == GPE_OK;
        const uint64_t cap = capacity ? capacity : count_contacts();
        const uint64_t room = std::max<uint64_t>(cap, 1);
        ContactResult q;
        q.a.resize(room);
        q.b.resize(room);
        q.uid_a.resize(with_uids ? room : 0);
        q.uid_b.resize(with_uids ? room : 0);
        q.overlap.resize(room);
        gpe_contact_result r = empty_contacts();
        r.capacity = cap;
        r.index_a = q.a.data();
        r.index_b = q.b.data();
        r.uid_a = with_uids ? q.uid_a.data() : nullptr;
        r.uid_b = with_uids ? q.uid_b.data() : nullptr;
        r.overlap = q.overlap.data();
        ctx_->call(gpe_query_contacts(ctx_->raw(), &r));
        const uint64_t k = std::min<uint64_t>(r.count, cap);
        q.a.resize(k);
        q.b.resize(k);
        q.uid_a.resize(with_uids ? k : 0);
        q.uid_b.resize(with_uids ? k : 0);
        q.overlap.resize(k);
        return q;
    }
    uint64_t count_contacts() const
    {
        gpe_contact_result r = empty_contacts();
        ctx_->call(gpe_query_contacts(ctx_->raw(), &r));
        return r.count;
    }
    std::vector<uint32_t> contact_degrees() const
    {
        std::vector<uint32_t> degree(len());
        uint32_t none = 0;
        gpe_contact_result r = empty_contacts();
        r.degree = degree.empty() ? &none : degree.data();
        ctx_->call(gpe_query_contacts(ctx_->raw(), &r));
        return degree;
    }
    // not in the reference: which particles make up one clump -- the connected components of the contact graph
    // (include/gpe.h), labelled on the device.  clusters(): per particle the lowest storage index of its cluster, that
    // cluster's size and, while uids are on, the uid of particle label[i]; cluster_of(): the rows of the cluster that holds
    // the particle `key` names (a storage index, or a uid with by_uid), ascending storage index -- none for an unknown uid.
    struct ClusterResult {
        std::vector<uint32_t> label, size, label_uid;
        uint64_t count = 0;
        uint32_t largest_size = 0, largest_label = 0;
    };
    ClusterResult clusters() const
    {
        uint64_t next = 0;
        const bool with_uids = gpe_next_uid(ctx_->raw(), &next) == GPE_OK;
        const size_t n = len();
        uint32_t none = 0;
        ClusterResult q;
        q.label.resize(n);
        q.size.resize(n);
        q.label_uid.resize(with_uids ? n : 0);
        gpe_cluster_result r = empty_clusters();
        r.label = n ? q.label.data() : &none;
        r.size = n ? q.size.data() : &none;
        r.label_uid = with_uids ? (n ? q.label_uid.data() : &none) : nullptr;
        ctx_->call(gpe_query_clusters(ctx_->raw(), &r));
        q.count = r.count;
        q.largest_size = r.largest_size;
        q.largest_label = r.largest_label;
        return q;
    }
    uint64_t count_clusters() const
    {
        gpe_cluster_result r = empty_clusters();
        ctx_->call(gpe_query_clusters(ctx_->raw(), &r));
        return r.count;
    }
    QueryResult cluster_of(uint32_t key, bool by_uid = false) const
    {
        const uint32_t kind = by_uid ? GPE_CLUSTER_BY_UID : GPE_CLUSTER_BY_INDEX;
        return query([&](gpe_query_result *r) { return gpe_query_cluster_of(ctx_->raw(), kind, key, r); });
    }
    // not in the reference: what each ray from origins[i] to ends[i] touches first, and everything one segment crosses
    // (include/gpe.h), on the device.  cast_rays(): one row per ray -- index GPE_RAY_MISS, uid GPE_UID_ABSENT and NaN for a
    // miss; uid only with with_uids (uids must be on), pos / radius only with rows.
    struct RayHits {
        std::vector<uint32_t> index, uid;
        std::vector<float> t, radius;
        std::vector<Vec2> pos;
        uint64_t hits = 0;
    };
    RayHits cast_rays(const std::vector<Vec2> &origins, const std::vector<Vec2> &ends, bool with_uids = false,
                      bool rows = false) const
    {
        if (origins.size() != ends.size()) throw std::invalid_argument("cast_rays: origins and ends differ in length");
        const size_t k = origins.size();
        RayHits q;
        q.index.resize(k);
        q.t.resize(k);
        q.uid.resize(with_uids ? k : 0);
        q.pos.resize(rows ? k : 0);
        q.radius.resize(rows ? k : 0);
        gpe_ray_cast r{};
        r.struct_size = sizeof(r);
        r.k = k;
        r.from_xy = k ? &origins[0].x : nullptr;
        r.to_xy = k ? &ends[0].x : nullptr;
        r.index = k ? q.index.data() : nullptr;
        r.t = k ? q.t.data() : nullptr;
        r.uid = with_uids && k ? q.uid.data() : nullptr;
        r.pos_xy = rows && k ? &q.pos[0].x : nullptr;
        r.radius = rows && k ? q.radius.data() : nullptr;
        ctx_->call(gpe_cast_rays(ctx_->raw(), &r));
        q.hits = r.hits;
        return q;
    }
    // not in the reference: the m particles whose centres are closest to each point (include/gpe.h), searched on the
    // device.  One row of m slots per point, ascending by (d2, index): past count[i] index GPE_NEAREST_NONE, uid
    // GPE_UID_ABSENT and NaN; uid only with with_uids (uids must be on), pos / radius only with rows.  A point on a
    // particle finds it at d2 = 0: for the neighbours of a particle ask for m + 1 and drop the first.
    struct Neighbours {
        uint32_t m = 0;
        std::vector<uint32_t> count, index, uid;
        std::vector<float> dist2, radius;
        std::vector<Vec2> pos;
        uint64_t found = 0;
    };
    Neighbours nearest(const std::vector<Vec2> &points, uint32_t m = 1,
                       float max_distance = std::numeric_limits<float>::infinity(), bool with_uids = false,
                       bool rows = false) const
    {
        if (m == 0 || m > GPE_NEAREST_MAX_M) throw std::invalid_argument("nearest: m must be 1 .. 64");
        const size_t k = points.size(), slots = k * m;
        Neighbours q;
        q.m = m;
        q.count.resize(k);
        q.index.resize(slots);
        q.dist2.resize(slots);
        q.uid.resize(with_uids ? slots : 0);
        q.pos.resize(rows ? slots : 0);
        q.radius.resize(rows ? slots : 0);
        gpe_nearest_query r{};
        r.struct_size = sizeof(r);
        r.k = k;
        r.m = m;
        r.max_distance = max_distance;
        r.point_xy = k ? &points[0].x : nullptr;
        r.count = k ? q.count.data() : nullptr;
        r.index = k ? q.index.data() : nullptr;
        r.dist2 = k ? q.dist2.data() : nullptr;
        r.uid = with_uids && k ? q.uid.data() : nullptr;
        r.pos_xy = rows && k ? &q.pos[0].x : nullptr;
        r.radius = rows && k ? q.radius.data() : nullptr;
        ctx_->call(gpe_query_nearest(ctx_->raw(), &r));
        q.found = r.found;
        return q;
    }
    QueryResult query_segment(Vec2 a, Vec2 b) const
    {
        return query([&](gpe_query_result *r) { return gpe_query_segment(ctx_->raw(), a.x, a.y, b.x, b.y, r); });
    }
    uint64_t count_segment(Vec2 a, Vec2 b) const
    {
        gpe_query_result r = empty_query();
        ctx_->call(gpe_query_segment(ctx_->raw(), a.x, a.y, b.x, b.y, &r));
        return r.count;
    }
    // not in the reference: edit particles in place on the device (include/gpe.h).  The particles named by `keys` --
    // storage indices, or uids with by_uid -- take row i of every array given (NULL: that field stays; positions without
    // previous: at rest, prev = pos).  Unknown uids are skipped.  Returns the number of particles written.
    uint64_t edit_particles(const std::vector<uint32_t> &keys, bool by_uid, const std::vector<Vec2> *positions,
                            const std::vector<Vec2> *previous = nullptr, const std::vector<float> *radii = nullptr)
    {
        if ((positions && positions->size() != keys.size()) || (previous && previous->size() != keys.size()) ||
            (radii && radii->size() != keys.size()))
            throw std::invalid_argument("edit_particles: an array differs from the keys in length");
        const uint32_t none = 0;
        const Vec2 none2{};
        const bool empty = keys.empty();                                     // (k == 0: the arrays are not read)
        gpe_particle_edit e{};
        e.struct_size = sizeof(gpe_particle_edit);
        e.key_kind = by_uid ? GPE_EDIT_BY_UID : GPE_EDIT_BY_INDEX;
        e.k = keys.size();
        e.keys = empty ? &none : keys.data();
        e.pos_xy = positions ? (empty ? &none2.x : &(*positions)[0].x) : nullptr;
        e.prev_xy = previous ? (empty ? &none2.x : &(*previous)[0].x) : nullptr;
        e.radius = radii ? (empty ? &none2.x : radii->data()) : nullptr;
        ctx_->call(gpe_edit_particles(ctx_->raw(), &e));
        return e.edited;
    }
    // ... and kick the velocity pos - prev of every particle query_circle / query_box would return: op GPE_VEL_ADD
    // (prev -= a), GPE_VEL_SET (prev = pos - a) or GPE_VEL_SCALE (prev = pos - (pos - prev) * a), per component.  Returns
    // the number kicked; count = false returns 0 without waiting for the device (stream-ordered, like State::update).
    uint64_t kick_circle(Vec2 center, float radius, uint32_t op, Vec2 a, bool count = true)
    {
        uint64_t kicked = 0;
        ctx_->call(gpe_kick_circle(ctx_->raw(), center.x, center.y, radius, op, a.x, a.y, count ? &kicked : nullptr));
        return kicked;
    }
    uint64_t kick_box(Vec2 lo, Vec2 hi, uint32_t op, Vec2 a, bool count = true)
    {
        uint64_t kicked = 0;
        ctx_->call(gpe_kick_box(ctx_->raw(), lo.x, lo.y, hi.x, hi.y, op, a.x, a.y, count ? &kicked : nullptr));
        return kicked;
    }
    size_t len() const { uint64_t n = 0; ctx_->call(gpe_len(ctx_->raw(), &n)); return n; }               // :275
    float get_max_radius() const { float r = 0; ctx_->call(gpe_max_radius(ctx_->raw(), &r)); return r; } // :291
    void sort_by_cell_id(float /*cell_size: the Grid's, state.rs:123*/) { ctx_->call(gpe_morton_resort(ctx_->raw())); }
    void update_positions(float dt) { ctx_->call(gpe_integrate(ctx_->raw(), dt)); }                      // :245
    void mouse_click_callback(bool pressed, Vec2 p)                                                      // :221-224
    {
        mouse_pressed_ = pressed;
        ctx_->call(gpe_set_mouse(ctx_->raw(), pressed, p.x, p.y));
    }
    void mouse_move_callback(Vec2 p) { ctx_->call(gpe_set_mouse(ctx_->raw(), mouse_pressed_, p.x, p.y)); } // :225-227
    // the reference's wall-clock re-sort policy (SORT_INTERVAL = 4 s, :13-14; the first frame sorts, :45,97)
    bool is_it_time_to_sort() const                                                                      // :229-231
    {
        return !sorted_once_ || std::chrono::steady_clock::now() - last_sort_time_ >= std::chrono::seconds(4);
    }
    void reset_last_sort_time() { last_sort_time_ = std::chrono::steady_clock::now(); sorted_once_ = true; } // :233-235
    std::vector<uint32_t> download_home_cell_ids() const { return ctx_->download<uint32_t>(GPE_HOME_CELL_IDS); }
    std::vector<uint32_t> download_particle_ids() const { return ctx_->download<uint32_t>(GPE_PARTICLE_IDS); }
    ParticleBuffers download_particle_buffers() const                                                    // :258-265
    {
        ParticleBuffers b;
        b.current_positions = ctx_->download<Vec2>(GPE_POS);
        b.previous_positions = ctx_->download<Vec2>(GPE_PREV);
        b.radii = ctx_->download<float>(GPE_RADIUS);
        b.home_cell_ids = ctx_->download<uint32_t>(GPE_HOME_CELL_IDS);
        return b;
    }

   private:
    explicit ParticleSystem(const Context &ctx) : ctx_(&ctx) {}
    static gpe_query_result empty_query()
    {
        gpe_query_result r{};
        r.struct_size = sizeof(gpe_query_result);
        return r;
    }
    static gpe_contact_result empty_contacts()
    {
        gpe_contact_result r{};
        r.struct_size = sizeof(gpe_contact_result);
        return r;
    }
    static gpe_cluster_result empty_clusters()
    {
        gpe_cluster_result r{};
        r.struct_size = sizeof(gpe_cluster_result);
        return r;
    }
    // one call with `capacity` rows, a second with capacity = count only if the first ran over
    template <typename Call>
    QueryResult query(Call call, uint64_t capacity = 1024) const
    {
        uint64_t next = 0;
        const bool with_uids = gpe_next_uid(ctx_->raw(), &next) == GPE_OK;
        QueryResult q;
        for (;;) {
            const uint64_t cap = std::max<uint64_t>(capacity, 1);
            q.index.resize(cap);
            q.uid.resize(with_uids ? cap : 0);
            q.pos.resize(cap);
            q.prev.resize(cap);
            q.radius.resize(cap);
            gpe_query_result r = empty_query();
            r.capacity = cap;
            r.index = q.index.data();
            r.uid = with_uids ? q.uid.data() : nullptr;
            r.pos_xy = &q.pos[0].x;
            r.prev_xy = &q.prev[0].x;
            r.radius = q.radius.data();
            ctx_->call(call(&r));
            if (r.count <= cap) {
                q.index.resize(r.count);
                q.uid.resize(with_uids ? r.count : 0);
                q.pos.resize(r.count);
                q.prev.resize(r.count);
                q.radius.resize(r.count);
                return q;
            }
            capacity = r.count;
        }
    }
    const Context *ctx_;
    uint64_t tracers_k_ = 0;                 // tracers_begin's k and fields: the shape of the frames tracers_read sizes
    uint32_t tracers_fields_ = 0;
    bool mouse_pressed_ = false;
    bool sorted_once_ = false;
    std::chrono::steady_clock::time_point last_sort_time_{};
};

class Grid {
   public:
    // grid.rs:74-149 : cell size from an explicit max radius (tests) ...
    static Grid new_without_camera(const Context &ctx, float max_obj_radius, const ParticleSystem &)
    {
        ctx.call(gpe_grid_set_max_radius(ctx.raw(), max_obj_radius));
        return Grid(ctx);
    }
    // ... or from the particle system's (grid.rs:66-71)
    Grid(const Context &ctx, const ParticleSystem &) : ctx_(&ctx) {}
    static float compute_cell_size(float max_obj_radius) { return gpe_compute_cell_size(max_obj_radius); }   // :159
    float cell_size() const { float cs = 0; ctx_->call(gpe_cell_size(ctx_->raw(), &cs)); return cs; }
    float max_radius() const { float r = 0; ctx_->call(gpe_grid_max_radius(ctx_->raw(), &r)); return r; }   // cell size / 2.2
    void build_cell_ids() { ctx_->call(gpe_grid_build(ctx_->raw())); }        // :296-306
    void sort_map() { ctx_->call(gpe_grid_sort(ctx_->raw())); }               // :310-312
    void update() { ctx_->call(gpe_grid_update(ctx_->raw())); }               // :322-332
    std::vector<uint32_t> download_cell_ids() const { return ctx_->download<uint32_t>(GPE_CELL_IDS); }       // :314
    std::vector<uint32_t> download_object_ids() const { return ctx_->download<uint32_t>(GPE_OBJECT_IDS); }   // :318

   private:
    explicit Grid(const Context &ctx) : ctx_(&ctx) {}
    const Context *ctx_;
};

class CollisionSystem {
   public:
    CollisionSystem(const Context &ctx, uint32_t dim, const ParticleSystem &, const Grid &) : ctx_(&ctx)   // :14-22
    {
        if (dim != 2) throw std::invalid_argument("2-D only (state.rs:18)");
    }
    void solve_collisions() { ctx_->call(gpe_solve_collisions(ctx_->raw())); }                             // :30-39
    std::vector<uint32_t> download_collision_cells() const { return ctx_->download<uint32_t>(GPE_COLLISION_CELLS); }

   private:
    const Context *ctx_;
};

struct PushConstants { uint32_t num_elements, current_shift, num_workgroups, num_blocks_per_workgroup; };   // radix_sort.rs:53-58

class GPUSorter {
   public:
    GPUSorter(const Context &ctx, uint32_t length, GpuBuffer<uint32_t> &keys, GpuBuffer<uint32_t> &payload)  // :61
        : ctx_(&ctx), length_(length), keys_(&keys), payload_(&payload), keys_b_(ctx, std::vector<uint32_t>(length, 0)),
          payload_b_(ctx, std::vector<uint32_t>(length, 0)), histogram_(ctx, std::vector<uint32_t>(RADIX_SORT_BUCKETS, 0))
    {
        if (length == 0) throw std::invalid_argument("NonZeroU32 length");
    }
    void sort(const uint32_t *sort_first_n = nullptr)                                                        // :199-217
    {
        ctx_->call(gpe_sort_pairs_u32(ctx_->raw(), keys_->device(), payload_->device(), sort_first_n ? *sort_first_n : length_));
    }
    void build_histogram(const PushConstants &pc, bool /*ping*/)                                             // :180-188
    {
        ctx_->call(gpe_sort_histogram_u32(ctx_->raw(), keys_->device(), pc.num_elements, pc.current_shift, histogram_.device()));
    }
    void scatter(const PushConstants &pc, bool /*ping*/)                                                     // :190-198
    {
        ctx_->call(gpe_sort_scatter_pass_u32(ctx_->raw(), keys_->device(), payload_->device(), keys_b_.device(),
                                             payload_b_.device(), pc.num_elements, pc.current_shift));
    }
    const std::vector<uint32_t> &get_keys_b() { return keys_b_.download(); }                                 // :219
    const std::vector<uint32_t> &get_histogram() { return histogram_.download(); }                           // :223

   private:
    const Context *ctx_;
    uint32_t length_;
    GpuBuffer<uint32_t> *keys_, *payload_;
    GpuBuffer<uint32_t> keys_b_, payload_b_, histogram_;
};

class PrefixSum {
   public:
    PrefixSum(const Context &ctx, GpuBuffer<uint32_t> &buffer) : ctx_(&ctx), buffer_(&buffer) {}             // :21
    void execute(uint32_t num_items) { ctx_->call(gpe_inclusive_scan_u32(ctx_->raw(), buffer_->device(), num_items)); }  // :143-160
    void update_buffers(GpuBuffer<uint32_t> &buffer) { buffer_ = &buffer; }                                 // :172

   private:
    const Context *ctx_;
    GpuBuffer<uint32_t> *buffer_;
};

// state.rs:21-31 without window / renderer
class State {
   public:
    State(const std::vector<Vec2> &positions, const std::vector<float> &radii, Vec2 world, uint32_t mode = GPE_MODE_NATIVE)
        : ctx_(world, mode), particles_(ParticleSystem::new_from_buffers(ctx_, positions, radii)), grid_(ctx_, particles_),
          collision_system_(ctx_, 2, particles_, grid_) {}
    void update(float dt, bool resort) { ctx_.call(gpe_step(ctx_.raw(), dt, resort ? GPE_STEP_RESORT : 0u)); }   // state.rs:115-131
    // ... with the reference's own wall-clock re-sort policy (state.rs:122-125, particle_system.rs:229-235)
    bool update(float dt)
    {
        const bool resort = particles_.is_it_time_to_sort();
        update(dt, resort);
        if (resort) particles_.reset_last_sort_time();
        return resort;
    }
    gpe_pipeline_info pipeline_info() const
    {
        gpe_pipeline_info info{};
        info.struct_size = sizeof(info);
        ctx_.call(gpe_get_pipeline_info(ctx_.raw(), &info));
        return info;
    }
    ParticleSystem &particles() { return particles_; }
    Grid &grid() { return grid_; }
    CollisionSystem &collision_system() { return collision_system_; }
    const Context &context() const { return ctx_; }

   private:
    Context ctx_;
    ParticleSystem particles_;
    Grid grid_;
    CollisionSystem collision_system_;
};

}  // namespace gpe
