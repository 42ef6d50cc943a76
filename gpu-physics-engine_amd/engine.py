"""Host-side mirror of the reference's module API over the C-ABI (include/gpe.h).

Same names and argument meaning as the Rust types the reference's State::update() and tests use
(citations into /root/reference/src), so the parity tests read like tests/*.rs:

    WgpuContext      -> Context            (renderer/wgpu_context.rs:8; here: one HIP stream)
    GpuBuffer<T>     -> GpuBuffer          (utils/gpu_buffer.rs:7)
    ParticleSystem   -> ParticleSystem     (particles/particle_system.rs:16)
    Grid             -> Grid               (grid/grid.rs:24)
    CollisionSystem  -> CollisionSystem    (physics/collision_system.rs:9)
    GPUSorter        -> GPUSorter          (utils/radix_sort/radix_sort.rs:44)
    PrefixSum        -> PrefixSum          (utils/prefix_sum/prefix_sum.rs:11)
    State            -> State              (state.rs:21; update() == gpe_step)

One Context owns one gpe_ctx, i.e. one particle system + grid + collision system, which is how
State composes them (state.rs:34-70).  Errors surface as GpeError (the reference panics).
numpy is used only to hold host arrays; every call goes through ctypes to libgpe.so.
"""
import ctypes as C
import collections
import sys

import numpy as np

from . import _lib as L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# gpe_query_circle / gpe_query_box / gpe_pick: every match, ascending storage index (uid None while uids are off)
QueryResult = collections.namedtuple("QueryResult", "index uid pos prev radius")
# gpe_query_contacts: the touching pairs (a < b), ascending by a then b (uid_a / uid_b None while uids are off, overlap
# None unless asked for)
ContactResult = collections.namedtuple("ContactResult", "a b uid_a uid_b overlap")
# gpe_query_clusters: per particle the lowest index of its contact cluster, that cluster's size and the uid of particle
# label[i] (None while uids are off); the number of clusters, and the size and label of the largest one
ClusterResult = collections.namedtuple("ClusterResult", "label size label_uid count largest_size largest_label")
# cast_rays: one row per ray; index L.RAY_MISS, uid L.UID_ABSENT and NaN for a miss; uid / pos / radius None unless requested
RayHits = collections.namedtuple("RayHits", "index t uid pos radius hits")
# nearest: one row of m slots per point, ascending by (d2, index); count (k,), index / dist2 / uid / radius (k, m), pos
# (k, m, 2); past count[i] index L.NEAREST_NONE, uid L.UID_ABSENT and NaN; uid / pos / radius None unless requested
Neighbours = collections.namedtuple("Neighbours", "count index dist2 uid pos radius found")
# tracers_read: the frames held in the ring, oldest first; step (count,) u64 = steps since tracers_begin, pos / prev
# (count, k, 2), index (count, k); row j belongs to uids[j], NaN / L.UID_ABSENT while no such particle exists; prev /
# index None unless recorded; recorded = frames taken since begin
TracerFrames = collections.namedtuple("TracerFrames", "step pos prev index recorded")
# measure: one gpe_measures record (include/gpe.h) field for field; monitor_read delivers the same fields as a numpy
# structured array of dtype MEASURES_DTYPE (120 bytes per record, the struct's layout)
MEASURES_DTYPE = np.dtype([(name, {C.c_uint64: np.uint64, C.c_double: np.float64, C.c_float: np.float32,
                                   C.c_uint32: np.uint32}[ctype]) for name, ctype in L.GpeMeasures._fields_])
assert MEASURES_DTYPE.itemsize == C.sizeof(L.GpeMeasures)
Measures = collections.namedtuple("Measures", [name for name, _ in L.GpeMeasures._fields_])
# set_colliders / colliders: the rows of gpe_collider (24 bytes each, the struct's layout)
COLLIDER_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeCollider._fields_])
assert COLLIDER_DTYPE.itemsize == C.sizeof(L.GpeCollider)
# set_bonds / bonds: the rows of gpe_bond (32 bytes each, the struct's layout)
BOND_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeBond._fields_])
assert BOND_DTYPE.itemsize == C.sizeof(L.GpeBond)


def pair_bonds(uid_a, uid_b, rest_length, stiffness=1.0, max_length=0.0):
    """Rows of BOND_DTYPE that tie particle uid_a[i] to particle uid_b[i] (scalars are broadcast)."""
    ua = np.asarray(uid_a, np.uint32).reshape(-1)
    rows = np.zeros(len(ua), BOND_DTYPE)
    rows["uid_a"], rows["uid_b"] = ua, uid_b
    rows["rest_length"], rows["stiffness"], rows["max_length"] = rest_length, stiffness, max_length
    return rows


def anchor_bonds(uids, points, rest_length=0.0, stiffness=1.0, max_length=0.0):
    """Rows of BOND_DTYPE that tie particle uids[i] to the fixed point points[i] (GPE_BOND_ANCHOR)."""
    ua = np.asarray(uids, np.uint32).reshape(-1)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    rows = np.zeros(len(ua), BOND_DTYPE)
    rows["uid_a"], rows["uid_b"], rows["flags"] = ua, L.UID_ABSENT, L.BOND_ANCHOR
    rows["rest_length"], rows["stiffness"], rows["max_length"] = rest_length, stiffness, max_length
    rows["anchor_x"], rows["anchor_y"] = pts[:, 0], pts[:, 1]
    return rows


# set_bends / bends: the rows of gpe_bend (32 bytes each, the struct's layout)
BEND_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeBend._fields_])
assert BEND_DTYPE.itemsize == C.sizeof(L.GpeBend)


def bends_from_angles(uid_a, uid_b, uid_c, angle, stiffness=1.0):
    """Rows of BEND_DTYPE that hold the angle at the hinge uid_b[i] from (uid_a[i] - uid_b[i]) to (uid_c[i] - uid_b[i])
    at angle[i] radians (scalars are broadcast): cos and sin in float64, rounded once to float32."""
    ua = np.asarray(uid_a, np.uint32).reshape(-1)
    rows = np.zeros(len(ua), BEND_DTYPE)
    rows["uid_a"], rows["uid_b"], rows["uid_c"] = ua, uid_b, uid_c
    theta = np.broadcast_to(np.asarray(angle, np.float64), ua.shape)
    rows["rest_cos"], rows["rest_sin"], rows["stiffness"] = np.cos(theta), np.sin(theta), stiffness
    return rows


# set_areas / areas: the rows of gpe_area (24 bytes each, the struct's layout)
AREA_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeArea._fields_])
assert AREA_DTYPE.itemsize == C.sizeof(L.GpeArea)


# set_movers / movers: the rows of gpe_mover (56 bytes each); mover_poses: the rows of gpe_mover_pose (24 bytes each)
MOVER_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeMover._fields_])
MOVER_POSE_DTYPE = np.dtype([(name, np.float32) for name, _ in L.GpeMoverPose._fields_])
assert MOVER_DTYPE.itemsize == C.sizeof(L.GpeMover) == 56 and MOVER_POSE_DTYPE.itemsize == C.sizeof(L.GpeMoverPose) == 24
# set_surfaces / surfaces: the rows of gpe_surface (16 bytes each), one per static collider or per mover
SURFACE_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeSurface._fields_])
assert SURFACE_DTYPE.itemsize == C.sizeof(L.GpeSurface) == 16
SURFACE_TARGETS = {"colliders": L.SURFACES_OF_COLLIDERS, "movers": L.SURFACES_OF_MOVERS}


def surface_rows(k, restitution=0.0, friction=0.0, flags=0):
    """k rows of SURFACE_DTYPE with the same material (each argument may also be an array of k)."""
    rows = np.zeros(k, SURFACE_DTYPE)
    rows["restitution"], rows["friction"], rows["flags"] = restitution, friction, flags
    return rows


# set_bodies / bodies: the rows of gpe_body (24 bytes each, the struct's layout)
# set_fields / fields: the rows of gpe_field (56 bytes each, the struct's layout)
FIELD_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeField._fields_])
assert FIELD_DTYPE.itemsize == C.sizeof(L.GpeField) == 56
BODY_DTYPE = np.dtype([(name, np.uint32 if ctype is C.c_uint32 else np.float32) for name, ctype in L.GpeBody._fields_])
assert BODY_DTYPE.itemsize == C.sizeof(L.GpeBody)


def body_rows(counts, stiffness=1.0, break_distance=0.0):
    """Rows of BODY_DTYPE for bodies of counts[i] members each, laid out one behind the other in the member arrays
    (stiffness and break_distance: scalars, or one value per body)."""
    counts = np.asarray(counts, np.uint32).reshape(-1)
    rows = np.zeros(len(counts), BODY_DTYPE)
    rows["count"] = counts
    rows["first"] = np.cumsum(counts, dtype=np.uint64) - counts
    rows["stiffness"], rows["break_distance"] = stiffness, break_distance
    return rows


class Context:
    """WgpuContext::new_for_test() stand-in (wgpu_context.rs:73-101): device + queue == HIP stream."""

    def __init__(self, world=(3048.0, 1048.0), gravity=(0.0, 0.0), mode=None, device=-1,
                 profiling=False, stream=None, flags=0, guard_words=None):
        self.lib = L.load()
        cfg = L.GpeConfig()
        L.check(self.lib.gpe_config_default(C.byref(cfg)))
        cfg.device = device
        cfg.world_width, cfg.world_height = world
        cfg.gravity_x, cfg.gravity_y = gravity
        if mode is not None:            # default: gpe_config_default's (NATIVE)
            cfg.mode = mode
        cfg.profiling = int(profiling)
        cfg.flags = int(flags)          # L.FLAG_*
        if guard_words is not None:     # (canary, poison) of L.FLAG_GUARD_ALLOCS; default: the library's
            cfg.guard_canary, cfg.guard_poison = guard_words
        h = C.c_void_p()
        L.check(self.lib.gpe_create(C.byref(cfg), C.byref(h)))
        self.h = h
        if stream is not None:          # a hipStream_t the caller owns and keeps alive (gpe_set_stream)
            self.call("gpe_set_stream", C.c_void_p(int(stream)))

    def world(self):
        """gpe_world: the world size the context's wall clamp uses, however it was set."""
        w, h = C.c_float(), C.c_float()
        self.call("gpe_world", C.byref(w), C.byref(h))
        return (w.value, h.value)

    def gravity(self):
        """gpe_gravity: the context's gravity, however it was set."""
        gx, gy = C.c_float(), C.c_float()
        self.call("gpe_gravity", C.byref(gx), C.byref(gy))
        return (gx.value, gy.value)

    def mouse(self):
        """gpe_mouse -> (pressed, (x, y)): the mouse state the next integration uses."""
        pressed, x, y = C.c_int32(), C.c_float(), C.c_float()
        self.call("gpe_mouse", C.byref(pressed), C.byref(x), C.byref(y))
        return (bool(pressed.value), (x.value, y.value))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpe_destroy(self.h)
            self.h = None

    def __del__(self):
        # not during interpreter shutdown: the HIP runtime may already have been torn down by then, and the
        # process is about to release everything anyway
        try:
            if sys is None or sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def call(self, name, *args):
        L.check(getattr(self.lib, name)(self.h, *args), self.h)

    def add_particles_free(self, positions, radii, separate=False, inside_world=False, dry_run=False):
        """gpe_add_particles_free: of the candidates (positions f32[k,2], radii f32[k]) append those with room -- not
        touching a particle of the context, with `inside_world` inside the world by their radius, with `separate` not
        touching an earlier accepted candidate either.  dry_run decides without appending.  Returns (added, verdict):
        the number accepted and u8[k] of L.SPAWN_* per candidate, in input order."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1)
        rad = np.ascontiguousarray(radii, np.float32).reshape(-1)
        k = rad.shape[0]
        if pos.shape[0] != 2 * k:
            raise ValueError("positions and radii differ in length")
        verdict = np.zeros(k, np.uint8)
        flags = (L.SPAWN_SEPARATE if separate else 0) | (L.SPAWN_INSIDE_WORLD if inside_world else 0) | \
            (L.SPAWN_DRY_RUN if dry_run else 0)
        sp = L.GpeParticleSpawn(struct_size=C.sizeof(L.GpeParticleSpawn), flags=flags, k=k)
        if k:
            sp.pos_xy = pos.ctypes.data_as(C.POINTER(C.c_float))
            sp.radius = rad.ctypes.data_as(C.POINTER(C.c_float))
            sp.verdict = verdict.ctypes.data_as(C.POINTER(C.c_uint8))
        self.call("gpe_add_particles_free", C.byref(sp))
        return sp.added, verdict

    def sync(self):
        self.call("gpe_sync")

    def pipeline_info(self):
        """gpe_get_pipeline_info: which kernels the next step runs (L.PIPELINE_*), why (L.REASON_*), and the counts."""
        info = L.GpePipelineInfoUniform()
        info.struct_size = C.sizeof(L.GpePipelineInfoUniform)
        self.call("gpe_get_pipeline_info", C.byref(info))
        return {k: getattr(info, k) for k, _ in L.GpePipelineInfoUniform._fields_ if k not in ("struct_size", "reserved")}

    def guard_check(self):
        """gpe_guard_check: the damaged red zones of the context's device allocations, as dicts (tag, side "front" /
        "rear", first_offset, last_offset, first_word, payload_bytes), those of buffers released since included.  Empty
        without L.FLAG_GUARD_ALLOCS.  Raises nothing by itself; `damaged` zones beyond L.GUARD_MAX_ZONES are only
        counted (self.guard_damaged holds the count of the last call)."""
        rep = L.GpeGuardReport()
        rep.struct_size = C.sizeof(L.GpeGuardReport)
        self.call("gpe_guard_check", C.byref(rep))
        self.guard_damaged, self.guard_allocations = rep.damaged, rep.allocations
        return [{"tag": z.tag.decode(), "side": "rear" if z.side == L.GUARD_REAR else "front",
                 "first_offset": z.first_offset, "last_offset": z.last_offset, "first_word": z.first_word,
                 "payload_bytes": z.payload_bytes} for z in rep.zones[:rep.listed]]

    def guard_registry(self):
        """gpe_guard_registry: [(tag, payload bytes, slack bytes, "live" / "released" / "pinned")] -- the context's live
        device allocations, then the last released one of every tag that has seen a release, then its pinned host blocks
        (one entry per allocation made)."""
        need = C.c_uint64()
        self.call("gpe_guard_registry", None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value)
        self.call("gpe_guard_registry", buf, need.value, None)
        return [(t, int(p), int(s), state) for t, p, s, state in (line.split() for line in buf.value.decode().splitlines())]

    def device_ptr(self, what):
        """gpe_device_ptr: (address, bytes) of a particle / grid array on the device (render hand-off, state.rs:150-176)."""
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        self.call("gpe_device_ptr", what, C.byref(ptr), C.byref(nbytes))
        return ptr, nbytes.value

    def download(self, what, dtype, shape=None):
        nbytes = C.c_uint64()
        self.call("gpe_array_bytes", what, C.byref(nbytes))
        out = np.empty(nbytes.value // np.dtype(dtype).itemsize, dtype)
        self.call("gpe_download", what, _ptr(out), nbytes.value)
        return out.reshape(shape) if shape else out

    def timings(self):
        cnt = C.c_uint32(0)
        self.call("gpe_get_timings", None, C.byref(cnt))
        arr = (L.GpeTiming * max(1, cnt.value))()
        cnt2 = C.c_uint32(cnt.value)
        self.call("gpe_get_timings", arr, C.byref(cnt2))
        return {arr[i].name.decode(): (arr[i].total_ms, arr[i].calls) for i in range(min(cnt.value, cnt2.value))}

    def trace(self):
        """[(scope name, start ms, duration ms)] of the recorded scope instances, oldest first (gpe_get_trace)."""
        cnt = C.c_uint32(0)
        self.call("gpe_get_trace", None, C.byref(cnt))
        arr = (L.GpeTraceEvent * max(1, cnt.value))()
        cnt2 = C.c_uint32(cnt.value)
        self.call("gpe_get_trace", arr, C.byref(cnt2))
        return [(arr[i].name.decode(), arr[i].start_ms, arr[i].duration_ms) for i in range(min(cnt.value, cnt2.value))]

    def write_chrome_trace(self, path):
        """The reference's `benchmark.json` (state.rs:108-112): one complete event ("ph": "X", microseconds) per
        recorded scope, loadable by chrome://tracing / Perfetto."""
        import json
        events = [{"name": n, "cat": "gpu", "ph": "X", "ts": t0 * 1e3, "dur": d * 1e3, "pid": 0, "tid": 0}
                  for n, t0, d in self.trace()]
        with open(path, "w") as f:
            json.dump({"traceEvents": events, "displayTimeUnit": "ms"}, f)
        return len(events)

    def reset_timings(self):
        self.call("gpe_reset_timings")

    def set_profiling(self, on):
        """False/0 off, True/1 every scope, k > 1: the scopes of every k-th step only (sampled)."""
        self.call("gpe_set_profiling", int(on))


class GpuBuffer:
    """utils/gpu_buffer.rs:7-29 for u32 data: device buffer + host mirror (`data()`).  Like the reference's, the device
    buffer grows by doubling (gpu_buffer.rs:54-76) and keeps its DEVICE contents when it does."""

    def __init__(self, ctx, data):
        self.ctx = ctx
        self._data = np.ascontiguousarray(data, dtype=np.uint32).copy()
        self._cap_bytes = max(1, self._data.nbytes)
        self.dptr = C.c_void_p()
        ctx.call("gpe_buffer_alloc", self._cap_bytes, C.byref(self.dptr))
        ctx.call("gpe_buffer_upload", self.dptr, _ptr(self._data), self._data.nbytes)

    def len(self):
        return len(self._data)

    def data(self):
        return self._data

    def capacity_bytes(self):
        return self._cap_bytes

    def _at(self, index):
        return C.c_void_p(self.dptr.value + 4 * int(index))

    def download(self):
        """gpu_buffer.rs:96-175: read the device buffer back into the host mirror."""
        self.ctx.call("gpe_buffer_download", self.dptr, _ptr(self._data), self._data.nbytes)
        return self._data

    def download_last(self):
        """gpu_buffer.rs:177-262: the last element as the DEVICE holds it (None for an empty buffer); the mirror stays."""
        if len(self._data) == 0:
            return None
        out = np.zeros(1, np.uint32)
        self.ctx.call("gpe_buffer_download", self._at(len(self._data) - 1), _ptr(out), 4)
        return int(out[0])

    def _append(self, values):
        # gpu_buffer.rs:49-87 (`upload`): a buffer that is too small is replaced by one of twice the needed size, the old
        # device contents are carried over (buffer-to-buffer copy there; through the host here: the C-ABI has no
        # device-to-device copy and this is off the step path), then only the new tail is written
        values = np.ascontiguousarray(values, np.uint32).reshape(-1)
        old_n = len(self._data)
        need = 4 * (old_n + len(values))
        if need > self._cap_bytes:
            kept = np.zeros(old_n, np.uint32)
            self.ctx.call("gpe_buffer_download", self.dptr, _ptr(kept), kept.nbytes)
            fresh = C.c_void_p()
            self.ctx.call("gpe_buffer_alloc", 2 * max(need, 1), C.byref(fresh))
            self.ctx.call("gpe_buffer_upload", fresh, _ptr(kept), kept.nbytes)
            self.ctx.call("gpe_buffer_free", self.dptr)
            self.dptr, self._cap_bytes = fresh, 2 * max(need, 1)
        self._data = np.concatenate([self._data, values])
        self.ctx.call("gpe_buffer_upload", self._at(old_n), _ptr(values), values.nbytes)

    def push(self, value):
        """gpu_buffer.rs:30-33."""
        self._append([value])

    def push_all(self, values):
        """gpu_buffer.rs:35-38."""
        self._append(values)

    def replace_elem(self, new_data, index):
        """gpu_buffer.rs:264-275: one element of the mirror and of the device buffer."""
        if index < 0 or index >= len(self._data):
            raise IndexError("Index out of bounds")                    # (the reference panics)
        self._data[index] = np.uint32(new_data)
        one = np.array([new_data], np.uint32)
        self.ctx.call("gpe_buffer_upload", self._at(index), _ptr(one), 4)

    def free(self):
        if self.dptr:
            self.ctx.call("gpe_buffer_free", self.dptr)
            self.dptr = C.c_void_p()


class ParticleSystem:
    """particles/particle_system.rs:16-24."""

    SORT_INTERVAL = 4.0      # seconds (particle_system.rs:13-14)

    def __init__(self, ctx):
        import time
        self.ctx = ctx
        self._mouse = (False, (0.0, 0.0))
        self._clock = time.monotonic
        self.last_sort_time = self._clock() - self.SORT_INTERVAL     # :45,97: the first frame sorts

    def is_it_time_to_sort(self):
        """particle_system.rs:229-231 (wall clock, like the reference)."""
        return self._clock() - self.last_sort_time >= self.SORT_INTERVAL

    def reset_last_sort_time(self):
        """particle_system.rs:233-235."""
        self.last_sort_time = self._clock()

    @classmethod
    def new_from_buffers(cls, ctx, positions, radii, prev=None):
        """particle_system.rs:49-99 (the test constructor; prev = cur; integrator world 1920x1080 there --
        here the world is the Context's, set it explicitly to mirror that quirk)."""
        self = cls(ctx)
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 2)
        rad = np.ascontiguousarray(radii, np.float32).reshape(-1)
        if pos.shape[0] != rad.shape[0]:
            raise ValueError("positions and radii differ in length")
        pp = None
        if prev is not None:
            pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
            pp = _ptr(pv)
        ctx.call("gpe_set_particles", _ptr(pos), pp, _ptr(rad), pos.shape[0])
        return self

    def add_particles(self, positions, radii):
        """particle_system.rs:163-220 (the reference draws 100 random ones around the mouse)."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 2)
        rad = np.ascontiguousarray(radii, np.float32).reshape(-1)
        self.ctx.call("gpe_add_particles", _ptr(pos), _ptr(rad), pos.shape[0])

    def add_particles_free(self, positions, radii, separate=False, inside_world=False, dry_run=False):
        """Context.add_particles_free (gpe_add_particles_free, not in the reference) -> (added, verdict)."""
        return self.ctx.add_particles_free(positions, radii, separate=separate, inside_world=inside_world,
                                           dry_run=dry_run)

    def remove_particles(self, mask):
        """gpe_remove_particles (not in the reference): remove every particle i (storage order, as
        download_particle_buffers returns them) with mask[i] true / non-zero; len(mask) must equal len().  The
        survivors keep their order.  Returns the number removed."""
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            m = m.astype(np.uint8)
        m = np.ascontiguousarray(m, np.uint8).reshape(-1)
        removed = C.c_uint64()
        self.ctx.call("gpe_remove_particles", _ptr(m), m.shape[0], C.byref(removed))
        return removed.value

    def remove_particles_in_circle(self, center, radius):
        """gpe_remove_particles_in_circle (not in the reference): remove every particle whose centre p has
        |p - center|^2 <= radius^2 in float32 (an eraser brush).  Returns the number removed."""
        removed = C.c_uint64()
        self.ctx.call("gpe_remove_particles_in_circle", float(center[0]), float(center[1]), float(radius),
                      C.byref(removed))
        return removed.value

    # Particle uids (not in the reference; include/gpe.h): an opt-in u32 per particle that the library carries through
    # every re-sort, removal and growth, so that a host can key its own per-particle data (colours, tracers) by uid.
    def enable_uids(self, on=True):
        """gpe_enable_uids: off -> on gives uid = storage index and next_uid = len(); on -> on keeps them; off drops them."""
        self.ctx.call("gpe_enable_uids", 1 if on else 0)

    def uids(self):
        """The uids in storage order (u32[len()], as download_particle_buffers orders the particles)."""
        return self.ctx.download(L.UIDS, np.uint32)

    def set_uids(self, uids):
        """gpe_set_uids: uids[i] for storage index i, pairwise distinct; next_uid becomes max + 1."""
        u = np.ascontiguousarray(uids, np.uint32).reshape(-1)
        self.ctx.call("gpe_set_uids", _ptr(u), u.shape[0])

    def next_uid(self):
        """The uid the next added particle gets (GpeError GPE_ERR_STATE while uids are off)."""
        n = C.c_uint64()
        self.ctx.call("gpe_next_uid", C.byref(n))
        return n.value

    def set_next_uid(self, next_uid):
        self.ctx.call("gpe_set_next_uid", int(next_uid))

    def find_uids(self, uids):
        """gpe_find_uids -> (index u32[k], pos f32[k,2], prev f32[k,2], radius f32[k]): the particles' current storage
        indices (L.UID_ABSENT for an unknown uid) and their bits (NaN when absent)."""
        q = np.ascontiguousarray(uids, np.uint32).reshape(-1)
        k = q.shape[0]
        index = np.empty(max(k, 1), np.uint32)
        pos = np.empty((max(k, 1), 2), np.float32)
        prev = np.empty((max(k, 1), 2), np.float32)
        rad = np.empty(max(k, 1), np.float32)
        qq = q if k else np.zeros(1, np.uint32)
        self.ctx.call("gpe_find_uids", _ptr(qq), k, _ptr(index), _ptr(pos), _ptr(prev), _ptr(rad))
        return index[:k], pos[:k], prev[:k], rad[:k]

    def remove_particles_by_uid(self, uids):
        """gpe_remove_particles_by_uid: the particles with these uids leave (unknown uids are ignored, duplicates count
        once); otherwise as remove_particles.  Returns the number removed."""
        q = np.ascontiguousarray(uids, np.uint32).reshape(-1)
        qq = q if q.shape[0] else np.zeros(1, np.uint32)
        removed = C.c_uint64()
        self.ctx.call("gpe_remove_particles_by_uid", _ptr(qq), q.shape[0], C.byref(removed))
        return removed.value

    # Tracers (not in the reference; include/gpe.h): the path of k particles named by uid, recorded on the device while
    # update() / run() go on -- a frame after every every-th step into a ring of `frames` frames, no synchronisation until
    # tracers_read.  Nothing a step can see changes.
    def tracers_begin(self, uids, every=1, frames=1024, prev=False, index=False):
        """gpe_tracers_begin: follow the particles with these uids (1 .. L.TRACERS_MAX of them, pairwise distinct; row j of
        every frame belongs to uids[j]).  Positions are always recorded, prev=True / index=True add the previous
        positions / the storage indices.  Needs uids on."""
        u = np.asarray(uids)
        if u.ndim != 1 or u.dtype.kind not in "iu":
            raise ValueError("tracers_begin: uids must be a 1-d integer array, got %s %r" % (u.dtype, u.shape))
        if not 1 <= u.shape[0] <= L.TRACERS_MAX:
            raise ValueError("tracers_begin: 1 .. %d uids, got %d" % (L.TRACERS_MAX, u.shape[0]))
        if int(u.min()) < 0 or int(u.max()) > 0xFFFFFFFF:
            raise ValueError("tracers_begin: a uid is a u32")
        u = np.ascontiguousarray(u, np.uint32)
        if np.unique(u).shape[0] != u.shape[0]:
            raise ValueError("tracers_begin: two tracers share a uid")
        every, frames = int(every), int(frames)
        if every < 1 or frames < 1:
            raise ValueError("tracers_begin: every and frames must be >= 1, got %d and %d" % (every, frames))
        fields = L.TRACER_POS | (L.TRACER_PREV if prev else 0) | (L.TRACER_INDEX if index else 0)
        cfg = L.GpeTracerConfig(struct_size=C.sizeof(L.GpeTracerConfig), fields=fields, k=u.shape[0], every=every,
                                frames=frames)
        cfg.uids = u.ctypes.data_as(C.POINTER(C.c_uint32))
        self.ctx.call("gpe_tracers_begin", C.byref(cfg))
        self._tracers = (u.shape[0], bool(prev), bool(index))

    def tracers_sample(self):
        """gpe_tracers_sample: one frame now, at the current step count (the frame at step 0).  Does not synchronise."""
        self.ctx.call("gpe_tracers_sample")

    def tracers_read(self, consume=False):
        """gpe_tracers_read -> TracerFrames(step, pos, prev, index, recorded): the frames the ring holds, oldest first.
        consume=True empties the ring afterwards.  Blocks like a download."""
        if getattr(self, "_tracers", None) is None:
            raise ValueError("tracers_read: tracers_begin has not been called")
        k, with_prev, with_index = self._tracers
        flags = L.TRACERS_CONSUME if consume else 0
        fr = L.GpeTracerFrames(struct_size=C.sizeof(L.GpeTracerFrames), flags=0, capacity=0)
        self.ctx.call("gpe_tracers_read", C.byref(fr))                 # every array NULL: count only
        count = fr.count
        room = max(count, 1)
        step = np.empty(room, np.uint64)
        pos = np.empty((room, k, 2), np.float32)
        prev = np.empty((room, k, 2), np.float32) if with_prev else None
        index = np.empty((room, k), np.uint32) if with_index else None
        fr = L.GpeTracerFrames(struct_size=C.sizeof(L.GpeTracerFrames), flags=flags, capacity=count)
        fr.step = step.ctypes.data_as(C.POINTER(C.c_uint64))
        fr.pos_xy = pos.ctypes.data_as(C.POINTER(C.c_float))
        if with_prev:
            fr.prev_xy = prev.ctypes.data_as(C.POINTER(C.c_float))
        if with_index:
            fr.index = index.ctypes.data_as(C.POINTER(C.c_uint32))
        self.ctx.call("gpe_tracers_read", C.byref(fr))
        return TracerFrames(step[:count], pos[:count], prev[:count] if with_prev else None,
                            index[:count] if with_index else None, fr.recorded)

    def tracers_end(self):
        """gpe_tracers_end: stop recording and free the ring (frames not read are lost)."""
        self.ctx.call("gpe_tracers_end")
        self._tracers = None

    # Run monitor (not in the reference; include/gpe.h): scalars of the whole system -- motion, extent, health -- from a
    # full-pass reduction on the device: one record now (measure), or one per frame into a ring while update() / run()
    # go on, no synchronisation until monitor_read.  Nothing a step can see changes.
    @staticmethod
    def _rest_speed(who, rest_speed):
        r = float(rest_speed)
        if not r >= 0.0:
            raise ValueError("%s: rest_speed must be >= 0 (or +inf), got %r" % (who, rest_speed))
        return r

    def measure(self, rest_speed=0.0):
        """gpe_measure -> Measures: one record of the particles as they are now (step = 0).  rest_speed: a particle
        counts as moving when its squared displacement per step exceeds rest_speed ** 2.  Blocks like a download."""
        r = self._rest_speed("measure", rest_speed)
        out = L.GpeMeasures()
        self.ctx.call("gpe_measure", C.c_float(r), C.byref(out))
        return Measures(*[getattr(out, name) for name in Measures._fields])

    def monitor_begin(self, every=1, frames=1024, rest_speed=0.0):
        """gpe_monitor_begin: a record after every every-th step into a ring of `frames` records."""
        every, frames = int(every), int(frames)
        if every < 1 or frames < 1:
            raise ValueError("monitor_begin: every and frames must be >= 1, got %d and %d" % (every, frames))
        r = self._rest_speed("monitor_begin", rest_speed)
        cfg = L.GpeMonitorConfig(struct_size=C.sizeof(L.GpeMonitorConfig), flags=0, every=every, frames=frames,
                                 rest_speed=r)
        self.ctx.call("gpe_monitor_begin", C.byref(cfg))

    def monitor_sample(self):
        """gpe_monitor_sample: one record now, at the current step count (the frame at step 0).  Does not synchronise."""
        self.ctx.call("gpe_monitor_sample")

    def monitor_read(self, consume=False):
        """gpe_monitor_read -> (records, recorded): the records the ring holds, oldest first, as a structured array of
        MEASURES_DTYPE, and the number taken since monitor_begin.  consume=True empties the ring afterwards.  Blocks
        like a download."""
        fr = L.GpeMonitorFrames(struct_size=C.sizeof(L.GpeMonitorFrames), flags=0, capacity=0)
        self.ctx.call("gpe_monitor_read", C.byref(fr))                 # frames NULL: count only
        count = fr.count
        records = np.zeros(max(count, 1), MEASURES_DTYPE)
        fr = L.GpeMonitorFrames(struct_size=C.sizeof(L.GpeMonitorFrames), flags=L.MONITOR_CONSUME if consume else 0,
                                capacity=count)
        fr.frames = records.ctypes.data_as(C.POINTER(L.GpeMeasures))
        self.ctx.call("gpe_monitor_read", C.byref(fr))
        return records[:count], fr.recorded

    def monitor_end(self):
        """gpe_monitor_end: stop recording and free the ring (records not read are lost)."""
        self.ctx.call("gpe_monitor_end")

    # Static colliders (not in the reference; include/gpe.h): capsules the particles cannot enter, applied on the device
    # after every update() / step of run(), before the tracers and the monitor.  Step state: save() keeps them.
    def set_colliders(self, capsules):
        """gpe_set_colliders: replace the set by the rows (ax, ay, bx, by, radius) of a (k, 5) float array; k == 0
        clears it."""
        caps = np.ascontiguousarray(capsules, np.float32)
        if caps.size == 0:
            caps = caps.reshape(0, 5)
        if caps.ndim != 2 or caps.shape[1] != 5:
            raise ValueError("set_colliders: capsules must have shape (k, 5), got %r" % (caps.shape,))
        k = len(caps)
        rows = np.zeros(k, COLLIDER_DTYPE)
        for col, name in enumerate(("ax", "ay", "bx", "by", "radius")):
            rows[name] = caps[:, col]
        self.ctx.call("gpe_set_colliders", rows.ctypes.data_as(C.POINTER(L.GpeCollider)) if k else None, k)

    def colliders(self):
        """gpe_get_colliders -> f32[k, 5]: the rows (ax, ay, bx, by, radius) of the set."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_colliders", None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), COLLIDER_DTYPE)
        self.ctx.call("gpe_get_colliders", rows.ctypes.data_as(C.POINTER(L.GpeCollider)), k.value, C.byref(k))
        rows = rows[:k.value]
        return np.stack([rows[name] for name in ("ax", "ay", "bx", "by", "radius")], axis=1).astype(np.float32)

    def clear_colliders(self):
        """gpe_set_colliders with k = 0."""
        self.ctx.call("gpe_set_colliders", None, 0)

    def apply_colliders(self):
        """gpe_apply_colliders: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_colliders")

    def colliders_info(self):
        """gpe_get_colliders_info -> dict(k, passes, pushed, grid_x, grid_y, list_entries).  Blocks like a download."""
        info = L.GpeCollidersInfo(struct_size=C.sizeof(L.GpeCollidersInfo))
        self.ctx.call("gpe_get_colliders_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeCollidersInfo._fields_ if name != "struct_size"}

    def set_collider_sweep(self, on):
        """gpe_set_collider_sweep: on, the static colliders' pass judges every particle by its path prev -> pos of the step
        (csrc/k_sweep.h), so walls thinner than a step's displacement hold.  A mode of the pass: it outlives
        set_colliders and set_surfaces.  Zeroes the sweep's counters; blocks."""
        self.ctx.call("gpe_set_collider_sweep", L.SWEEP_ON if on else L.SWEEP_OFF)

    def collider_sweep(self):
        """gpe_get_collider_sweep -> bool."""
        mode = C.c_uint32(0)
        self.ctx.call("gpe_get_collider_sweep", C.byref(mode))
        return mode.value == L.SWEEP_ON

    def sweep_info(self):
        """gpe_get_sweep_info -> dict(mode, passes, swept, stopped).  Blocks like a download."""
        info = L.GpeSweepInfo(struct_size=C.sizeof(L.GpeSweepInfo))
        self.ctx.call("gpe_get_sweep_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeSweepInfo._fields_ if name != "struct_size"}

    # Moving colliders (not in the reference; include/gpe.h): capsules with a motion -- pistons and rotors -- advanced,
    # listed and applied on the device after every update() / step of run(), behind the bodies and before the static
    # colliders.  Step state: save() keeps the set and the poses.
    def set_movers(self, movers):
        """gpe_set_movers: replace the set by the rows of a MOVER_DTYPE array; no rows clear it.  Every pose starts
        fresh, the counters anew."""
        rows = np.ascontiguousarray(movers, MOVER_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_movers", rows.ctypes.data_as(C.POINTER(L.GpeMover)) if k else None, k)

    def movers(self):
        """gpe_get_movers -> MOVER_DTYPE[k]: the set."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_movers", None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), MOVER_DTYPE)
        self.ctx.call("gpe_get_movers", rows.ctypes.data_as(C.POINTER(L.GpeMover)), k.value, C.byref(k))
        return rows[:k.value]

    def clear_movers(self):
        """gpe_set_movers with k = 0."""
        self.ctx.call("gpe_set_movers", None, 0)

    def apply_movers(self, dt):
        """gpe_apply_movers: advance once and run one pass now (the hook of a host that steps module by module).  Does
        not synchronise."""
        self.ctx.call("gpe_apply_movers", float(dt))

    def mover_poses(self):
        """gpe_get_mover_poses -> MOVER_POSE_DTYPE[k]: the posed capsule and the state of every mover.  Blocks like a
        download."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_mover_poses", None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), MOVER_POSE_DTYPE)
        self.ctx.call("gpe_get_mover_poses", rows.ctypes.data_as(C.POINTER(L.GpeMoverPose)), k.value, C.byref(k))
        return rows[:k.value]

    def set_mover_poses(self, poses):
        """gpe_set_mover_poses: restore the states q0, q1 of a MOVER_POSE_DTYPE array, one row per mover; the capsules are
        recomputed from them."""
        rows = np.ascontiguousarray(poses, MOVER_POSE_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_mover_poses", rows.ctypes.data_as(C.POINTER(L.GpeMoverPose)) if k else None, k)

    def movers_info(self):
        """gpe_get_movers_info -> dict(k, passes, pushed, grid_x, grid_y, mask_words, listed).  Blocks like a download."""
        info = L.GpeMoversInfo(struct_size=C.sizeof(L.GpeMoversInfo))
        self.ctx.call("gpe_get_movers_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeMoversInfo._fields_ if name not in ("struct_size", "reserved")}

    def set_mover_sweep(self, on):
        """gpe_set_mover_sweep: on, the movers' pass judges every particle by its path relative to each mover over the step
        (csrc/k_mover_sweep.h), so a thin piston or blade no longer jumps across particles.  A mode of the pass,
        independent of set_collider_sweep: it outlives set_movers, set_surfaces and set_mover_poses.  Zeroes the mode's
        counters; blocks."""
        self.ctx.call("gpe_set_mover_sweep", L.SWEEP_ON if on else L.SWEEP_OFF)

    def mover_sweep(self):
        """gpe_get_mover_sweep -> bool."""
        mode = C.c_uint32(0)
        self.ctx.call("gpe_get_mover_sweep", C.byref(mode))
        return mode.value == L.SWEEP_ON

    def mover_sweep_info(self):
        """gpe_get_mover_sweep_info -> dict(mode, passes, swept, stopped).  Blocks like a download."""
        info = L.GpeSweepInfo(struct_size=C.sizeof(L.GpeSweepInfo))
        self.ctx.call("gpe_get_mover_sweep_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeSweepInfo._fields_ if name != "struct_size"}

    # Surface materials (not in the reference; include/gpe.h): bounce and friction per static collider or per mover.  While
    # a set holds surfaces its pass also rewrites prev for the particles an obstacle touches.  Step state: save() keeps
    # them; set_colliders / set_movers drop their target's.
    @staticmethod
    def _surface_target(target):
        if target not in SURFACE_TARGETS:
            raise ValueError("target must be 'colliders' or 'movers'")
        return SURFACE_TARGETS[target]

    def set_surfaces(self, target, rows):
        """gpe_set_surfaces: one SURFACE_DTYPE row per collider (target "colliders") or per mover ("movers") of the set
        held now; no rows clear them."""
        t = self._surface_target(target)
        rows = np.ascontiguousarray(rows, SURFACE_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_surfaces", t, rows.ctypes.data_as(C.POINTER(L.GpeSurface)) if k else None, k)

    def surfaces(self, target):
        """gpe_get_surfaces -> SURFACE_DTYPE[k]: the rows of the target's surfaces (k = 0: none)."""
        t = self._surface_target(target)
        k = C.c_uint64()
        self.ctx.call("gpe_get_surfaces", t, None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), SURFACE_DTYPE)
        self.ctx.call("gpe_get_surfaces", t, rows.ctypes.data_as(C.POINTER(L.GpeSurface)), k.value, C.byref(k))
        return rows[:k.value]

    def clear_surfaces(self, target):
        """gpe_set_surfaces with k = 0."""
        self.ctx.call("gpe_set_surfaces", self._surface_target(target), None, 0)

    # Distance bonds (not in the reference; include/gpe.h): particles tied to each other, or to a fixed point, by uid,
    # relaxed on the device after every update() / step of run(), before the colliders.  Step state: save() keeps them.
    def set_bonds(self, bonds, iterations=1):
        """gpe_set_bonds: replace the set by the rows of a BOND_DTYPE array (pair_bonds / anchor_bonds build them),
        relaxed `iterations` times per pass; no rows clear it.  The broken flags and the counters start anew."""
        rows = np.ascontiguousarray(bonds, BOND_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_bonds", rows.ctypes.data_as(C.POINTER(L.GpeBond)) if k else None, k, int(iterations))

    def bonds(self):
        """gpe_get_bonds -> (records BOND_DTYPE[k], broken bool[k])."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_bonds", None, None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), BOND_DTYPE)
        broken = np.zeros(max(k.value, 1), np.uint8)
        self.ctx.call("gpe_get_bonds", rows.ctypes.data_as(C.POINTER(L.GpeBond)),
                      broken.ctypes.data_as(C.POINTER(C.c_uint8)), k.value, C.byref(k))
        return rows[:k.value], broken[:k.value].astype(bool)

    def clear_bonds(self):
        """gpe_set_bonds with k = 0."""
        self.ctx.call("gpe_set_bonds", None, 0, 1)

    def apply_bonds(self):
        """gpe_apply_bonds: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_bonds")

    def bonds_info(self):
        """gpe_get_bonds_info -> dict(iterations, k, nodes, passes, live, broken, resolves).  Blocks like a download."""
        info = L.GpeBondsInfo(struct_size=C.sizeof(L.GpeBondsInfo))
        self.ctx.call("gpe_get_bonds_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeBondsInfo._fields_ if name != "struct_size"}

    def set_bond_solver(self, solver):
        """gpe_set_bond_solver: "jacobi" (the default: every bond judged from the positions a relaxation starts with) or
        "coloured" (graph-coloured Gauss-Seidel: the bonds relaxed colour after colour, every bond seeing the corrections
        of the colours before it -- stiffness 1 is stable, a rope stretches about a quarter as much).  Step state: it
        outlives set_bonds; save() keeps it with the bonds it belongs to (not for a context without bonds).  Synchronises."""
        modes = {"jacobi": L.BOND_SOLVER_JACOBI, "coloured": L.BOND_SOLVER_COLOURED}
        if solver not in modes:
            raise ValueError('the bond solver is "jacobi" or "coloured"')
        self.ctx.call("gpe_set_bond_solver", modes[solver])

    def bond_solver(self):
        """gpe_get_bond_solver -> "jacobi" | "coloured"."""
        mode = C.c_uint32(0)
        self.ctx.call("gpe_get_bond_solver", C.byref(mode))
        return "coloured" if mode.value == L.BOND_SOLVER_COLOURED else "jacobi"

    def bond_solver_info(self):
        """gpe_get_bond_solver_info -> dict(mode, colours, largest_colour, form, lds_nodes_max, passes)."""
        info = L.GpeBondSolverInfo(struct_size=C.sizeof(L.GpeBondSolverInfo))
        self.ctx.call("gpe_get_bond_solver_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeBondSolverInfo._fields_ if name != "struct_size"}

    # Bend constraints (not in the reference; include/gpe.h): the angle at a hinge particle between two others, by uid,
    # relaxed on the device after every update() / step of run(), in front of the bonds.  Step state: save() keeps them.
    def set_bends(self, bends, iterations=1):
        """gpe_set_bends: replace the set by the rows of a BEND_DTYPE array (bends_from_angles / bends_from_positions
        build them), relaxed `iterations` times per pass; no rows clear it.  The counters start anew."""
        rows = np.ascontiguousarray(bends, BEND_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_bends", rows.ctypes.data_as(C.POINTER(L.GpeBend)) if k else None, k, int(iterations))

    def bends(self):
        """gpe_get_bends -> records BEND_DTYPE[k]."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_bends", None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), BEND_DTYPE)
        self.ctx.call("gpe_get_bends", rows.ctypes.data_as(C.POINTER(L.GpeBend)), k.value, C.byref(k))
        return rows[:k.value]

    def clear_bends(self):
        """gpe_set_bends with k = 0."""
        self.ctx.call("gpe_set_bends", None, 0, 1)

    def apply_bends(self):
        """gpe_apply_bends: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_bends")

    def bends_info(self):
        """gpe_get_bends_info -> dict(iterations, k, nodes, passes, resolves)."""
        info = L.GpeBendsInfo(struct_size=C.sizeof(L.GpeBendsInfo))
        self.ctx.call("gpe_get_bends_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeBendsInfo._fields_ if name != "struct_size"}

    def set_bend_solver(self, solver):
        """gpe_set_bend_solver: "jacobi" (the default: every bend judged from the positions a relaxation starts with) or
        "coloured" (graph-coloured Gauss-Seidel: the bends relaxed colour after colour, every bend seeing the corrections
        of the colours before it -- stiffness 1 is stable, a short cantilever droops less than half as far; no gain on
        long chains).  Step state: it outlives set_bends; save() keeps it with the bends it belongs to (not for a
        context without bends).  Synchronises."""
        modes = {"jacobi": L.BEND_SOLVER_JACOBI, "coloured": L.BEND_SOLVER_COLOURED}
        if solver not in modes:
            raise ValueError('the bend solver is "jacobi" or "coloured"')
        self.ctx.call("gpe_set_bend_solver", modes[solver])

    def bend_solver(self):
        """gpe_get_bend_solver -> "jacobi" | "coloured"."""
        mode = C.c_uint32(0)
        self.ctx.call("gpe_get_bend_solver", C.byref(mode))
        return "coloured" if mode.value == L.BEND_SOLVER_COLOURED else "jacobi"

    def bend_solver_info(self):
        """gpe_get_bend_solver_info -> dict(mode, colours, largest_colour, form, lds_nodes_max, passes)."""
        info = L.GpeBendSolverInfo(struct_size=C.sizeof(L.GpeBendSolverInfo))
        self.ctx.call("gpe_get_bend_solver_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeBendSolverInfo._fields_ if name != "struct_size"}

    # Area constraints (not in the reference; include/gpe.h): closed loops of particles, named by uid in order around a
    # polygon, that keep a signed rest area; relaxed on the device after every update() / step of run(), behind the bends
    # and in front of the bonds.  Step state: save() keeps them.
    def set_areas(self, areas, member_uid, iterations=1):
        """gpe_set_areas: replace the set by the rows of an AREA_DTYPE array (State.areas_from_loops builds them) over
        the members' uids u32[m], relaxed `iterations` times per pass; no rows clear it.  The counters start anew."""
        rows = np.ascontiguousarray(areas, AREA_DTYPE).reshape(-1)
        uid = np.ascontiguousarray(member_uid, np.uint32).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_areas", rows.ctypes.data_as(C.POINTER(L.GpeArea)) if k else None, k,
                      uid.ctypes.data_as(C.POINTER(C.c_uint32)) if k else None, len(uid) if k else 0, int(iterations))

    def areas(self):
        """gpe_get_areas -> (records AREA_DTYPE[k], member_uid u32[m])."""
        k, m = C.c_uint64(), C.c_uint64()
        self.ctx.call("gpe_get_areas", None, 0, C.byref(k), None, 0, C.byref(m))
        rows = np.zeros(max(k.value, 1), AREA_DTYPE)
        uid = np.zeros(max(m.value, 1), np.uint32)
        self.ctx.call("gpe_get_areas", rows.ctypes.data_as(C.POINTER(L.GpeArea)), k.value, C.byref(k),
                      uid.ctypes.data_as(C.POINTER(C.c_uint32)), m.value, C.byref(m))
        return rows[:k.value], uid[:m.value]

    def clear_areas(self):
        """gpe_set_areas with k = 0."""
        self.ctx.call("gpe_set_areas", None, 0, None, 0, 1)

    def apply_areas(self):
        """gpe_apply_areas: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_areas")

    def areas_info(self):
        """gpe_get_areas_info -> dict(iterations, k, members, nodes, passes, resolves)."""
        info = L.GpeAreasInfo(struct_size=C.sizeof(L.GpeAreasInfo))
        self.ctx.call("gpe_get_areas_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeAreasInfo._fields_ if name != "struct_size"}

    def area_values(self):
        """gpe_get_area_values -> f32[k, 2]: (area, lambda) of every loop as of the last relaxation, NaNs for a loop
        that was inert in it and before the first pass.  Blocks like a download."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_area_values", None, 0, C.byref(k))
        out = np.zeros((max(k.value, 1), 2), np.float32)
        self.ctx.call("gpe_get_area_values", out.ctypes.data_as(C.POINTER(C.c_float)), k.value, C.byref(k))
        return out[:k.value]

    def set_area_targets(self, first, rest_area):
        """gpe_set_area_targets: new rest areas for loops first .. first + len(rest_area) - 1, in place (the pump)."""
        t = np.ascontiguousarray(rest_area, np.float32).reshape(-1)
        self.ctx.call("gpe_set_area_targets", int(first), len(t), t.ctypes.data_as(C.POINTER(C.c_float)))

    # Rigid and soft bodies (not in the reference; include/gpe.h): groups of particles, named by uid, that keep their rest
    # shape: one shape matching pass on the device after every update() / step of run(), behind the bonds and before the
    # colliders.  Step state: save() keeps them.
    def set_bodies(self, bodies, member_uid, member_rest):
        """gpe_set_bodies: replace the set by the rows of a BODY_DTYPE array (bodies_from_groups builds them) over the
        members' uids u32[m] and rest positions f32[m, 2]; no rows clear it.  The broken flags and the counters start
        anew."""
        rows = np.ascontiguousarray(bodies, BODY_DTYPE).reshape(-1)
        uid = np.ascontiguousarray(member_uid, np.uint32).reshape(-1)
        rest = np.ascontiguousarray(member_rest, np.float32).reshape(-1)
        if len(rest) != 2 * len(uid):
            raise ValueError("set_bodies: member_rest must hold two coordinates per member uid")
        k = len(rows)
        self.ctx.call("gpe_set_bodies", rows.ctypes.data_as(C.POINTER(L.GpeBody)) if k else None, k,
                      uid.ctypes.data_as(C.POINTER(C.c_uint32)) if k else None,
                      rest.ctypes.data_as(C.POINTER(C.c_float)) if k else None, len(uid))

    def bodies_from_groups(self, uid_groups, stiffness=1.0, break_distance=0.0):
        """(rows of BODY_DTYPE, member_uid u32[m], member_rest f32[m, 2]) for set_bodies: one body per group of uids,
        the particles' current positions captured as the rest shape.  stiffness and break_distance: scalars, or one
        value per group."""
        groups = [np.asarray(g, np.uint32).reshape(-1) for g in uid_groups]
        member_uid = np.concatenate(groups) if groups else np.zeros(0, np.uint32)
        index, pos, _, _ = self.find_uids(member_uid)
        if (index == L.UID_ABSENT).any():
            raise ValueError("bodies_from_groups: a uid names no live particle")
        return body_rows([len(g) for g in groups], stiffness, break_distance), member_uid, pos.copy()

    def bodies(self):
        """gpe_get_bodies -> (records BODY_DTYPE[k], broken bool[k], member_uid u32[m], member_rest f32[m, 2])."""
        k, m = C.c_uint64(), C.c_uint64()
        self.ctx.call("gpe_get_bodies", None, None, 0, C.byref(k), None, None, 0, C.byref(m))
        rows = np.zeros(max(k.value, 1), BODY_DTYPE)
        broken = np.zeros(max(k.value, 1), np.uint8)
        uid = np.zeros(max(m.value, 1), np.uint32)
        rest = np.zeros((max(m.value, 1), 2), np.float32)
        self.ctx.call("gpe_get_bodies", rows.ctypes.data_as(C.POINTER(L.GpeBody)),
                      broken.ctypes.data_as(C.POINTER(C.c_uint8)), k.value, C.byref(k),
                      uid.ctypes.data_as(C.POINTER(C.c_uint32)), rest.ctypes.data_as(C.POINTER(C.c_float)), m.value,
                      C.byref(m))
        return rows[:k.value], broken[:k.value].astype(bool), uid[:m.value], rest[:m.value]

    def clear_bodies(self):
        """gpe_set_bodies with k = 0."""
        self.ctx.call("gpe_set_bodies", None, 0, None, None, 0)

    def apply_bodies(self):
        """gpe_apply_bodies: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_bodies")

    def body_poses(self):
        """gpe_get_body_poses -> f32[k, 4]: (cx, cy, cos, sin) of every body as of the last pass, NaNs while a body is
        inert or broken and before the first pass.  Blocks like a download."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_body_poses", None, 0, C.byref(k))
        out = np.zeros((max(k.value, 1), 4), np.float32)
        self.ctx.call("gpe_get_body_poses", out.ctypes.data_as(C.POINTER(C.c_float)), k.value, C.byref(k))
        return out[:k.value]

    # Force fields (not in the reference; include/gpe.h): regions that push the particles whose centre lies in them -- a
    # uniform acceleration, a pull toward a pole, a swirl around one, a drag -- applied to prev on the device after every
    # update() / step of run(), behind the colliders and before the tracers and the monitor.  Step state: save() keeps them.
    def set_fields(self, fields):
        """gpe_set_fields: replace the set by the rows of a FIELD_DTYPE array; no rows clear it.  The counters start
        anew."""
        rows = np.ascontiguousarray(fields, FIELD_DTYPE).reshape(-1)
        k = len(rows)
        self.ctx.call("gpe_set_fields", rows.ctypes.data_as(C.POINTER(L.GpeField)) if k else None, k)

    def fields(self):
        """gpe_get_fields -> FIELD_DTYPE[k]: the set."""
        k = C.c_uint64()
        self.ctx.call("gpe_get_fields", None, 0, C.byref(k))
        rows = np.zeros(max(k.value, 1), FIELD_DTYPE)
        self.ctx.call("gpe_get_fields", rows.ctypes.data_as(C.POINTER(L.GpeField)), k.value, C.byref(k))
        return rows[:k.value]

    def clear_fields(self):
        """gpe_set_fields with k = 0."""
        self.ctx.call("gpe_set_fields", None, 0)

    def apply_fields(self, dt):
        """gpe_apply_fields: one pass now (the hook of a host that steps module by module).  Does not synchronise."""
        self.ctx.call("gpe_apply_fields", float(dt))

    def fields_info(self):
        """gpe_get_fields_info -> dict(k, passes, touched, grid_x, grid_y, list_entries).  Blocks like a download."""
        info = L.GpeFieldsInfo(struct_size=C.sizeof(L.GpeFieldsInfo))
        self.ctx.call("gpe_get_fields_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeFieldsInfo._fields_ if name != "struct_size"}

    def bodies_info(self):
        """gpe_get_bodies_info -> dict(k, members, passes, live, broken, resolves).  Blocks like a download."""
        info = L.GpeBodiesInfo(struct_size=C.sizeof(L.GpeBodiesInfo))
        self.ctx.call("gpe_get_bodies_info", C.byref(info))
        return {name: getattr(info, name) for name, _ in L.GpeBodiesInfo._fields_ if name not in ("struct_size", "reserved")}

    # Region queries and picking (not in the reference; include/gpe.h): which particles lie in a circle or a box, or
    # under a point, counted and gathered on the device.  The context is left exactly as it was.
    def _uids_on(self):
        n = C.c_uint64()
        return self.ctx.lib.gpe_next_uid(self.ctx.h, C.byref(n)) == L.GPE_OK

    def _query(self, name, args, capacity=1024):
        """Call `name` with a modest capacity, and once more with capacity = count only if it ran over."""
        with_uids = self._uids_on()
        while True:
            cap = max(int(capacity), 1)
            index = np.empty(cap, np.uint32)
            uid = np.empty(cap, np.uint32) if with_uids else None
            pos = np.empty((cap, 2), np.float32)
            prev = np.empty((cap, 2), np.float32)
            rad = np.empty(cap, np.float32)
            res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=cap)
            res.index = index.ctypes.data_as(C.POINTER(C.c_uint32))
            if with_uids:
                res.uid = uid.ctypes.data_as(C.POINTER(C.c_uint32))
            res.pos_xy = pos.ctypes.data_as(C.POINTER(C.c_float))
            res.prev_xy = prev.ctypes.data_as(C.POINTER(C.c_float))
            res.radius = rad.ctypes.data_as(C.POINTER(C.c_float))
            self.ctx.call(name, *args, C.byref(res))
            k = res.count
            if k <= cap:
                return QueryResult(index[:k], uid[:k] if with_uids else None, pos[:k], prev[:k], rad[:k])
            capacity = k

    def _count(self, name, args):
        res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=0)
        self.ctx.call(name, *args, C.byref(res))
        return res.count

    def query_circle(self, center, radius):
        """gpe_query_circle -> QueryResult(index, uid, pos, prev, radius) of every particle whose centre p has
        |p - center|^2 <= radius^2 in float32: exactly what remove_particles_in_circle(center, radius) would remove."""
        return self._query("gpe_query_circle", (float(center[0]), float(center[1]), float(radius)))

    def query_box(self, lo, hi):
        """gpe_query_box -> QueryResult of every particle with lo <= p <= hi per axis (closed; +-inf bounds allowed)."""
        return self._query("gpe_query_box", (float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])))

    def pick(self, point):
        """gpe_pick -> QueryResult of the one particle whose own disc contains `point` nearest its centre (lowest index
        on a tie), or None when no disc contains it."""
        r = self._query("gpe_pick", (float(point[0]), float(point[1])), capacity=1)
        return r if r.index.shape[0] else None

    def count_circle(self, center, radius):
        """gpe_query_circle with no outputs: the number of particles query_circle would return."""
        return self._count("gpe_query_circle", (float(center[0]), float(center[1]), float(radius)))

    def count_box(self, lo, hi):
        """gpe_query_box with no outputs: the number of particles query_box would return."""
        return self._count("gpe_query_box", (float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])))

    # Ray casts and segment queries (not in the reference; include/gpe.h): what each ray hits first, walked on the device
    # along the contact query's cell table, and everything one segment crosses.  The context is left exactly as it was.
    def cast_rays(self, origins, ends, uids=False, rows=False):
        """gpe_cast_rays -> RayHits(index, t, uid, pos, radius, hits): per ray from origins[i] to ends[i] the storage
        index of the first particle it touches (L.RAY_MISS for none) and the fraction t of the way there (NaN for none);
        uids=True adds the uids, rows=True the hit particles' centres and stored radii."""
        origins = np.ascontiguousarray(origins, np.float32)
        ends = np.ascontiguousarray(ends, np.float32)
        if origins.ndim != 2 or origins.shape[1] != 2 or origins.shape != ends.shape:
            raise ValueError("cast_rays: origins and ends must both be (k, 2), got %r and %r" % (origins.shape, ends.shape))
        k = origins.shape[0]
        room = max(k, 1)
        f32, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        index, t = np.empty(room, np.uint32), np.empty(room, np.float32)
        uid = np.empty(room, np.uint32) if uids else None
        pos = np.empty((room, 2), np.float32) if rows else None
        rad = np.empty(room, np.float32) if rows else None
        cast = L.GpeRayCast(struct_size=C.sizeof(L.GpeRayCast), flags=0, k=k)
        cast.from_xy, cast.to_xy = origins.ctypes.data_as(f32), ends.ctypes.data_as(f32)
        cast.index, cast.t = index.ctypes.data_as(u32), t.ctypes.data_as(f32)
        if uids:
            cast.uid = uid.ctypes.data_as(u32)
        if rows:
            cast.pos_xy, cast.radius = pos.ctypes.data_as(f32), rad.ctypes.data_as(f32)
        self.ctx.call("gpe_cast_rays", C.byref(cast))
        return RayHits(index[:k], t[:k], uid[:k] if uids else None, pos[:k] if rows else None,
                       rad[:k] if rows else None, cast.hits)

    # Nearest neighbours (not in the reference; include/gpe.h): the m particles whose centres are closest to each point,
    # searched on the device outward from the point along the contact query's cell table.  The context is left as it was.
    def nearest(self, points, m=1, max_distance=float("inf"), uids=False, rows=False):
        """gpe_query_nearest -> Neighbours(count, index, dist2, uid, pos, radius, found): per point the storage indices of
        the min(m, candidates) particles with the least squared centre distance d2 <= max_distance^2 (float32; the
        lowest index on a tie), ascending, and those d2; the slots past count[i] hold L.NEAREST_NONE and NaN.  uids=True
        adds the uids, rows=True the neighbours' centres and stored radii.  A point on a particle finds it at d2 = 0: for
        the neighbours of a particle ask for m + 1 and drop the first."""
        points = np.ascontiguousarray(points, np.float32)
        if points.ndim != 2 or points.shape[1] != 2:
            raise ValueError("nearest: points must be (k, 2), got %r" % (points.shape,))
        m = int(m)
        if not 1 <= m <= L.NEAREST_MAX_M:
            raise ValueError("nearest: m must be 1 .. %d, got %d" % (L.NEAREST_MAX_M, m))
        k = points.shape[0]
        room = max(k, 1)
        f32, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        count = np.empty(room, np.uint32)
        index, dist2 = np.empty((room, m), np.uint32), np.empty((room, m), np.float32)
        uid = np.empty((room, m), np.uint32) if uids else None
        pos = np.empty((room, m, 2), np.float32) if rows else None
        rad = np.empty((room, m), np.float32) if rows else None
        q = L.GpeNearestQuery(struct_size=C.sizeof(L.GpeNearestQuery), flags=0, k=k, m=m, max_distance=float(max_distance))
        q.point_xy = points.ctypes.data_as(f32)
        q.count, q.index, q.dist2 = count.ctypes.data_as(u32), index.ctypes.data_as(u32), dist2.ctypes.data_as(f32)
        if uids:
            q.uid = uid.ctypes.data_as(u32)
        if rows:
            q.pos_xy, q.radius = pos.ctypes.data_as(f32), rad.ctypes.data_as(f32)
        self.ctx.call("gpe_query_nearest", C.byref(q))
        return Neighbours(count[:k], index[:k], dist2[:k], uid[:k] if uids else None, pos[:k] if rows else None,
                          rad[:k] if rows else None, q.found)

    def query_segment(self, a, b):
        """gpe_query_segment -> QueryResult of every particle the segment from a to b touches (the function cast_rays
        applies), ascending by index."""
        return self._query("gpe_query_segment", (float(a[0]), float(a[1]), float(b[0]), float(b[1])))

    def count_segment(self, a, b):
        """gpe_query_segment with no outputs: the number of particles query_segment would return."""
        return self._count("gpe_query_segment", (float(a[0]), float(a[1]), float(b[0]), float(b[1])))

    # Contact queries (not in the reference; include/gpe.h): which particles touch -- dx*dx + dy*dy < (ri + rj)^2 in
    # float32 -- and how many neighbours each one has, searched on the device.  The context is left exactly as it was.
    def contacts(self, capacity=None, overlap=False):
        """gpe_query_contacts -> ContactResult(a, b, uid_a, uid_b, overlap): the touching pairs, a < b, ascending by a
        then b; at most `capacity` of them, all of them with capacity=None (one counting call first).  overlap=True
        adds the penetration depths (ri + rj) - sqrt(dx*dx + dy*dy) in float32."""
        with_uids = self._uids_on()
        cap = self.count_contacts() if capacity is None else int(capacity)
        room = max(cap, 1)
        u32 = C.POINTER(C.c_uint32)
        a, b = np.empty(room, np.uint32), np.empty(room, np.uint32)
        ua = np.empty(room, np.uint32) if with_uids else None
        ub = np.empty(room, np.uint32) if with_uids else None
        ov = np.empty(room, np.float32) if overlap else None
        res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=cap)
        res.index_a, res.index_b = a.ctypes.data_as(u32), b.ctypes.data_as(u32)
        if with_uids:
            res.uid_a, res.uid_b = ua.ctypes.data_as(u32), ub.ctypes.data_as(u32)
        if overlap:
            res.overlap = ov.ctypes.data_as(C.POINTER(C.c_float))
        self.ctx.call("gpe_query_contacts", C.byref(res))
        k = min(res.count, cap)
        return ContactResult(a[:k], b[:k], ua[:k] if with_uids else None, ub[:k] if with_uids else None,
                             ov[:k] if overlap else None)

    def count_contacts(self):
        """gpe_query_contacts with no outputs: the number of touching pairs (exact; may exceed 2^32)."""
        res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=0)
        self.ctx.call("gpe_query_contacts", C.byref(res))
        return res.count

    def contact_degrees(self):
        """gpe_query_contacts with the degree array only: u32[len], the number of particles touching each one."""
        n = self.len()
        deg = np.zeros(max(n, 1), np.uint32)
        res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=0)
        res.degree = deg.ctypes.data_as(C.POINTER(C.c_uint32))
        self.ctx.call("gpe_query_contacts", C.byref(res))
        return deg[:n]

    # Contact clusters (not in the reference; include/gpe.h): the connected components of the contact graph, labelled on
    # the device by the lowest storage index of each.  The context is left exactly as it was.
    def clusters(self):
        """gpe_query_clusters -> ClusterResult(label, size, label_uid, count, largest_size, largest_label): label[i] =
        the lowest index among the particles a chain of contacts joins to i, size[i] = how many they are, label_uid[i]
        = the uid of particle label[i] (None while uids are off)."""
        with_uids = self._uids_on()
        n = self.len()
        u32 = C.POINTER(C.c_uint32)
        label, size = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        label_uid = np.zeros(max(n, 1), np.uint32) if with_uids else None
        res = L.GpeClusterResult(struct_size=C.sizeof(L.GpeClusterResult))
        res.label, res.size = label.ctypes.data_as(u32), size.ctypes.data_as(u32)
        if with_uids:
            res.label_uid = label_uid.ctypes.data_as(u32)
        self.ctx.call("gpe_query_clusters", C.byref(res))
        return ClusterResult(label[:n], size[:n], label_uid[:n] if with_uids else None, res.count, res.largest_size,
                             res.largest_label)

    def count_clusters(self):
        """gpe_query_clusters with no arrays: the number of clusters, singletons included."""
        res = L.GpeClusterResult(struct_size=C.sizeof(L.GpeClusterResult))
        self.ctx.call("gpe_query_clusters", C.byref(res))
        return res.count

    def cluster_of(self, index=None, uid=None, capacity=None):
        """gpe_query_cluster_of -> QueryResult of the cluster that holds the particle named by storage `index` or by
        `uid` -- exactly one of the two -- in ascending storage index; at most `capacity` rows, all of them with
        capacity=None (one counting call first).  An unknown uid gives no rows."""
        if (index is None) == (uid is None):
            raise ValueError("cluster_of: give exactly one of index and uid")
        kind, key = (L.CLUSTER_BY_INDEX, int(index)) if uid is None else (L.CLUSTER_BY_UID, int(uid))
        if capacity is None:
            capacity = self._count("gpe_query_cluster_of", (kind, key))
        with_uids = self._uids_on()
        cap = int(capacity)
        room = max(cap, 1)
        idx = np.empty(room, np.uint32)
        uids = np.empty(room, np.uint32) if with_uids else None
        pos, prev = np.empty((room, 2), np.float32), np.empty((room, 2), np.float32)
        rad = np.empty(room, np.float32)
        res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=cap)
        res.index = idx.ctypes.data_as(C.POINTER(C.c_uint32))
        if with_uids:
            res.uid = uids.ctypes.data_as(C.POINTER(C.c_uint32))
        res.pos_xy = pos.ctypes.data_as(C.POINTER(C.c_float))
        res.prev_xy = prev.ctypes.data_as(C.POINTER(C.c_float))
        res.radius = rad.ctypes.data_as(C.POINTER(C.c_float))
        self.ctx.call("gpe_query_cluster_of", kind, key, C.byref(res))
        k = min(res.count, cap)
        return QueryResult(idx[:k], uids[:k] if with_uids else None, pos[:k], prev[:k], rad[:k])

    # Editing particles in place (not in the reference; include/gpe.h): new pos / prev / radius for particles named by
    # storage index or by uid, and velocity kicks of every particle in a circle or a box -- all on the device, the
    # uids, the order and the native counters kept.
    def edit_particles(self, indices=None, uids=None, positions=None, previous=None, radii=None):
        """gpe_edit_particles: the particles named by `indices` (storage order) or by `uids` -- exactly one of the two --
        take row i of every array given (positions f32[k,2], previous f32[k,2], radii f32[k]); an array left None leaves
        that field alone, positions without previous puts the particle at rest (prev = pos).  Unknown uids are skipped.
        Returns the number of particles written."""
        if (indices is None) == (uids is None):
            raise ValueError("exactly one of indices / uids must be given")
        keys = np.ascontiguousarray(indices if uids is None else uids, np.uint32).reshape(-1)
        k = keys.shape[0]
        e = L.GpeParticleEdit(struct_size=C.sizeof(L.GpeParticleEdit), k=k,
                              key_kind=L.EDIT_BY_INDEX if uids is None else L.EDIT_BY_UID)
        keep = [keys if k else np.zeros(1, np.uint32)]                 # (alive until the call returns)
        e.keys = keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
        for field, rows, width in (("pos_xy", positions, 2), ("prev_xy", previous, 2), ("radius", radii, 1)):
            if rows is None:
                continue
            a = np.ascontiguousarray(rows, np.float32).reshape(-1)
            if a.shape[0] != width * k:
                raise ValueError("%s: expected %d values for %d keys" % (field, width * k, k))
            keep.append(a if k else np.zeros(width, np.float32))
            setattr(e, field, keep[-1].ctypes.data_as(C.POINTER(C.c_float)))
        self.ctx.call("gpe_edit_particles", C.byref(e))
        return e.edited

    def _kick(self, name, args, op, a, count):
        kicked = C.c_uint64()
        self.ctx.call(name, *args, int(op), float(a[0]), float(a[1]), C.byref(kicked) if count else None)
        return kicked.value if count else None

    def kick_circle(self, center, radius, op, a, count=True):
        """gpe_kick_circle: for every particle query_circle(center, radius) returns, per component in float32,
        L.VEL_ADD prev -= a, L.VEL_SET prev = pos - a, L.VEL_SCALE prev = pos - (pos - prev) * a.  Returns the number
        kicked; count=False returns None without waiting for the device (stream-ordered, like update)."""
        return self._kick("gpe_kick_circle", (float(center[0]), float(center[1]), float(radius)), op, a, count)

    def kick_box(self, lo, hi, op, a, count=True):
        """gpe_kick_box: kick_circle for the particles query_box(lo, hi) returns."""
        return self._kick("gpe_kick_box", (float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])), op, a, count)

    def len(self):
        n = C.c_uint64()
        self.ctx.call("gpe_len", C.byref(n))
        return n.value

    def get_max_radius(self):
        r = C.c_float()
        self.ctx.call("gpe_max_radius", C.byref(r))
        return r.value

    def sort_by_cell_id(self, cell_size=None):
        """particle_system.rs:236-243.  The cell size is the Grid's (state.rs:123)."""
        self.ctx.call("gpe_morton_resort")

    def update_positions(self, dt):
        """particle_system.rs:245-247."""
        self.ctx.call("gpe_integrate", float(dt))

    def mouse_click_callback(self, pressed, position):
        """particle_system.rs:221-224 -> particle_integration.rs:176-181."""
        self._mouse = (bool(pressed), (float(position[0]), float(position[1])))
        self.ctx.call("gpe_set_mouse", 1 if pressed else 0, float(position[0]), float(position[1]))

    def mouse_move_callback(self, position):
        """particle_system.rs:225-227 -> particle_integration.rs:182-185: the position moves, the button state stays."""
        self._mouse = (self._mouse[0], (float(position[0]), float(position[1])))
        self.ctx.call("gpe_set_mouse", 1 if self._mouse[0] else 0, float(position[0]), float(position[1]))

    def download_home_cell_ids(self):
        return self.ctx.download(L.HOME_CELL_IDS, np.uint32)

    def download_particle_ids(self):
        return self.ctx.download(L.PARTICLE_IDS, np.uint32)

    def download_particle_buffers(self):
        """particle_system.rs:258-265 -> (current_positions, previous_positions, radii)."""
        return (self.ctx.download(L.POS, np.float32, (-1, 2)),
                self.ctx.download(L.PREV, np.float32, (-1, 2)),
                self.ctx.download(L.RADIUS, np.float32))


class Grid:
    """grid/grid.rs:24-33."""

    def __init__(self, ctx, particle_system):
        """Grid::new (grid.rs:66-71): cell size from the particle system's max radius."""
        self.ctx = ctx

    @classmethod
    def new_without_camera(cls, ctx, max_obj_radius, particle_system):
        """grid.rs:74-149."""
        self = cls(ctx, particle_system)
        ctx.call("gpe_grid_set_max_radius", float(max_obj_radius))
        return self

    @staticmethod
    def compute_cell_size(max_obj_radius):
        """grid.rs:159-161."""
        return float(L.load().gpe_compute_cell_size(float(max_obj_radius)))

    def cell_size(self):
        cs = C.c_float()
        self.ctx.call("gpe_cell_size", C.byref(cs))
        return cs.value

    def max_radius(self):
        """gpe_grid_max_radius: the radius the cell size is derived from (new_without_camera's, or the particle
        system's max radius since the last set / add / remove)."""
        r = C.c_float()
        self.ctx.call("gpe_grid_max_radius", C.byref(r))
        return r.value

    def build_cell_ids(self):
        self.ctx.call("gpe_grid_build")        # grid.rs:296-306

    def sort_map(self):
        self.ctx.call("gpe_grid_sort")         # grid.rs:310-312

    def update(self):
        self.ctx.call("gpe_grid_update")       # grid.rs:322-332

    def download_cell_ids(self):
        return self.ctx.download(L.CELL_IDS, np.uint32)      # grid.rs:314

    def download_object_ids(self):
        return self.ctx.download(L.OBJECT_IDS, np.uint32)    # grid.rs:318


class CollisionSystem:
    """physics/collision_system.rs:9-12."""

    def __init__(self, ctx, dim, particle_system, grid):
        if dim != 2:
            raise ValueError("2-D only (state.rs:18 DIMENSION = 2)")
        self.ctx = ctx

    def solve_collisions(self):
        self.ctx.call("gpe_solve_collisions")  # collision_system.rs:30-39

    def build_collision_cells(self):
        self.ctx.call("gpe_build_collision_cells")

    def download_collision_cells(self):
        return self.ctx.download(L.COLLISION_CELLS, np.uint32)   # collision_system.rs:41

    def num_collision_cells(self):
        return int(self.ctx.download(L.NUM_COLLISION_CELLS, np.uint32)[0])


NUM_BLOCKS_PER_WORKGROUP = 45      # radix_sort.rs:40
RADIX_SORT_BUCKETS = 256           # radix_sort.rs:30


class GPUSorter:
    """utils/radix_sort/radix_sort.rs:44-48 over two caller-owned GpuBuffers."""

    def __init__(self, ctx, length, keys, payload):
        self.ctx, self.length, self.keys, self.payload = ctx, int(length), keys, payload
        self.keys_b = GpuBuffer(ctx, np.zeros(self.length, np.uint32))      # radix_sort.rs:260-276
        self.payload_b = GpuBuffer(ctx, np.zeros(self.length, np.uint32))
        self.histogram = GpuBuffer(ctx, np.zeros(RADIX_SORT_BUCKETS, np.uint32))

    def sort(self, sort_first_n=None):
        n = self.length if sort_first_n is None else int(sort_first_n)      # radix_sort.rs:202
        self.ctx.call("gpe_sort_pairs_u32", self.keys.dptr, self.payload.dptr, n)

    def build_histogram(self, num_elements, current_shift):
        """radix_sort.rs:180-188 (ping = true: reads keys_a)."""
        self.ctx.call("gpe_sort_histogram_u32", self.keys.dptr, int(num_elements), int(current_shift),
                      self.histogram.dptr)

    def scatter(self, num_elements, current_shift):
        """radix_sort.rs:190-198 (ping = true: keys_a/payload_a -> keys_b/payload_b)."""
        self.ctx.call("gpe_sort_scatter_pass_u32", self.keys.dptr, self.payload.dptr, self.keys_b.dptr,
                      self.payload_b.dptr, int(num_elements), int(current_shift))

    def get_keys_b(self):
        return self.keys_b.download()

    def get_payload_b(self):
        return self.payload_b.download()

    def get_histogram(self):
        return self.histogram.download()


class PrefixSum:
    """utils/prefix_sum/prefix_sum.rs:11-18."""

    def __init__(self, ctx, buffer):
        self.ctx, self.buffer = ctx, buffer

    def execute(self, num_items):
        self.ctx.call("gpe_inclusive_scan_u32", self.buffer.dptr, int(num_items))   # prefix_sum.rs:143-160

    def update_buffers(self, buffer):
        self.buffer = buffer                                                         # prefix_sum.rs:172


class State:
    """state.rs:21-31 without window/renderer: particles + grid + collision system and update()."""

    def __init__(self, positions, radii, world=(3048.0, 1048.0), gravity=(0.0, 0.0), mode=None,
                 prev=None, device=-1, profiling=False, flags=0):
        self.world, self.gravity, self.mode = tuple(map(float, world)), tuple(map(float, gravity)), mode
        self.ctx = Context(world=world, gravity=gravity, mode=mode, device=device, profiling=profiling, flags=flags)
        self.particles = ParticleSystem.new_from_buffers(self.ctx, positions, radii, prev=prev)
        self.grid = Grid(self.ctx, self.particles)
        self.collision_system = CollisionSystem(self.ctx, 2, self.particles, self.grid)

    def update(self, dt, resort=False):
        """state.rs:115-131 (dt is explicit instead of wall clock, the re-sort an explicit flag)."""
        self.ctx.call("gpe_step", float(dt), L.STEP_RESORT if resort else 0)

    def update_wallclock(self, dt):
        """state.rs:115-131 with the reference's own re-sort policy: every SORT_INTERVAL seconds of wall clock
        (particle_system.rs:229-235), first frame included."""
        resort = self.particles.is_it_time_to_sort()
        self.update(dt, resort=resort)
        if resort:
            self.particles.reset_last_sort_time()
        return resort

    def run(self, dt, steps, resort_every=0, resort_first=True):
        self.ctx.call("gpe_run", float(dt), int(steps), int(resort_every), 1 if resort_first else 0)

    def add_particles(self, positions, radii):
        """state.rs:187-200."""
        self.particles.add_particles(positions, radii)

    def add_particles_free(self, positions, radii, separate=False, inside_world=False, dry_run=False):
        """Context.add_particles_free: append the candidates that have room -> (added, verdict)."""
        return self.ctx.add_particles_free(positions, radii, separate=separate, inside_world=inside_world,
                                           dry_run=dry_run)

    def remove_particles(self, mask):
        """ParticleSystem.remove_particles: the particles with mask[i] set leave; returns how many."""
        return self.particles.remove_particles(mask)

    def remove_particles_in_circle(self, center, radius):
        """ParticleSystem.remove_particles_in_circle: the particles inside the disc leave; returns how many."""
        return self.particles.remove_particles_in_circle(center, radius)

    def enable_uids(self, on=True):
        """ParticleSystem.enable_uids."""
        self.particles.enable_uids(on)

    def uids(self):
        return self.particles.uids()

    def set_uids(self, uids):
        self.particles.set_uids(uids)

    def next_uid(self):
        return self.particles.next_uid()

    def set_next_uid(self, next_uid):
        self.particles.set_next_uid(next_uid)

    def find_uids(self, uids):
        """ParticleSystem.find_uids -> (index, pos, prev, radius)."""
        return self.particles.find_uids(uids)

    def remove_particles_by_uid(self, uids):
        """ParticleSystem.remove_particles_by_uid: returns how many left."""
        return self.particles.remove_particles_by_uid(uids)

    def tracers_begin(self, uids, every=1, frames=1024, prev=False, index=False):
        """ParticleSystem.tracers_begin: record the path of the particles with these uids while update() / run() go on."""
        self.particles.tracers_begin(uids, every=every, frames=frames, prev=prev, index=index)

    def tracers_sample(self):
        """ParticleSystem.tracers_sample: one frame now."""
        self.particles.tracers_sample()

    def tracers_read(self, consume=False):
        """ParticleSystem.tracers_read -> TracerFrames(step, pos, prev, index, recorded)."""
        return self.particles.tracers_read(consume=consume)

    def tracers_end(self):
        """ParticleSystem.tracers_end."""
        self.particles.tracers_end()

    def measure(self, rest_speed=0.0):
        """ParticleSystem.measure -> Measures: motion, extent and health of the whole system, reduced on the device."""
        return self.particles.measure(rest_speed=rest_speed)

    def monitor_begin(self, every=1, frames=1024, rest_speed=0.0):
        """ParticleSystem.monitor_begin: record one Measures per frame while update() / run() go on."""
        self.particles.monitor_begin(every=every, frames=frames, rest_speed=rest_speed)

    def monitor_sample(self):
        """ParticleSystem.monitor_sample: one record now."""
        self.particles.monitor_sample()

    def monitor_read(self, consume=False):
        """ParticleSystem.monitor_read -> (records, recorded)."""
        return self.particles.monitor_read(consume=consume)

    def monitor_end(self):
        """ParticleSystem.monitor_end."""
        self.particles.monitor_end()

    def set_colliders(self, capsules):
        """ParticleSystem.set_colliders: static capsules (ax, ay, bx, by, radius) applied after every step."""
        self.particles.set_colliders(capsules)

    def colliders(self):
        """ParticleSystem.colliders -> f32[k, 5]."""
        return self.particles.colliders()

    def clear_colliders(self):
        """ParticleSystem.clear_colliders."""
        self.particles.clear_colliders()

    def apply_colliders(self):
        """ParticleSystem.apply_colliders: one pass now."""
        self.particles.apply_colliders()

    def colliders_info(self):
        """ParticleSystem.colliders_info -> dict(k, passes, pushed, grid_x, grid_y, list_entries)."""
        return self.particles.colliders_info()

    def set_collider_sweep(self, on):
        """ParticleSystem.set_collider_sweep: the static colliders' pass judges the path prev -> pos while on."""
        self.particles.set_collider_sweep(on)

    def collider_sweep(self):
        """ParticleSystem.collider_sweep -> bool."""
        return self.particles.collider_sweep()

    def sweep_info(self):
        """ParticleSystem.sweep_info -> dict(mode, passes, swept, stopped)."""
        return self.particles.sweep_info()

    def set_movers(self, movers):
        """ParticleSystem.set_movers: moving colliders (rows of MOVER_DTYPE) advanced and applied after every step, behind
        the bodies and before the static colliders."""
        self.particles.set_movers(movers)

    def movers(self):
        """ParticleSystem.movers -> MOVER_DTYPE[k]."""
        return self.particles.movers()

    def clear_movers(self):
        """ParticleSystem.clear_movers."""
        self.particles.clear_movers()

    def apply_movers(self, dt):
        """ParticleSystem.apply_movers: advance once and run one pass now."""
        self.particles.apply_movers(dt)

    def mover_poses(self):
        """ParticleSystem.mover_poses -> MOVER_POSE_DTYPE[k]."""
        return self.particles.mover_poses()

    def set_mover_poses(self, poses):
        """ParticleSystem.set_mover_poses."""
        self.particles.set_mover_poses(poses)

    def movers_info(self):
        """ParticleSystem.movers_info -> dict(k, passes, pushed, grid_x, grid_y, mask_words, listed)."""
        return self.particles.movers_info()

    def set_mover_sweep(self, on):
        """ParticleSystem.set_mover_sweep: the movers' pass judges the path relative to each mover while on."""
        self.particles.set_mover_sweep(on)

    def mover_sweep(self):
        """ParticleSystem.mover_sweep -> bool."""
        return self.particles.mover_sweep()

    def mover_sweep_info(self):
        """ParticleSystem.mover_sweep_info -> dict(mode, passes, swept, stopped)."""
        return self.particles.mover_sweep_info()

    def set_surfaces(self, target, rows):
        """ParticleSystem.set_surfaces: bounce and friction (rows of SURFACE_DTYPE) per collider ("colliders") or per
        mover ("movers")."""
        self.particles.set_surfaces(target, rows)

    def surfaces(self, target):
        """ParticleSystem.surfaces -> SURFACE_DTYPE[k]."""
        return self.particles.surfaces(target)

    def clear_surfaces(self, target):
        """ParticleSystem.clear_surfaces."""
        self.particles.clear_surfaces(target)

    def set_bonds(self, bonds, iterations=1):
        """ParticleSystem.set_bonds: distance bonds (rows of BOND_DTYPE) relaxed after every step, before the colliders."""
        self.particles.set_bonds(bonds, iterations)

    def bonds(self):
        """ParticleSystem.bonds -> (records BOND_DTYPE[k], broken bool[k])."""
        return self.particles.bonds()

    def clear_bonds(self):
        """ParticleSystem.clear_bonds."""
        self.particles.clear_bonds()

    def apply_bonds(self):
        """ParticleSystem.apply_bonds: one pass now."""
        self.particles.apply_bonds()

    def bonds_info(self):
        """ParticleSystem.bonds_info -> dict(iterations, k, nodes, passes, live, broken, resolves)."""
        return self.particles.bonds_info()

    def set_bond_solver(self, solver):
        """ParticleSystem.set_bond_solver: "jacobi" | "coloured"."""
        self.particles.set_bond_solver(solver)

    def bond_solver(self):
        """ParticleSystem.bond_solver -> "jacobi" | "coloured"."""
        return self.particles.bond_solver()

    def bond_solver_info(self):
        """ParticleSystem.bond_solver_info -> dict(mode, colours, largest_colour, form, lds_nodes_max, passes)."""
        return self.particles.bond_solver_info()

    def set_bends(self, bends, iterations=1):
        """ParticleSystem.set_bends: bend constraints (rows of BEND_DTYPE) relaxed after every step, in front of the bonds."""
        self.particles.set_bends(bends, iterations)

    def bends(self):
        """ParticleSystem.bends -> records BEND_DTYPE[k]."""
        return self.particles.bends()

    def clear_bends(self):
        """ParticleSystem.clear_bends."""
        self.particles.clear_bends()

    def apply_bends(self):
        """ParticleSystem.apply_bends: one pass now."""
        self.particles.apply_bends()

    def bends_info(self):
        """ParticleSystem.bends_info -> dict(iterations, k, nodes, passes, resolves)."""
        return self.particles.bends_info()

    def set_bend_solver(self, solver):
        """ParticleSystem.set_bend_solver: "jacobi" | "coloured"."""
        self.particles.set_bend_solver(solver)

    def bend_solver(self):
        """ParticleSystem.bend_solver -> "jacobi" | "coloured"."""
        return self.particles.bend_solver()

    def bend_solver_info(self):
        """ParticleSystem.bend_solver_info -> dict(mode, colours, largest_colour, form, lds_nodes_max, passes)."""
        return self.particles.bend_solver_info()

    def bends_from_positions(self, triples, stiffness=1.0):
        """Rows of BEND_DTYPE for the uid triples (a, hinge b, c) whose rest angles are the angles the particles hold
        now: the cosine and sine of the angle from a - b to c - b in float64 from the downloaded positions, rounded once
        to float32.  Every uid must name a live particle and no arm may have length 0."""
        t = np.asarray(triples, np.uint32).reshape(-1, 3)
        uids = self.uids()
        order = np.argsort(uids, kind="stable")
        at = np.searchsorted(uids[order], t)
        if (at >= len(uids)).any() or (uids[order[np.minimum(at, len(uids) - 1)]] != t).any():
            raise ValueError("bends_from_positions: a uid names no particle")
        p = self.positions().astype(np.float64)[order[at]]             # (k, 3, 2)
        u, v = p[:, 0] - p[:, 1], p[:, 2] - p[:, 1]
        den = np.sqrt((u * u).sum(axis=1) * (v * v).sum(axis=1))
        if not (den > 0).all():
            raise ValueError("bends_from_positions: an arm of length 0")
        rows = np.zeros(len(t), BEND_DTYPE)
        rows["uid_a"], rows["uid_b"], rows["uid_c"] = t[:, 0], t[:, 1], t[:, 2]
        rows["rest_cos"] = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) / den
        rows["rest_sin"] = (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]) / den
        rows["stiffness"] = stiffness
        return rows

    def set_areas(self, areas, member_uid, iterations=1):
        """ParticleSystem.set_areas: area constraints (rows of AREA_DTYPE over member uids) relaxed after every step,
        behind the bends and in front of the bonds."""
        self.particles.set_areas(areas, member_uid, iterations)

    def areas(self):
        """ParticleSystem.areas -> (records AREA_DTYPE[k], member_uid u32[m])."""
        return self.particles.areas()

    def clear_areas(self):
        """ParticleSystem.clear_areas."""
        self.particles.clear_areas()

    def apply_areas(self):
        """ParticleSystem.apply_areas: one pass now."""
        self.particles.apply_areas()

    def areas_info(self):
        """ParticleSystem.areas_info -> dict(iterations, k, members, nodes, passes, resolves)."""
        return self.particles.areas_info()

    def area_values(self):
        """ParticleSystem.area_values -> f32[k, 2]: (area, lambda) per loop as of the last relaxation."""
        return self.particles.area_values()

    def set_area_targets(self, first, rest_area):
        """ParticleSystem.set_area_targets: new rest areas for loops first .. first + len(rest_area) - 1."""
        self.particles.set_area_targets(first, rest_area)

    def areas_from_loops(self, loops, stiffness=1.0, pressure=1.0):
        """(rows of AREA_DTYPE, member_uid u32[m]) for set_areas: one loop per sequence of uids, in order around its
        polygon; the rest area is the signed area the particles enclose now (the shoelace sum in float64 from the
        downloaded positions, taken from member 0) times `pressure`, rounded once to float32.  stiffness and pressure:
        scalars, or one value per loop.  Every uid must name a live particle."""
        groups = [np.asarray(g, np.uint32).reshape(-1) for g in loops]
        member_uid = np.concatenate(groups) if groups else np.zeros(0, np.uint32)
        uids = self.uids()
        order = np.argsort(uids, kind="stable")
        at = np.searchsorted(uids[order], member_uid)
        if len(member_uid) and ((at >= len(uids)).any() or (uids[order[np.minimum(at, len(uids) - 1)]] != member_uid).any()):
            raise ValueError("areas_from_loops: a uid names no particle")
        p = self.positions().astype(np.float64)
        rows = np.zeros(len(groups), AREA_DTYPE)
        first = 0
        area = np.zeros(len(groups), np.float64)
        for j, g in enumerate(groups):
            q = p[order[at[first:first + len(g)]]]
            q = q - q[:1]
            nx, ny = np.roll(q[:, 0], -1), np.roll(q[:, 1], -1)
            area[j] = 0.5 * float((q[:, 0] * ny - nx * q[:, 1]).sum())
            rows["first"][j], rows["count"][j] = first, len(g)
            first += len(g)
        rows["rest_area"] = area * np.broadcast_to(np.asarray(pressure, np.float64), area.shape)
        rows["stiffness"] = stiffness
        return rows, member_uid

    def set_bodies(self, bodies, member_uid, member_rest):
        """ParticleSystem.set_bodies: groups of particles (rows of BODY_DTYPE) matched to their rest shape after every
        step, behind the bonds and before the colliders."""
        self.particles.set_bodies(bodies, member_uid, member_rest)

    def bodies_from_groups(self, uid_groups, stiffness=1.0, break_distance=0.0):
        """ParticleSystem.bodies_from_groups -> (rows, member_uid, member_rest): the current positions as the rest shape."""
        return self.particles.bodies_from_groups(uid_groups, stiffness, break_distance)

    def bodies(self):
        """ParticleSystem.bodies -> (records BODY_DTYPE[k], broken bool[k], member_uid u32[m], member_rest f32[m, 2])."""
        return self.particles.bodies()

    def clear_bodies(self):
        """ParticleSystem.clear_bodies."""
        self.particles.clear_bodies()

    def apply_bodies(self):
        """ParticleSystem.apply_bodies: one pass now."""
        self.particles.apply_bodies()

    def body_poses(self):
        """ParticleSystem.body_poses -> f32[k, 4]: (cx, cy, cos, sin) as of the last pass."""
        return self.particles.body_poses()

    def bodies_info(self):
        """ParticleSystem.bodies_info -> dict(k, members, passes, live, broken, resolves)."""
        return self.particles.bodies_info()

    def set_fields(self, fields):
        """ParticleSystem.set_fields: force fields (rows of FIELD_DTYPE) applied to prev after every step, behind the
        colliders."""
        self.particles.set_fields(fields)

    def fields(self):
        """ParticleSystem.fields -> FIELD_DTYPE[k]."""
        return self.particles.fields()

    def clear_fields(self):
        """ParticleSystem.clear_fields."""
        self.particles.clear_fields()

    def apply_fields(self, dt):
        """ParticleSystem.apply_fields: one pass now."""
        self.particles.apply_fields(dt)

    def fields_info(self):
        """ParticleSystem.fields_info -> dict(k, passes, touched, grid_x, grid_y, list_entries)."""
        return self.particles.fields_info()

    def query_circle(self, center, radius):
        """ParticleSystem.query_circle -> QueryResult(index, uid, pos, prev, radius)."""
        return self.particles.query_circle(center, radius)

    def query_box(self, lo, hi):
        """ParticleSystem.query_box -> QueryResult."""
        return self.particles.query_box(lo, hi)

    def pick(self, point):
        """ParticleSystem.pick -> QueryResult of one particle, or None."""
        return self.particles.pick(point)

    def contacts(self, capacity=None, overlap=False):
        """ParticleSystem.contacts -> ContactResult(a, b, uid_a, uid_b, overlap) of the touching pairs."""
        return self.particles.contacts(capacity, overlap)

    def count_contacts(self):
        """ParticleSystem.count_contacts -> the number of touching pairs."""
        return self.particles.count_contacts()

    def contact_degrees(self):
        """ParticleSystem.contact_degrees -> u32[len], the contacts of every particle."""
        return self.particles.contact_degrees()

    def clusters(self):
        """ParticleSystem.clusters -> ClusterResult(label, size, label_uid, count, largest_size, largest_label)."""
        return self.particles.clusters()

    def count_clusters(self):
        """ParticleSystem.count_clusters -> the number of contact clusters, singletons included."""
        return self.particles.count_clusters()

    def cluster_of(self, index=None, uid=None, capacity=None):
        """ParticleSystem.cluster_of -> QueryResult of the cluster that holds the particle `index` or `uid`."""
        return self.particles.cluster_of(index=index, uid=uid, capacity=capacity)

    def cast_rays(self, origins, ends, uids=False, rows=False):
        """ParticleSystem.cast_rays -> RayHits(index, t, uid, pos, radius, hits): the first hit of every ray."""
        return self.particles.cast_rays(origins, ends, uids=uids, rows=rows)

    def nearest(self, points, m=1, max_distance=float("inf"), uids=False, rows=False):
        """ParticleSystem.nearest -> Neighbours(count, index, dist2, uid, pos, radius, found): the m closest particles."""
        return self.particles.nearest(points, m=m, max_distance=max_distance, uids=uids, rows=rows)

    def query_segment(self, a, b):
        """ParticleSystem.query_segment -> QueryResult of everything the segment from a to b touches."""
        return self.particles.query_segment(a, b)

    def count_segment(self, a, b):
        return self.particles.count_segment(a, b)

    def count_circle(self, center, radius):
        return self.particles.count_circle(center, radius)

    def count_box(self, lo, hi):
        return self.particles.count_box(lo, hi)

    def edit_particles(self, indices=None, uids=None, positions=None, previous=None, radii=None):
        """ParticleSystem.edit_particles: returns how many particles were written."""
        return self.particles.edit_particles(indices=indices, uids=uids, positions=positions, previous=previous,
                                             radii=radii)

    def kick_circle(self, center, radius, op, a, count=True):
        """ParticleSystem.kick_circle: returns how many were kicked (None with count=False)."""
        return self.particles.kick_circle(center, radius, op, a, count=count)

    def kick_box(self, lo, hi, op, a, count=True):
        """ParticleSystem.kick_box."""
        return self.particles.kick_box(lo, hi, op, a, count=count)

    def _uids_on(self):
        try:
            self.particles.next_uid()
        except L.GpeError as e:
            if e.status == L.GPE_ERR_STATE:
                return False
            raise
        return True

    def positions(self):
        return self.ctx.download(L.POS, np.float32, (-1, 2))

    def previous_positions(self):
        return self.ctx.download(L.PREV, np.float32, (-1, 2))

    def radii(self):
        return self.ctx.download(L.RADIUS, np.float32)

    # Checkpoint / restore (the reference's only state dump is download_particle_buffers,
    # particle_system.rs:258-265): the three arrays the step evolves plus the constants a step depends on, as the
    # context holds them (they may have been set through ctx.call as well as through this class).
    def save(self, path):
        """Binary snapshot (numpy .npz, no pickle): positions, previous positions, radii, world, gravity; with uids on
        also the uids and next_uid; with the mouse pressed its position (`mouse`); with a grid radius other than the
        one gpe_set_particles derives from the saved radii (Grid.new_without_camera) that radius (`grid_max_radius`).
        A tracer recorder (tracers_begin) is not stored: it is observation state, not step state -- a loaded State steps
        the same bits without it and is armed again by its host.  The run monitor (monitor_begin) is not stored either,
        for the same reason.  Static colliders are step state: a set that is present is written (`colliders`), and so
        are distance bonds with their relaxation count and broken flags (`bonds`, `bond_iterations`, `bonds_broken`) and
        bend constraints with their relaxation count (`bends`, `bend_iterations`) and
        area constraints with their members and relaxation count (`areas`, `area_member_uid`, `area_iterations`) and
        bodies with their members and broken flags (`bodies`, `bodies_broken`, `body_member_uid`, `body_member_rest`) and
        force fields (`fields`) and moving colliders with their poses (`movers`, `mover_poses`), and the surfaces of
        the two sets where present (`collider_surfaces`, `mover_surfaces`), and the static colliders' sweep where it is
        on (`collider_sweep`), and the movers' sweep where it is on (`mover_sweep`), and the bonds' solver where bonds are held
        and it is the coloured one (`bond_solver`).  A coloured mode set on a context that holds no bonds is NOT
        written -- it has moved nothing -- and such a snapshot loads as Jacobi: a host that sets its bonds after load()
        sets the solver again with them.  The bends' solver is kept the same way (`bend_solver`: only where bends are
        held and it is the coloured one)."""
        extra = {}
        if self.mover_sweep():
            extra.update(mover_sweep=np.array([L.SWEEP_ON], np.uint32))
        if self.collider_sweep():
            extra.update(collider_sweep=np.array([L.SWEEP_ON], np.uint32))
        for target in ("colliders", "movers"):
            rows = self.surfaces(target)
            if len(rows):
                extra[target[:-1] + "_surfaces"] = rows
        movers = self.movers()
        if len(movers):
            extra.update(movers=movers, mover_poses=self.mover_poses())
        fields = self.fields()
        if len(fields):
            extra.update(fields=fields)
        bodies, bodies_broken, member_uid, member_rest = self.bodies()
        if len(bodies):
            extra.update(bodies=bodies, bodies_broken=bodies_broken, body_member_uid=member_uid,
                         body_member_rest=member_rest)
        bonds, broken = self.bonds()
        if len(bonds):
            extra.update(bonds=bonds, bond_iterations=np.array([self.bonds_info()["iterations"]], np.uint32),
                         bonds_broken=broken)
            if self.bond_solver() == "coloured":                       # (asked where bonds are held: the mode alone moves nothing)
                extra.update(bond_solver=np.array([L.BOND_SOLVER_COLOURED], np.uint32))
        caps = self.colliders()
        if len(caps):
            extra.update(colliders=caps)
        if self._uids_on():
            extra.update(uids=self.uids(), next_uid=np.array([self.next_uid()], np.uint64))
            bends = self.bends()                                       # (they name particles by uid: none without uids)
            if len(bends):
                extra.update(bends=bends, bend_iterations=np.array([self.bends_info()["iterations"]], np.uint32))
                if self.bend_solver() == "coloured":                   # (asked where bends are held: the mode alone moves nothing)
                    extra.update(bend_solver=np.array([L.BEND_SOLVER_COLOURED], np.uint32))
            areas, area_member_uid = self.areas()
            if len(areas):
                extra.update(areas=areas, area_member_uid=area_member_uid,
                             area_iterations=np.array([self.areas_info()["iterations"]], np.uint32))
        pressed, at = self.ctx.mouse()
        if pressed:
            extra.update(mouse=np.array(at, np.float32))
        radius = self.radii()
        # load() sets the particles, whose grid radius is then the radius of largest magnitude (last on ties, sign kept:
        # gpe_set_particles); anything else -- an override, or an add's fmaxf rule with negative radii -- is written
        a = np.abs(radius)
        set_r = radius[len(a) - 1 - int(np.argmax(a[::-1]))] if len(a) else np.float32(0)
        grid_r = np.array([self.grid.max_radius()], np.float32)
        if grid_r.view(np.uint32)[0] != np.array([set_r], np.float32).view(np.uint32)[0]:
            extra.update(grid_max_radius=grid_r)
        np.savez(path, format=np.array([1], np.int32), pos=self.positions(), prev=self.previous_positions(),
                 radius=radius, world=np.array(self.ctx.world(), np.float32),
                 gravity=np.array(self.ctx.gravity(), np.float32), **extra)

    @classmethod
    def load(cls, path, mode=None, device=-1, flags=0):
        """A State that continues from a snapshot written by save(): the next update() yields the same bits as
        the saved run's next update() would have (the step has no hidden state beyond these arrays and constants)."""
        with np.load(path, allow_pickle=False) as d:
            if int(d["format"][0]) != 1:
                raise ValueError("unknown snapshot format")
            st = cls(d["pos"], d["radius"], world=tuple(d["world"]), gravity=tuple(d["gravity"]), mode=mode,
                     prev=d["prev"], device=device, flags=flags)
            if "uids" in d.files:
                st.set_uids(d["uids"])
                st.set_next_uid(int(d["next_uid"][0]))
            if "mouse" in d.files:
                st.particles.mouse_click_callback(True, tuple(d["mouse"]))
            if "grid_max_radius" in d.files:
                st.ctx.call("gpe_grid_set_max_radius", float(d["grid_max_radius"][0]))
            if "colliders" in d.files:
                st.set_colliders(d["colliders"])
            if "collider_surfaces" in d.files:                     # (after their set)
                st.set_surfaces("colliders", d["collider_surfaces"].astype(SURFACE_DTYPE))
            if "collider_sweep" in d.files:                        # (a file without it: off)
                st.set_collider_sweep(bool(d["collider_sweep"][0]))
            if "bond_solver" in d.files and int(d["bond_solver"][0]) == L.BOND_SOLVER_COLOURED:
                st.set_bond_solver("coloured")                     # (before the bonds: their tables are built once; no key: Jacobi)
            if "bonds" in d.files:                                 # (after the uids they name; a broken bond starts broken)
                rows = d["bonds"].astype(BOND_DTYPE)
                rows["flags"] |= np.where(d["bonds_broken"], L.BOND_BROKEN, 0).astype(np.uint32)
                st.set_bonds(rows, int(d["bond_iterations"][0]))
            if "bend_solver" in d.files and int(d["bend_solver"][0]) == L.BEND_SOLVER_COLOURED:
                st.set_bend_solver("coloured")                     # (before the bends: their tables are built once; no key: Jacobi)
            if "bends" in d.files:                                 # (after the uids they name)
                st.set_bends(d["bends"].astype(BEND_DTYPE), int(d["bend_iterations"][0]))
            if "areas" in d.files:                                 # (after the uids they name)
                st.set_areas(d["areas"].astype(AREA_DTYPE), d["area_member_uid"], int(d["area_iterations"][0]))
            if "bodies" in d.files:                                # (after the uids and the bonds; a broken body starts broken)
                rows = d["bodies"].astype(BODY_DTYPE)
                rows["flags"] |= np.where(d["bodies_broken"], L.BODY_BROKEN, 0).astype(np.uint32)
                st.set_bodies(rows, d["body_member_uid"], d["body_member_rest"])
            if "fields" in d.files:
                st.set_fields(d["fields"].astype(FIELD_DTYPE))
            if "movers" in d.files:
                st.set_movers(d["movers"].astype(MOVER_DTYPE))
                st.set_mover_poses(d["mover_poses"].astype(MOVER_POSE_DTYPE))
            if "mover_surfaces" in d.files:                        # (after their set and its poses)
                st.set_surfaces("movers", d["mover_surfaces"].astype(SURFACE_DTYPE))
            if "mover_sweep" in d.files:                           # (a file without it: off)
                st.set_mover_sweep(bool(d["mover_sweep"][0]))
            return st

    def close(self):
        self.ctx.close()
