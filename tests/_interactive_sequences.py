"""Random call sequences that include the interactive calls of include/gpe.h -- keyed edits, kicks, the overlap-checked
add and its dry run, region / contact / cluster queries -- between the calls tests/test_gpu_api_sequences.py already
mixes.  TEST INFRASTRUCTURE ONLY.

plan(seed) gives the scene and the list of operations; Sequence applies them one by one to the oracle model of a context
(tests/_oracle_model.py) and, when it has one, to a State, and compares what the State returns with what the model
returns.  Every random draw comes from one generator seeded by the plan and depends on nothing but the model's state, so
the same plan runs with the model alone on a CPU (tests/test_interactive_sequences_cpu.py), where the coverage counters
below are checked before any GPU time is spent.

What the plan pins, because chance would not: a lookup by uid straight after each thing that leaves the uid -> index map
stale (re-sort, removal, uids off and on); contact and cluster searches straight after a growth, with particles outside
a shrunken world, and in the other mode; save / load straight after an edit and after a checked add; a radius edit with
and without a grid override pending.

plan_observed(seed) is the same plan with the observers in it, run by ObservedSequence: the tracer recorder and the run
monitor armed all along (begun anew three times, and around every save / load, which stores neither), gpe_measure,
gpe_cast_rays, gpe_query_segment and gpe_query_nearest.  The operations of plan(seed), their order and every draw they
make from Sequence.rng stay as they are: where the new operations go is drawn by a generator of plan_observed's own, and
what they do by ObservedSequence.rng2.  The recorders' models (tests/_tracers_model.py, tests/_monitor_model.py) look at
the same OracleModel; the Sequence tells them of every step it makes (after_step).  What this plan pins, because chance
would not: a frame and a gpe_tracers_read straight after each thing that leaves the tracers' slot table stale (re-sort,
a run that re-sorts, removal by mask / circle / of a tracked uid, add, an accepted checked add, gpe_set_uids, uids off
and on); a tracked uid handed out by the add that grows the buffers; frames of both recorders across that growth, the
spell in the other mode, a shrunken world with particles outside, teleports, stops, edits outside the world and kicks;
rings that have wrapped before they are read; a consuming read with a frame and a read behind it; both refused begins;
and casts, segment and nearest queries straight after the growth, the shrink, a removal, a radius edit with and without
a grid override, an understated grid radius, and in the other mode (Coverage.check_observed lists the counters)."""
import collections
import ctypes as C
import os
import tempfile

import numpy as np

from tests import _spawn_model
from tests._oracle_model import OracleModel, VEL_ADD, VEL_SET, VEL_SCALE, box_mask, circle_mask

F32 = np.float32
DT = 1.0 / 60.0
DENSITY = 1_000_000 / (3048.0 * 1048.0)        # the reference scene's particles per unit area
SEEDS = list(range(1, 7))
SMALL = (2, 3, 4)                              # seeds whose scene is at the small end (their run time: see plan())
SENTINEL = 0xA5A5A5A5                          # fills the host arrays of a query: what lies past the rows must keep it
FIELD_SUBSETS = [("pos",), ("pos", "prev"), ("prev",), ("radius",), ("pos", "prev", "radius")]

Plan = collections.namedtuple("Plan", "seed pos rad world ops spawn_flags")

# the operations every sequence contains: blocks stay together, in this order
BLOCKS = [
    ["uids_on", "resort", "cluster_of_uid"], ["uids_on", "resort", "edit_uid"],
    ["uids_on", "remove_mask", "cluster_of_uid"], ["uids_on", "remove_circle", "edit_uid"],
    ["uids_cycle", "cluster_of_uid"], ["uids_cycle", "edit_uid"],
    ["add", "contacts", "clusters"],                           # (placed before every other add: it grows the buffers)
    ["edit_index", "save_load"], ["add_free", "save_load"],
    ["save_load", "step", "add_free"],                         # (capacity == len after a load: an accepted row grows)
    ["world_shrink_out", "contacts", "clusters"],
    ["edit_radius_up_override", "step", "edit_radius_down"], ["edit_radius_up", "step", "edit_radius_down_override"],
] + [[op] for op in (
    "step", "run", "module", "mouse", "gravity", "remove_uid", "uids_set", "uids_toggle", "world_grow",
    "world_shrink_in", "world_back", "grid_under", "grid_over", "grid_exact", "set_mode", "stop", "teleport",
    "edit_index", "edit_pos_override", "edit_outside_and_back", "kick_circle", "kick_circle_nosync", "kick_box",
    "kick_box_nosync", "add_free", "add_free", "query_circle", "query_box", "pick", "cluster_of_index")]
DRAWN = ["step", "step", "run", "module", "resort", "mouse", "gravity", "add", "remove_mask", "remove_circle",
         "remove_uid", "uids_toggle", "grid_under", "grid_exact", "world_back", "stop", "teleport", "edit_index",
         "edit_uid", "kick_circle", "kick_box_nosync", "query_box", "pick"]
ADDS = ("add", "add_free")
# (separate, inside_world, dry_run) of a sequence's add_free calls, in order: the first two in every seed -- candidates
# blocked by candidates need `separate` without the world test, OUTSIDE_WORLD needs the world test -- then two of the
# other six, so that seeds 1 .. 6 use all eight
OTHER_FLAGS = [(0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def _inside(p, world, margin):
    lo = F32(margin)
    hi = np.array(world, F32) - F32(margin)
    return np.clip(p, lo, np.maximum(hi, lo)).astype(F32)


def plan(seed):
    """The scene and the operations of one sequence: see _plan_and_blocks."""
    return _plan_and_blocks(seed)[0]


def _plan_and_blocks(seed):
    """-> (the plan, its operations as the blocks they were placed in).
    The scene and the operations of one sequence: 1 500 .. 6 000 particles at the reference density in a world of
    90 .. 160 x 60 .. 110, radius 0.5 (seeds 3 and 6: a share at 1.0 and 1.5), even seeds with a blob at four times the
    density; 65 .. 70 operations, BLOCKS in a random order with a few of DRAWN between them.  Seeds 2, 3 and 4 take the
    smallest worlds of that range: with larger ones their cases ran longer than the same seeds of
    test_random_api_sequences_match_the_oracle, mostly in the model's brute-force contact search."""
    rng = np.random.default_rng(9100 + seed)
    world = (float(rng.integers(90, 161)), float(rng.integers(60, 111)))
    if seed in SMALL:
        world = (float(rng.integers(90, 101)), float(rng.integers(60, 67)))
    n = int(np.clip(DENSITY * world[0] * world[1], 1500, 6000))
    blob = seed % 2 == 0
    if blob:
        n = min(n, 4000)
    pos = _inside((rng.random((n, 2), dtype=F32) * np.array(world, F32)).astype(F32), world, 0.5)
    rad = np.full(n, 0.5, F32)
    if seed % 3 == 0:
        rad = rng.choice(np.array([0.5, 1.0, 1.5], F32), n, p=[0.8, 0.12, 0.08]).astype(F32)
    if blob:
        m = n // 2
        bw = float(np.sqrt(m / (4.0 * DENSITY) * 1.25))
        bh = bw / 1.25
        corner = np.array([rng.random() * (world[0] - bw - 10.0) + 5.0, rng.random() * (world[1] - bh - 10.0) + 5.0], F32)
        extra = (rng.random((m, 2), dtype=F32) * np.array([bw, bh], F32) + corner).astype(F32)
        pos = np.concatenate([pos, _inside(extra, world, 0.5)])
        rad = np.concatenate([rad, np.full(m, 0.5, F32)])
    blocks = [list(b) for b in BLOCKS] + [[DRAWN[int(rng.integers(0, len(DRAWN)))]] for _ in range(int(rng.integers(0, 6)))]
    order = rng.permutation(len(blocks))
    blocks = [blocks[i] for i in order]
    # the block whose add must grow the buffers comes before every other add: a context starts with capacity == len
    grow = next(i for i, b in enumerate(blocks) if b[0] == "add" and len(b) == 3)
    first = next(i for i, b in enumerate(blocks) if any(op in ADDS for op in b))
    blocks[grow], blocks[first] = blocks[first], blocks[grow]
    ops = [op for b in blocks for op in b]
    flags = [(1, 0, 0), (0, 1, 0), OTHER_FLAGS[(seed - 1) % 6], OTHER_FLAGS[(seed + 2) % 6]]
    return Plan(seed, pos, rad, world, ops, flags), blocks


class Coverage(collections.Counter):
    """What a sequence reached, counted on the model's side.  check() is the list of conditions a sequence must meet."""

    def check(self, spawn_flags):
        need = ["keyed_edits_written", "uid_edits_skipping_absent", "kicks_nonzero", "verdict_added",
                "verdict_blocked_by_particle", "add_free_appended", "add_free_grew", "add_grew", "contacts_nonzero",
                "clusters_of_3_or_more", "picks_hit", "uid_lookups_on_a_stale_map", "dry_runs", "edit_outside_and_back",
                "contacts_after_growth", "contacts_outside_world", "contacts_other_mode", "save_load_after_edit",
                "save_load_after_add_free", "radius_up_with_override", "radius_down_with_override",
                "pos_edit_keeps_override", "stale_after_resort", "stale_after_removal", "stale_after_uids_on"]
        if any(s and not w for s, w, _ in spawn_flags):
            need.append("verdict_blocked_by_candidate")
        if any(w for _, w, _ in spawn_flags):
            need.append("verdict_outside_world")
        if not any(d for _, _, d in spawn_flags):
            need.remove("dry_runs")
        missing = [k for k in need if self[k] == 0]
        assert not missing, "the sequence never reached: %s\n%s" % (", ".join(missing), dict(self))

    def check_observed(self):
        """What an observed sequence (plan_observed) must have met on top of check(): every pin of the plan, by its
        counter, and the conditions on the inputs of the recorders and the late queries."""
        need = (["tracers_after_" + p for p in TRACER_PINS]
                + ["%s_across_%s" % (r, p) for r in ("tracers", "monitor") for p in ACROSS_PINS]
                + ["%s_after_%s" % (q, p) for q in ("cast", "segment", "nearest") for p in QUERY_PINS]
                + ["tracer_rows_present", "tracer_rows_absent", "tracer_rows_appeared", "tracer_future_uid_handed_out",
                   "tracer_index_changed_between_frames", "tracer_ring_wrapped", "monitor_ring_wrapped",
                   "monitor_outside_nonzero", "monitor_moving_between_0_and_n", "rays_hit", "rays_missed",
                   "ray_from_inside", "segment_rows_at_least_3", "nearest_cut_by_max_distance", "nearest_m_64_delivered",
                   "tracers_consume_sample_read", "monitor_consume_sample_read", "monitor_kick_changed_max_v2",
                   "monitor_kick_changed_max_v2_uid", "both_recorders_armed_different_every", "save_load_while_armed",
                   "tracers_begin_refused_armed", "tracers_begin_refused_uids_off", "measures", "segment_of_a_cast_ray",
                   "cast_uids_asked", "cast_uids_not_asked", "nearest_uids_asked", "nearest_uids_not_asked"])
        missing = [k for k in need if self[k] == 0]
        assert not missing, "the observed sequence never reached: %s\n%s" % (", ".join(missing), dict(self))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Sequence:
    """One plan applied to the model and (gpe given) to a State.  compare(st, model, where) is called after every
    operation; mode_name picks the State's mode and flags its gpe_config flags."""

    def __init__(self, plan_, oracle, gpe=None, mode_name="native", compare=None, flags=0):
        self.plan, self.gpe, self.compare, self.mode_name = plan_, gpe, compare, mode_name
        self.rng = np.random.default_rng(9200 + plan_.seed)
        self.world0 = self.world = plan_.world
        self.model = OracleModel(oracle, plan_.pos, plan_.rad, world=plan_.world)
        self.cov = Coverage()
        self.log = []
        self.cap = len(self.model)                     # gpe_capacity, as gpe_add_particles grows it
        self.map_stale = False                         # uids on and the uid -> index map behind them
        self.stale_because = None
        self.spawn_calls = 0
        self.edits = plan_.seed                        # (rotates the field subsets / the kick ops from seed to seed)
        self.kicks = plan_.seed
        self.last = None                               # the operation before this one
        self.grew = False                              # the last add grew the buffers
        self.outside = 0                               # particles the last world_shrink_out left outside
        self.st = self.L = None
        self.tm = self.mm = None                       # the recorders' models, while armed (ObservedSequence)
        self.native_steps = self.compat_steps = 0
        self.tmp = tempfile.TemporaryDirectory()
        if gpe is not None:
            self.L = gpe._lib
            self.mode = self.L.MODE_NATIVE if mode_name == "native" else self.L.MODE_COMPAT
            self.other = self.L.MODE_COMPAT if mode_name == "native" else self.L.MODE_NATIVE
            self.flags = flags
            self.st = gpe.State(plan_.pos, plan_.rad, world=plan_.world, mode=self.mode, flags=flags)

    # ---- plumbing -----------------------------------------------------------------------------------------------------
    def where(self, i, op):
        return "seed %d %s op #%d (%s)\n  %s" % (self.plan.seed, self.mode_name, i, op, "\n  ".join(self.log))

    def close(self):
        if self.st is not None:
            self.st.close()
            self.st = None
        self.model.close()
        self.tmp.cleanup()

    def retire(self):
        """pipeline_info() of a State that leaves (save / load replaces it): the rosters' stamp is the sort count."""
        info = self.st.ctx.pipeline_info()
        assert info["roster_stamp"] == info["native_sorts"] & 0xFFFFFFFF, (info, self.log)
        self.native_steps += info["native_steps"]
        self.compat_steps += info["compat_steps"]

    def _counters(self):
        info = self.st.ctx.pipeline_info()
        return {k: info[k] for k in ("native_sorts", "roster_stamp", "native_steps", "compat_steps")}

    def _frozen(self, before, what):
        """A read-only call, a dry run, an add of nothing and a kick leave the counters alone."""
        after = self._counters()
        assert after == before, "%s moved the counters: %r -> %r\n  %s" % (what, before, after, "\n  ".join(self.log))

    def _capacity(self):
        cap = C.c_uint64()
        self.st.ctx.call("gpe_capacity", C.byref(cap))
        return cap.value

    def _grow(self, new_n):
        """gpe_add_particles: past the capacity the buffers double, or take what is needed if that is more."""
        self.grew = new_n > self.cap
        if self.grew:
            self.cap = max(new_n, 2 * self.cap)
        return self.grew

    def _stale(self, because):
        if self.model.uids is not None:
            self.map_stale, self.stale_because = True, because

    def _uids_on(self):
        if self.model.uids is None:
            if self.st is not None:
                self.st.enable_uids()
            self.model.enable_uids()
            self._stale("uids_on")
            self.log.append("uids on")

    def _lookup_by_uid(self, counts=True):
        """A call that resolves uids: it meets the map as the calls before left it, and leaves it rebuilt."""
        if self.map_stale and counts:
            self.cov["uid_lookups_on_a_stale_map"] += 1
            self.cov["stale_after_" + self.stale_because] += 1
        self.map_stale = False

    def _a_particle(self):
        p = self.model.arrays()[0]
        return p[int(self.rng.integers(0, len(p)))]

    def _upload(self, what, arr):
        ptr, nbytes = self.st.ctx.device_ptr(what)
        assert nbytes == arr.nbytes
        self.st.ctx.call("gpe_buffer_upload", ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes)

    # ---- the raw query calls: host arrays filled with SENTINEL, so that what lies past the rows shows -----------------
    def _rows_call(self, name, args, capacity, want, what):
        """gpe_query_circle / box / pick / cluster_of with room for `capacity` rows: count, the first min(count, capacity)
        rows of `want` in every array, and nothing written behind them."""
        L, room, uids_on = self.L, max(capacity, 1) + 3, self.model.uids is not None
        arr = {"index": np.full(room, SENTINEL, np.uint32), "pos_xy": np.full(2 * room, SENTINEL, np.uint32),
               "prev_xy": np.full(2 * room, SENTINEL, np.uint32), "radius": np.full(room, SENTINEL, np.uint32)}
        if uids_on:
            arr["uid"] = np.full(room, SENTINEL, np.uint32)
        res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=capacity)
        for k, a in arr.items():
            setattr(res, k, a.ctypes.data_as(C.POINTER(C.c_float if k in ("pos_xy", "prev_xy", "radius") else C.c_uint32)))
        before = self._counters()
        self.st.ctx.call(name, *args, C.byref(res))
        self._frozen(before, what)
        assert res.count == len(want.index), "%s: count %d, model %d" % (what, res.count, len(want.index))
        m = min(res.count, capacity)
        wanted = {"index": want.index, "pos_xy": _bits(want.pos).reshape(-1), "prev_xy": _bits(want.prev).reshape(-1),
                  "radius": _bits(want.radius), "uid": want.uid}
        for k, a in arr.items():
            w = 2 if k in ("pos_xy", "prev_xy") else 1
            assert np.array_equal(a[:w * m], wanted[k][:w * m]), "%s: %s differs" % (what, k)
            assert (a[w * m:] == SENTINEL).all(), "%s: %s written past row %d" % (what, k, m)

    def _contacts_call(self, capacity, want, what):
        L, room, uids_on = self.L, max(capacity, 1) + 3, self.model.uids is not None
        names = ["index_a", "index_b", "overlap"] + (["uid_a", "uid_b"] if uids_on else [])
        arr = {k: np.full(room, SENTINEL, np.uint32) for k in names}
        arr["degree"] = np.full(len(self.model) + 3, SENTINEL, np.uint32)
        res = L.GpeContactResult(struct_size=C.sizeof(L.GpeContactResult), capacity=capacity)
        for k, a in arr.items():
            setattr(res, k, a.ctypes.data_as(C.POINTER(C.c_float if k == "overlap" else C.c_uint32)))
        before = self._counters()
        self.st.ctx.call("gpe_query_contacts", C.byref(res))
        self._frozen(before, what)
        assert res.count == want.count, "%s: count %d, model %d" % (what, res.count, want.count)
        m = min(res.count, capacity)
        wanted = {"index_a": want.a, "index_b": want.b, "overlap": _bits(want.overlap), "uid_a": want.uid_a,
                  "uid_b": want.uid_b}
        for k in names:
            assert np.array_equal(arr[k][:m], wanted[k][:m]), "%s: %s differs" % (what, k)
            assert (arr[k][m:] == SENTINEL).all(), "%s: %s written past pair %d" % (what, k, m)
        n = len(self.model)
        assert np.array_equal(arr["degree"][:n], want.degree), "%s: degrees differ" % what
        assert (arr["degree"][n:] == SENTINEL).all(), "%s: degrees written past gpe_len" % what

    # ---- the operations -----------------------------------------------------------------------------------------------
    def apply(self, i, op):
        getattr(self, "op_" + op)(len(self.model))
        if self.st is not None:
            assert self._capacity() == self.cap, "capacity %d, expected %d\n%s" % (self._capacity(), self.cap, self.where(i, op))
            self.compare(self.st, self.model, self.where(i, op))
        if op not in OBSERVING:
            self.last = op

    def _observe(self, where):
        """Called inside the operations, at the points where an ObservedSequence looks at the State."""

    def _after_step(self):
        for recorder in (self.tm, self.mm):
            if recorder is not None:
                recorder.after_step()

    def run(self):
        for i, op in enumerate(self.plan.ops):
            self.apply(i, op)
        if self.st is not None:
            self.retire()

    # steps
    def _step(self, resort=False):
        if resort:
            self._stale("resort")
        if self.st is not None:
            self.st.update(DT, resort=resort)
        self.model.step(DT, resort=resort)
        self._after_step()

    def op_step(self, cnt):
        k = int(self.rng.integers(1, 5)); resort = bool(self.rng.integers(0, 4) == 0)
        for s in range(k):
            self._step(resort and s == 0)
        self.log.append("step x%d%s" % (k, " resort" if resort else ""))

    def _run(self, k, every, first):
        """gpe_run; the model makes its steps one at a time (as OracleModel.run does), a recorder counting each."""
        if first or (every and k > every):
            self._stale("resort")
        if self.st is not None:
            self.st.run(DT, k, resort_every=every, resort_first=first)
        for s in range(k):
            self.model.step(DT, resort=bool((s == 0 and first) or (every and s > 0 and s % every == 0)))
            self._after_step()

    def op_run(self, cnt):
        k = int(self.rng.integers(5, 20)); every = int(self.rng.choice([0, 7])); first = bool(self.rng.integers(0, 2))
        self._run(k, every, first)
        self.log.append("run %d every %d first %s" % (k, every, first))

    def op_module(self, cnt):
        st = self.st
        if st is not None:
            st.grid.update(); st.collision_system.solve_collisions(); st.particles.update_positions(DT)
        self.model.module_calls(DT)
        self.log.append("module calls")

    def op_resort(self, cnt):
        if self.st is not None:
            self.st.particles.sort_by_cell_id()
        self.model.morton_resort()
        self._stale("resort")
        self.log.append("morton resort")

    def op_mouse(self, cnt):
        rng, world = self.rng, self.world
        pressed = bool(rng.integers(0, 2))
        at = (float(F32(rng.random() * world[0])), float(F32(rng.random() * world[1])))
        if self.st is not None:
            self.st.particles.mouse_click_callback(pressed, at)
        self.model.set_mouse(pressed, *at)
        self.log.append("mouse %s %s" % (pressed, at))

    def op_gravity(self, cnt):
        g = (float(self.rng.choice([0.0, 3.0, -3.0])), float(self.rng.choice([0.0, -9.81, 9.81])))
        if self.st is not None:
            self.st.ctx.call("gpe_set_gravity", g[0], g[1])
        self.model.set_gravity(*g)
        self.log.append("gravity %s" % (g,))

    # particles come and go
    def op_add(self, cnt):
        rng = self.rng
        m = int(rng.integers(1, 300)); big = bool(rng.integers(0, 3) == 0)
        p_new = _inside((rng.random((m, 2), dtype=F32) * np.array(self.world, F32)).astype(F32), self.world, 2.0)
        r_new = rng.choice(np.array((0.5, 1.0, 1.5) if big else (0.5,), F32), m).astype(F32)
        if self.st is not None:
            self.st.add_particles(p_new, r_new)
        self.model.add(p_new, r_new)
        self._stale("add")
        if self._grow(cnt + m):
            self.cov["add_grew"] += 1
        self.log.append("add %d%s%s" % (m, " mixed radii" if big else "", " (grew to %d)" % self.cap if self.grew else ""))

    def op_add_free(self, cnt):
        rng, model = self.rng, self.model
        sep, inw, dry = self.plan.spawn_flags[self.spawn_calls % len(self.plan.spawn_flags)]
        self.spawn_calls += 1
        cpos, crad = _spawn_model.reference_spray(rng, self._a_particle(), int(rng.integers(120, 320)))
        # (a few candidates of the particles' own size, near the point: rows with room inside the cloud)
        near = int(rng.integers(20, 60))
        cpos = np.concatenate([cpos, (self._a_particle() + rng.uniform(-12.0, 12.0, (near, 2))).astype(F32)])
        crad = np.concatenate([crad, np.full(near, 0.5, F32)])
        if self.st is not None:
            before = self._counters()
            added, verdict = self.st.add_particles_free(cpos, crad, separate=bool(sep), inside_world=bool(inw),
                                                        dry_run=bool(dry))
        want_verdict, want_added = model.add_free(cpos, crad, separate=bool(sep), inside_world=bool(inw), dry_run=bool(dry))
        what = "add_free %d candidates, flags %d%d%d" % (len(crad), sep, inw, dry)
        if self.st is not None:
            assert added == want_added, "%s: added %d, model %d\n%s" % (what, added, want_added, "\n".join(self.log))
            assert np.array_equal(verdict, want_verdict), "%s: %d verdicts differ" % (what, int((verdict != want_verdict).sum()))
            if dry or want_added == 0:
                self._frozen(before, what)
        for v, name in ((_spawn_model.ADDED, "added"), (_spawn_model.BLOCKED_BY_PARTICLE, "blocked_by_particle"),
                        (_spawn_model.BLOCKED_BY_CANDIDATE, "blocked_by_candidate"),
                        (_spawn_model.OUTSIDE_WORLD, "outside_world")):
            self.cov["verdict_" + name] += int((want_verdict == v).sum())
        self.grew = False
        if dry:
            self.cov["dry_runs"] += 1
        elif want_added:
            self.cov["add_free_appended"] += 1
            self._stale("add")
            if self._grow(cnt + want_added):
                self.cov["add_free_grew"] += 1
        self.log.append("%s: %d added%s, verdicts %s" % (what, want_added, " (grew to %d)" % self.cap if self.grew else "",
                                                       np.bincount(want_verdict, minlength=4).tolist()))

    def _removed(self, got, want, what):
        if got is not None:
            assert got == want, "%s: removed %d, model %d\n  %s" % (what, got, want, "\n  ".join(self.log))
        if want:
            self._stale("removal")
        self.log.append("%s: %d" % (what, want))

    def op_remove_mask(self, cnt):
        rng = self.rng
        mask = (rng.random(cnt) < rng.choice([0.001, 0.02, 0.1])).astype(np.uint8)
        mask[int(rng.integers(0, cnt))] = 1                      # (at least one leaves)
        if mask.all():
            mask[0] = 0
        got = self.st.remove_particles(mask) if self.st is not None else None
        self._removed(got, self.model.remove_mask(mask), "remove mask")

    def op_remove_circle(self, cnt):
        c = self._a_particle()                                   # (its own centre: at least one leaves)
        c = (float(c[0]), float(c[1]))
        r = float(F32(self.rng.random() * 0.1 * min(self.world0)))
        if circle_mask(self.model.arrays()[0], c[0], c[1], r).all():
            r = 0.0
        got = self.st.remove_particles_in_circle(c, r) if self.st is not None else None
        self._removed(got, self.model.remove_circle(c[0], c[1], r), "remove circle %s r %g" % (c, r))

    def op_remove_uid(self, cnt):
        self._uids_on()
        model = self.model
        q = self.rng.choice(np.append(model.uids, [model.next_uid, 0xFFFFFFFE]).astype(np.uint32),
                            size=int(self.rng.integers(1, max(2, cnt // 20))))
        if np.isin(model.uids, q).all():
            q = q[:0]
        got = self.st.remove_particles_by_uid(q) if self.st is not None else None
        self._lookup_by_uid(counts=False)
        self._removed(got, model.remove_uids(q), "remove %d uids" % len(q))

    # uids
    def op_uids_on(self, cnt):
        self._uids_on()

    def _uids(self, on):
        if self.st is not None:
            self.st.enable_uids(on)
        was = self.model.uids is not None
        self.model.enable_uids(on)
        self.map_stale = False
        if on and not was:
            self._stale("uids_on")
        self.log.append("uids %s" % ("on" if on else "off"))

    def op_uids_toggle(self, cnt):
        self._uids(self.model.uids is None)

    def op_uids_cycle(self, cnt):
        """Off (when they are on; compared there too), then on again."""
        if self.model.uids is not None:
            self._uids(False)
            if self.st is not None:
                self.compare(self.st, self.model, "uids off\n  " + "\n  ".join(self.log))
        self._uids(True)

    def op_uids_set(self, cnt):
        model = self.model
        u = self.rng.choice(3 * cnt + 10, size=cnt, replace=False).astype(np.uint32)
        if self.st is not None:
            self.st.set_uids(u)
        model.set_uids(u)
        nxt = model.next_uid + int(self.rng.integers(0, 1000))
        if self.st is not None:
            self.st.set_next_uid(nxt)
        model.set_next_uid(nxt)
        self.map_stale = False                                   # gpe_set_uids leaves the map it checked them with
        self.log.append("set uids, next %d" % nxt)

    # world and grid
    def _world(self, op, w):
        if self.st is not None:
            self.st.ctx.call("gpe_set_world", w[0], w[1])
        self.model.set_world(*w)
        self.world = w
        self.log.append("%s %s" % (op, w))
        if self.st is not None:
            info = self.st.ctx.pipeline_info()
            self.log[-1] += ": pipeline %d reason %d" % (info["pipeline"], info["reason"])
            return info

    def op_world_grow(self, cnt):
        f = float(self.rng.choice([6.0, 12.0, 25.0]))            # past the allocated block table, lists and rosters
        self._world("world_grow", (float(F32(self.world0[0] * f)), float(F32(self.world0[1] * f))))

    def op_world_shrink_in(self, cnt):
        p = self.model.arrays()[0]                               # every particle stays inside [0, world]
        self._world("world_shrink_in", (float(F32(max(p[:, 0].max(), 1.0) + 0.25)), float(F32(max(p[:, 1].max(), 1.0) + 0.25))))

    def op_world_shrink_out(self, cnt):
        w = (float(F32(self.world0[0] * 0.7)), float(F32(self.world0[1] * 0.75)))
        info = self._world("world_shrink_out", w)                # some are left outside: the next integration clamps them
        p = self.model.arrays()[0]
        self.outside = int(((p[:, 0] > F32(w[0])) | (p[:, 1] > F32(w[1]))).sum())
        if info is not None and self.mode == self.L.MODE_NATIVE and self.outside:
            assert info["reason"] == self.L.REASON_OUT_OF_BOX, (info, self.log)

    def op_world_back(self, cnt):
        self._world("world_back", self.world0)

    def _grid(self, op, f):
        r = float(F32(self.model.max_radius) * F32(f))
        if self.st is not None:
            self.st.ctx.call("gpe_grid_set_max_radius", r)
        self.model.grid_set_max_radius(r)
        self.log.append("%s %g" % (op, r))

    def op_grid_under(self, cnt):
        # understated only down to 0.92: below 1 / 1.1 a particle can sit in two cells of one colour, and the colour
        # passes race on it (tests/test_gpu_api_sequences.py, test_understated_grid_radius_*)
        self._grid("grid_under", self.rng.uniform(0.92, 0.99))

    def op_grid_over(self, cnt):
        self._grid("grid_over", self.rng.uniform(1.5, 3.0))

    def op_grid_exact(self, cnt):
        self._grid("grid_exact", 1.0)

    def op_set_mode(self, cnt):
        """A spell in the other mode, with a contact and a cluster search in its middle."""
        k = int(self.rng.integers(1, 4))
        if self.st is not None:
            self.st.ctx.call("gpe_set_mode", self.other)
        for _ in range(k):
            self._step()
        self.log.append("mode -> other, %d steps" % k)
        self.op_contacts(len(self.model)); self.op_clusters(len(self.model))
        self.cov["contacts_other_mode"] += 1
        self._observe("other_mode")
        self._step()
        if self.st is not None:
            self.st.ctx.call("gpe_set_mode", self.mode)
        self.log.append("mode back")

    # writes through gpe_device_ptr
    def op_stop(self, cnt):
        now = np.ascontiguousarray(self.model.arrays()[0])
        if self.st is not None:
            self._upload(self.L.PREV, now)
        self.model.stop_all()
        self.log.append("prev = pos")

    def op_teleport(self, cnt):
        rng, world = self.rng, self.world
        who = rng.choice(cnt, size=max(1, cnt // 10), replace=False)
        where = _inside(rng.random((len(who), 2), dtype=F32) * np.array(world, F32), world, 2.0)
        self.model.teleport(who, where)
        if self.st is not None:
            p, q, _ = self.model.arrays()
            self._upload(self.L.POS, np.ascontiguousarray(p)); self._upload(self.L.PREV, np.ascontiguousarray(q))
        self.log.append("teleport %d" % len(who))

    def op_save_load(self, cnt):
        self._observe("before_save")
        if self.last in ("edit_index", "edit_uid"):
            self.cov["save_load_after_edit"] += 1
        if self.last == "add_free":
            self.cov["save_load_after_add_free"] += 1
        if self.st is not None:
            path = os.path.join(self.tmp.name, "snap_%d.npz" % len(self.log))
            self.st.save(path)
            self.retire()
            self.st.close()
            self.st = self.gpe.State.load(path, mode=self.mode)
        self.cap = cnt                                           # gpe_set_particles: exactly what it was given
        self.map_stale = False                                   # (gpe_set_uids, when the snapshot has uids)
        self.log.append("save / load")
        self._observe("after_load")

    # keyed edits
    def _edit(self, keys, by, fields, pos=None, prev=None, radius=None, what="edit"):
        model = self.model
        k = len(keys)
        rng = self.rng
        if pos is None and "pos" in fields:
            pos = _inside(rng.random((k, 2), dtype=F32) * np.array(self.world, F32), self.world, 2.0)
        if prev is None and "prev" in fields:
            at = pos if pos is not None else self._rows_of(keys, by)
            prev = (at + rng.uniform(-0.05, 0.05, (k, 2)).astype(F32)).astype(F32)
        if radius is None and "radius" in fields:
            radius = rng.choice(np.array([0.4, 0.5, 0.6, 1.0], F32), k).astype(F32)
        got = None
        if self.st is not None:
            kw = {"indices" if by == "index" else "uids": keys}
            got = self.st.edit_particles(positions=pos, previous=prev, radii=radius, **kw)
        want = model.edit(keys, by, pos=pos, prev=prev, radius=radius)
        if got is not None:
            assert got == want, "%s: edited %d, model %d\n  %s" % (what, got, want, "\n  ".join(self.log))
        if by == "uid":
            self._lookup_by_uid()
            if want < k:
                self.cov["uid_edits_skipping_absent"] += 1
        if want:
            self.cov["keyed_edits_written"] += 1
        self.cov["edit_fields_" + "_".join(fields)] += 1
        self.log.append("%s by %s: %d keys, %s, %d written" % (what, by, k, "+".join(fields), want))
        return want

    def _rows_of(self, keys, by):
        """The current positions of the particles the keys name (an absent uid: a point inside the world)."""
        p = self.model.arrays()[0]
        if by == "index":
            return p[np.asarray(keys, np.int64)]
        out = np.full((len(keys), 2), 3.0, F32)
        for j, u in enumerate(keys):
            at = np.nonzero(self.model.uids == u)[0]
            if at.size:
                out[j] = p[at[0]]
        return out

    def _fields(self):
        self.edits += 1
        return FIELD_SUBSETS[self.edits % len(FIELD_SUBSETS)]

    def op_edit_index(self, cnt):
        k = int(self.rng.integers(1, max(2, cnt // 10) + 1))
        keys = self.rng.choice(cnt, size=k, replace=False).astype(np.uint32)
        self._edit(keys, "index", self._fields())

    def op_edit_uid(self, cnt):
        self._uids_on()
        model, rng = self.model, self.rng
        k = int(rng.integers(1, max(2, cnt // 10) + 1))
        present = rng.choice(model.uids, size=k, replace=False)
        absent = np.unique(np.array([u for u in (model.next_uid, model.next_uid + 5, 0xFFFFFFFE, 0xFFFFFFF0)
                                     if u < (1 << 32)], np.uint64).astype(np.uint32))
        absent = absent[~np.isin(absent, model.uids)][:int(rng.integers(1, 4))]
        keys = rng.permutation(np.concatenate([present, absent]).astype(np.uint32))
        self._edit(keys, "uid", self._fields())

    def op_edit_pos_override(self, cnt):
        """radius NULL: a pending gpe_grid_set_max_radius override stays (the comparison after the call checks it)."""
        self._grid("grid_over", self.rng.uniform(1.5, 3.0))
        keys = self.rng.choice(cnt, size=int(self.rng.integers(1, 40)), replace=False).astype(np.uint32)
        self._edit(keys, "index", ("pos",), what="edit under an override")
        assert self.model.grid_max_radius != self.model.max_radius
        self.cov["pos_edit_keeps_override"] += 1

    def _radius_edit(self, up, override):
        model = self.model
        if override:
            self._grid("grid_over", self.rng.uniform(1.5, 3.0))
        r = model.arrays()[2]
        if up:                                                   # a new largest radius, on any particle
            who = int(self.rng.integers(0, len(r)))
            new = F32(F32(model.max_radius) * F32(1.2))
        else:                                                    # the largest particle (the last of them) shrinks
            who = int(np.nonzero(np.abs(r) == abs(model.max_radius))[0][-1])
            new = F32(F32(model.max_radius) * F32(0.8))
        self._edit(np.array([who], np.uint32), "index", ("radius",), radius=np.array([new], F32),
                   what="radius %s%s" % ("up" if up else "down", " under an override" if override else ""))
        assert model.grid_max_radius == model.max_radius         # radius non-NULL: the grid radius follows
        if override:
            self.cov["radius_%s_with_override" % ("up" if up else "down")] += 1

    def op_edit_radius_up(self, cnt):
        self._radius_edit(True, False)

    def op_edit_radius_up_override(self, cnt):
        self._radius_edit(True, True)

    def op_edit_radius_down(self, cnt):
        self._radius_edit(False, False)

    def op_edit_radius_down_override(self, cnt):
        self._radius_edit(False, True)

    def _expect(self, pipeline, reason, what):
        if self.st is not None and self.mode == self.L.MODE_NATIVE:
            info = self.st.ctx.pipeline_info()
            want = (getattr(self.L, pipeline), getattr(self.L, reason))
            assert (info["pipeline"], info["reason"]) == want, "%s: %r, expected %s %s\n  %s" % (
                what, info, pipeline, reason, "\n  ".join(self.log))

    def op_edit_outside_and_back(self, cnt):
        """A step (its wall clamp brings every particle inside), a few particles moved well outside [0, world]:
        GPE_REASON_OUT_OF_BOX; a step; moved back to where they were: the NATIVE kernels again."""
        self._step()
        model, rng = self.model, self.rng
        who = rng.choice(cnt, size=int(rng.integers(2, 6)), replace=False).astype(np.uint32)
        home = model.arrays()[0][who].copy()
        far = F32(3.0) * F32(abs(model.cell_size)) + F32(2.0)
        away = home.copy()
        away[::2, 0] = -far                                      # to the left of the box, and beyond its far corner
        away[1::2] = np.array(self.world, F32) + far
        self._edit(who, "index", ("pos",), pos=away, what="edit outside")
        self._expect("PIPELINE_COMPAT", "REASON_OUT_OF_BOX", "particles moved outside")
        self._step()
        if self.st is not None:
            self.compare(self.st, model, "the step with particles outside\n  " + "\n  ".join(self.log))
        self._observe("edited_outside")
        self._edit(who, "index", ("pos",), pos=home, what="edit back")
        self._expect("PIPELINE_NATIVE", "REASON_NONE", "particles moved back")
        self._step()
        self._expect("PIPELINE_NATIVE", "REASON_NONE", "the step after the particles moved back")
        self.cov["edit_outside_and_back"] += 1

    # kicks
    def _kick(self, box, count):
        model, rng = self.model, self.rng
        self._step(); self._step()                               # (so that the kick falls between steps of one run)
        self.kicks += 1
        op = (VEL_ADD, VEL_SET, VEL_SCALE)[self.kicks % 3]
        lim = {VEL_ADD: 3.0, VEL_SET: 1.0, VEL_SCALE: 1.5}[op]
        a = (float(F32(rng.uniform(-lim, lim))), float(F32(rng.uniform(-lim, lim))))
        c = self._a_particle()
        pos = model.arrays()[0]
        if box:
            h = rng.uniform(3.0, 20.0, 2)
            region = (float(F32(c[0] - h[0])), float(F32(c[1] - h[1])), float(F32(c[0] + h[0])), float(F32(c[1] + h[1])))
            mask = box_mask(pos, *region)
        else:
            region = (float(c[0]), float(c[1]), float(F32(rng.uniform(2.0, 15.0))))
            mask = circle_mask(pos, *region)
        got = None
        if self.st is not None:
            before = self._counters()
            if box:
                got = self.st.kick_box(region[:2], region[2:], op, a, count=count)
            else:
                got = self.st.kick_circle(region[:2], region[2], op, a, count=count)
        want = model.kick(mask, op, *a)
        self._observe("after_kick")
        what = "kick %s %s op %d a %s" % ("box" if box else "circle", region, op, a)
        if count:
            if self.st is not None:
                assert got == want, "%s: kicked %d, model %d\n  %s" % (what, got, want, "\n  ".join(self.log))
                self._frozen(before, what)
        else:                                                    # stream-ordered: the step follows with no sync between
            assert got is None
            self._step()
            if self.st is not None:
                after = self._counters()
                assert after["native_steps"] + after["compat_steps"] == before["native_steps"] + before["compat_steps"] + 1
            what += ", then a step"
        if want:
            self.cov["kicks_nonzero"] += 1
        self.cov["kick_op_%d" % op] += 1
        self.log.append("%s: %d kicked" % (what, want))

    def op_kick_circle(self, cnt):
        self._kick(False, True)

    def op_kick_circle_nosync(self, cnt):
        self._kick(False, False)

    def op_kick_box(self, cnt):
        self._kick(True, True)

    def op_kick_box_nosync(self, cnt):
        self._kick(True, False)

    # read-only queries
    def op_query_circle(self, cnt):
        c = self._a_particle()
        args = (float(c[0]), float(c[1]), float(F32(self.rng.uniform(0.5, 12.0))))
        want = self.model.query_circle(*args)
        k = len(want.index)
        cap = int(self.rng.choice([0, max(k - 1, 0), k, k + 5]))
        if self.st is not None:
            self._rows_call("gpe_query_circle", args, cap, want, "query_circle %s capacity %d" % (args, cap))
        assert k > 0
        self.log.append("query circle %s capacity %d: %d" % (args, cap, k))

    def op_query_box(self, cnt):
        c, h = self._a_particle(), self.rng.uniform(0.0, 15.0, 2)
        args = (float(F32(c[0] - h[0])), float(F32(c[1] - h[1])), float(F32(c[0] + h[0])), float(F32(c[1] + h[1])))
        want = self.model.query_box(*args)
        k = len(want.index)
        cap = int(self.rng.choice([0, max(k - 1, 0), k, k + 5]))
        if self.st is not None:
            self._rows_call("gpe_query_box", args, cap, want, "query_box %s capacity %d" % (args, cap))
        assert k > 0
        self.log.append("query box %s capacity %d: %d" % (args, cap, k))

    def op_pick(self, cnt):
        """A particle's own centre (a hit), then a point up to 0.7 beside it (a hit or a miss)."""
        c = self._a_particle()
        for at in ((float(c[0]), float(c[1])),
                   (float(F32(c[0] + self.rng.uniform(-0.7, 0.7))), float(F32(c[1] + self.rng.uniform(-0.7, 0.7))))):
            want = self.model.pick(*at)
            rows = want if want is not None else self.model.rows([])
            if self.st is not None:
                self._rows_call("gpe_pick", at, 1, rows, "pick %s" % (at,))
            if want is not None:
                self.cov["picks_hit"] += 1
            self.log.append("pick %s: %s" % (at, None if want is None else int(want.index[0])))

    def op_contacts(self, cnt):
        """gpe_query_contacts with a capacity below, at or above the count, the count alone and the degrees alone."""
        want = self.model.contacts()
        k = want.count
        cap = int(self.rng.choice([0, 1, max(k - 1, 0), k, k + 7]))
        if self.st is not None:
            self._contacts_call(cap, want, "contacts capacity %d" % cap)
            before = self._counters()
            assert self.st.count_contacts() == k
            assert np.array_equal(self.st.contact_degrees(), want.degree)
            self._frozen(before, "count_contacts / contact_degrees")
        if k:
            self.cov["contacts_nonzero"] += 1
        if self.last == "add" and self.grew:
            self.cov["contacts_after_growth"] += 1
        if self.last == "world_shrink_out" and self.outside:
            self.cov["contacts_outside_world"] += 1
        self.log.append("contacts capacity %d: %d" % (cap, k))

    def op_clusters(self, cnt):
        want = self.model.clusters()
        if self.st is not None:
            before = self._counters()
            got = self.st.clusters()
            assert self.st.count_clusters() == want.count
            self._frozen(before, "clusters / count_clusters")
            assert np.array_equal(got.label, want.label), "cluster labels differ"
            assert np.array_equal(got.size, want.size), "cluster sizes differ"
            assert (got.label_uid is None) == (want.label_uid is None)
            if want.label_uid is not None:
                assert np.array_equal(got.label_uid, want.label_uid), "cluster label uids differ"
            assert (got.count, got.largest_size, got.largest_label) == (want.count, want.largest_size, want.largest_label)
        if want.largest_size >= 3:
            self.cov["clusters_of_3_or_more"] += 1
        self.log.append("clusters: %d, largest %d at %d" % (want.count, want.largest_size, want.largest_label))

    def _cluster_of(self, by_uid):
        model, rng = self.model, self.rng
        label = model.clusters().label
        # a particle of the largest cluster, a random one, and (by uid) one that is absent
        keys = [int(rng.choice(np.nonzero(label == model.clusters().largest_label)[0])), int(rng.integers(0, len(model)))]
        for j, index in enumerate(keys):
            if by_uid:
                key = {"uid": int(model.uids[index])}
                kind = self.L.CLUSTER_BY_UID if self.L else 1
            else:
                key = {"index": index}
                kind = self.L.CLUSTER_BY_INDEX if self.L else 0
            want = model.cluster_of(label=label, **key)
            k = len(want.index)
            cap = int(rng.choice([max(k - 1, 0), k + 3] if j == 0 else [0, k, k + 3]))
            if self.st is not None:
                self._rows_call("gpe_query_cluster_of", (kind, list(key.values())[0]), cap, want,
                                "cluster_of %s capacity %d" % (key, cap))
            if by_uid:
                self._lookup_by_uid()
            if k >= 3:
                self.cov["clusters_of_3_or_more"] += 1
            self.log.append("cluster_of %s capacity %d: %d" % (key, cap, k))
        if by_uid:
            absent = model.next_uid if model.next_uid < (1 << 32) else None
            if absent is not None and self.st is not None:
                self._rows_call("gpe_query_cluster_of", (kind, absent), 4, model.rows([]), "cluster_of an absent uid")

    def op_cluster_of_index(self, cnt):
        self._cluster_of(False)

    def op_cluster_of_uid(self, cnt):
        self._uids_on()
        self._cluster_of(True)


# ------------------------------------------------------------------------------------------------------------------------
# Observed sequences: the same plans with the two recorders armed and the late queries between the calls
# ------------------------------------------------------------------------------------------------------------------------
TRACER_K = (1, 7, 64, 300)
EVERY = (1, 2, 3)
FRAMES = (4, 16, 64)
TRACER_FIELDS = (1, 2, 3, 4, 5, 6, 7)          # every combination of GPE_TRACER_POS | PREV | INDEX
RAY_K = (1, 3, 65)
NEAREST_K = (1, 3, 65)
NEAREST_M = (1, 5, 64)
CAPACITY_CLASSES = ("below", "at", "above")
CYCLES = 4                                     # recordings per sequence: each k, every and frames is used in every seed
FAR_UID = 0xFFFFFFF0
SENTINEL64 = 0xA5A5A5A5A5A5A5A5
KICKS = ("kick_circle", "kick_circle_nosync", "kick_box", "kick_box_nosync")
REMOVALS = ("remove_mask", "remove_circle", "remove_uid", "remove_tracked_uid")
# the existing operations that change nothing: the one before them is still "the last thing that happened"
READ_ONLY = ("contacts", "clusters", "cluster_of_uid", "cluster_of_index", "query_circle", "query_box", "pick")
# what can leave the tracers' slot table stale: a frame (tracers_sample, or the steps of obs_step) and a read follow
STALE_MAKERS = ("resort", "run", "remove_mask", "remove_circle", "remove_uid", "add", "add_free", "uids_set", "uids_cycle",
                "uids_toggle")
# the recorders look at the State after these (they are armed all along, so there are frames from before; a kick is
# looked at from inside as well, before the step that may follow it unsynchronised)
ACROSS = ("set_mode", "world_shrink_out", "teleport", "stop", "edit_outside_and_back") + KICKS
CHANGING = ("obs_step", "obs_run_resort", "obs_wrap", "obs_kick", "remove_tracked_uid")     # (of OBSERVING: these do change the particles)
QUERIES = ["cast_rays", "query_segment", "nearest"]
QUERIES_AFTER = ("edit_radius_up_override", "edit_radius_down", "grid_under", "remove_mask", "remove_circle")
LOOK = ["tracers_sample", "monitor_sample", "tracers_read", "monitor_read"]
BEGIN = ["tracers_begin", "monitor_begin", "obs_wrap", "tracers_read", "monitor_read"]
END = ["tracers_read", "monitor_read", "tracers_end", "monitor_end"]
OBSERVING = frozenset(
    ["tracers_begin", "tracers_sample", "tracers_read", "tracers_read_consume", "tracers_end", "monitor_begin",
     "monitor_sample", "monitor_read", "monitor_read_consume", "monitor_end", "measure", "cast_rays", "query_segment",
     "nearest", "tracers_begin_armed", "tracers_begin_uids_off", "obs_step", "obs_run_resort", "obs_wrap", "obs_kick",
     "remove_tracked_uid"])
TRACER_PINS = ("resort", "run_resort", "remove_mask", "remove_circle", "remove_uid_tracked", "add", "add_free_appended",
               "uids_set", "uids_cycle")
ACROSS_PINS = ("growth", "set_mode", "world_shrink_out", "teleport", "stop", "edit_outside_and_back", "kick")
QUERY_PINS = ("growth", "world_shrink_out", "other_mode", "radius_up_override", "radius_down", "grid_under", "removal")


def plan_observed(seed):
    """plan(seed) with the observing operations inserted: the scene, the flags and -- once the names in OBSERVING are
    taken out -- the operations are plan(seed)'s.  Where things go is decided here, by a generator of its own; what the
    new operations draw when they run comes from ObservedSequence.rng2.

    Both recorders are armed before the first operation and stay armed: CYCLES recordings, the second begun straight
    before the add that grows the buffers (with a tracked uid that this add hands out), the others at drawn block
    boundaries; each begin is followed by obs_wrap (frames taken until both rings have wrapped, where the ring has 4
    frames) and a read.  A frame and a tracers_read follow everything in STALE_MAKERS (the frame comes from a step
    instead of tracers_sample at some of those that end their block); LOOK follows everything in ACROSS; QUERIES follow
    the growth and world_shrink_out (before or after the block's own contact search, by the seed's parity) and
    everything in QUERIES_AFTER, and run inside set_mode's spell in the other mode.  Placed at drawn block boundaries: a
    run that re-sorts, the removal of a tracked uid, a kick of particles at rest (obs_kick), a consuming read with a
    frame and a read behind it (both recorders), the two refused begins, and three measures."""
    base, blocks = _plan_and_blocks(seed)
    pick = np.random.default_rng(9300 + seed)
    grow = next(i for i, b in enumerate(blocks) if b == ["add", "contacts", "clusters"])
    inner = [i for i in range(1, len(blocks)) if i != grow]
    rearm = sorted(int(i) for i in pick.choice(inner, size=CYCLES - 1 - (grow != 0), replace=False))
    cycle_at = sorted(set([0, grow] + rearm))                     # (cycle c begins before block cycle_at[c])
    # the tracked uid to remove: in a recording that follows more than one (k = 1 may track nobody who is there)
    late = [c for c in range(len(cycle_at)) if c >= 2 and TRACER_K[(seed + c) % len(TRACER_K)] != 1]
    before = collections.defaultdict(list)
    before[cycle_at[late[0]]] += ["remove_tracked_uid", "tracers_sample", "tracers_read"] + QUERIES
    extras = [["obs_run_resort", "tracers_read", "monitor_read"], ["obs_kick", "tracers_read", "monitor_read"],
              ["tracers_read_consume", "tracers_sample", "tracers_read", "monitor_read_consume", "monitor_sample",
               "monitor_read"],
              ["tracers_begin_armed"], ["tracers_begin_uids_off"], ["measure"], ["measure"], ["measure"]]
    for ops, at in zip(extras, pick.choice(inner, size=len(extras))):
        before[int(at)] += ops
    out = []
    for bi, block in enumerate(blocks):
        if bi in cycle_at:
            out += (END if bi else []) + BEGIN
            if bi == grow:
                out += ["tracers_sample"]                           # (a frame in which the add's uids are absent)
        out += before[bi]
        first = seed % 2 == 1                                       # the new queries before the block's contact search
        for j, op in enumerate(block):
            out.append(op)
            if op in STALE_MAKERS:
                by_step = j == len(block) - 1 and bool(pick.integers(0, 2))
                out += ["obs_step" if by_step else "tracers_sample", "tracers_read"]
            if bi == grow and op == "add":
                out += ["monitor_sample", "monitor_read"] + (QUERIES if first else [])
            if op == "world_shrink_out":
                out += LOOK + ([] if first else QUERIES)
            if op in ACROSS and op != "world_shrink_out":
                out += LOOK
            if op in QUERIES_AFTER:
                out += QUERIES
        if bi == grow and not first:
            out += QUERIES
        if block[0] == "world_shrink_out" and first:
            out += QUERIES
    out += END
    assert [op for op in out if op not in OBSERVING] == base.ops
    return base._replace(ops=out)


def _key(t, index):
    return (np.ascontiguousarray(t, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)


class ObservedSequence(Sequence):
    """A Sequence that can run plan_observed(seed): the operations in OBSERVING, and what the hooks of the existing
    operations do while a recorder is armed.  Every draw of the new operations comes from rng2; which k, every, frames,
    fields, capacity class and flag a call uses rotates with the seed and a counter, so that each is used."""

    def __init__(self, plan_, oracle, **kw):
        super().__init__(plan_, oracle, **kw)
        self.rng2 = np.random.default_rng(9400 + plan_.seed)
        self.tcfg = self.mcfg = None                   # the configuration of the armed recorders
        self.cycle = -1                                # recordings begun so far - 1
        self.t_mark = self.m_mark = 0                  # `recorded` at the begin or at the last consuming read
        self.t_chain = self.m_chain = 0                # consuming read (1), then a frame (2), then a read
        self.reads = self.casts = self.segments = self.nearests = plan_.seed
        self.gone = set()                              # uids that left during the sequence
        self.after = None                              # the last operation that changed the particles or the context
        self.t_stale = self.t_followed = None          # what left the slot table stale; ... and a frame has followed
        self.last_cast = None                          # (origins, ends, hits of the model) while nothing has changed
        self.prev_op = self.cur_op = None
        self.i = 0
        self.events = 0                                # how often something has left the slot table stale
        self.removed_any = False
        self.saved = (None, None)

    # ---- plumbing -----------------------------------------------------------------------------------------------------
    def apply(self, i, op):
        model = self.model
        uids_before = None if model.uids is None else model.uids.copy()
        n_before, events = len(model), self.events
        changing = (op not in OBSERVING or op in CHANGING) and op not in READ_ONLY
        if changing:
            self.last_cast = self.t_followed = None
        self.i, self.cur_op = i, op
        try:
            super().apply(i, op)
        except AssertionError as e:                    # (the calls so far, with whatever failed inside the operation)
            if "op #%d" % i in str(e):
                raise
            raise AssertionError("%s\n%s" % (e, self.where(i, op))) from None
        self.prev_op = op
        if not changing:
            return
        self.after = op
        because = op
        if op in REMOVALS:
            self.removed_any = len(model) < n_before
            if uids_before is not None and model.uids is not None:
                left = np.setdiff1d(uids_before, model.uids)
                self.gone.update(int(u) for u in left)
                if op in ("remove_uid", "remove_tracked_uid") and self.tcfg is not None and np.isin(left, self.tcfg["uids"]).any():
                    because = "remove_uid_tracked"
        if self.events > events or op in ("uids_set", "uids_cycle", "uids_toggle"):
            self.t_stale = {"run": "run_resort", "obs_run_resort": "run_resort", "add_free": "add_free_appended"}.get(
                because, because)

    def _stale(self, because):
        super()._stale(because)
        self.events += 1                               # (the library's slot table is stale with uids off as well)
        if self.cur_op in ("run", "obs_run_resort"):
            self.t_stale = "run_resort"                # (the frames taken inside the run are the ones that follow)

    def _status(self, name, *args):
        return getattr(self.st.ctx.lib, name)(self.st.ctx.h, *args)

    def _now(self):
        """The model's pos, prev, radius without closing its Sim."""
        m = self.model
        return (m._sim.pos, m._sim.prev, m._sim.radius) if m._sim is not None else (m.pos, m.prev, m.radius)

    def _class(self, counter, count, least=0):
        """A capacity below, at or above `count`, by rotation -> (capacity, its class as it turned out).  least = 1: a
        read of a ring that holds something delivers at least its newest frame, so that this frame is compared."""
        want = CAPACITY_CLASSES[counter % 3]
        cap = {"below": max(count - 1, min(least, count)), "at": count, "above": count + 3}[want]
        return cap, "below" if cap < count else "at" if cap == count else "above"

    # ---- tracers ------------------------------------------------------------------------------------------------------
    def _tracked(self, k):
        """k distinct uids: live ones, ones that left earlier, ones at or above next_uid, one far above."""
        model, rng = self.model, self.rng2
        live, nxt = model.uids, int(model.next_uid)
        gone = np.array(sorted(u for u in self.gone if u < nxt), np.uint32)
        gone = gone[~np.isin(gone, live)]
        future = np.arange(nxt, min(nxt + 2, FAR_UID), dtype=np.uint64).astype(np.uint32)
        far = np.array([FAR_UID], np.uint32)
        upcoming = [op for op in self.plan.ops[self.i + 1:] if op not in OBSERVING][:1]
        if k == 1:
            kind = "future" if upcoming == ["add"] else ("live", "gone", "future", "far")[self.cycle % 4]
            pool = {"live": live, "gone": gone if len(gone) else live, "future": future, "far": far}[kind]
            return rng.choice(pool, size=1).astype(np.uint32)
        take_gone = gone[rng.permutation(len(gone))[:max(1, k // 6)]]
        rest = k - len(take_gone) - len(future) - 1
        assert rest <= len(live), (k, len(live))
        picked = np.concatenate([rng.choice(live, size=rest, replace=False), take_gone, future, far]).astype(np.uint32)
        assert len(np.unique(picked)) == k
        return rng.permutation(picked)

    def _tracers_cfg(self, cfg):
        L = self.L
        c = L.GpeTracerConfig(struct_size=C.sizeof(L.GpeTracerConfig), fields=cfg["fields"], k=len(cfg["uids"]),
                              every=cfg["every"], frames=cfg["frames"])
        c.uids = cfg["uids"].ctypes.data_as(C.POINTER(C.c_uint32))
        return c

    def _tracers_arm(self, cfg):
        from tests import _tracers_model
        self._uids_on()
        if self.st is not None:
            self.st.ctx.call("gpe_tracers_begin", C.byref(self._tracers_cfg(cfg)))
        self.tcfg, self.tm = cfg, _tracers_model.TracerModel(self.model, cfg["uids"], every=cfg["every"], frames=cfg["frames"])
        self.t_mark = self.t_chain = 0
        self.t_stale = None                                      # (gpe_tracers_begin leaves the table to the first frame)
        self.log.append("tracers begin: k %d every %d frames %d fields %d" % (
            len(cfg["uids"]), cfg["every"], cfg["frames"], cfg["fields"]))

    def _tracers_disarm(self):
        if self.st is not None:
            self.st.ctx.call("gpe_tracers_end")
        self.tm = None
        self.log.append("tracers end")

    def op_tracers_begin(self, cnt):
        self.cycle += 1
        seed, c = self.plan.seed, self.cycle
        self._uids_on()
        k = TRACER_K[(seed + c) % len(TRACER_K)]
        cfg = dict(uids=np.ascontiguousarray(self._tracked(k)), every=EVERY[(seed + c) % 3], frames=FRAMES[(seed + 2 * c) % 3],
                   fields=TRACER_FIELDS[(CYCLES * seed + c) % len(TRACER_FIELDS)])
        cfg["future"] = cfg["uids"] >= np.uint32(min(int(self.model.next_uid), 0xFFFFFFFF))
        self._tracers_arm(cfg)
        for what in ("k", "every", "frames", "fields"):
            self.cov["tracer_%s_%d" % (what, k if what == "k" else cfg[what])] += 1

    def op_tracers_end(self, cnt):
        self._tracers_disarm()

    def _frame_taken(self, who):
        """A frame of the tracers (who "t") or the monitor ("m") has just been taken, on both sides."""
        if who == "t":
            if self.t_stale is not None:
                self.t_followed, self.t_stale = self.t_stale, None
            self.t_chain = 2 if self.t_chain == 1 else 0
        else:
            self.m_chain = 2 if self.m_chain == 1 else 0
            rec = self.mm.ring[-1]
            if rec.outside > 0:
                self.cov["monitor_outside_nonzero"] += 1
            if 0 < rec.moving < rec.n:
                self.cov["monitor_moving_between_0_and_n"] += 1
        across = {"add": "growth" if self.grew else None}.get(self.after, "kick" if self.after in KICKS + ("obs_kick",) else self.after)
        if across in ACROSS_PINS and self.tm is not None and self.mm is not None:
            self.cov["%s_across_%s" % ("tracers" if who == "t" else "monitor", across)] += 1

    def _after_step(self):
        taken = [(w, r.recorded) for w, r in (("t", self.tm), ("m", self.mm)) if r is not None]
        super()._after_step()
        for w, recorded in taken:
            if (self.tm if w == "t" else self.mm).recorded > recorded:
                self._frame_taken(w)

    def op_tracers_sample(self, cnt):
        if self.st is not None:
            before = self._counters()
            self.st.ctx.call("gpe_tracers_sample")
            self._frozen(before, "tracers_sample")
        self.tm.sample()
        self._frame_taken("t")
        self.log.append("tracers sample at step %d" % self.tm.steps_seen)

    def _tracer_coverage(self, held):
        cov, index = self.cov, held.index
        present = index != 0xFFFFFFFF
        cov["tracer_rows_present"] += int(present.sum())
        cov["tracer_rows_absent"] += int((~present).sum())
        if len(index) > 1:
            appeared = present[1:] & ~present[:-1]
            cov["tracer_rows_appeared"] += int(appeared.sum())
            # (a uid at or above next_uid when the recording began: an add -- or gpe_set_uids -- has handed it out since)
            cov["tracer_future_uid_handed_out"] += int(appeared[:, self.tcfg["future"]].sum())
            cov["tracer_index_changed_between_frames"] += int((present[1:] & present[:-1] & (index[1:] != index[:-1])).sum())
        if self.tm.recorded - self.t_mark > self.tcfg["frames"]:
            cov["tracer_ring_wrapped"] += 1
        if self.t_followed is not None:
            cov["tracers_after_" + self.t_followed] += 1
            self.t_followed = None

    def _tracers_read(self, capacity, consume, what):
        """gpe_tracers_read into sentinel-filled arrays of capacity + 2 frames: count, recorded, every delivered frame of
        every configured field bit for bit, the sentinel behind them."""
        tm, cfg = self.tm, self.tcfg
        k, fields = len(cfg["uids"]), cfg["fields"]
        want = tm.read(capacity, consume)
        if self.st is not None:
            L, room = self.L, capacity + 2
            arr = {"step": np.full(room, SENTINEL64, np.uint64), "pos": np.full((room, k, 2), SENTINEL, np.uint32),
                   "prev": np.full((room, k, 2), SENTINEL, np.uint32), "index": np.full((room, k), SENTINEL, np.uint32)}
            fr = L.GpeTracerFrames(struct_size=C.sizeof(L.GpeTracerFrames), flags=L.TRACERS_CONSUME if consume else 0,
                                   capacity=capacity)
            fr.step = arr["step"].ctypes.data_as(C.POINTER(C.c_uint64))
            if fields & L.TRACER_POS:
                fr.pos_xy = arr["pos"].ctypes.data_as(C.POINTER(C.c_float))
            if fields & L.TRACER_PREV:
                fr.prev_xy = arr["prev"].ctypes.data_as(C.POINTER(C.c_float))
            if fields & L.TRACER_INDEX:
                fr.index = arr["index"].ctypes.data_as(C.POINTER(C.c_uint32))
            before = self._counters()
            self.st.ctx.call("gpe_tracers_read", C.byref(fr))
            self._frozen(before, what)
            assert (fr.count, fr.recorded) == (want.count, want.recorded), "%s: count %d recorded %d, model %d %d" % (
                what, fr.count, fr.recorded, want.count, want.recorded)
            m = len(want.step)
            wanted = {"step": want.step, "pos": _bits(want.pos), "prev": _bits(want.prev), "index": want.index}
            for name, bit in (("step", 0), ("pos", L.TRACER_POS), ("prev", L.TRACER_PREV), ("index", L.TRACER_INDEX)):
                if name == "step" or fields & bit:
                    same = arr[name][:m] == wanted[name]
                    assert same.all(), "%s: %s differs in frame %d of %d (step %d)" % (
                        what, name, int(np.nonzero(~same.reshape(m, -1).all(axis=1))[0][0]), m,
                        int(want.step[np.nonzero(~same.reshape(m, -1).all(axis=1))[0][0]]))
                    assert (arr[name][m:] == (SENTINEL64 if name == "step" else SENTINEL)).all(), \
                        "%s: %s written past frame %d" % (what, name, m)
        if consume:
            self.t_mark = tm.recorded
        return want

    def _op_tracers_read(self, consume=None):
        held = self.tm.read()
        self._tracer_coverage(held)
        self.reads += 1
        capacity, cls = self._class(self.reads, held.count, least=1)
        if consume is None:
            consume = bool((self.reads // 3) % 2)
        else:
            capacity, cls = held.count + (self.reads % 2), "above" if self.reads % 2 else "at"
        what = "tracers_read capacity %d (%s, of %d) consume %d" % (capacity, cls, held.count, consume)
        self.log.append(what)
        self._tracers_read(capacity, consume, what)
        self.cov["tracer_read_" + cls] += 1
        self.cov["tracer_read_consume_%d" % consume] += 1
        if self.t_chain == 2:
            self.cov["tracers_consume_sample_read"] += 1
        self.t_chain = 1 if consume else 0

    def op_tracers_read(self, cnt):
        self._op_tracers_read()

    def op_tracers_read_consume(self, cnt):
        self._op_tracers_read(consume=True)

    def _refused(self, status, what):
        L = self.L
        assert status == L.GPE_ERR_STATE, "%s: status %d, expected GPE_ERR_STATE" % (what, status)
        assert self.st.ctx.lib.gpe_last_error(self.st.ctx.h), "%s: last_error is empty" % what

    def op_tracers_begin_armed(self, cnt):
        """gpe_tracers_begin while armed: GPE_ERR_STATE, and the recording goes on as if nothing had been asked."""
        self._uids_on()                                          # (so that being armed is the only reason to refuse)
        other = dict(self.tcfg, uids=np.ascontiguousarray(self.model.uids[:3]), every=5, frames=2, fields=7)
        if self.st is not None:
            self._refused(self._status("gpe_tracers_begin", C.byref(self._tracers_cfg(other))), "begin while armed")
        self.cov["tracers_begin_refused_armed"] += 1
        self.log.append("tracers begin while armed: refused")
        self.op_tracers_sample(cnt)
        self._op_tracers_read()

    def op_tracers_begin_uids_off(self, cnt):
        """The tracers read and ended, uids off, gpe_tracers_begin: GPE_ERR_STATE; the monitor's recording is unharmed;
        then the same tracers again (which turns the uids on)."""
        cfg = self.tcfg
        self._op_tracers_read(consume=False)
        self._tracers_disarm()
        if self.model.uids is not None:
            self._uids(False)
        if self.st is not None:
            self._refused(self._status("gpe_tracers_begin", C.byref(self._tracers_cfg(cfg))), "begin while uids are off")
            assert self._status("gpe_tracers_sample") == self.L.GPE_ERR_STATE, "armed after a refused begin"
        self.cov["tracers_begin_refused_uids_off"] += 1
        self.log.append("tracers begin while uids are off: refused")
        self.op_monitor_sample(cnt)
        self._op_monitor_read()
        self._tracers_arm(cfg)

    # ---- the monitor --------------------------------------------------------------------------------------------------
    def _monitor_arm(self, cfg):
        from tests import _monitor_model
        if self.st is not None:
            L = self.L
            c = L.GpeMonitorConfig(struct_size=C.sizeof(L.GpeMonitorConfig), flags=0, every=cfg["every"],
                                   frames=cfg["frames"], rest_speed=cfg["rest_speed"])
            self.st.ctx.call("gpe_monitor_begin", C.byref(c))
        self.mcfg, self.mm = cfg, _monitor_model.MonitorModel(self.model, **cfg)
        self.m_mark = self.m_chain = 0
        self.log.append("monitor begin: every %d frames %d rest_speed %r" % (cfg["every"], cfg["frames"], cfg["rest_speed"]))

    def _monitor_disarm(self):
        if self.st is not None:
            self.st.ctx.call("gpe_monitor_end")
        self.mm = None
        self.log.append("monitor end")

    def _typical_speed(self):
        """Near the scene's typical displacement per step (the median; what gravity adds in a step while all are at rest)."""
        pos, prev, _ = self._now()
        v = np.sqrt(((pos - prev).astype(np.float64) ** 2).sum(axis=1))
        typical = float(np.median(v[np.isfinite(v)]))
        return float(F32(typical if typical > 0.0 else 9.81 * DT * DT))

    def op_monitor_begin(self, cnt):
        seed, c = self.plan.seed, self.cycle
        cfg = dict(every=EVERY[(seed + c + 1) % 3], frames=FRAMES[(seed + 2 * c) % 3],
                   rest_speed=0.0 if (seed + c) % 2 else self._typical_speed())
        self._monitor_arm(cfg)
        self.cov["monitor_every_%d" % cfg["every"]] += 1
        self.cov["monitor_frames_%d" % cfg["frames"]] += 1
        self.cov["monitor_rest_speed_%s" % ("zero" if cfg["rest_speed"] == 0.0 else "typical")] += 1
        if self.tm is not None and self.tcfg["every"] != cfg["every"]:
            self.cov["both_recorders_armed_different_every"] += 1

    def op_monitor_end(self, cnt):
        self._monitor_disarm()

    def op_monitor_sample(self, cnt):
        if self.st is not None:
            before = self._counters()
            self.st.ctx.call("gpe_monitor_sample")
            self._frozen(before, "monitor_sample")
        self.mm.sample()
        self._frame_taken("m")
        self.log.append("monitor sample at step %d" % self.mm.steps_seen)

    def _monitor_read(self, capacity, consume, what):
        from tests import _monitor_model as M
        give, count, recorded = self.mm.read(capacity, consume)
        if self.st is not None:
            L, room = self.L, capacity + 2
            words = M.DTYPE.itemsize // 4
            raw = np.full(room * words, SENTINEL, np.uint32)
            fr = L.GpeMonitorFrames(struct_size=C.sizeof(L.GpeMonitorFrames), flags=L.MONITOR_CONSUME if consume else 0,
                                    capacity=capacity)
            fr.frames = raw.ctypes.data_as(C.POINTER(L.GpeMeasures))
            before = self._counters()
            self.st.ctx.call("gpe_monitor_read", C.byref(fr))
            self._frozen(before, what)
            assert (fr.count, fr.recorded) == (count, recorded), "%s: count %d recorded %d, model %d %d" % (
                what, fr.count, fr.recorded, count, recorded)
            records = raw.view(M.DTYPE)
            for j, want in enumerate(give):
                bad = M.same(records[j], want)
                assert bad is None, "%s: record %d of %d (step %d): %s" % (what, j, len(give), want.step, bad)
            assert (raw[len(give) * words:] == SENTINEL).all(), "%s: written past record %d" % (what, len(give))
        if consume:
            self.m_mark = self.mm.recorded
        return give

    def _op_monitor_read(self, consume=None):
        mm = self.mm
        held = len(mm.ring)
        if mm.recorded - self.m_mark > self.mcfg["frames"]:
            self.cov["monitor_ring_wrapped"] += 1
        self.reads += 1
        capacity, cls = self._class(self.reads, held, least=1)
        if consume is None:
            consume = bool((self.reads // 3) % 2)
        else:
            capacity, cls = held + (self.reads % 2), "above" if self.reads % 2 else "at"
        what = "monitor_read capacity %d (%s, of %d) consume %d" % (capacity, cls, held, consume)
        self.log.append(what)
        self._monitor_read(capacity, consume, what)
        self.cov["monitor_read_" + cls] += 1
        self.cov["monitor_read_consume_%d" % consume] += 1
        if self.m_chain == 2:
            self.cov["monitor_consume_sample_read"] += 1
        self.m_chain = 1 if consume else 0

    def op_monitor_read(self, cnt):
        self._op_monitor_read()

    def op_monitor_read_consume(self, cnt):
        self._op_monitor_read(consume=True)

    def op_measure(self, cnt):
        from tests import _monitor_model as M
        rest = 0.0 if self.rng2.integers(0, 2) else self._typical_speed()
        pos, prev, _ = self._now()
        want = M.measure(pos, prev, self.model.uids, self.model.world, rest)
        if self.st is not None:
            before = self._counters()
            got = self.st.measure(rest)
            self._frozen(before, "measure")
            bad = M.same(got, want)
            assert bad is None, "measure(%r): %s" % (rest, bad)
        self.cov["measures"] += 1
        self.log.append("measure rest_speed %r: moving %d of %d, outside %d" % (rest, want.moving, want.n, want.outside))

    # ---- what the hooks of the existing operations do -----------------------------------------------------------------
    def _observe(self, where):
        if where == "before_save":
            # State.save stores no recorder: read and end them; after the load the same recordings begin anew
            self.saved = (self.tcfg if self.tm is not None else None, self.mcfg if self.mm is not None else None)
            if self.tm is not None:
                self._op_tracers_read(consume=False)
                self._tracers_disarm()
            if self.mm is not None:
                self._op_monitor_read(consume=False)
                self._monitor_disarm()
        elif where == "after_load":
            tcfg, mcfg = self.saved
            if tcfg is not None:
                self._tracers_arm(tcfg)
            if mcfg is not None:
                self._monitor_arm(mcfg)
            if tcfg is not None and mcfg is not None:
                self.cov["save_load_while_armed"] += 1
        elif where == "other_mode":
            self.after = "set_mode"                                 # frames taken in the other mode
            if self.tm is not None:
                self.op_tracers_sample(len(self.model))
            if self.mm is not None:
                self.op_monitor_sample(len(self.model))
            self.after = "other_mode"
            for op in QUERIES:
                getattr(self, "op_" + op)(len(self.model))
                self.prev_op = op
            self.after = "set_mode"
        elif where in ("after_kick", "edited_outside") and self.mm is not None:
            # a record of the kicked particles before the step that follows, and of the particles outside the world
            self.after = self.cur_op if where == "after_kick" else self.after
            self.op_monitor_sample(len(self.model))

    # ---- operations that change the particles, so that a pin does not hang on the draws of the existing ones ----------
    def op_obs_kick(self, cnt):
        """Every particle at rest (the fastest is then the first, with max_v2 = +0), a frame, a kick of a circle that
        does not hold the first particle, a frame: max_v2 and its uid have changed.  (The kicks of the plan need not do
        that: a teleport or a collision leaves particles faster than any kick makes them.)"""
        model, rng = self.model, self.rng2
        self._uids_on()
        self.op_stop(cnt)
        self.op_tracers_sample(cnt); self.op_monitor_sample(cnt)
        before = self.mm.ring[-1]
        pos = model.arrays()[0]
        far = np.nonzero(((pos - pos[0]).astype(np.float64) ** 2).sum(axis=1) > 9.0 ** 2)[0]
        c = pos[int(rng.choice(far))]
        region = (float(c[0]), float(c[1]), float(F32(rng.uniform(2.0, 8.0))))
        a = (float(F32(rng.uniform(0.5, 3.0))), float(F32(rng.uniform(-3.0, 3.0))))
        mask = circle_mask(pos, *region)
        assert mask.any() and not mask[0]
        want = model.kick(mask, VEL_ADD, *a)
        if self.st is not None:
            got = self.st.kick_circle(region[:2], region[2], VEL_ADD, a, count=True)
            assert got == want, "kick of particles at rest: kicked %d, model %d" % (got, want)
        self.after = "obs_kick"
        self.op_tracers_sample(cnt); self.op_monitor_sample(cnt)
        after = self.mm.ring[-1]
        assert before.max_v2 == 0.0 and after.max_v2 > 0.0 and before.max_v2_uid != after.max_v2_uid, (before, after)
        self.cov["monitor_kick_changed_max_v2"] += 1
        self.cov["monitor_kick_changed_max_v2_uid"] += 1
        self.log.append("kick circle %s add %s of particles at rest: %d kicked" % (region, a, want))

    def op_obs_step(self, cnt):
        """Steps until the tracers have taken a frame (at most `every`)."""
        k = self.tcfg["every"] - self.tm.steps_seen % self.tcfg["every"]
        for _ in range(k):
            self._step()
        self.log.append("step x%d (to the tracers' next frame)" % k)

    def op_obs_run_resort(self, cnt):
        k = int(self.rng2.integers(5, 10))
        self._run(k, 3, True)
        self.log.append("run %d every 3 first True" % k)

    def op_obs_wrap(self, cnt):
        """Where the rings are shortest (4 frames; once or twice in every seed): frames, and every third time a step,
        until both have wrapped.  (Longer rings wrap in some seeds by themselves; wrapping them here as well took the
        small scenes past twice the run time of their interactive counterparts.)"""
        if self.tcfg["frames"] > FRAMES[0]:
            return
        turn = 0
        while min(self.tm.recorded, self.mm.recorded) <= self.tcfg["frames"]:
            turn += 1
            if turn % 3 == 0:
                self._step()
            else:
                self.op_tracers_sample(cnt); self.op_monitor_sample(cnt)
        self.log.append("wrapped both rings in %d turns" % turn)

    def op_remove_tracked_uid(self, cnt):
        model, rng = self.model, self.rng2
        self._uids_on()
        tracked = self.tcfg["uids"][np.isin(self.tcfg["uids"], model.uids)]
        assert len(tracked), "no tracked uid is live\n  " + "\n  ".join(self.log)
        q = np.concatenate([rng.choice(tracked, size=1), rng.choice(model.uids, size=3)]).astype(np.uint32)
        got = self.st.remove_particles_by_uid(q) if self.st is not None else None
        self._lookup_by_uid(counts=False)
        self._removed(got, model.remove_uids(q), "remove %d uids, one of them tracked" % len(q))

    # ---- ray casts, segments, nearest ---------------------------------------------------------------------------------
    def _query_pin(self, kind):
        a = self.after
        pin = {"add": "growth" if self.grew else None, "world_shrink_out": "world_shrink_out" if self.outside else None,
               "other_mode": "other_mode", "edit_radius_up_override": "radius_up_override",
               "edit_radius_down": "radius_down", "grid_under": "grid_under"}.get(a)
        if a in REMOVALS and self.removed_any:
            pin = "removal"
        if pin is not None:
            self.cov["%s_after_%s" % (kind, pin)] += 1

    def _dense_point(self):
        pos = self._now()[0]
        ok = np.isfinite(pos).all(axis=1)
        hist, xe, ye = np.histogram2d(pos[ok, 0], pos[ok, 1], bins=(12, 8))
        i, j = np.unravel_index(int(np.argmax(hist)), hist.shape)
        return np.array([0.5 * (xe[i] + xe[i + 1]), 0.5 * (ye[j] + ye[j + 1])], F32)

    def _ray(self, kind):
        """-> (origin, end) of one ray of this kind, float32."""
        rng, world = self.rng2, np.array(self.world, F32)
        pos, _, rad = self._now()
        turn = rng.uniform(0.0, 2.0 * np.pi)
        along = np.array([np.cos(turn), np.sin(turn)])
        if kind == "dense":
            c = self._dense_point()
            o, e = c - 9.0 * along, c + 9.0 * along
        elif kind == "inside":
            j = int(rng.integers(0, len(pos)))
            o = pos[j] + 0.3 * abs(float(rad[j])) * along
            e = o + rng.uniform(0.0, 8.0) * np.array([along[1], -along[0]])
        elif kind == "zero":
            o = pos[int(rng.integers(0, len(pos)))] if rng.integers(0, 2) else rng.random(2) * world
            e = o
        elif kind == "outside":
            o = np.array([-5.0 if rng.integers(0, 2) else world[0] + 7.0, rng.random() * world[1]])
            e = np.array([rng.random() * world[0], rng.random() * world[1]])
        elif kind == "boundary":
            from tests._oracle_model import CELL_SIZE_MULTIPLIER
            cell = F32(F32(abs(self.model.max_radius)) * CELL_SIZE_MULTIPLIER)     # the contact query's own cell size
            x = F32(F32(rng.integers(1, max(2, int(world[0] / cell)))) * cell)
            y = rng.random() * world[1]
            o, e = np.array([x, y]), np.array([x, y + rng.uniform(-15.0, 15.0)])
        else:
            o = rng.random(2) * world
            e = o + rng.uniform(0.0, 20.0) * along
        return np.asarray(o, F32), np.asarray(e, F32)

    def op_cast_rays(self, cnt):
        from tests import _ray_model
        L, model = self.L, self.model
        self.casts += 1
        k = RAY_K[self.casts % 3]
        kinds = ["dense", "inside", "zero", "outside", "boundary"]
        kinds = [kinds[(self.casts + j) % 5] for j in range(min(k, 5))] + ["random"] * max(k - 5, 0)
        rays = [self._ray(kind) for kind in kinds]
        o = np.ascontiguousarray([r[0] for r in rays], F32)
        e = np.ascontiguousarray([r[1] for r in rays], F32)
        pos, _, rad = self._now()
        ask_uid = model.uids is not None and self.casts % 2 == 0
        want = _ray_model.cast(o, e, pos, rad, uids=model.uids)
        what = "cast %d rays (%s%s)" % (k, " ".join(kinds[:5]), ", uids" if ask_uid else "")
        if self.st is not None:
            room = k + 2
            arr = {"index": np.full(room, SENTINEL, np.uint32), "t": np.full(room, SENTINEL, np.uint32),
                   "uid": np.full(room, SENTINEL, np.uint32), "pos_xy": np.full((room, 2), SENTINEL, np.uint32),
                   "radius": np.full(room, SENTINEL, np.uint32)}
            cast = L.GpeRayCast(struct_size=C.sizeof(L.GpeRayCast), flags=0, k=k)
            cast.from_xy, cast.to_xy = o.ctypes.data_as(C.POINTER(C.c_float)), e.ctypes.data_as(C.POINTER(C.c_float))
            for name, a in arr.items():
                if name != "uid" or ask_uid:
                    setattr(cast, name, a.ctypes.data_as(C.POINTER(C.c_float if name in ("t", "pos_xy", "radius") else C.c_uint32)))
            before = self._counters()
            self.st.ctx.call("gpe_cast_rays", C.byref(cast))
            self._frozen(before, what)
            assert cast.hits == want["hits"], "%s: %d hits, model %d" % (what, cast.hits, want["hits"])
            wanted = {"index": want["index"], "t": _bits(want["t"]), "uid": want["uid"], "pos_xy": _bits(want["pos"]),
                      "radius": _bits(want["radius"])}
            for name, a in arr.items():
                if name == "uid" and not ask_uid:
                    assert (a == SENTINEL).all(), "%s: uid written without being asked for" % what
                    continue
                assert np.array_equal(a[:k], wanted[name]), "%s: %s differs at ray %s" % (
                    what, name, np.nonzero((a[:k] != wanted[name]).reshape(k, -1).any(axis=1))[0].tolist())
                assert (a[k:] == SENTINEL).all(), "%s: %s written past ray %d" % (what, name, k)
        hit = want["index"] != 0xFFFFFFFF
        self.cov["rays_hit"] += int(hit.sum())
        self.cov["rays_missed"] += int((~hit).sum())
        self.cov["ray_from_inside"] += sum(1 for j, kind in enumerate(kinds) if kind == "inside" and hit[j] and want["t"][j] == 0)
        self.cov["ray_k_%d" % k] += 1
        self.cov["cast_uids_%s" % ("asked" if ask_uid else "not_asked")] += 1
        self._query_pin("cast")
        self.last_cast = (o, e, want)
        self.log.append("%s: %d hits" % (what, want["hits"]))

    def op_query_segment(self, cnt):
        """gpe_query_segment (and its count alone) along a ray of the cast before it -- the one that touches most, of the
        first six -- whose first hit must be this set's member with the least t."""
        from tests import _ray_model
        pos, _, rad = self._now()
        self.segments += 1
        if self.last_cast is not None and self.prev_op == "cast_rays":
            o, e, hits = self.last_cast
            sets = [_ray_model.segment_set(o[j], e[j], pos, rad) for j in range(min(len(o), 6))]
            j = int(np.argmax([len(s[0]) for s in sets]))
            a, b, (idx, t) = o[j], e[j], sets[j]
            if len(idx):
                assert hits["index"][j] == idx[np.argmin(_key(t, idx))], "the cast's hit is not the segment's first"
            else:
                assert hits["index"][j] == 0xFFFFFFFF
            self.cov["segment_of_a_cast_ray"] += 1
        else:
            a, b = self._ray("dense")
            idx, t = _ray_model.segment_set(a, b, pos, rad)
        want = self.model.rows(idx)
        cap, cls = self._class(self.segments, len(idx))
        args = (float(a[0]), float(a[1]), float(b[0]), float(b[1]))
        what = "query_segment %s capacity %d (%s)" % (args, cap, cls)
        if self.st is not None:
            self._rows_call("gpe_query_segment", args, cap, want, what)
            before = self._counters()
            assert self.st.count_segment(a, b) == len(idx), "count_segment differs"
            self._frozen(before, "count_segment")
        self.cov["segment_capacity_" + cls] += 1
        if len(idx) >= 3:
            self.cov["segment_rows_at_least_3"] += 1
        self._query_pin("segment")
        self.log.append("%s: %d" % (what, len(idx)))

    def op_nearest(self, cnt):
        from tests import _nearest_model as N
        L, model, rng = self.L, self.model, self.rng2
        self.nearests += 1
        c = self.nearests
        k, m = NEAREST_K[c % 3], NEAREST_M[(2 * c) % 3]
        pos, _, rad = self._now()
        world = np.array(self.world, F32)
        kinds = ["outside", "on_a_particle", "random"]
        kinds = [kinds[(c + j) % 3] for j in range(min(k, 3))] + ["random"] * max(k - 3, 0)
        pts = np.empty((k, 2), F32)
        for j, kind in enumerate(kinds):
            if kind == "outside":
                pts[j] = (-3.0 if rng.integers(0, 2) else world[0] + 4.0, rng.random() * world[1])
            elif kind == "on_a_particle":
                pts[j] = pos[int(rng.integers(0, len(pos)))]
            else:
                pts[j] = rng.random(2) * world
        finite = c % 2 == 1
        md = np.inf
        if finite:
            # a cutoff that takes rows away: the median over the points of the distance to their m-th neighbour (half that
            # for a single point)
            d2 = np.sort(N.dist2_matrix(pts, pos).astype(np.float64), axis=1)[:, min(m, len(pos)) - 1]
            md = float(F32(np.sqrt(np.median(d2)) * (0.5 if k == 1 else 1.0)))
        ask_uid = model.uids is not None and (c // 2) % 2 == 0
        want = N.nearest(pts, pos, m=m, max_distance=md, rad=rad, uids=model.uids)
        what = "nearest %d points m %d max_distance %r%s" % (k, m, md, ", uids" if ask_uid else "")
        if self.st is not None:
            room = k + 1
            arr = {"count": np.full(room, SENTINEL, np.uint32), "index": np.full((room, m), SENTINEL, np.uint32),
                   "uid": np.full((room, m), SENTINEL, np.uint32), "dist2": np.full((room, m), SENTINEL, np.uint32),
                   "pos_xy": np.full((room, m, 2), SENTINEL, np.uint32), "radius": np.full((room, m), SENTINEL, np.uint32)}
            q = L.GpeNearestQuery(struct_size=C.sizeof(L.GpeNearestQuery), flags=0, k=k, m=m, max_distance=md)
            q.point_xy = pts.ctypes.data_as(C.POINTER(C.c_float))
            for name, a in arr.items():
                if name != "uid" or ask_uid:
                    setattr(q, name, a.ctypes.data_as(C.POINTER(C.c_float if name in ("dist2", "pos_xy", "radius") else C.c_uint32)))
            before = self._counters()
            self.st.ctx.call("gpe_query_nearest", C.byref(q))
            self._frozen(before, what)
            assert q.found == want["found"], "%s: found %d, model %d" % (what, q.found, want["found"])
            wanted = {"count": want["count"], "index": want["index"], "uid": want["uid"], "dist2": _bits(want["dist2"]),
                      "pos_xy": _bits(want["pos"]), "radius": _bits(want["radius"])}
            for name, a in arr.items():
                if name == "uid" and not ask_uid:
                    assert (a == SENTINEL).all(), "%s: uid written without being asked for" % what
                    continue
                assert np.array_equal(a[:k], wanted[name]), "%s: %s differs at point %s" % (
                    what, name, np.nonzero((a[:k] != wanted[name]).reshape(k, -1).any(axis=1))[0].tolist())
                assert (a[k:] == SENTINEL).all(), "%s: %s written past point %d" % (what, name, k)
        if finite and (want["count"] < min(m, len(pos))).any():
            self.cov["nearest_cut_by_max_distance"] += 1
        if m == 64 and (want["count"] == 64).any():
            self.cov["nearest_m_64_delivered"] += 1
        self.cov["nearest_k_%d" % k] += 1
        self.cov["nearest_m_%d" % m] += 1
        self.cov["nearest_max_distance_%s" % ("finite" if finite else "infinite")] += 1
        self.cov["nearest_uids_%s" % ("asked" if ask_uid else "not_asked")] += 1
        self._query_pin("nearest")
        self.log.append("%s: %d found" % (what, want["found"]))
