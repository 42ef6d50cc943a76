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
and without a grid override pending."""
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
    """The scene and the operations of one sequence: 1 500 .. 6 000 particles at the reference density in a world of
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
    return Plan(seed, pos, rad, world, ops, flags)


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
        self.last = op

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

    def op_step(self, cnt):
        k = int(self.rng.integers(1, 5)); resort = bool(self.rng.integers(0, 4) == 0)
        for s in range(k):
            self._step(resort and s == 0)
        self.log.append("step x%d%s" % (k, " resort" if resort else ""))

    def op_run(self, cnt):
        k = int(self.rng.integers(5, 20)); every = int(self.rng.choice([0, 7])); first = bool(self.rng.integers(0, 2))
        if first or (every and k > every):
            self._stale("resort")
        if self.st is not None:
            self.st.run(DT, k, resort_every=every, resort_first=first)
        self.model.run(DT, k, resort_every=every, resort_first=first)
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
