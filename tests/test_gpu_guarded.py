"""GPU (-m gpu): what the kernels were NOT supposed to write.  Every context of a case is created with
FLAG_GUARD_ALLOCS: each device allocation lies between two red zones filled with a canary, its fresh payload is
poisoned (csrc/gpe_api.hip, "device memory").  A case asserts that

  * guard_check() reports no damaged zone -- on every context, when it is closed and at the end of the case (zones of
    buffers released on the way were checked when they went and are reported with the rest), and
  * the outputs are the bits the existing test of that scene compares against: the cases below RUN the existing tests'
    own bodies (their scenes, their oracle / twin comparisons, their pipeline_info() proofs of the path taken) with the
    package's Context switched to guarded ones, so a consumed poison word or canary shows as a bit difference there.

The contexts of a case get two different (canary, poison) settings in turn, in the order of their creation
(gpe_config.guard_canary / guard_poison: a field of each context, nothing process-wide): a case that compares two
library contexts with each other (native against compat, ranks against a single context) compares runs that would have
consumed different words.
"""
import importlib
import inspect
import itertools
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (canary, poison): nonzero, a nonzero finite f32, and as an index of 16-byte elements inside a 16 KiB red zone
WORDS = [(0x3C3, 0x2A5), (0x1B7, 0x35A)]


class _Guard:
    """Switches engine.Context to guarded contexts for one test and collects what their red zones show."""

    def __init__(self, gpe):
        self.gpe, self.L = gpe, gpe._lib
        self.words = None           # a fixed WORDS entry, or None: alternate
        self.created, self._serial = 0, itertools.count()
        self.open, self.reports, self.tags, self.allocations = [], [], set(), 0

    def install(self, monkeypatch):
        eng = importlib.import_module(self.gpe.__name__ + ".engine")
        init0, close0 = eng.Context.__init__, eng.Context.close
        sig = inspect.signature(init0)
        guard = self

        def init(ctx, *a, **kw):
            b = sig.bind(ctx, *a, **kw)
            b.apply_defaults()
            b.arguments["flags"] = int(b.arguments["flags"]) | guard.L.FLAG_GUARD_ALLOCS
            k = next(guard._serial)                    # (rank contexts are created on a thread each: one number each)
            b.arguments["guard_words"] = guard.words or WORDS[k % len(WORDS)]
            init0(*b.args, **b.kwargs)
            guard.created += 1
            guard.open.append(ctx)

        def close(ctx):
            if getattr(ctx, "h", None) and any(c is ctx for c in guard.open):
                guard.note(ctx)
                guard.open = [c for c in guard.open if c is not ctx]
            close0(ctx)

        monkeypatch.setattr(eng.Context, "__init__", init)
        monkeypatch.setattr(eng.Context, "close", close)

    def note(self, ctx):
        zones = ctx.guard_check()
        self.reports.append((zones, ctx.guard_damaged))
        self.allocations = max(self.allocations, ctx.guard_allocations)
        self.tags.update(t for t, _, _, _ in ctx.guard_registry())

    def finish(self):
        for ctx in list(self.open):
            ctx.close()
        assert self.created > 0, "the case created no guarded context"
        bad = [(z, n) for z, n in self.reports if n or z]
        print("guard: %d contexts, %d allocations at most, tags %s" % (self.created, self.allocations, " ".join(sorted(self.tags))))
        assert not bad, "damaged red zones: %r" % (bad,)


@pytest.fixture
def guard(gpe, monkeypatch):
    g = _Guard(gpe)
    g.install(monkeypatch)
    yield g
    g.finish()


def _module(name):
    for full in ("tests." + name, name):
        if full in sys.modules:
            return sys.modules[full]
    return importlib.import_module(name)


def _rerun(request, module, test, **params):
    """The body of an existing test, its fixtures resolved here and its parameters given by the case."""
    fn = getattr(_module(module), test)
    kw = {p: params[p] if p in params else request.getfixturevalue(p) for p in inspect.signature(fn).parameters}
    fn(**kw)


def _cases(rows):
    return [pytest.param(m, t, p, id=i) for i, m, t, p in rows]


# ---- the checker itself ---------------------------------------------------------------------------------------------
def _small_state(gpe, n=3000, **kw):
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=7)
    return gpe.State(pos, rad, world=world, **kw), world, pos, rad


@pytest.mark.parametrize("side", ["rear", "front"])
def test_checker_names_the_damaged_zone_and_keeps_it_after_the_free(gpe, side):
    """Four bytes written from the HOST (gpe_buffer_upload: a copy into memory the allocation owns, no kernel out of
    bounds) just behind / just before the payload of a gpe_buffer_alloc buffer of exactly n elements: guard_check()
    names the buffer's tag, the side, offset 0 / -4 and the word written; the context still steps; the report survives
    the buffer's release."""
    import ctypes as C
    L = gpe._lib
    st, world, pos, rad = _small_state(gpe, flags=L.FLAG_GUARD_ALLOCS)
    ctx = st.ctx
    st.update(1 / 60, resort=True)
    n = 1000
    buf = gpe.GpuBuffer(ctx, np.arange(n, dtype=np.uint32))
    ctx.call("gpe_inclusive_scan_u32", buf.dptr, n)
    assert ctx.guard_check() == [] and ctx.guard_damaged == 0 and ctx.guard_allocations > 10
    assert ("user.buffer", 4 * n, 64, "live") in ctx.guard_registry()
    word = np.array([0xC0FFEE11], np.uint32)
    at = buf.dptr.value + (4 * n if side == "rear" else -4)
    ctx.call("gpe_buffer_upload", C.c_void_p(at), word.ctypes.data_as(C.c_void_p), 4)
    want = {"tag": "user.buffer", "side": side, "first_offset": 0 if side == "rear" else -4,
            "last_offset": 3 if side == "rear" else -1, "first_word": 0xC0FFEE11, "payload_bytes": 4 * n}
    assert ctx.guard_check() == [want] and ctx.guard_damaged == 1
    assert b"user.buffer" in L.load().gpe_last_error(ctx.h)
    st.update(1 / 60)                                      # the context still steps
    twin, *_ = _small_state(gpe)
    twin.update(1 / 60, resort=True)
    twin.update(1 / 60)
    assert np.array_equal(st.positions(), twin.positions())
    assert np.array_equal(buf.download(), np.cumsum(np.arange(n, dtype=np.uint64)).astype(np.uint32))
    buf.free()                                             # sticky: the zone went with the buffer, the finding stays
    assert ctx.guard_check() == [want] and ctx.guard_damaged == 1
    st.close(); twin.close()


def test_checker_is_silent_without_the_flag(gpe):
    st, *_ = _small_state(gpe)
    st.update(1 / 60, resort=True)
    buf = gpe.GpuBuffer(st.ctx, np.arange(100, dtype=np.uint32))
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0 and st.ctx.guard_allocations == 0
    # the registry is kept all the same, and unguarded sizes are payload + slack = what they always were
    assert ("user.buffer", 400, 64, "live") in st.ctx.guard_registry()
    buf.free()
    st.close()


def test_words_must_keep_a_consumed_poison_harmless(gpe):
    """All-ones, NaN patterns and anything else that is not a small nonzero word are refused at gpe_create; 0 selects
    the default of that word."""
    for bad in ((5, 5), (0xFFFFFFFF, 5), (5, 0x7FC00000), (1024, 5), (0x2A5, 0), (0, 0x3C3)):
        with pytest.raises(gpe.GpeError) as e:
            gpe.Context(flags=gpe._lib.FLAG_GUARD_ALLOCS, guard_words=bad)
        assert e.value.status == gpe._lib.GPE_ERR_INVALID_ARG, bad
    for good in (WORDS[1], (0, 0), (0, 7), (7, 0)):
        gpe.Context(flags=gpe._lib.FLAG_GUARD_ALLOCS, guard_words=good).close()


# ---- the workspaces' allocations: tag, payload and slack --------------------------------------------------------------
# What the registry must hold once every workspace has been used once on WS_N particles in touching pairs, uids on.
# Written out from the reserve functions as they stood before the API's host side was split by feature: 300 particles
# are query_tiles = 1 tile of 2048 and contacts_tiles = 2 workgroups of 256; 64 bytes (16 words) of slack behind what
# sort_pairs sorts and what the scan runs on in place, none elsewhere; the query.* buffers keep dev_alloc's historical
# slack, max(count, 4) elements + 64 bytes less the payload.
WS_N, WS_PAIRS = 300, 150
WS_ROW_WORDS = 65537                                       # ray.row_start / nearest.row_start: one word per clamped row + 1
WS_TABLE = {
    # a circle query that returns all 300 rows with every field: 2 parts of 2400 -> 2560 bytes, 3 of 1200 -> 1280
    "query.tile_count": (4, 76), "query.tile_key": (8, 88), "query.pick": (8, 88), "query.stage": (8960, 64),
    # 150 pairs with index_a, index_b, uid_a, uid_b and overlap: 5 parts of 600 -> 768 bytes
    "contacts.keys": (1200, 64), "contacts.vals": (1200, 64), "contacts.rec": (4800, 0), "contacts.degree": (1200, 0),
    "contacts.upper": (1200, 64), "contacts.tile_sum": (16, 0), "contacts.total": (8, 0), "contacts.stage": (3840, 0),
    "clusters.parent": (1200, 0), "clusters.label": (1200, 0), "clusters.root_size": (1200, 0), "clusters.size": (1200, 0),
    "clusters.tile_word": (16, 0), "clusters.words": (16, 0),
    # 5 rays
    "ray.row_start": (4 * WS_ROW_WORDS, 0), "ray.from": (40, 0), "ray.to": (40, 0), "ray.index": (20, 0), "ray.uid": (20, 0),
    "ray.t": (20, 0), "ray.pos": (40, 0), "ray.radius": (20, 0),
    # 5 points of 3 slots
    "nearest.row_start": (4 * WS_ROW_WORDS, 0), "nearest.points": (40, 0), "nearest.count": (20, 0), "nearest.index": (60, 0),
    "nearest.uid": (60, 0), "nearest.dist2": (60, 0), "nearest.pos": (120, 0), "nearest.radius": (60, 0),
    # 7 candidates; ctl: 4 box words + 8 round counters
    "spawn.pos": (56, 0), "spawn.radius": (28, 0), "spawn.keys": (28, 64), "spawn.vals": (28, 64), "spawn.rec": (112, 0),
    "spawn.blocked": (28, 0), "spawn.state": (28, 0), "spawn.rank": (28, 64), "spawn.verdict": (7, 0), "spawn.ctl": (48, 0),
    # 4 keys with pos, prev and radius: 3 parts of 256 bytes; the radius edit's tile keys (1 tile) and their maximum
    "edit.keys": (16, 64), "edit.slots": (16, 64), "edit.fields": (768, 0), "edit.flag": (8, 0), "edit.tile_key": (8, 0),
    "edit.max_key": (8, 0),
    # 3 tracers x 2 frames with pos, prev and index
    "tracers.keys": (12, 0), "tracers.perm": (12, 0), "tracers.slot_index": (12, 0), "tracers.ring_pos": (48, 0),
    "tracers.ring_prev": (48, 0), "tracers.ring_index": (24, 0),
    # 2048 partial records of 80 bytes and one gpe_measures of 120
    "monitor.partials": (2048 * 80 + 120, 0),
}


def test_workspace_allocations_keep_their_tags_payloads_and_slack(gpe):
    """Every workspace used once on a guarded context: the registry lists each buffer of WS_TABLE with exactly that
    payload and slack and no other workspace buffer, the tracers' go to "released" unchanged at tracers_end, no red zone
    is damaged, and the context closes."""
    L = gpe._lib
    i = np.arange(WS_N)
    # rows of 10 pairs: partners 1.5 apart (radius 1: touching), pairs 6 and rows 3 apart (not touching)
    pos = np.stack([10.0 + 6.0 * ((i % 20) // 2) + 1.5 * (i % 2), 10.0 + 3.0 * (i // 20)], axis=1).astype(np.float32)
    rad = np.ones(WS_N, np.float32)
    st = gpe.State(pos, rad, world=(80.0, 64.0), flags=L.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    assert len(st.query_circle((40.0, 30.0), 1000.0).index) == WS_N
    assert st.pick((10.0, 10.0)).index[0] == 0
    assert len(st.contacts(capacity=1000, overlap=True).a) == WS_PAIRS
    assert st.clusters().count == WS_PAIRS
    ends = np.array([[10.0, 5.0], [16.0, 5.0], [22.0, 5.0], [28.0, 5.0], [3.0, 3.0]], np.float32)
    assert st.cast_rays(ends, ends + np.float32([0.0, 10.0]), uids=True, rows=True).hits == 4
    assert st.nearest(ends, m=3, uids=True, rows=True).found == 15
    cand = np.concatenate([ends, [[70.0, 60.0], [75.0, 60.0]]]).astype(np.float32)
    added, verdict = st.add_particles_free(cand, np.ones(7, np.float32), dry_run=True)
    assert len(verdict) == 7 and st.positions().shape[0] == WS_N
    keys = np.array([0, 7, 150, 299])
    assert st.edit_particles(indices=keys, positions=pos[keys], previous=pos[keys], radii=rad[keys]) == 4
    st.tracers_begin(np.array([3, 4, 298]), every=1, frames=2, prev=True, index=True)
    st.update(1 / 60); st.update(1 / 60)
    assert st.tracers_read().recorded == 2
    assert st.measure().n == WS_N

    def workspace(state):
        rows = [(t, p, s) for t, p, s, when in st.ctx.guard_registry() if when == state and t.split(".")[0] in
                ("query", "contacts", "clusters", "ray", "nearest", "spawn", "edit", "tracers", "monitor")]
        assert len(rows) == len(set(t for t, _, _ in rows)), rows
        return {t: (p, s) for t, p, s in rows}
    live = workspace("live")
    assert live == WS_TABLE
    st.tracers_end()
    gone = workspace("released")
    assert {t: v for t, v in gone.items() if t.startswith("tracers.")} == {t: v for t, v in WS_TABLE.items() if t.startswith("tracers.")}
    assert not any(t.startswith("tracers.") for t in workspace("live"))
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    st.close()


# ---- the step sets: replacing one leaks nothing and frees nothing twice ----------------------------------------------
def _step_set_case(gpe, st, feature):
    """(set(k), clear(), the feature's tags as a predicate, the tags that stay live behind the clear) of one step set on
    the 8 x 8 lattice of _step_set_state: k walls / fields / pistons, k pair bonds, k bodies of 4 members."""
    L = gpe._lib

    def walls(k):
        return np.float32([[5.0 + 10.0 * j, 2.0, 5.0 + 10.0 * j, 50.0, 0.5] for j in range(k)])

    def pistons(k):
        m = np.zeros(k, gpe.MOVER_DTYPE)
        m["ax"] = m["bx"] = 5.0 + 10.0 * np.arange(k)
        m["ay"], m["by"], m["radius"] = 2.0, 20.0, 0.5
        m["kind"], m["vx"], m["travel"] = L.MOVER_LINEAR, 1.0, 10.0
        return m

    def winds(k):
        f = np.zeros(k, gpe.FIELD_DTYPE)
        f["shape"], f["kind"], f["falloff"], f["fx"] = L.FIELD_EVERYWHERE, L.FIELD_UNIFORM, L.FALLOFF_NONE, 1.0
        return f

    def bodies(k):
        return st.bodies_from_groups([[16 * g, 16 * g + 1, 16 * g + 8, 16 * g + 9] for g in range(k)])

    def hinges(k):                                         # particles 4 g, 4 g + 1, 4 g + 2 of the first two rows: straight
        g = 4 * np.arange(k)
        return gpe.bends_from_angles(g, g + 1, g + 2, np.pi, 0.5)

    def triangles(k):                                      # (g, g + 1, g + 8): neighbours share two uids
        return st.areas_from_loops([[g, g + 1, g + 8] for g in range(k)], stiffness=0.5)

    def surfaces_of(target, obstacles):
        def set_(k):
            obstacles(k)                                   # (a new set drops its surfaces: the rows are always new ones)
            st.set_surfaces(target, gpe.surface_rows(k, restitution=0.5, friction=0.1))
        return set_

    def sweep_of(obstacles, switch):
        def set_(k):
            obstacles(k)
            switch(True)
        return set_

    def set_walls(k): st.set_colliders(walls(k))
    def set_pistons(k): st.set_movers(pistons(k))
    msweep = {"grid.msweep_counts", "grid.msweep_carry", "grid.msweep_old"}
    return {
        "colliders": (set_walls, st.clear_colliders, lambda t: t.startswith("grid.collider_"), set()),
        "fields": (lambda k: st.set_fields(winds(k)), st.clear_fields, lambda t: t.startswith("grid.field_"), set()),
        "movers": (set_pistons, st.clear_movers, lambda t: t.startswith("grid.mover_"), set()),
        "bonds": (lambda k: st.set_bonds(gpe.pair_bonds(2 * np.arange(k), 2 * np.arange(k) + 1, 3.0)), st.clear_bonds,
                  lambda t: t.startswith("uid.bond_"), set()),
        "bends": (lambda k: st.set_bends(hinges(k)), st.clear_bends, lambda t: t.startswith("uid.bend_"), set()),
        "areas": (lambda k: st.set_areas(*triangles(k)), st.clear_areas, lambda t: t.startswith("uid.area_"), set()),
        "bodies": (lambda k: st.set_bodies(*bodies(k)), st.clear_bodies, lambda t: t.startswith("uid.body_"), set()),
        "surfaces-of-colliders": (surfaces_of("colliders", set_walls), lambda: st.clear_surfaces("colliders"),
                                  lambda t: t == "grid.collider_surf", set()),
        "surfaces-of-movers": (surfaces_of("movers", set_pistons), lambda: st.clear_surfaces("movers"),
                               lambda t: t in ("grid.mover_surf", "grid.mover_old"), set()),
        # the two modes keep their buffers until the context goes: live exactly once each behind the switch-off
        "collider-sweep": (sweep_of(set_walls, st.set_collider_sweep), lambda: st.set_collider_sweep(False),
                           lambda t: t == "grid.sweep_counts", {"grid.sweep_counts"}),
        "mover-sweep": (sweep_of(set_pistons, st.set_mover_sweep), lambda: st.set_mover_sweep(False),
                        lambda t: t in msweep, msweep),
    }[feature]


@pytest.mark.parametrize("feature", ["colliders", "fields", "movers", "bonds", "bends", "areas", "bodies",
                                     "surfaces-of-colliders", "surfaces-of-movers", "collider-sweep", "mover-sweep"])
def test_replacing_a_step_set_leaks_nothing_and_frees_nothing_twice(gpe, feature):
    """64 particles with uids on, guarded.  The set with k = 1, a step, replaced with k = 3, a step, with k = 1 again, a
    step, cleared: after every call guard_check() reports no damage and no tag of the feature is live more than once
    (a leak of the commit path shows as a second live entry, a double free as a damaged report or a fault); after the
    clear no tag of the feature is live -- the two sweep modes, which keep their buffers, hold each of theirs once."""
    i = np.arange(64)
    pos = np.stack([10.0 + 3.0 * (i % 8), 10.0 + 3.0 * (i // 8)], axis=1).astype(np.float32)
    st = gpe.State(pos, np.ones(64, np.float32), world=(60.0, 60.0), flags=gpe._lib.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    set_, clear, mine, kept = _step_set_case(gpe, st, feature)

    def live():
        assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
        tags = [t for t, _, _, state in st.ctx.guard_registry() if state == "live" and mine(t)]
        assert len(tags) == len(set(tags)), tags
        return set(tags)
    assert live() == set()
    for k in (1, 3, 1):
        set_(k)
        assert live(), (feature, k)                        # (the predicate names tags the feature really uses)
        st.update(1 / 60)
        assert live(), (feature, k)
    clear()
    assert live() == kept
    st.close()


# ---- primitives on user buffers of exactly n elements ---------------------------------------------------------------
SORT_SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 8191, 8193, (3 << 20) - 1, (3 << 20) + 1]


@pytest.mark.parametrize("safe_sort", [False, True], ids=["onesweep", "safe-sort"])
@pytest.mark.parametrize("words", WORDS, ids=["words0", "words1"])
def test_primitives_on_exact_user_buffers(gpe, guard, words, safe_sort):
    guard.words = words
    ctx = gpe.Context(flags=gpe._lib.FLAG_SAFE_SORT if safe_sort else 0)
    for n in SORT_SIZES:
        rng = np.random.default_rng(n)
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        vals = np.arange(n, dtype=np.uint32)
        kb, vb = gpe.GpuBuffer(ctx, keys), gpe.GpuBuffer(ctx, vals)
        assert kb.capacity_bytes() == 4 * n
        ctx.call("gpe_sort_pairs_u32", kb.dptr, vb.dptr, n)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(kb.download(), keys[order]), n
        assert np.array_equal(vb.download(), vals[order]), n
        kb.free(); vb.free()
    for n in [1, 63, 64, 65, 4095, 4096, 4097, 8191, 8193]:
        rng = np.random.default_rng(n + 1)
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        for shift in (0, 24):
            ka, va = gpe.GpuBuffer(ctx, keys), gpe.GpuBuffer(ctx, vals)
            kb, vb = gpe.GpuBuffer(ctx, np.zeros(n, np.uint32)), gpe.GpuBuffer(ctx, np.zeros(n, np.uint32))
            hist = gpe.GpuBuffer(ctx, np.zeros(256, np.uint32))
            ctx.call("gpe_sort_histogram_u32", ka.dptr, n, shift, hist.dptr)
            ctx.call("gpe_sort_scatter_pass_u32", ka.dptr, va.dptr, kb.dptr, vb.dptr, n, shift)
            digit = (keys >> np.uint32(shift)) & np.uint32(255)
            order = np.argsort(digit, kind="stable")
            assert np.array_equal(hist.download(), np.bincount(digit, minlength=256).astype(np.uint32)), (n, shift)
            assert np.array_equal(kb.download(), keys[order]) and np.array_equal(vb.download(), vals[order]), (n, shift)
            for b in (ka, va, kb, vb, hist):
                b.free()
    for n in SORT_SIZES + [(1 << 24) + 1]:
        rng = np.random.default_rng(n % 1000)
        data = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        buf = gpe.GpuBuffer(ctx, data)
        ctx.call("gpe_inclusive_scan_u32", buf.dptr, n)
        assert np.array_equal(buf.download(), np.cumsum(data, dtype=np.uint64).astype(np.uint32)), n
        buf.free()
    ctx.close()


def test_gpu_buffer_growth(gpe, guard, request):
    ctx = gpe.Context()
    _rerun(request, "test_gpu_primitives", "test_gpu_buffer_push_replace_download_last", ctx=ctx)
    ctx.close()


@pytest.mark.parametrize("test", ["test_grid_build_cell_ids_sort_and_build_collision_cells_list", "test_sort_particles",
                                  "test_sort_small_sized_array", "test_inclusive_prefix_sum_resize"])
def test_reference_vectors(gpe, guard, request, test):
    ctx = gpe.Context(mode=gpe.MODE_COMPAT)
    _rerun(request, "test_gpu_reference_vectors", test, ctx=ctx)
    ctx.close()


# ---- the existing scenes, guarded -------------------------------------------------------------------------------------
COMPAT = _cases([
    ("step-dense", "test_gpu_parity_step", "test_step_matches_oracle", dict(kind="dense", n=20_000, steps=8)),
    ("step-mixed-radii", "test_gpu_parity_step", "test_step_matches_oracle", dict(kind="mixed_radii", n=20_000, steps=8)),
    ("step-one-particle", "test_gpu_parity_step", "test_step_matches_oracle", dict(kind="reference_density", n=1, steps=3)),
    ("phantom-cells-at-minus-one", "test_gpu_parity_step", "test_negative_phantom_cells_and_unused_alias", {}),
    ("module-calls", "test_gpu_parity_step", "test_module_calls_compose_like_step", {}),
    ("add-particles", "test_gpu_parity_step", "test_add_particles_matches_fresh_system", {}),
    ("grid-buffers-on-demand", "test_gpu_parity_step", "test_native_context_allocates_grid_buffers_on_demand", {}),
    ("switching-pipelines", "test_gpu_parity_step", "test_switching_pipelines_mid_run_keeps_the_trajectory", {}),
])

NATIVE = _cases([
    ("direct-slot", "test_gpu_native", "test_native_step_matches_oracle", dict(kind="uniform", n=20_000, steps=12, density=None)),
    ("dense-cells", "test_gpu_native", "test_native_step_matches_oracle", dict(kind="uniform", n=30_000, steps=6, density=1.0)),
    ("windows-8x8", "test_gpu_native", "test_native_step_matches_oracle", dict(kind="uniform", n=60_000, steps=4, density=2.0)),
    ("phantoms-of-big-particles", "test_gpu_native", "test_native_step_matches_oracle", dict(kind="mixed", n=20_000, steps=8, density=0.02)),
    ("counting-sort-tiles", "test_gpu_native", "test_other_tile_forms_give_the_same_bits", dict(flag="FLAG_COUNTING_SORT_TILES")),
    ("xcd-eighths", "test_gpu_native", "test_other_tile_forms_give_the_same_bits", dict(flag="FLAG_XCD_EIGHTHS")),
    ("fused-histograms", "test_gpu_native", "test_other_tile_forms_give_the_same_bits", dict(flag="FLAG_FUSED_HISTOGRAMS")),
    ("half-tiles-and-no-half-tiles", "test_gpu_native", "test_half_tiles_take_what_runs_over_the_direct_slot_form", {}),
    ("more-than-32-hinted-tiles", "test_gpu_native", "test_more_hinted_tiles_than_the_front_workgroups_take", {}),
    ("hints-two-collides-per-grid", "test_gpu_native", "test_hinted_tiles_when_a_host_collides_twice_on_one_grid", {}),
    ("spill-arena", "test_gpu_native", "test_native_spill_arena_is_exact", {}),
    ("crushed-cells-90-150-240", "test_gpu_native", "test_native_crushed_cells_are_exact", dict(sizes=(90, 150, 240))),
    ("crushed-cells-300-640-1000", "test_gpu_native", "test_native_crushed_cells_are_exact", dict(sizes=(300, 640, 1000))),
    ("crushed-cells-30-1100-257", "test_gpu_native", "test_native_crushed_cells_are_exact", dict(sizes=(30, 1100, 257))),
    ("cells-of-9-to-16-a", "test_gpu_native", "test_native_cells_of_nine_to_sixteen_members_are_exact", dict(n=2400)),
    ("cells-of-9-to-16-b", "test_gpu_native", "test_native_cells_of_nine_to_sixteen_members_are_exact", dict(n=4200)),
    ("stragglers-overflow-into-a-sort", "test_gpu_native", "test_stragglers_flying_into_empty_space_are_not_lost", {}),
    ("sort-every-step-and-kept-table", "test_gpu_native", "test_kept_block_table_equals_sorting_every_step", {}),
    ("kept-table-drift", "test_gpu_native", "test_kept_block_table_survives_drift_in_every_direction", {}),
    ("table-kept-again", "test_gpu_native", "test_table_is_kept_again_after_a_spell_of_sorting_every_step", {}),
    ("roster-stamp", "test_gpu_native", "test_roster_stamp_follows_every_sort", {}),
    ("world-of-63636-columns", "test_gpu_native", "test_native_sparse_huge_worlds", dict(world=(70000.0, 900.0), n=150_000)),
    ("world-too-wide-compat", "test_gpu_native", "test_native_sparse_huge_worlds", dict(world=(72000.0, 900.0), n=50_000)),
    ("walls-and-unused-alias", "test_gpu_native", "test_native_walls_and_unused_alias", {}),
    ("coincident-particles", "test_gpu_native", "test_native_coincident_particles", {}),
    ("out-of-box-compat", "test_gpu_native", "test_native_out_of_box_scene_uses_compat_kernels", {}),
    ("overfull-windows-compat", "test_gpu_native", "test_native_overfull_windows_use_compat_kernels", {}),
    ("mouse-blob-hand-over", "test_gpu_native", "test_native_mouse_blob_hands_over_without_error", {}),
    ("isolated-pairs", "test_gpu_pair_math", "test_isolated_edge_pairs_match_oracle", dict(native=True)),
    ("crushed-blob-mixed-radii", "test_gpu_pair_math", "test_crushed_blobs_of_mixed_radii_match_oracle", dict(seed=11, negative=False)),
    ("crushed-blob-negative-radii", "test_gpu_pair_math", "test_crushed_blobs_of_mixed_radii_match_oracle", dict(seed=13, negative=True)),
    ("negative-zero-walls", "test_gpu_pair_math", "test_negative_zero_wall_cells_match_oracle", {}),
] + [("fuzz-%d" % s, "test_gpu_native", "test_native_fuzz_scenes_match_oracle", dict(seed=s)) for s in range(0, 24, 2)])

GROWTH = _cases([
    ("add-beyond-capacity", "test_gpu_native", "test_native_add_particles", {}),
    ("growth-then-module-calls", "test_gpu_native", "test_native_growth_then_module_calls", {}),
    ("remove-add-remove-grow", "test_gpu_remove", "test_remove_add_remove_grow_then_step", {}),
    ("removal-in-a-live-run", "test_gpu_remove", "test_removal_in_a_live_native_run", {}),
    ("largest-leaves-new-cell-size", "test_gpu_remove", "test_removing_the_largest_particle_shrinks_the_cell_size", {}),
    ("circle", "test_gpu_remove", "test_circle_removes_exactly_the_float32_disc", {}),
    ("circle-none", "test_gpu_remove", "test_circle_that_catches_nothing_changes_nothing", {}),
    ("remove-errors", "test_gpu_remove", "test_errors_leave_the_context_as_it_was", {}),
    ("set-world-grow", "test_gpu_api_sequences", "test_set_world_mid_native_run", dict(case="grow")),
    ("save-load-add-rule", "test_gpu_api_sequences", "test_save_load_keeps_the_context_constants", dict(case="add_rule", mode_name="native")),
    ("uids-late-on-off", "test_gpu_uids", "test_off_on_off", {}),
    ("uids-set", "test_gpu_uids", "test_set_uids_and_next_uid", {}),
    ("uids-save-load", "test_gpu_uids", "test_save_load", dict(mode="native")),
    ("uids-run-100k", "test_gpu_uids", "test_identity_through_a_run_and_no_effect_on_physics", dict(mode="native", n=100_000)),
] + [("mask-%s-%s-%d" % (m, k, n), "test_gpu_remove", "test_mask_removal_equals_fresh_twin_and_oracle", dict(mode=m, n=n, kind=k))
     for m in ("native", "compat") for n, k in ((2, "first"), (1000, "p0.99"), (20_000, "p0.5"), (20_000, "none"), (20_000, "run"))]
  + [("find-uids-%s-%d" % (m, n), "test_gpu_uids", "test_find", dict(mode=m, n=n)) for m in ("native", "compat") for n in (1, 2049)]
  + [("remove-by-uid-%s-%d" % (m, n), "test_gpu_uids", "test_remove_by_uid_equals_mask_removal", dict(mode=m, n=n))
     for m in ("native", "compat") for n in (2, 2049, 100_000)])

QUERIES = _cases([
    ("capacity-0-1-count-native", "test_gpu_query", "test_capacity_below_count_writes_exactly_capacity_rows", dict(mode="native")),
    ("capacity-0-1-count-compat", "test_gpu_query", "test_capacity_below_count_writes_exactly_capacity_rows", dict(mode="compat")),
    ("pick-native", "test_gpu_query", "test_pick_is_the_nearest_containing_disc", dict(mode="native")),
    ("pick-compat", "test_gpu_query", "test_pick_is_the_nearest_containing_disc", dict(mode="compat")),
    ("predicate-1", "test_gpu_query", "test_queries_equal_the_float32_predicate", dict(mode="native", n=1)),
    ("predicate-2049", "test_gpu_query", "test_queries_equal_the_float32_predicate", dict(mode="native", n=2049)),
    ("predicate-200k", "test_gpu_query", "test_queries_equal_the_float32_predicate", dict(mode="compat", n=200_000)),
    ("after-100-steps-uids", "test_gpu_query", "test_queries_after_100_native_steps", dict(uids_on=True)),
    ("circle-is-what-removal-removes", "test_gpu_query", "test_circle_query_is_what_removal_removes", dict(mode="native")),
    ("queried-twin", "test_gpu_query", "test_queried_run_is_bit_identical_to_an_unqueried_twin", {}),
    ("errors", "test_gpu_query", "test_errors_leave_outputs_and_context_untouched", {}),
])

SEQUENCES = _cases(
    [("native-equals-compat-%d" % s, "test_gpu_native", "test_random_api_sequences_native_equals_compat", dict(seed=s)) for s in (1, 2, 3)]
    + [("against-the-oracle-%s-%d" % (m, s), "test_gpu_api_sequences", "test_random_api_sequences_match_the_oracle", dict(seed=s, mode_name=m))
       for m, s in (("native", 1), ("native", 2), ("compat", 2))]
    + [("interactive-%s-%d" % (m, s), "test_gpu_api_sequences", "test_random_interactive_sequences_match_the_oracle", dict(seed=s, mode_name=m))
       for m, s in (("native", 1), ("native", 2), ("compat", 2))]
    + [("observed-%s-%d" % (m, s), "test_gpu_api_sequences", "test_random_observed_sequences_match_the_oracle", dict(seed=s, mode_name=m))
       for m, s in (("native", 1), ("compat", 2))])

_LG = "test_local_group_in_one_process_equals_single_context"
SHARDED = _cases(
    [("%d-ranks%s" % (ws, "-overlap" if o else ""), "test_gpu_sharded", _LG, dict(ws=ws, n=n, world=w, gravity=g, overlap=o))
     for ws, n, w, g in ((2, 40_000, (420.0, 300.0), (40.0, 0.0)), (4, 60_000, (500.0, 380.0), (25.0, -30.0))) for o in (False, True)]
    + [("pile-up-grows-and-recuts%s" % ("-overlap" if o else ""), "test_gpu_sharded", _LG,
        dict(ws=2, n=40_000, world=(420.0, 300.0), gravity=(0.0, -80.0), overlap=o)) for o in (False, True)]
    + [("dense-patch-astride-the-cut%s" % ("-overlap" if o else ""), "test_gpu_sharded",
        "test_dense_patch_on_the_border_between_two_ranks", dict(overlap=o)) for o in (False, True)]
    + [("edge-scene-%s" % s, "test_gpu_pair_math", "test_edge_scenes_local_group_equals_single_context", dict(scene=s))
       for s in ("isolated", "blobs_negative")]
    # the refusals of tests/test_gpu_sharded_fuzz.py: the rows that had no place were dropped inside their buffers
    + [("refusal-%s" % c, "test_gpu_sharded_fuzz", "test_refusal_is_loud_on_every_rank", dict(case=c))
       for c in ("no-slot", "holes", "capacity", "recv-overflow", "empty-after-re-cut")]
    + [("fuzz-%d" % s, "test_gpu_sharded_fuzz", "test_sharded_fuzz_scenes_equal_single_context_and_oracle", dict(seed=s))
       for s in (5, 8, 21)])


@pytest.mark.parametrize("module,test,params", COMPAT)
def test_compat_scenes(guard, request, module, test, params):
    _rerun(request, module, test, **params)


@pytest.mark.parametrize("module,test,params", NATIVE)
def test_native_tile_forms(guard, request, module, test, params):
    _rerun(request, module, test, **params)


@pytest.mark.parametrize("module,test,params", GROWTH)
def test_growth_and_shrinkage(guard, request, module, test, params):
    _rerun(request, module, test, **params)


@pytest.mark.parametrize("module,test,params", QUERIES)
def test_queries(guard, request, module, test, params):
    _rerun(request, module, test, **params)


@pytest.mark.parametrize("module,test,params", SEQUENCES)
def test_random_api_sequences(guard, request, module, test, params):
    _rerun(request, module, test, **params)


@pytest.mark.parametrize("module,test,params", SHARDED)
def test_sharded_local_group(guard, request, module, test, params):
    _rerun(request, module, test, **params)


# (measured: 100 000 particles hand out 791 000 slots per step.  150 000 would need more than the 2^20 the first arena
# has before the lagged statistic can grow it, which the library reports as an unresolved step.)
ARENA_N, ARENA_WORLD = 100_000, (95.3, 95.3)


def test_spill_arena_grows_in_the_middle_of_a_forced_run(gpe, guard, oracle):
    """tests/test_gpu_native.py::test_native_spill_arena_is_exact's recipe (11 particles per unit area, kept on the
    native kernels by FLAG_NATIVE_FORCE, so every 8x8 tile goes through the spill arena) at 8 times the particles:
    a step hands out more than half of the arena's 2^20 slots, and the next one replaces the arena by one of twice the
    size -- the one buffer a native run releases in its middle, checked as it goes.  pipeline_info() and the registry
    prove the path; the positions are the oracle's."""
    L = gpe._lib
    pos, rad = gpe.scenes.uniform_cloud(ARENA_N, ARENA_WORLD, seed=12)
    st = gpe.State(pos, rad, world=ARENA_WORLD, mode=gpe.MODE_NATIVE, flags=L.FLAG_NATIVE_FORCE)
    sim = oracle.Sim(pos, rad, oracle.default_params(ARENA_WORLD[0], ARENA_WORLD[1], 0.5))

    def arena(state):
        return [p for t, p, _, s in st.ctx.guard_registry() if t == "native.arena" and s == state]
    before, used, spills = arena("live"), [], []
    assert len(before) == 1 and arena("released") == []
    for s in range(5):
        st.update(1 / 60, resort=(s == 0)); sim.step(1 / 60, resort=(s == 0))
        st.ctx.sync()
        info = st.ctx.pipeline_info()
        used.append(info["arena_slots"]); spills.append(info["overflow_spills"])
        print("step %d: arena slots handed out %d, spill windows %d, arena bytes %r" % (s, used[-1], spills[-1], arena("live")))
        assert info["pipeline"] == L.PIPELINE_NATIVE and info["compat_steps"] == 0, info
    assert max(spills) > 0, spills
    assert max(used) > (1 << 19), used                     # more than half of the 2^20 slots: what makes it grow
    assert arena("released") == before, (arena("released"), before)      # the first arena went (and was checked)
    assert len(arena("live")) == 1 and arena("live")[0] >= 2 * before[0] - 256, (arena("live"), before)
    got, want = st.positions(), sim.pos
    assert np.array_equal(got, want), "max abs difference %g" % np.abs(got - want).max()
    st.close(); sim.close()


def test_removing_all_but_one_and_none(gpe, guard):
    """Mask removal of all but one particle, then of none, then steps: as a fresh context on the survivor."""
    st, world, pos, rad = _small_state(gpe, n=5000, gravity=(0.0, -9.0))
    st.update(1 / 60, resort=True)
    p, q, r = st.positions(), st.previous_positions(), st.radii()
    mask = np.ones(len(r), np.uint8)
    mask[-1] = 0
    assert st.remove_particles(mask) == len(r) - 1
    assert st.remove_particles(np.zeros(1, np.uint8)) == 0
    twin = gpe.State(p[-1:], r[-1:], world=world, gravity=(0.0, -9.0), prev=q[-1:])
    for s in range(3):
        st.update(1 / 60, resort=(s == 1))
        twin.update(1 / 60, resort=(s == 1))
    assert np.array_equal(st.positions(), twin.positions()) and np.array_equal(st.previous_positions(), twin.previous_positions())
    st.close(); twin.close()


def test_migrants_into_a_spill_window_local_group(gpe, guard):
    """tests/test_gpu_sharded.py's spill-blob scene (its migrants arrive in a spill window on steps that keep their
    table) over a local group of two ranks: bit-identical to the single-context run, every rank's zones clean."""
    lg = importlib.import_module(gpe.__name__ + ".local_group")
    world, pos, prev, rad = _module("test_gpu_sharded")._spill_blob_scene()
    steps, dt, every = 12, 1 / 60, 7
    run = lg.LocalShardedRun(pos, rad, world, 2, prev=prev)
    run.run(dt, steps, resort_every=every, resort_first=True)
    owned = run.owned()
    infos = [c.pipeline_info() for c in run.ctx]
    run.close()
    ref = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, prev=prev)
    ref.run(dt, steps, resort_every=every, resort_first=True)
    want_pos, want_prev = ref.positions(), ref.previous_positions()
    ref.close()
    seen = np.zeros(len(rad), bool)
    for r, (gid, p, q) in enumerate(owned):
        seen[gid] = True
        assert np.array_equal(p, want_pos[gid]) and np.array_equal(q, want_prev[gid]), "rank %d" % r
        assert infos[r]["window_max"] > 2500, infos[r]          # the blob filled spill windows (the existing test's bound)
    assert seen.all()


def test_undersized_segments_drop_rows_inside_the_segment(gpe, guard):
    """Neighbour segments of a handful of rows (capacity_scale 0.002, what GPE_SHARD_CAP_SCALE=0.002 gives the torch
    front end): the run fails loudly, and the rows that did not fit were dropped, not written behind the segment."""
    lg = importlib.import_module(gpe.__name__ + ".local_group")
    n, world = 40_000, (420.0, 300.0)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=5)
    run = lg.LocalShardedRun(pos, rad, world, 2, gravity=(40.0, 0.0), capacity_scale=0.002)
    try:
        with pytest.raises(gpe.GpeError, match="segment overflowed"):      # (as tests/test_gpu_sharded.py asserts it)
            run.run(0.05, 14, resort_every=6, resort_first=True)
            for c in run.ctx:
                c.sync()
    finally:
        run.close()
