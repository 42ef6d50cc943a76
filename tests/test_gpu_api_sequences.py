"""GPU (-m gpu): sequences of host calls on one context, checked against the oracle model of a context
(tests/_oracle_model.py) bit for bit after every call that changes state.  The per-kernel and per-step tests compare
one operation at a time; these cover the host control code both pipelines share -- the cell-size and max-radius rules
after add / remove, reconfigure() after gpe_set_world / gpe_grid_set_max_radius / gpe_set_mode, snapshots, uids, the
wall clamp -- and the native pipeline's state carried across all of it.  Then the transitions no scene reaches by
itself: an understated grid radius (2r > cell size), the world growing past the allocated block table and rosters,
shrinking around or past the particles, a grid too wide for 16-bit cell coordinates, a box narrower than 2r, and
save / load after constants were changed through the C-ABI."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import _interactive_sequences as interactive
from _oracle_model import OracleModel, circle_mask

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _first_diff(got, want):
    g, w = _bits(got).reshape(len(got), -1), _bits(want).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    return "%d differ, first at %d: %s vs %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


def _compare(st, model, where):
    """Everything a host can read back, bit for bit: len, pos, prev, radius, uids / next_uid, max radius, cell size."""
    n = st.particles.len()
    assert n == len(model), "%s: len %d, model %d" % (where, n, len(model))
    p, q, r = model.arrays()
    for what, got, want in (("pos", st.positions(), p), ("prev", st.previous_positions(), q), ("radius", st.radii(), r)):
        assert np.array_equal(_bits(got), _bits(want)), "%s: %s %s" % (where, what, _first_diff(got, want))
    if model.uids is None:
        assert not st._uids_on(), "%s: uids are on, the model has them off" % where
    else:
        assert np.array_equal(st.uids(), model.uids), "%s: uids differ" % where
        assert st.next_uid() == model.next_uid, "%s: next_uid %d, model %d" % (where, st.next_uid(), model.next_uid)
    assert _bits(np.float32(st.particles.get_max_radius())) == _bits(model.max_radius), \
        "%s: max radius %r, model %r" % (where, st.particles.get_max_radius(), model.max_radius)
    assert _bits(np.float32(st.grid.cell_size())) == _bits(model.cell_size), \
        "%s: cell size %r, model %r" % (where, st.grid.cell_size(), model.cell_size)
    assert _bits(np.float32(st.grid.max_radius())) == _bits(model.grid_max_radius), where


def _upload(st, what, arr):
    ptr, nbytes = st.ctx.device_ptr(what)
    assert nbytes == arr.nbytes
    st.ctx.call("gpe_buffer_upload", ptr, _ptr(arr), arr.nbytes)


def _inside(p, world, margin):
    lo = np.float32(margin)
    hi = np.array(world, np.float32) - np.float32(margin)
    return np.clip(p, lo, np.maximum(hi, lo)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# 1. random call sequences against the model
# ------------------------------------------------------------------------------------------------------------------------
class _Counters:
    """pipeline_info() of every State a sequence used (save / load replaces it): native steps in all."""

    def __init__(self):
        self.native_steps = 0
        self.compat_steps = 0

    def retire(self, st, log):
        info = st.ctx.pipeline_info()
        assert info["roster_stamp"] == info["native_sorts"] & 0xFFFFFFFF, (info, log)
        self.native_steps += info["native_steps"]
        self.compat_steps += info["compat_steps"]


@pytest.mark.parametrize("seed", list(range(1, 7)))
@pytest.mark.parametrize("mode_name", ["native", "compat"])
def test_random_api_sequences_match_the_oracle(gpe, oracle, seed, mode_name):
    """60-100 random host calls on one State -- steps, gpe_run, module calls, re-sorts, mouse, gravity, world growth /
    shrink / regrowth, grid radii under, over and at the max radius, add, removal by mask / circle / uid, uids on / off /
    set, gpe_set_mode, writes through gpe_device_ptr, save -> load -> continue -- and the same calls on the oracle model:
    the same bits after every call that changes state."""
    L = gpe._lib
    mode = L.MODE_NATIVE if mode_name == "native" else L.MODE_COMPAT
    other = L.MODE_COMPAT if mode == L.MODE_NATIVE else L.MODE_NATIVE
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(5_000, 14_000))
    world0 = (float(rng.integers(160, 300)), float(rng.integers(90, 170)))
    pos, rad = gpe.scenes.uniform_cloud(n, world0, seed=seed)
    pos = _inside(pos, world0, 0.5)
    if seed % 2 == 0:
        # a blob at four times the density (over-capacity tiles, rosters that say "too many"), as the native fuzz has
        m = min(n // 2, 20_000 - n)
        corner = np.array([rng.random() * (world0[0] - 60.0) + 5.0, rng.random() * (world0[1] - 50.0) + 5.0], np.float32)
        blob = (rng.random((m, 2), dtype=np.float32) * np.array([50.0, 40.0], np.float32) + corner).astype(np.float32)
        pos = np.concatenate([pos, blob]); rad = np.concatenate([rad, np.full(m, 0.5, np.float32)])
    st = gpe.State(pos, rad, world=world0, mode=mode)
    model = OracleModel(oracle, pos, rad, world=world0)
    counters = _Counters()
    log = []
    world = world0
    # the operations every sequence must include, spread over it; the rest are drawn at random
    must = ["world_grow", "world_shrink_in", "world_shrink_out", "world_back", "grid_under", "grid_over", "grid_exact",
            "save_load", "remove_mask", "remove_circle", "remove_uid", "uids_set", "uids_toggle", "set_mode", "stop",
            "teleport", "add", "module", "resort", "mouse", "gravity", "run"]
    n_ops = int(rng.integers(60, 101))
    slots = rng.choice(n_ops, size=len(must), replace=False)
    plan = {int(s): name for s, name in zip(slots, must)}
    drawn = ["step", "step", "step", "run", "module", "resort", "mouse", "gravity", "add", "remove_mask",
             "remove_circle", "remove_uid", "uids_toggle", "uids_set", "grid_under", "grid_over", "grid_exact",
             "world_grow", "world_shrink_in", "world_back", "set_mode", "stop", "teleport", "save_load"]
    tmp = tempfile.TemporaryDirectory()
    try:
        for i in range(n_ops):
            op = plan.get(i) or drawn[int(rng.integers(0, len(drawn)))]
            cnt = len(model)
            if op == "step":
                k = int(rng.integers(1, 6)); resort = bool(rng.integers(0, 4) == 0)
                for s in range(k):
                    st.update(DT, resort=(resort and s == 0)); model.step(DT, resort=(resort and s == 0))
                log.append("step x%d%s" % (k, " resort" if resort else ""))
            elif op == "run":
                k = int(rng.integers(5, 40)); every = int(rng.choice([0, 7, 16])); first = bool(rng.integers(0, 2))
                st.run(DT, k, resort_every=every, resort_first=first)
                model.run(DT, k, resort_every=every, resort_first=first)
                log.append("run %d every %d first %s" % (k, every, first))
            elif op == "module":
                st.grid.update(); st.collision_system.solve_collisions(); st.particles.update_positions(DT)
                model.module_calls(DT)
                log.append("module calls")
            elif op == "resort":
                st.particles.sort_by_cell_id(); model.morton_resort()
                log.append("morton resort")
            elif op == "mouse":
                pressed = bool(rng.integers(0, 2))
                at = (float(np.float32(rng.random() * world[0])), float(np.float32(rng.random() * world[1])))
                st.particles.mouse_click_callback(pressed, at); model.set_mouse(pressed, *at)
                log.append("mouse %s %s" % (pressed, at))
            elif op == "gravity":
                g = (float(rng.choice([0.0, 3.0, -3.0])), float(rng.choice([0.0, -9.81, 9.81])))
                st.ctx.call("gpe_set_gravity", g[0], g[1]); model.set_gravity(*g)
                log.append("gravity %s" % (g,))
            elif op == "add":
                m = int(rng.integers(1, 300)); big = bool(rng.integers(0, 3) == 0)
                p_new, r_new = gpe.scenes.mixed_radius_cloud(m, world, seed=int(rng.integers(1 << 30)),
                                                             radii=(0.5, 1.0, 1.5) if big else (0.5,))
                p_new = _inside(p_new, world, 2.0)
                st.add_particles(p_new, r_new); model.add(p_new, r_new)
                log.append("add %d%s" % (m, " mixed radii" if big else ""))
            elif op == "remove_mask":
                mask = (rng.random(cnt) < rng.choice([0.001, 0.02, 0.1])).astype(np.uint8)
                if mask.all():
                    mask[0] = 0
                got = st.remove_particles(mask); want = model.remove_mask(mask)
                assert got == want, (seed, i, log)
                log.append("remove mask %d" % got)
            elif op == "remove_circle":
                c = (float(np.float32(rng.random() * world[0])), float(np.float32(rng.random() * world[1])))
                r = float(np.float32(rng.random() * 0.1 * min(world)))
                if circle_mask(model.arrays()[0], c[0], c[1], r).all():
                    continue
                got = st.remove_particles_in_circle(c, r); want = model.remove_circle(*c, r)
                assert got == want, (seed, i, log)
                log.append("remove circle %s r %g: %d" % (c, r, got))
            elif op == "remove_uid":
                if model.uids is None:
                    st.enable_uids(); model.enable_uids()
                    log.append("uids on")
                q = rng.choice(np.append(model.uids, [model.next_uid, 0xFFFFFFFE]).astype(np.uint32),
                               size=int(rng.integers(1, max(2, cnt // 20))))
                if np.isin(model.uids, q).all():
                    continue
                got = st.remove_particles_by_uid(q); want = model.remove_uids(q)
                assert got == want, (seed, i, log)
                log.append("remove %d uids: %d" % (len(q), got))
            elif op == "uids_toggle":
                on = model.uids is None
                st.enable_uids(on); model.enable_uids(on)
                log.append("uids %s" % ("on" if on else "off"))
            elif op == "uids_set":
                u = rng.choice(3 * cnt + 10, size=cnt, replace=False).astype(np.uint32)
                st.set_uids(u); model.set_uids(u)
                nxt = model.next_uid + int(rng.integers(0, 1000))
                st.set_next_uid(nxt); model.set_next_uid(nxt)
                log.append("set uids, next %d" % nxt)
            elif op in ("world_grow", "world_shrink_in", "world_shrink_out", "world_back"):
                p = model.arrays()[0]
                if op == "world_grow":                 # past the allocated block table, straggler lists and rosters
                    f = float(rng.choice([6.0, 12.0, 25.0]))
                    w = (float(np.float32(world0[0] * f)), float(np.float32(world0[1] * f)))
                elif op == "world_shrink_in":          # every particle stays inside [0, world]
                    w = (float(np.float32(p[:, 0].max() + 0.25)), float(np.float32(p[:, 1].max() + 0.25)))
                elif op == "world_shrink_out":         # some are left outside: the next integration clamps them
                    w = (float(np.float32(world0[0] * 0.7)), float(np.float32(world0[1] * 0.75)))
                else:
                    w = world0
                st.ctx.call("gpe_set_world", w[0], w[1]); model.set_world(*w)
                world = w
                info = st.ctx.pipeline_info()
                log.append("%s %s: pipeline %d reason %d" % (op, w, info["pipeline"], info["reason"]))
                if op == "world_shrink_out" and mode == L.MODE_NATIVE:
                    assert info["reason"] == L.REASON_OUT_OF_BOX, (info, log)
            elif op in ("grid_under", "grid_over", "grid_exact"):
                # understated only down to 0.92: below 1 / 1.1 a particle can sit in two cells of one colour, and
                # the colour passes race on it (test_understated_grid_radius_* below)
                f = {"grid_under": rng.uniform(0.92, 0.99), "grid_over": rng.uniform(1.5, 3.0), "grid_exact": 1.0}[op]
                r = float(np.float32(model.max_radius) * np.float32(f))
                st.ctx.call("gpe_grid_set_max_radius", r); model.grid_set_max_radius(r)
                info = st.ctx.pipeline_info()
                log.append("%s %g: pipeline %d reason %d" % (op, r, info["pipeline"], info["reason"]))
            elif op == "set_mode":
                k = int(rng.integers(1, 5))
                st.ctx.call("gpe_set_mode", other); model.set_mode(other)
                for _ in range(k):
                    st.update(DT); model.step(DT)
                st.ctx.call("gpe_set_mode", mode); model.set_mode(mode)
                log.append("mode %d for %d steps" % (other, k))
            elif op == "stop":
                now = np.ascontiguousarray(st.positions())
                _upload(st, L.PREV, now); model.stop_all()
                log.append("prev = pos")
            elif op == "teleport":
                who = rng.choice(cnt, size=max(1, cnt // 10), replace=False)
                where = _inside(rng.random((len(who), 2), dtype=np.float32) * np.array(world, np.float32), world, 2.0)
                now, before = np.ascontiguousarray(st.positions()), np.ascontiguousarray(st.previous_positions())
                now[who] = where; before[who] = where
                _upload(st, L.POS, now); _upload(st, L.PREV, before); model.teleport(who, where)
                log.append("teleport %d" % len(who))
            elif op == "save_load":
                path = os.path.join(tmp.name, "snap_%d.npz" % i)
                st.save(path)
                counters.retire(st, log)
                st.close()
                st = gpe.State.load(path, mode=mode)
                log.append("save / load")
            _compare(st, model, "seed %d %s op #%d (%s)\n  %s" % (seed, mode_name, i, op, "\n  ".join(log)))
        counters.retire(st, log)
        if mode == L.MODE_NATIVE:
            assert counters.native_steps > 0, log
        else:
            assert counters.compat_steps > 0, log
    finally:
        st.close(); model.close(); tmp.cleanup()


@pytest.mark.parametrize("seed", interactive.SEEDS)
@pytest.mark.parametrize("mode_name", ["native", "compat"])
def test_random_interactive_sequences_match_the_oracle(gpe, oracle, seed, mode_name):
    """65-70 host calls on one State, planned by tests/_interactive_sequences.py: the calls of the test above, and between
    them keyed edits by index and by uid (every field subset, absent uids, particles moved outside the world and back, a
    new largest radius and the largest shrunk, with and without a grid override pending), kicks of all three ops (counted,
    and uncounted with the next step enqueued behind them), gpe_add_particles_free with every flag combination, region
    queries, picks, contact and cluster queries and flood selections at capacities below, at and above their counts.
    After every call the State holds the model's bits; every query returns the model's rows and writes nothing behind
    them; read-only calls, dry runs, adds of nothing and kicks leave native_sorts, roster_stamp and the step counters
    alone; and the sequence reached what tests/test_interactive_sequences_cpu.py says it reaches."""
    run = interactive.Sequence(interactive.plan(seed), oracle, gpe=gpe, mode_name=mode_name, compare=_compare)
    try:
        run.run()
        print("\nseed %d %s: %d ops, native %d / compat %d steps, %d particles at the end; coverage %s" % (
            seed, mode_name, len(run.plan.ops), run.native_steps, run.compat_steps, len(run.model), dict(run.cov)))
        if mode_name == "native":
            assert run.native_steps > 0, run.log
        else:
            assert run.compat_steps > 0, run.log
        run.cov.check(run.plan.spawn_flags)
    finally:
        run.close()


@pytest.mark.parametrize("seed", interactive.SEEDS)
@pytest.mark.parametrize("mode_name", ["native", "compat"])
def test_random_observed_sequences_match_the_oracle(gpe, oracle, seed, mode_name):
    """The sequences of the test above with the observers in them (interactive.plan_observed: the same operations, and
    some 150 more between them): the tracer recorder and the run monitor armed all along, with different `every`, ended
    and begun anew three times and around every save / load; a frame and a gpe_tracers_read straight after each thing
    that leaves the tracers' slot table stale; frames and reads of both across the growth, the spell in the other mode,
    the shrunken world, teleports, stops, edits outside the world and kicks; rings that wrap; consuming reads; reads at
    capacities below, at and above the held count into sentinel-filled arrays; the refused begins; gpe_measure; and
    gpe_cast_rays, gpe_query_segment and gpe_query_nearest straight after the growth, the shrink, a removal, a radius
    edit and a grid override, and in the other mode.  Every frame, record, hit, row and neighbour equals the models of
    tests/_tracers_model.py, _monitor_model.py, _ray_model.py and _nearest_model.py (the monitor's five sums within the
    header's bound, everything else bit for bit); none of these calls moves a counter or a particle; and the sequence
    reached what tests/test_interactive_sequences_cpu.py says it reaches."""
    run = interactive.ObservedSequence(interactive.plan_observed(seed), oracle, gpe=gpe, mode_name=mode_name, compare=_compare)
    try:
        run.run()
        print("\nobserved seed %d %s: %d ops, native %d / compat %d steps, %d particles at the end; coverage %s" % (
            seed, mode_name, len(run.plan.ops), run.native_steps, run.compat_steps, len(run.model), dict(run.cov)))
        if mode_name == "native":
            assert run.native_steps > 0, run.log
        else:
            assert run.compat_steps > 0, run.log
        run.cov.check(run.plan.spawn_flags)
        run.cov.check_observed()
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. an understated grid radius: 2r > cell size, a particle overlaps up to eight neighbour cells and keeps three
# ------------------------------------------------------------------------------------------------------------------------
def _stats(st, acc):
    info = st.ctx.pipeline_info()
    for k in ("overflow_tiles", "overflow_subtiles", "overflow_spills", "arena_slots", "window_max"):
        acc[k] = max(acc.get(k, 0), info[k])
    return info


def _understated_scene(gpe):
    """Radii 0.5 .. 2, a crowded corner and a pile crowded far beyond it (half tiles, over-capacity windows, the arena)."""
    n = 40_000
    world = gpe.scenes.world_for(n, density=0.04)
    pos, rad = gpe.scenes.mixed_radius_cloud(n, world, seed=31, radii=(0.5, 1.0, 2.0))
    rng = np.random.default_rng(32)
    pos[:1500] = (rng.random((1500, 2), dtype=np.float32) * np.float32(28.0) + np.float32(4.0)).astype(np.float32)
    pos[1500:2000] = (rng.random((500, 2), dtype=np.float32) * np.float32(6.0) + np.float32(150.0)).astype(np.float32)
    return _inside(pos, world, 2.0), rad, world


def _understated_state(gpe, flag, factor):
    L = gpe._lib
    pos, rad, world = _understated_scene(gpe)
    g = (2.0, -9.81)
    st = gpe.State(pos, rad, world=world, gravity=g, flags=0 if flag == "default" else getattr(L, flag))
    r = float(np.float32(2.0) * np.float32(factor))
    st.ctx.call("gpe_grid_set_max_radius", r)
    return st, (pos, rad, world, g, r)


def _report(st, flag, what, reason0, acc):
    info = st.ctx.pipeline_info()
    print("\n%s [%s]: configure reason %d; pipeline %d reason %d, native %d / compat %d steps; max overflow_tiles %d "
          "subtiles %d spills %d arena %d window %d" % (
              what, flag, reason0, info["pipeline"], info["reason"], info["native_steps"], info["compat_steps"],
              acc["overflow_tiles"], acc["overflow_subtiles"], acc["overflow_spills"], acc["arena_slots"],
              acc["window_max"]))
    return info


@pytest.mark.parametrize("flag", ["default", "FLAG_COUNTING_SORT_TILES"])
def test_understated_grid_radius_matches_the_oracle(gpe, oracle, flag):
    """The grid radius 0.93 x the true maximum (cell 4.09 for r = 2: understated, but still wider than 2r, so the
    colour passes' invariant -- cells of one colour share no particle -- holds): against the oracle bit for bit over 30
    steps with gravity and re-sorts, on the default tile form and on the counting-sort tiles."""
    L = gpe._lib
    st, (pos, rad, world, g, r) = _understated_state(gpe, flag, 0.93)
    model = OracleModel(oracle, pos, rad, world=world, gravity=g)
    model.grid_set_max_radius(r)
    reason0 = st.ctx.pipeline_info()["reason"]
    acc = {}
    oracle.set_threads(8)
    try:
        for s in range(30):
            rs = s in (0, 12, 25)
            st.update(DT, resort=rs); model.step(DT, resort=rs)
            _stats(st, acc)
            if s % 6 == 5 or s in (0, 29):
                _compare(st, model, "%s, step %d" % (flag, s))
    finally:
        oracle.set_threads(1)
    st.ctx.sync()
    info = _report(st, flag, "grid radius 0.93 x", reason0, acc)
    if info["native_steps"] == 0:
        assert reason0 == L.REASON_DENSE_WINDOWS, info          # declined for a documented reason, not silently
    else:
        assert info["roster_stamp"] == info["native_sorts"] & 0xFFFFFFFF, info
        assert acc["overflow_tiles"] > 0, acc                    # the crowded corner ran over the direct-slot tiles
    st.close(); model.close()


@pytest.mark.parametrize("flag", ["default", "FLAG_COUNTING_SORT_TILES"])
def test_understated_grid_radius_below_2r_runs_safely(gpe, oracle, flag):
    """The grid radius 0.4 x the true maximum (cell 1.76 < 2r = 4): a particle overlaps up to eight neighbour cells,
    keeps three (grid.wgsl:68-90), and can sit in two cells of one colour.  The colour passes then update it from two
    lanes at once, as the reference's shader does -- no bits to match (gpe.h, gpe_grid_set_max_radius).  What must hold:
    the native kernels run it (or decline for a documented reason) without a device error, every particle stays finite
    and inside the box, and the cell size is the one asked for."""
    L = gpe._lib
    st, (pos, rad, world, g, r) = _understated_state(gpe, flag, 0.4)
    assert _bits(np.float32(st.grid.cell_size())) == _bits(np.float32(r) * np.float32(2.2))
    reason0 = st.ctx.pipeline_info()["reason"]
    acc = {}
    for s in range(30):
        st.update(DT, resort=s in (0, 12, 25))
        _stats(st, acc)
    st.ctx.sync()                                               # raises on a device-side error
    info = _report(st, flag, "grid radius 0.4 x", reason0, acc)
    _assert_cell_ids(st, oracle, "%s, crowded, after 30 steps" % flag)
    p = st.positions()
    assert np.isfinite(p).all()
    assert (p >= 0).all() and (p[:, 0] <= np.float32(world[0])).all() and (p[:, 1] <= np.float32(world[1])).all()
    if info["native_steps"] == 0:
        assert reason0 == L.REASON_DENSE_WINDOWS, info
    else:
        assert info["roster_stamp"] == info["native_sorts"] & 0xFFFFFFFF, info
    st.close()


def _assert_cell_ids(st, oracle, what):
    """gpe_grid_build (the compat kernels' copy of the three-phantom cap) against oracle.build_cell_ids, at the
    context's current positions: both the cell ids and the object ids, slot for slot.  (Like grid.wgsl, the build
    leaves the object ids of unused slots as the buffer held them: the oracle starts from the context's buffer.)"""
    before = st.grid.download_object_ids().copy()
    st.grid.build_cell_ids()
    cells, objs = oracle.build_cell_ids(st.positions(), st.radii(), np.float32(st.grid.cell_size()), object_ids=before)
    assert np.array_equal(st.grid.download_cell_ids(), cells), what + ": cell ids"
    assert np.array_equal(st.grid.download_object_ids(), objs), what + ": object ids"


def _overlap_masks(pos, rad, cs):
    """The 3 x 3 overlap of each particle (grid.wgsl:68-90 before the cap): bit k for neighbour k in scan order
    (y outer, x inner, centre skipped), as the binary32 is_obj_in_cell computes it."""
    cs = np.float32(cs)
    home = np.floor(pos / cs).astype(np.int64)
    sq = rad * rad
    masks = np.zeros(len(pos), np.uint32)
    k = 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            lo = ((home + np.array([dx, dy])).astype(np.float32) * cs).astype(np.float32)
            hi = (lo + cs).astype(np.float32)
            q = np.minimum(np.maximum(pos, lo), hi)
            d = (pos - q).astype(np.float32)
            masks |= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < sq).astype(np.uint32) << np.uint32(k)
            k += 1
    return home, masks


@pytest.mark.parametrize("flag", ["default", "FLAG_COUNTING_SORT_TILES"])
def test_understated_grid_radius_capped_phantoms_match_the_oracle(gpe, oracle, flag):
    """The grid radius 0.4 x the true maximum (cell 1.76 < 2r = 4) in a scene where no particle is written by two lanes
    of one colour pass: sparse r = 2 particles, each overlapping exactly one r = 0.5 partner placed around it, up to two
    cells from its home cell.  A partner spans at most 2 x 2 cells (four colours), so each colour pass handles each pair
    in at most one lane, and the step is reproducible.  The big particles overlap four to eight neighbour cells and keep
    three: some pairs meet in a kept phantom cell two cells from the big particle's home, others meet in no kept cell
    (the cap, or a partner outside the 3 x 3 block) and do not collide.  Bit for bit against the oracle, on the native kernels (both tile forms), and the cell ids of
    gpe_grid_build against oracle.build_cell_ids."""
    L = gpe._lib
    rng = np.random.default_rng(61)
    world = (600.0, 420.0)
    gx, gy = np.meshgrid(np.arange(12.0, world[0] - 12.0, 12.0), np.arange(12.0, world[1] - 12.0, 12.0))
    big = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    big += (rng.random(big.shape, dtype=np.float32) * np.float32(3.0) - np.float32(1.5)).astype(np.float32)
    theta = rng.random(len(big)) * 2.0 * np.pi
    dist = 2.5 * rng.uniform(0.6, 0.97, len(big))
    small = (big + np.stack([np.cos(theta), np.sin(theta)], 1) * dist[:, None]).astype(np.float32)
    m = len(big)
    pos = np.concatenate([big, small]).astype(np.float32)
    rad = np.concatenate([np.full(m, 2.0, np.float32), np.full(m, 0.5, np.float32)])
    st = gpe.State(pos, rad, world=world, mode=L.MODE_NATIVE, flags=0 if flag == "default" else getattr(L, flag))
    r = float(np.float32(2.0) * np.float32(0.4))
    st.ctx.call("gpe_grid_set_max_radius", r)
    model = OracleModel(oracle, pos, rad, world=world)
    model.grid_set_max_radius(r)
    cs = model.cell_size
    assert _bits(np.float32(st.grid.cell_size())) == _bits(cs)
    # what the scene exercises, from the oracle's cell ids: pairs that share a kept cell with the partner's home two
    # cells away, and pairs whose only meeting cells were dropped by the cap
    cells, _ = oracle.build_cell_ids(pos, rad, cs)
    cells = cells.reshape(-1, 4)
    home, masks = _overlap_masks(pos, rad, cs)
    capped = np.array([bin(int(v)).count("1") > 3 for v in masks[:m]])
    assert capped.all()                                    # every big particle overlaps more than three neighbours
    far_kept = dropped = 0
    for b in range(m):
        shared = set(cells[b].tolist()) & set(cells[m + b].tolist()) - {oracle.UNUSED_CELL_ID}
        if shared and np.abs(home[m + b] - home[b]).max() == 2:
            far_kept += 1
        if not shared:
            dropped += 1
    print("\ncapped phantoms [%s]: %d pairs, %d meet in a kept cell two cells from the big home, %d meet in no kept cell"
          % (flag, m, far_kept, dropped))
    assert far_kept > 20 and dropped > 20, (far_kept, dropped)
    _assert_cell_ids(st, oracle, "%s, before the steps" % flag)
    for s in range(8):
        st.update(DT, resort=(s == 0)); model.step(DT, resort=(s == 0))
        _compare(st, model, "%s, step %d" % (flag, s))
    _assert_cell_ids(st, oracle, "%s, after 8 steps" % flag)
    st.ctx.sync()
    info = st.ctx.pipeline_info()
    print("  pipeline %d reason %d, native %d / compat %d steps" % (info["pipeline"], info["reason"],
                                                                    info["native_steps"], info["compat_steps"]))
    assert info["pipeline"] == L.PIPELINE_NATIVE and info["native_steps"] == 8 and info["compat_steps"] == 0, info
    assert info["roster_stamp"] == info["native_sorts"] & 0xFFFFFFFF, info
    # the partners moved: the pairs did collide
    assert not np.array_equal(_bits(st.positions()), _bits(pos))
    st.close(); model.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. gpe_set_world mid native run
# ------------------------------------------------------------------------------------------------------------------------
def _world_scene(gpe, n=8000, world=(140.0, 100.0), seed=41):
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=seed)
    return _inside(pos, world, 0.5), rad, world


def _run_and_compare(st, model, steps, what, resort_every=8):
    for s in range(steps):
        rs = s % resort_every == 0
        st.update(DT, resort=rs); model.step(DT, resort=rs)
        if s % 10 == 9 or s == steps - 1:
            _compare(st, model, "%s, step %d" % (what, s))


@pytest.mark.parametrize("case", ["grow", "shrink_out", "too_wide", "below_2r"])
def test_set_world_mid_native_run(gpe, oracle, case):
    L = gpe._lib
    pos, rad, world = _world_scene(gpe)
    g = (0.0, -9.81)
    st = gpe.State(pos, rad, world=world, gravity=g, mode=L.MODE_NATIVE)
    model = OracleModel(oracle, pos, rad, world=world, gravity=g)
    _run_and_compare(st, model, 12, "before")
    assert st.ctx.pipeline_info()["native_steps"] == 12
    if case == "grow":
        # 17 x: 271 x 194 = 52.6 k 8x8-cell blocks instead of 16 x 12 = 192, 3.3 k 32x32-cell tiles instead of 12:
        # past the allocated block table, straggler lists and rosters
        w = (world[0] * 17.0, world[1] * 17.0)
        want_reason = L.REASON_NONE
    elif case == "shrink_out":
        w = (world[0] * 0.6, world[1] * 0.8)
        want_reason = L.REASON_OUT_OF_BOX
    elif case == "too_wide":
        w = (80_000.0, world[1])                 # floor(80000 / 1.1) = 72727 > 65000 cells across
        want_reason = L.REASON_GRID_TOO_WIDE
    else:
        w = (0.6, world[1])                      # narrower than 2r = 1: the wall clamp has lo = 0.5 > hi = 0.1
        want_reason = L.REASON_OUT_OF_BOX
    st.ctx.call("gpe_set_world", w[0], w[1]); model.set_world(*w)
    assert st.ctx.world() == (np.float32(w[0]), np.float32(w[1]))
    info = st.ctx.pipeline_info()
    print("\nset_world %s -> %s: pipeline %d reason %d" % (case, w, info["pipeline"], info["reason"]))
    assert info["reason"] == want_reason, info
    assert info["pipeline"] == (L.PIPELINE_NATIVE if want_reason == L.REASON_NONE else L.PIPELINE_COMPAT), info
    steps0 = info["native_steps"]
    _run_and_compare(st, model, 40, case)
    info = st.ctx.pipeline_info()
    print("  after 40 steps: pipeline %d reason %d, native steps %d" % (info["pipeline"], info["reason"],
                                                                        info["native_steps"] - steps0))
    if case == "grow":
        assert info["native_steps"] - steps0 == 40, info
        # ... and back: the kept (larger) allocations serve the original box again
        st.ctx.call("gpe_set_world", world[0], world[1]); model.set_world(*world)
        assert st.ctx.pipeline_info()["reason"] in (L.REASON_NONE, L.REASON_OUT_OF_BOX)
        _run_and_compare(st, model, 20, "grown back")
    if case == "shrink_out":
        # every particle is back inside: a world set again re-runs the box check
        st.ctx.call("gpe_set_world", w[0], w[1]); model.set_world(*w)
        info = st.ctx.pipeline_info()
        print("  set again: pipeline %d reason %d" % (info["pipeline"], info["reason"]))
        assert info["reason"] in (L.REASON_NONE, L.REASON_DENSE_WINDOWS), info
        _run_and_compare(st, model, 20, "shrunk, set again")
    st.ctx.sync()
    st.close(); model.close()


def test_set_world_before_particles(gpe, oracle):
    """gpe_set_world on a context without particles, then set and add: the particles live in the new box."""
    L = gpe._lib
    pos, rad, world = _world_scene(gpe, n=6000, world=(120.0, 90.0), seed=43)
    ctx = gpe.Context(world=(40.0, 30.0), mode=L.MODE_NATIVE)
    try:
        ctx.call("gpe_set_world", world[0], world[1])
        info = ctx.pipeline_info()
        assert info["reason"] == L.REASON_NO_PARTICLES, info
        assert ctx.world() == world
        st = gpe.State.__new__(gpe.State)           # a State around this context: the reference's module objects
        st.ctx = ctx
        st.particles = gpe.ParticleSystem.new_from_buffers(ctx, pos[:5000], rad[:5000])
        st.grid = gpe.Grid(ctx, st.particles)
        st.collision_system = gpe.CollisionSystem(ctx, 2, st.particles, st.grid)
        model = OracleModel(oracle, pos[:5000], rad[:5000], world=world)
        assert ctx.pipeline_info()["pipeline"] == L.PIPELINE_NATIVE
        _run_and_compare(st, model, 20, "set before particles")
        st.add_particles(pos[5000:], rad[5000:]); model.add(pos[5000:], rad[5000:])
        _run_and_compare(st, model, 20, "after add")
        info = ctx.pipeline_info()
        assert info["pipeline"] == L.PIPELINE_NATIVE and info["native_steps"] == 40, info
        ctx.sync()
        model.close()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. save / load after constants changed behind the State's back
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", ["native", "compat"])
@pytest.mark.parametrize("case", ["gravity", "world", "mouse", "grid_radius", "add_rule"])
def test_save_load_keeps_the_context_constants(gpe, case, mode_name):
    """A snapshot taken after gpe_set_gravity / gpe_set_world through ctx.call, with the mouse pressed, with the grid
    radius overridden, or after an add whose fmaxf rule picked a grid radius other than the one gpe_set_particles derives
    from the same radii (a negative radius of larger magnitude): the loaded State's next 10 steps are those of the run
    that was not interrupted."""
    L = gpe._lib
    mode = L.MODE_NATIVE if mode_name == "native" else L.MODE_COMPAT
    n = 20_000
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=51)
    if case == "add_rule":
        rad[7] = -0.6                                  # set: grid radius -0.6 (largest magnitude, sign kept)
    st = gpe.State(pos, rad, world=world, mode=mode)
    st.run(DT, 5, resort_every=0, resort_first=True)
    if case == "gravity":
        st.ctx.call("gpe_set_gravity", 1.0, -9.81)
    elif case == "world":
        st.ctx.call("gpe_set_world", world[0] * 0.9, world[1] * 0.85)    # some particles outside: clamped next step
    elif case == "mouse":
        st.particles.mouse_click_callback(True, (world[0] * 0.3, world[1] * 0.6))
    elif case == "grid_radius":
        st.ctx.call("gpe_grid_set_max_radius", 0.75)                    # cell 1.65 instead of 1.1
    else:
        # add: fmaxf(-0.6, 0.55) = 0.55, cell 1.21; set_particles on the same radii would give -0.6
        st.add_particles(np.array([[world[0] * 0.5, world[1] * 0.5]], np.float32), np.array([0.55], np.float32))
        assert st.grid.max_radius() == np.float32(0.55)
    st.run(DT, 3, resort_every=0, resort_first=False)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "snap.npz")
        st.save(path)
        with np.load(path) as z:
            files = sorted(z.files)
        back = gpe.State.load(path, mode=mode)
    for s in range(10):
        st.update(DT, resort=(s == 4)); back.update(DT, resort=(s == 4))
    for what in (L.POS, L.PREV, L.RADIUS):
        a, b = st.ctx.download(what, np.uint32), back.ctx.download(what, np.uint32)
        assert np.array_equal(a, b), "%s (%s): %d values differ after load" % (case, mode_name, int((a != b).sum()))
    assert back.ctx.world() == st.ctx.world() and back.ctx.gravity() == st.ctx.gravity()
    assert back.ctx.mouse()[0] == st.ctx.mouse()[0] and (back.ctx.mouse() == st.ctx.mouse() or not st.ctx.mouse()[0])
    assert _bits(np.float32(back.grid.cell_size())) == _bits(np.float32(st.grid.cell_size()))
    extra = {"mouse": ["mouse"], "grid_radius": ["grid_max_radius"], "add_rule": ["grid_max_radius"]}.get(case, [])
    assert files == sorted(["format", "gravity", "pos", "prev", "radius", "world"] + extra)
    st.ctx.sync(); back.ctx.sync()
    st.close(); back.close()
