"""GPU (-m gpu): the swept form of the static colliders' pass (gpe_set_collider_sweep / gpe_get_collider_sweep /
gpe_get_sweep_info; csrc/k_sweep.h, csrc/k_sweep.hip, csrc/gpe_sweep.hip).

The rule is a binary32 function: every comparison is bit for bit (uint32 views; a NaN of the model must be a NaN on the
device) against the numpy model (tests/_sweep_model.py: brute force, no grid), and the steps against the CPU oracle with
the model's passes behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red
zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _surfaces_model as SM
from tests import _sweep_model as S

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = S.STEP_DT


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    """the same bits; where the model has a NaN the device has a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _differ(got, want):
    return np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]


def _state(gpe, pos, rad, world=S.BOX_WORLD, mode=None, prev=None, gravity=(0.0, 0.0), flags=0, sweep=True, **kw):
    st = gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=gpe.MODE_NATIVE if mode is None else mode,
                   flags=gpe._lib.FLAG_GUARD_ALLOCS | flags, **kw)
    if sweep:
        st.set_collider_sweep(True)
    return st


def _end(st):
    """every context ends here: no red zone of a live or a released buffer is damaged"""
    zones = st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0, zones
    tags = {t for t, _, _, _ in st.ctx.guard_registry()}
    st.close()
    return tags


def _arrays(st):
    return st.positions(), st.previous_positions(), st.radii()


def _set(st, pos, prev, rad):
    f = C.POINTER(C.c_float)
    pos, prev, rad = (np.ascontiguousarray(a, F32) for a in (pos, prev, rad))
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), prev.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else None


def _counters(st):
    info = st.sweep_info()
    return st.colliders_info()["pushed"], info["swept"], info["stopped"]


# ---- 0. the entry points ---------------------------------------------------------------------------------------------
def test_the_entry_points_exist_and_the_mode_reads_back(gpe):
    L = gpe._lib
    pos, rad = CM.floor_scene(100)
    st = _state(gpe, pos, rad, world=CM.FLOOR_WORLD, sweep=False)
    assert st.collider_sweep() is False
    assert st.sweep_info() == dict(mode=L.SWEEP_OFF, passes=0, swept=0, stopped=0)
    st.set_collider_sweep(True)                                        # allowed with no colliders set
    assert st.collider_sweep() is True and st.sweep_info()["mode"] == L.SWEEP_ON
    st.update(DT)
    assert st.sweep_info() == dict(mode=L.SWEEP_ON, passes=0, swept=0, stopped=0)   # no colliders: no pass
    st.set_collider_sweep(False)
    assert st.collider_sweep() is False
    tags = _end(st)
    assert "grid.sweep_counts" in tags


# ---- 1. the pass alone -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """-> (colliders, surfaces, pos, prev, rad): test_gpu_colliders' set (the far, overflowing and outside-the-world
    capsules among them) plus the box scene's; the box scene's paths and the colliders' one-pass scene with small
    velocities, shuffled, a swept, a stopped and a resting touched particle first"""
    from tests.test_gpu_colliders import _scene_colliders
    box, start, end, rad_b = S.box_scene(0.05)
    cs = np.concatenate([_scene_colliders(), box]).astype(F32)
    _, _, pos_c, prev_c, rad_c = SM.collider_scene(2000)
    pos = np.concatenate([end, pos_c])
    prev = np.concatenate([S.box_prev(start), prev_c])
    prev[4000:4300] = pos[4000:4300]                                   # resting: the plain rule
    rad = np.concatenate([rad_b, rad_c])
    surf = SM.scene_surfaces(len(cs), seed=41)
    assert (surf["flags"] == SM.PLAIN).any() and (surf["restitution"] == 1).any() and (surf["friction"] == 0).any()
    _, _, info = S.apply(pos, prev, rad, cs, S.BOX_WORLD)
    order = np.random.default_rng(3).permutation(len(rad))
    first = [np.nonzero(info["swept"] & ~info["stopped"])[0][0], np.nonzero(info["stopped"])[0][0],
             np.nonzero(info["plain"] & info["moved"])[0][0]]
    order = np.concatenate([first, order[~np.isin(order, first)]])
    return cs, surf, pos[order], prev[order], rad[order]


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("surfaces", [False, True], ids=["plain", "surfaces"])
@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1025])
def test_one_pass_equals_the_model(gpe, pool, n, surfaces, mode):
    """gpe_apply_colliders alone with the sweep on: pos, prev and the three counters as the model, twice (the second
    pass starts from the first one's result).  The counts cover the pair lanes, the odd tail and a block edge."""
    cs, surf, pos, prev, rad = pool
    pos, prev, rad = pos[:n], prev[:n], rad[:n]
    surf = surf if surfaces else None
    st = _state(gpe, pos, rad, prev=prev, mode=_mode(gpe, mode))
    st.set_colliders(cs)
    if surfaces:
        st.set_surfaces("colliders", surf)
    want = [0, 0, 0]
    for turn in range(2):
        w_pos, w_prev, info = S.apply(pos, prev, rad, cs, S.BOX_WORLD, surfaces=surf)
        st.apply_colliders()
        got, got_prev, got_rad = _arrays(st)
        bad = _differ(got, w_pos)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], prev[bad[:5]], got[bad[:5]], w_pos[bad[:5]])
        bad = _differ(got_prev, w_prev)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], prev[bad[:5]], got_prev[bad[:5]], w_prev[bad[:5]])
        assert np.array_equal(bits(got_rad), bits(rad))
        for k, name in enumerate(("moved", "swept", "stopped")):
            want[k] += int(info[name].sum())
        assert list(_counters(st)) == want, turn
        assert st.sweep_info()["passes"] == turn + 1 and st.colliders_info()["passes"] == turn + 1
        pos, prev = w_pos, w_prev
    if n >= 511:
        assert want[1] > 50 and want[2] > 20 and want[0] > want[1]
    elif n == 3:
        assert want[1] >= 2 and want[2] >= 1 and want[0] >= 3
    # a radius above the grid's bound (|r| = 3 > rb = 0.5) and paths that leave the grid: every collider is walked
    extra = np.array([[100.0, 130.0], [45.0, 100.0], [230.0, 150.0], [150.0, 150.0]], F32)
    extra_prev = np.array([[100.0, 90.0], [30.0, 100.0], [190.0, 120.0], [150.0, 250.0]], F32)
    extra_rad = np.array([-3.0, -3.0, 0.5, 0.5], F32)
    st.add_particles(extra, extra_rad)
    assert abs(st.particles.get_max_radius()) == 0.5
    st.edit_particles(indices=np.arange(n, n + 4, dtype=U32), previous=extra_prev)
    all_pos, all_prev, all_rad = np.concatenate([pos, extra]), np.concatenate([prev, extra_prev]), np.concatenate([rad, extra_rad])
    w_pos, w_prev, info = S.apply(all_pos, all_prev, all_rad, cs, S.BOX_WORLD, surfaces=surf)
    assert info["swept"][n:].all()
    st.apply_colliders()
    got, got_prev, _ = _arrays(st)
    assert same_bits(got, w_pos) and same_bits(got_prev, w_prev)
    _end(st)


def test_the_grid_strides_a_second_trip(gpe):
    """2048 workgroups x 256 lanes x 2 particles: from 1 048 577 particles on a lane takes a second pair"""
    n = 2048 * 256 * 2 + 3
    cs = np.array([[0, 100, 200, 100, 0], [100, 0, 100, 200, 0.5], [50, 50, 50, 50, 10]], F32)
    rng = np.random.default_rng(9)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    prev = (pos - rng.uniform(-4, 4, (n, 2)).astype(F32)).astype(F32)
    prev[::5] = pos[::5]                                               # resting ones among them
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=prev, mode=gpe.MODE_COMPAT)
    st.set_colliders(cs)
    w_pos, w_prev, info = S.apply(pos, prev, rad, cs, S.BOX_WORLD)
    st.apply_colliders()
    got, got_prev, _ = _arrays(st)
    assert same_bits(got, w_pos) and same_bits(got_prev, w_prev)
    assert list(_counters(st)) == [int(info[k].sum()) for k in ("moved", "swept", "stopped")]
    for k in ("moved", "swept", "stopped"):
        assert info[k][:1000000].any() and info[k][-40000:].any(), k
    _end(st)


# ---- 2. the box ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0.0, 0.05])
def test_nothing_leaves_the_box_on_the_device(gpe, R):
    """The CPU test's box in one pass on the device: float64, no tolerance, nothing leaves and no arm of the V is
    crossed; the counters are the model's; the same context with the sweep off loses particles."""
    cs, start, end, rad = S.box_scene(R)
    prev = S.box_prev(start)
    finite = np.isfinite(prev).all(axis=1)
    st = _state(gpe, end, rad, prev=prev)
    st.set_colliders(cs)
    st.apply_colliders()
    got, got_prev, _ = _arrays(st)
    outside, crossed = S.check_box(start, got, finite)
    assert not outside.any() and not crossed.any(), (np.nonzero(outside | crossed)[0][:5])
    w_pos, w_prev, info = S.apply(end, prev, rad, cs, S.BOX_WORLD)
    assert same_bits(got, w_pos) and same_bits(got_prev, w_prev)
    pushed, swept, stopped = _counters(st)
    assert (pushed, swept, stopped) == tuple(int(info[k].sum()) for k in ("moved", "swept", "stopped"))
    assert swept > 1000 and stopped > 100
    st.set_collider_sweep(False)
    _set(st, end, prev, rad)
    st.apply_colliders()
    lost, through = S.check_box(start, st.positions(), finite)
    assert lost.sum() > 500 and through.sum() > 50
    assert same_bits(st.positions(), CM.apply(end, rad, cs, S.BOX_WORLD)[0])
    _end(st)


# ---- 3. steps against a twin -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped(oracle):
    """oracle step + the model's passes (a piston, the swept box, a wind), a kick before every step, no re-sort"""
    return S.step_reference(oracle)


@pytest.fixture(scope="module")
def stepped_resorted(oracle):
    """the same with a kick before every fourth step and the re-sorts of gpe_run(resort_every = 16)"""
    return S.step_reference(oracle, resort_every=16, resort_first=True, kick_every=4)


@pytest.fixture(scope="module")
def stepped_plain(oracle):
    return S.step_reference(oracle, sweep=False, steps=20, apply_first=True)


def _step_state(gpe, mode=None, flags=0, sweep=True, **kw):
    pos, rad = S.step_scene()
    st = _state(gpe, pos, rad, world=S.STEP_WORLD, mode=mode, gravity=S.STEP_GRAVITY, flags=flags, sweep=sweep, **kw)
    st.set_colliders(S.step_colliders())
    st.set_movers(S.step_movers())
    st.set_fields(S.STEP_FIELDS)
    return st


def _kick(gpe, st, s):
    return st.kick_circle(S.STEP_KICK_DISC[:2], S.STEP_KICK_DISC[2], gpe._lib.VEL_SET, S.step_kick(s), count=False)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_oracle_plus_the_model(gpe, stepped, mode):
    """60 steps of the sparse box of R = 0.25 with gravity, kicks of 5 to 20 per step, a piston and a field, under
    GPE_FLAG_SORT_EVERY_STEP: pos and prev as the twin after every step, every particle inside all the way."""
    frames, counts = stepped
    st = _step_state(gpe, mode=_mode(gpe, mode), flags=gpe._lib.FLAG_SORT_EVERY_STEP)
    for s in range(S.STEP_STEPS):
        _kick(gpe, st, s)
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
        assert S.inside_step_box(pos).all(), s
    assert _counters(st) == (counts["pushed"], counts["swept"], counts["stopped"])
    assert st.sweep_info()["passes"] == S.STEP_STEPS and st.movers_info()["pushed"] == counts["movers"] > 0
    assert counts["swept"] > 100 and counts["stopped"] > 0
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_runs_equal_steps_and_the_twin(gpe, stepped_resorted, mode):
    """gpe_run(resort_every = 16) in runs of four steps, a kick before each, against gpe_step and the twin"""
    frames, counts = stepped_resorted
    m = _mode(gpe, mode)
    runner, stepper = _step_state(gpe, mode=m), _step_state(gpe, mode=m)
    for s in range(0, S.STEP_STEPS, 4):
        due = s % 16 == 0
        for st in (runner, stepper):
            _kick(gpe, st, s)
        runner.run(DT, 4, resort_every=0, resort_first=due)
        for k in range(4):
            stepper.update(DT, resort=due and k == 0)
            pos, prev, _ = _arrays(stepper)
            assert same_bits(pos, frames[s + k][0]) and same_bits(prev, frames[s + k][1]), s + k
        pos, prev, _ = _arrays(runner)
        assert same_bits(pos, frames[s + 3][0]) and same_bits(prev, frames[s + 3][1]), s
        assert S.inside_step_box(pos).all(), s
    for st in (runner, stepper):
        assert _counters(st) == (counts["pushed"], counts["swept"], counts["stopped"])
        _end(st)
    # one gpe_run over sixteen steps with its own re-sorts equals sixteen gpe_step
    runner, stepper = _step_state(gpe, mode=m), _step_state(gpe, mode=m)
    for st in (runner, stepper):
        _kick(gpe, st, 3)
    runner.run(DT, 24, resort_every=16, resort_first=True)
    for k in range(24):
        stepper.update(DT, resort=k % 16 == 0)
    assert all(same_bits(a, b) for a, b in zip(_arrays(runner), _arrays(stepper)))
    assert _counters(runner) == _counters(stepper) and _counters(runner)[1] > 0
    _end(runner)
    _end(stepper)


# ---- 4. off is today -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_off_is_the_plain_pass(gpe, stepped_plain, mode):
    """A context switched on and off again, and one never switched, step as the twin with the plain pass; with the sweep
    on and every particle at rest one pass gives the plain pass's bits."""
    frames, counts = stepped_plain
    m = _mode(gpe, mode)
    never = _step_state(gpe, mode=m, sweep=False)
    toggled = _step_state(gpe, mode=m, sweep=True)
    for st in (never, toggled):                                        # every particle rests: the swept pass is the plain one
        st.apply_colliders()
        assert st.colliders_info()["pushed"] == 2                      # (two start touching the shelf)
    assert toggled.sweep_info()["passes"] == 1 and never.sweep_info()["passes"] == 0
    toggled.set_collider_sweep(False)
    assert toggled.sweep_info() == dict(mode=0, passes=0, swept=0, stopped=0)
    for s in range(len(frames)):
        for st in (never, toggled):
            _kick(gpe, st, s)
            st.update(DT)
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    for st in (never, toggled):
        assert st.sweep_info() == dict(mode=0, passes=0, swept=0, stopped=0)
        assert st.colliders_info()["pushed"] == counts["pushed"] and st.colliders_info()["passes"] == len(frames) + 1
    assert "grid.sweep_counts" not in _end(never)                      # never allocated
    _end(toggled)
    for surfaces in (False, True):
        cs, surf, pos, _, rad = SM.collider_scene(3999)
        st = _state(gpe, pos, rad, prev=pos, mode=m)
        st.set_colliders(cs)
        if surfaces:
            st.set_surfaces("colliders", surf)
            want, want_prev, moved, _ = SM.apply(pos, pos, rad, cs, surf, SM.ONE_PASS_WORLD)
        else:
            (want, moved), want_prev = CM.apply(pos, rad, cs, SM.ONE_PASS_WORLD), pos
        st.apply_colliders()
        got, got_prev, _ = _arrays(st)
        assert same_bits(got, want) and same_bits(got_prev, want_prev)
        assert _counters(st) == (int(moved.sum()), 0, 0) and moved.sum() > 1000 and st.sweep_info()["passes"] == 1
        _end(st)


# ---- 5. the observers ------------------------------------------------------------------------------------------------
def test_tracer_and_monitor_frames_show_the_swept_positions(gpe, stepped_resorted):
    frames = stepped_resorted[0]
    st = _step_state(gpe)
    st.enable_uids()
    uids = np.arange(0, 240, 7, dtype=U32)
    st.tracers_begin(uids, every=1, frames=8, prev=True)
    st.monitor_begin(every=1, frames=8)
    _kick(gpe, st, 0)
    st.run(DT, 4, resort_every=0, resort_first=True)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 4 and recorded == 4
    order = np.argsort(st.uids())                                      # the re-sort moved the particles: rows by uid
    for s in range(4):
        pos, prev = frames[s]
        assert rec["max_x"][s] == pos[:, 0].max() and rec["min_y"][s] == pos[:, 1].min() and rec["n"][s] == len(pos), s
        assert same_bits(tr.pos[s], pos[order][uids]) and same_bits(tr.prev[s], prev[order][uids]), s
    assert same_bits(st.positions(), frames[3][0])
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 6. step state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_mode_survives_everything(gpe, oracle, mode):
    world = (100.0, 100.0)
    cs = S.step_colliders()
    csurf = SM.rows((0.5, 0.3), (1.0, 0.0), (0.0, 0.8), (0.9, 0.1, SM.PLAIN), (0.7, 0.2))
    rng = np.random.default_rng(12)
    n = 999
    pos = rng.uniform(23, 77, (n, 2)).astype(F32)
    rad = np.full(n, 0.25, F32)
    m = _mode(gpe, mode)
    st = _state(gpe, pos, rad, world=world, gravity=(0.0, 60.0), mode=m)
    tw = S.Twin(oracle, pos, rad, world=world, gravity=(0.0, 60.0))
    tw.set_collider_sweep(True)
    for h in (st, tw):
        h.set_colliders(cs)
        h.set_surfaces("colliders", csurf)
    from tests._oracle_model import VEL_SET, circle_mask
    turn = [0]

    def steps(what, k=2):
        for _ in range(k):
            a = S.step_kick(turn[0])
            turn[0] += 1
            p, _, _ = tw.arrays()
            tw.kick(circle_mask(p, 50.0, 50.0, 20.0), VEL_SET, *a)
            st.kick_circle((50.0, 50.0), 20.0, gpe._lib.VEL_SET, a, count=False)
            st.update(DT); tw.step(DT)
        got, want = _arrays(st), tw.arrays()
        assert all(same_bits(a, b) for a, b in zip(got, want)), what
        assert st.collider_sweep() is True, what
        assert _counters(st) == (tw.pushed, tw.swept, tw.stopped), what
        assert st.sweep_info()["passes"] == tw.sweep_passes, what

    steps("start")
    pos2 = rng.uniform(23, 77, (n - 200, 2)).astype(F32)
    _set(st, pos2, pos2, rad[:n - 200]); tw.set_particles(pos2, pos2, rad[:n - 200])
    steps("set_particles")
    add = rng.uniform(25, 75, (100, 2)).astype(F32)
    st.add_particles(add, np.full(100, 0.25, F32)); tw.add(add, np.full(100, 0.25, F32))
    steps("add")
    assert st.remove_particles_in_circle((50, 40), 8.0) == tw.remove_circle(50, 40, 8.0) > 0
    steps("remove")
    who = np.arange(0, 200, 2, dtype=U32)
    where = (rng.uniform(-4, 4, (100, 2)) + (50.0, 55.0)).astype(F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    grow = rng.uniform(25, 75, (3000, 2)).astype(F32)                  # past the capacity
    st.add_particles(grow, np.full(3000, 0.25, F32)); tw.add(grow, np.full(3000, 0.25, F32))
    steps("growth")
    st.ctx.call("gpe_set_world", 120.0, 100.0); tw.set_world(120.0, 100.0)
    steps("set_world")
    passes = st.sweep_info()["passes"]
    st.set_colliders(cs[:4]); tw.set_colliders(cs[:4])                 # a new set: the mode and its counters stay
    assert st.collider_sweep() is True and st.sweep_info()["passes"] == passes
    steps("new colliders")
    st.set_surfaces("colliders", csurf[:4]); tw.set_surfaces("colliders", csurf[:4])
    steps("new surfaces")
    # a fresh context built from the same arrays with the mode on steps to the same bits
    got = _arrays(st)
    fresh = _state(gpe, got[0], got[2], prev=got[1], world=(120.0, 100.0), gravity=(0.0, 60.0), mode=m)
    fresh.set_colliders(cs[:4])
    fresh.set_surfaces("colliders", csurf[:4])
    for h in (st, fresh):
        h.kick_circle((50.0, 50.0), 20.0, gpe._lib.VEL_SET, (9.0, -7.0), count=False)
        h.update(DT)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), _arrays(fresh)))
    st.clear_colliders()                                               # no colliders: still on
    assert st.collider_sweep() is True
    tw.close()
    _end(fresh)
    _end(st)


def test_save_and_load_keep_the_mode(gpe, tmp_path):
    L = gpe._lib
    st = _step_state(gpe)
    _kick(gpe, st, 1)
    st.run(DT, 6, resort_every=0, resort_first=False)
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["collider_sweep"].tolist() == [1]
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.collider_sweep() is True
    for h in (st, back):
        _kick(gpe, h, 2)
        h.run(DT, 6, resort_every=0, resort_first=False)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), _arrays(back)))
    assert back.sweep_info()["swept"] > 0
    _end(back)
    st.set_collider_sweep(False)
    st.save(path)
    with np.load(path) as d:
        assert "collider_sweep" not in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.collider_sweep() is False
    _end(back)
    _end(st)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_mode_the_counters_the_set_and_the_next_step_untouched(gpe, stepped):
    L = gpe._lib
    lib = L.load()
    frames = stepped[0]
    st = _step_state(gpe)
    for s in range(5):
        _kick(gpe, st, s)
        st.update(DT)
    before = _arrays(st)
    state = st.sweep_info(), st.colliders_info(), st.colliders()
    assert state[0]["swept"] > 0

    def untouched(what):
        assert st.collider_sweep() is True, what
        assert (st.sweep_info(), st.colliders_info()) == state[:2] and same_bits(st.colliders(), state[2]), what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    h = st.ctx.h
    mode = C.c_uint32(7)
    short = L.GpeSweepInfo(struct_size=C.sizeof(L.GpeSweepInfo) - 8)
    assert lib.gpe_set_collider_sweep(None, L.SWEEP_ON) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_collider_sweep(None, C.byref(mode)) == L.GPE_ERR_INVALID_ARG and mode.value == 7
    assert lib.gpe_get_sweep_info(None, C.byref(short)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    bad = {
        "mode 2": lambda: lib.gpe_set_collider_sweep(h, 2),
        "mode 0xFFFFFFFF": lambda: lib.gpe_set_collider_sweep(h, 0xFFFFFFFF),
        "get: NULL mode": lambda: lib.gpe_get_collider_sweep(h, None),
        "info: NULL": lambda: lib.gpe_get_sweep_info(h, None),
        "info: short struct_size": lambda: lib.gpe_get_sweep_info(h, C.byref(short)),
        "info: struct_size 0": lambda: lib.gpe_get_sweep_info(h, C.byref(L.GpeSweepInfo())),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        untouched(what)
    assert short.mode == 0 and short.swept == 0                        # a refused struct is not written
    for s in range(5, 8):                                              # the context goes on as the twin does
        _kick(gpe, st, s)
        st.update(DT)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[7][0]) and same_bits(prev, frames[7][1])
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_sweep(gpe, how):
    L = gpe._lib
    pos, rad = CM.floor_scene(600)
    st = _state(gpe, pos, rad, world=CM.FLOOR_WORLD, sweep=False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    for on in (True, False):
        with pytest.raises(gpe.GpeError) as e:
            st.set_collider_sweep(on)
        assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert st.collider_sweep() is False and st.sweep_info() == dict(mode=0, passes=0, swept=0, stopped=0)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    assert "grid.sweep_counts" not in _end(st)
