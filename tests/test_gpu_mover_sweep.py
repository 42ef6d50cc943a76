"""GPU (-m gpu): the swept form of the movers' pass (gpe_set_mover_sweep / gpe_get_mover_sweep /
gpe_get_mover_sweep_info; csrc/k_mover_sweep.h, csrc/k_mover_sweep.hip, csrc/gpe_movers.hip).

The rule is a binary32 function: every comparison is bit for bit (uint32 views; a NaN of the model must be a NaN on the
device) against the numpy model (tests/_mover_sweep_model.py: brute force, no grid), and the steps against the CPU oracle
with the model's passes behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red
zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _everything_model as E
from tests import _mover_sweep_model as MS
from tests import _movers_model as M
from tests import _surfaces_model as SM
from tests import _sweep_model as S

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
WORLD = SM.ONE_PASS_WORLD
SWEEP_TAGS = {"grid.msweep_counts", "grid.msweep_carry", "grid.msweep_old"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    """the same bits; where the model has a NaN the device has a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_rows(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _differ(got, want):
    return np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]


def _state(gpe, pos, rad, world=WORLD, mode=None, prev=None, gravity=(0.0, 0.0), flags=0, sweep=True, **kw):
    st = gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=gpe.MODE_NATIVE if mode is None else mode,
                   flags=gpe._lib.FLAG_GUARD_ALLOCS | flags, **kw)
    if sweep:
        st.set_mover_sweep(True)
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


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else None


def _counters(st):
    info = st.mover_sweep_info()
    return st.movers_info()["pushed"], info["swept"], info["stopped"]


def _model_counters(mv):
    return mv.pushed, mv.swept, mv.stopped


# ---- 0. the entry points ---------------------------------------------------------------------------------------------
def test_the_entry_points_exist_the_mode_reads_back_and_refusals_change_nothing(gpe):
    L = gpe._lib
    movers, pos, prev, rad = MS.gate_scene()
    st = _state(gpe, pos, rad, world=MS.SCENE_WORLD, prev=prev, sweep=False)
    assert st.mover_sweep() is False and st.mover_sweep_info() == dict(mode=L.SWEEP_OFF, passes=0, swept=0, stopped=0)
    st.set_mover_sweep(True)                                           # allowed with no movers set
    assert st.mover_sweep() is True and st.mover_sweep_info()["mode"] == L.SWEEP_ON
    assert st.collider_sweep() is False                                # the two modes are independent
    st.update(DT)
    assert st.mover_sweep_info() == dict(mode=L.SWEEP_ON, passes=0, swept=0, stopped=0)   # no movers: no pass
    st.set_movers(np.concatenate([movers, MS.BLADE]))
    st.apply_movers(DT)
    before = (st.mover_sweep_info(), st.movers_info(), st.movers().copy(), st.mover_poses().copy(), st.positions().copy())
    assert before[0]["passes"] == 1 and before[0]["swept"] == len(pos)
    # refusals: a bad mode, a NULL out, a dt that breaks the movers' contract -- nothing moves
    lib, h = L.load(), st.ctx.h
    short = L.GpeSweepInfo(struct_size=C.sizeof(L.GpeSweepInfo) - 8)
    mode = C.c_uint32(7)
    assert lib.gpe_set_mover_sweep(None, L.SWEEP_ON) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_mover_sweep(None, C.byref(mode)) == L.GPE_ERR_INVALID_ARG and mode.value == 7
    assert lib.gpe_get_mover_sweep_info(None, C.byref(short)) == L.GPE_ERR_INVALID_ARG
    for what, call in {"mode 2": lambda: lib.gpe_set_mover_sweep(h, 2),
                       "mode 0xFFFFFFFF": lambda: lib.gpe_set_mover_sweep(h, 0xFFFFFFFF),
                       "get: NULL mode": lambda: lib.gpe_get_mover_sweep(h, None),
                       "info: NULL": lambda: lib.gpe_get_mover_sweep_info(h, None),
                       "info: short struct_size": lambda: lib.gpe_get_mover_sweep_info(h, C.byref(short))}.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
    assert short.mode == 0 and short.swept == 0                        # a refused struct is not written
    for bad in (0.5 / 24.0 * 1.01, float("nan")):                      # |omega dt| > 0.5; not finite
        with pytest.raises(gpe.GpeError) as e:
            st.apply_movers(bad)
        assert e.value.status == L.GPE_ERR_INVALID_ARG
        with pytest.raises(gpe.GpeError):
            st.update(bad)
    after = (st.mover_sweep_info(), st.movers_info(), st.movers(), st.mover_poses(), st.positions())
    assert after[0] == before[0] and after[1] == before[1] and same_rows(after[2], before[2]) and same_rows(after[3], before[3])
    assert same_bits(after[4], before[4]) and st.mover_sweep() is True
    # the next pass is the one a context without the refusals runs
    twin = _state(gpe, pos, rad, world=MS.SCENE_WORLD, prev=prev)
    twin.update(DT)
    twin.set_movers(np.concatenate([movers, MS.BLADE]))
    twin.apply_movers(DT)
    for s in (st, twin):
        s.apply_movers(DT)
    assert same_bits(st.positions(), twin.positions()) and same_rows(st.mover_poses(), twin.mover_poses())
    assert st.mover_sweep_info() == twin.mover_sweep_info()
    st.set_mover_sweep(False)
    assert st.mover_sweep() is False and st.mover_sweep_info() == dict(mode=L.SWEEP_OFF, passes=0, swept=0, stopped=0)
    assert SWEEP_TAGS <= _end(st)
    _end(twin)


def test_a_sharded_context_refuses_the_mode(gpe):
    L = gpe._lib
    pos, rad = S.step_scene()
    st = _state(gpe, pos, rad, world=S.STEP_WORLD, sweep=False)
    st.ctx.call("gpe_use_order_keys", 1)
    with pytest.raises(gpe.GpeError) as e:
        st.set_mover_sweep(True)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED and st.mover_sweep() is False
    assert not SWEEP_TAGS & _end(st)


# ---- 1. the pass alone -----------------------------------------------------------------------------------------------
def _pool_movers(k=65):
    """test_gpu_movers' 40 movers (far, overflowing and outside-the-world ones, a zero-length capsule, stationary ones
    among them), then a thin gate at 15 per step, a thin blade at 0.4 rad per step, a thin LINEAR mover that turns
    around in its second step, and thin pegs on small circles up to k"""
    from tests.test_gpu_movers import _scene_movers
    extra = [M.linear((60, 20), (60, 120), 0.0, v=(900.0, 0.0)),
             M.rotor((140, 140), (175, 140), 0.0, (140, 140), 24.0),
             M.linear((20, 150), (20, 190), 0.0, v=(96.0, 0.0), travel=2.5)]
    rng = np.random.default_rng(5)
    while len(extra) < max(k - 40, 0):
        c = rng.uniform(10, 190, 2)
        extra.append(M.rotor(c + (1.5, 0), c + (1.5, 0), 0.25, c, float(rng.uniform(-24, 24))))
    return np.concatenate([_scene_movers(), M.rows(*extra)])[:k]


def _pool_particles(movers, turns=1):
    """particles around the capsules as the next advance poses them (small velocities, every 23rd prev not finite), then
    resting ones in what the gate and the blade sweep, fast ones all over the world (boxes wider than 16 cells among
    them), and paths that come from outside the grid; shuffled, a swept, a stopped and a plain-touched one first"""
    mv = MS.Movers(movers)
    pos, prev, rad = SM.mover_scene_particles(2200, mv, DT, seed=11)
    rng = np.random.default_rng(12)
    rest = np.concatenate([np.stack([rng.uniform(61.5, 74, 300), rng.uniform(25, 115, 300)], axis=1),
                           np.array([(140 + r * np.cos(t), 140 + r * np.sin(t)) for r, t in
                                     zip(rng.uniform(5, 34, 200), rng.uniform(0.05, 0.38, 200))])]).astype(F32)
    fast = rng.uniform(2, 198, (500, 2)).astype(F32)
    fast_prev = (fast - rng.uniform(-45, 45, (500, 2)).astype(F32)).astype(F32)
    fast_prev[:12] = fast[:12] + np.array([-210.0, 30.0], F32)         # from more than half a cell outside the grid
    pos = np.concatenate([pos, rest, fast])
    prev = np.concatenate([prev, rest, fast_prev])
    rad = np.concatenate([rad, np.full(len(rest) + len(fast), 0.5, F32)])
    mv.set_sweep(True)
    mv.apply_surface(pos, prev, rad, WORLD, DT)
    info = mv.last
    untouched_plain = info["moved"] & ~info["swept"] & ~info["stopped"]
    first = [np.nonzero(info["swept"] & ~info["stopped"])[0][0], np.nonzero(info["stopped"])[0][0], np.nonzero(untouched_plain)[0][0]]
    order = np.random.default_rng(3).permutation(len(rad))
    order = np.concatenate([first, order[~np.isin(order, first)]])
    return pos[order], prev[order], rad[order]


@pytest.fixture(scope="module")
def pool():
    movers = _pool_movers(65)
    assert M.dt_allowed(movers, DT)
    return (movers, SM.scene_surfaces(len(movers), seed=5)) + _pool_particles(movers)


def _one_pass(gpe, movers, surf, pos, prev, rad, mode, turns=2, extra=True):
    n = len(rad)
    st = _state(gpe, pos, rad, prev=prev, mode=_mode(gpe, mode))
    st.set_movers(movers)
    mv = MS.Movers(movers)
    mv.set_sweep(True)
    if surf is not None:
        st.set_surfaces("movers", surf)
        mv.set_surfaces(surf)
    for turn in range(turns):
        w_pos, w_prev, _, _ = mv.apply_surface(pos, prev, rad, WORLD, DT)
        st.apply_movers(DT)
        got, got_prev, got_rad = _arrays(st)
        bad = _differ(got, w_pos)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], prev[bad[:5]], got[bad[:5]], w_pos[bad[:5]], mv.last["who"][bad[:5]])
        bad = _differ(got_prev, w_prev)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], prev[bad[:5]], got_prev[bad[:5]], w_prev[bad[:5]])
        assert np.array_equal(bits(got_rad), bits(rad))
        assert same_rows(st.mover_poses(), mv.poses()), turn
        assert _counters(st) == _model_counters(mv), turn
        assert st.mover_sweep_info()["passes"] == turn + 1 == st.movers_info()["passes"]
        pos, prev = w_pos, w_prev
    if extra:
        # a radius above the grid's bound (|r| = 3 > rb = 0.5) and paths that leave the grid: every mover is walked
        more = np.array([[70.0, 60.0], [150.0, 150.0], [230.0, 150.0], [150.0, 150.0]], F32)
        more_prev = np.array([[70.0, 60.0], [150.0, 149.0], [190.0, 120.0], [150.0, 250.0]], F32)
        more_rad = np.array([-3.0, -3.0, 0.5, 0.5], F32)
        st.add_particles(more, more_rad)
        assert abs(st.particles.get_max_radius()) == 0.5
        st.edit_particles(indices=np.arange(n, n + 4, dtype=U32), previous=more_prev)
        pos, prev, rad = np.concatenate([pos, more]), np.concatenate([prev, more_prev]), np.concatenate([rad, more_rad])
        w_pos, w_prev, _, _ = mv.apply_surface(pos, prev, rad, WORLD, DT)
        st.apply_movers(DT)
        got, got_prev, _ = _arrays(st)
        assert same_bits(got, w_pos) and same_bits(got_prev, w_prev) and _counters(st) == _model_counters(mv)
    tags = _end(st)
    return mv, tags


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("surfaces", [False, True], ids=["plain", "surfaces"])
@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1025])
def test_one_pass_equals_the_model(gpe, pool, n, surfaces, mode):
    """gpe_apply_movers alone with the mode on, 65 movers (two mask words): pos, prev, the poses and the three counters
    as the model, twice (the thin LINEAR mover of travel 2.5 turns around in the second pass), then with particles that walk
    every mover.  The counts cover the pair lanes, the odd tail and a block edge."""
    movers, surf, pos, prev, rad = pool
    mv, tags = _one_pass(gpe, movers, surf if surfaces else None, pos[:n], prev[:n], rad[:n], mode)
    assert SWEEP_TAGS <= tags
    if n >= 511:
        assert mv.swept > 40 and mv.stopped > 5 and mv.pushed > mv.swept
    elif n == 3:
        assert mv.swept >= 1 and mv.stopped >= 1 and mv.pushed >= 3


@pytest.mark.parametrize("k", [1, 64, 65, 1024])
def test_mover_counts_across_the_mask_word_boundary(gpe, pool, k):
    _, _, pos, prev, rad = pool
    movers = _pool_movers(k) if k > 1 else _pool_movers(65)[40:41]     # k = 1: the thin gate alone
    n = 513 if k < 1024 else 257
    mv, _ = _one_pass(gpe, movers, None, pos[:n], prev[:n], rad[:n], "native", turns=1, extra=k <= 65)
    assert mv.pushed > 0


def test_the_grid_strides_a_second_trip(gpe):
    """2048 workgroups x 256 lanes x 2 particles: from 1 048 577 particles on a lane takes a second pair"""
    n = 2048 * 256 * 2 + 3
    movers = M.rows(M.linear((40, 10), (40, 190), 0.0, v=(600.0, 0.0)), M.rotor((140, 100), (180, 100), 0.0, (140, 100), 18.0),
                    M.linear((0, 150), (200, 150), 0.5, v=(0.0, 0.0)))
    rng = np.random.default_rng(9)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    prev = (pos - rng.uniform(-2, 2, (n, 2)).astype(F32)).astype(F32)
    prev[::3] = pos[::3]                                               # resting ones among them
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=prev, mode=gpe.MODE_COMPAT)
    st.set_movers(movers)
    mv = MS.Movers(movers)
    mv.set_sweep(True)
    w_pos, w_prev, _, _ = mv.apply_surface(pos, prev, rad, WORLD, DT)
    st.apply_movers(DT)
    got, got_prev, _ = _arrays(st)
    assert same_bits(got, w_pos) and same_bits(got_prev, w_prev)
    assert _counters(st) == _model_counters(mv)
    for name in ("moved", "swept"):
        assert mv.last[name][:1000000].any() and mv.last[name][-40000:].any(), name
    _end(st)


# ---- 2. the two tunnelling scenes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gate", "blade"])
def test_a_thin_mover_carries_every_particle_in_its_way_on_the_device(gpe, oracle, name):
    """The CPU test's scenes through gpe_step: float64, no tolerance, every particle ends on the leading side of the new
    pose, no nearer than s (1 - 2^-9); the step is the oracle's with the model's pass; the same context with the mode
    off leaves every particle behind."""
    scene, side = (MS.gate_scene, MS.GATE_SIDE) if name == "gate" else (MS.blade_scene, MS.BLADE_SIDE)
    movers, pos, prev, rad = scene()
    cap = MS.first_pose(movers)
    for sweep in (True, False):
        st = _state(gpe, pos, rad, world=MS.SCENE_WORLD, prev=prev, sweep=sweep)
        st.set_movers(movers)
        st.update(MS.SCENE_DT)
        got, got_prev, _ = _arrays(st)
        tw = MS.Twin(oracle, pos, rad, world=MS.SCENE_WORLD, gravity=(0.0, 0.0), prev=prev)
        tw.set_movers(movers)
        tw.set_mover_sweep(sweep)
        tw.step(MS.SCENE_DT)
        w_pos, w_prev, _ = tw.arrays()
        assert same_bits(got, w_pos) and same_bits(got_prev, w_prev)
        behind, close = MS.check_leading(cap, got, side)
        if sweep:
            assert not behind.any() and not close.any(), (np.nonzero(behind | close)[0][:5])
            assert _counters(st) == (len(pos), len(pos), 0)
        else:
            assert behind.all() and st.mover_sweep_info()["passes"] == 0
        tw.close()
        _end(st)


# ---- 3. steps against a twin -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped(oracle):
    return MS.step_reference(oracle, resort_every=16, resort_first=True)


@pytest.fixture(scope="module")
def stepped_surfaces(oracle):
    return MS.step_reference(oracle, surfaces=MS.STEP_MOVER_SURFACES, steps=24)


@pytest.fixture(scope="module")
def stepped_plain(oracle):
    return MS.step_reference(oracle, mover_sweep=False, steps=16)


def _step_state(gpe, mode=None, flags=0, sweep=True, surfaces=None, **kw):
    pos, rad = S.step_scene()
    st = _state(gpe, pos, rad, world=S.STEP_WORLD, mode=mode, gravity=S.STEP_GRAVITY, flags=flags, sweep=sweep, **kw)
    st.set_colliders(S.step_colliders())
    st.set_movers(MS.step_movers())
    st.set_fields(S.STEP_FIELDS)
    if surfaces is not None:
        st.set_surfaces("movers", surfaces)
    st.set_collider_sweep(True)
    return st


def _kick(gpe, st, s, every=4):
    if s % every == 0:
        st.kick_circle(S.STEP_KICK_DISC[:2], S.STEP_KICK_DISC[2], gpe._lib.VEL_SET, S.step_kick(s), count=False)


def _module_step(st, dt, resort):
    """what gpe_step does, by the per-module calls and the apply hooks in the documented order"""
    if resort:
        st.particles.sort_by_cell_id()
    st.grid.update()
    st.collision_system.solve_collisions()
    st.particles.update_positions(dt)
    st.apply_bonds()
    st.apply_bodies()
    st.apply_movers(dt)
    st.apply_colliders()
    st.apply_fields(dt)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_steps_runs_and_module_calls_equal_the_oracle_plus_the_model(gpe, stepped, mode):
    """48 steps of the sparse box with a thin piston (it turns around every 12 steps) and a thin blade, a kick every
    fourth step, both sweeps on, the re-sorts of gpe_run(resort_every = 16): by gpe_step, by gpe_run in runs of four and
    by the per-module calls with gpe_apply_movers -- all three the oracle's step with the model's passes behind it."""
    frames, counts = stepped
    m = _mode(gpe, mode)
    runner, stepper, modular = (_step_state(gpe, mode=m) for _ in range(3))
    for s in range(0, MS.STEP_STEPS, 4):
        due = s % 16 == 0
        for st in (runner, stepper, modular):
            _kick(gpe, st, s)
        runner.run(DT, 4, resort_every=0, resort_first=due)
        for k in range(4):
            stepper.update(DT, resort=due and k == 0)
            _module_step(modular, DT, due and k == 0)
            for st in (stepper, modular):
                pos, prev, _ = _arrays(st)
                assert same_bits(pos, frames[s + k][0]) and same_bits(prev, frames[s + k][1]), s + k
            assert same_rows(stepper.mover_poses(), frames[s + k][2]), s + k
        pos, prev, _ = _arrays(runner)
        assert same_bits(pos, frames[s + 3][0]) and same_bits(prev, frames[s + 3][1]), s
    for st in (runner, stepper, modular):
        assert _counters(st) == (counts["pushed"], counts["swept"], counts["stopped"])
        assert st.mover_sweep_info()["passes"] == MS.STEP_STEPS == counts["passes"]
        assert st.colliders_info()["pushed"] == counts["colliders"]
        _end(st)
    assert counts["swept"] > 50 and -1.0 in [float(f[2]["q1"][0]) for f in frames]


def test_steps_with_surfaces_on_the_movers(gpe, stepped_surfaces):
    frames, counts = stepped_surfaces
    st = _step_state(gpe, surfaces=MS.STEP_MOVER_SURFACES)
    for s in range(len(frames)):
        _kick(gpe, st, s)
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    assert _counters(st) == (counts["pushed"], counts["swept"], counts["stopped"]) and counts["swept"] > 20
    _end(st)


# ---- 4. off is today -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_off_is_the_plain_pass(gpe, stepped_plain, mode):
    """A context switched on and off again, and one that never called the entry point, step as the twin with the plain
    pass: positions, prev, poses, pushed and listed identical; the swept form's pass counter stays 0."""
    frames, counts = stepped_plain
    m = _mode(gpe, mode)
    never = _step_state(gpe, mode=m, sweep=False)
    toggled = _step_state(gpe, mode=m, sweep=True)
    toggled.set_mover_sweep(False)
    for s in range(len(frames)):
        for st in (never, toggled):
            _kick(gpe, st, s)
            st.update(DT)
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
            assert same_rows(st.mover_poses(), frames[s][2]), s
        assert never.movers_info() == toggled.movers_info(), s         # pushed and listed among them
    for st in (never, toggled):
        assert st.mover_sweep_info() == dict(mode=0, passes=0, swept=0, stopped=0)
        assert st.movers_info()["pushed"] == counts["pushed"] and st.movers_info()["passes"] == len(frames)
    assert not SWEEP_TAGS & _end(never)                                # never allocated
    _end(toggled)


# ---- 5. the mode survives everything ---------------------------------------------------------------------------------
def test_the_mode_survives_everything(gpe, oracle):
    """the context follows a twin through new mover sets (also the empty one), surfaces, restored poses, set_particles,
    add, remove, edit, a re-sort, growth and gpe_set_world: the mode stays on, its counters go on, every step is the
    twin's"""
    from tests._oracle_model import VEL_SET, circle_mask
    world = (100.0, 100.0)
    rng = np.random.default_rng(12)
    n = 999
    pos = rng.uniform(23, 77, (n, 2)).astype(F32)
    rad = np.full(n, 0.25, F32)
    st = _state(gpe, pos, rad, world=world, gravity=(0.0, 60.0))
    tw = MS.Twin(oracle, pos, rad, world=world, gravity=(0.0, 60.0))
    tw.set_mover_sweep(True)
    for h in (st, tw):
        h.set_colliders(S.step_colliders())
        h.set_movers(MS.step_movers())
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
        assert st.mover_sweep() is True, what
        assert _counters(st) == _model_counters(tw.m), what
        assert st.mover_sweep_info()["passes"] == tw.m.sweep_passes, what

    steps("start")
    pos2 = rng.uniform(23, 77, (n - 200, 2)).astype(F32)
    f = C.POINTER(C.c_float)
    st.ctx.call("gpe_set_particles", pos2.ctypes.data_as(f), pos2.ctypes.data_as(f), rad[:n - 200].ctypes.data_as(f), n - 200)
    tw.set_particles(pos2, pos2, rad[:n - 200])
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
    passes = st.mover_sweep_info()["passes"]
    assert passes == turn[0] and st.mover_sweep_info()["swept"] > 0
    for h in (st, tw):                                                 # a new set: the mode and its counters stay
        h.set_movers(MS.step_movers()[::-1].copy())
    assert st.mover_sweep() is True and st.mover_sweep_info()["passes"] == passes and st.movers_info()["passes"] == 0
    steps("new movers")
    for h in (st, tw):
        h.set_surfaces("movers", MS.STEP_MOVER_SURFACES)
    steps("new surfaces")
    poses = st.mover_poses()
    st.set_mover_poses(poses); tw.m.set_poses(poses)
    steps("restored poses")
    st.set_movers(np.zeros(0, M.MOVER_DTYPE))                          # no movers: still on, and on for the next set
    assert st.mover_sweep() is True and not any(t.startswith("grid.mover_") for t, _, _, state in st.ctx.guard_registry()
                                                if state == "live")
    st.update(DT)
    assert st.mover_sweep_info()["passes"] == turn[0]
    tw.close()
    assert SWEEP_TAGS <= _end(st)


def test_save_and_load_keep_the_mode(gpe, tmp_path):
    L = gpe._lib
    st = _step_state(gpe)
    _kick(gpe, st, 0)
    st.run(DT, 6, resort_every=0, resort_first=False)
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["mover_sweep"].tolist() == [1] and d["collider_sweep"].tolist() == [1]
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.mover_sweep() is True and back.collider_sweep() is True
    for h in (st, back):
        _kick(gpe, h, 4)
        h.run(DT, 6, resort_every=0, resort_first=False)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), _arrays(back)))
    assert same_rows(st.mover_poses(), back.mover_poses()) and back.mover_sweep_info()["passes"] == 6
    assert back.mover_sweep_info()["swept"] > 0
    _end(back)
    st.set_mover_sweep(False)
    st.save(path)
    with np.load(path) as d:
        assert "mover_sweep" not in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.mover_sweep() is False and back.collider_sweep() is True
    _end(back)
    _end(st)


@pytest.mark.parametrize("way", ["particles", "ctx_call"])
def test_save_keeps_a_mode_set_below_the_state(gpe, tmp_path, way):
    """save() asks the context for the mode: one switched on through ParticleSystem.set_mover_sweep or through ctx.call,
    not through State, is written and loaded, and the saved and the loaded state step the same bits"""
    L = gpe._lib
    st = _step_state(gpe, sweep=False)
    if way == "particles":
        st.particles.set_mover_sweep(True)
    else:
        st.ctx.call("gpe_set_mover_sweep", L.SWEEP_ON)
    assert st.mover_sweep() is True
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert "mover_sweep" in d.files and d["mover_sweep"].tolist() == [1]
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.mover_sweep() is True
    for h in (st, back):
        _kick(gpe, h, 0)
        h.run(DT, 6, resort_every=0, resort_first=False)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), _arrays(back)))
    assert same_rows(st.mover_poses(), back.mover_poses())
    assert st.mover_sweep_info() == back.mover_sweep_info() and back.mover_sweep_info()["passes"] == 6
    assert back.mover_sweep_info()["swept"] > 0
    _end(back)
    # the converse: on through State, off through ctx.call -- no key, and the loaded state is off
    st.set_mover_sweep(True)
    st.ctx.call("gpe_set_mover_sweep", L.SWEEP_OFF)
    assert st.mover_sweep() is False
    st.save(path)
    with np.load(path) as d:
        assert "mover_sweep" not in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.mover_sweep() is False and back.collider_sweep() is True
    _end(back)
    _end(st)


# ---- 6. composition with every other pass ----------------------------------------------------------------------------
def test_every_pass_armed_with_both_sweeps_equals_the_composed_twin(gpe, oracle):
    """bonds -> bodies -> movers (swept) -> static colliders (swept) -> fields -> observers, 16 steps of the everything
    scene (tests/_everything_model.py arms the movers' sweep itself) bit for bit; the tracer and monitor frames show the
    swept positions"""
    sc = E.scene()
    tw = E.twin(oracle, sc=sc)
    st = gpe.State(sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev, mode=gpe.MODE_NATIVE,
                   flags=gpe._lib.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    E.arm(st, sc)
    assert tw.fully_armed() and tw.m.sweep and st.collider_sweep() and st.mover_sweep()
    steps = 16
    watch = np.arange(0, E.N, 97, dtype=U32)
    st.tracers_begin(watch, every=1, frames=steps)
    st.monitor_begin(every=1, frames=steps)
    want = []
    for s in range(steps):
        tw.step(E.DT)
        st.update(E.DT)
        f = E.frame(tw)
        want.append(f)
        assert same_bits(st.positions(), f.pos) and same_bits(st.previous_positions(), f.prev), s
        assert same_rows(st.mover_poses(), f.mover_poses), s
    assert st.mover_sweep_info() == tw.mover_sweep_info() and st.mover_sweep_info()["passes"] == steps
    assert E.state_counters(st) == tw.counters()
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == steps and recorded == steps
    for s in range(steps):                                             # (no re-sort: uid = storage index)
        assert same_bits(tr.pos[s], want[s].pos[watch]), s
        assert rec["max_x"][s] == want[s].pos[:, 0].max() and rec["min_y"][s] == want[s].pos[:, 1].min(), s
    st.tracers_end(); st.monitor_end()
    tw.close()
    _end(st)


# ---- 7. guarded allocations ------------------------------------------------------------------------------------------
def test_the_carry_records_the_old_capsules_and_the_counters_keep_their_red_zones(gpe, pool):
    """GPE_MOVERS_MAX movers with surfaces under GPE_FLAG_GUARD_ALLOCS: the build writes the last row of the carry
    records and of the old capsules, the pass both counter words; no red zone is damaged, and the three buffers outlive
    the set"""
    _, _, pos, prev, rad = pool
    movers = _pool_movers(1024)
    n = 129
    st = _state(gpe, pos[:n], rad[:n], prev=prev[:n])
    st.set_movers(movers)
    st.set_surfaces("movers", SM.scene_surfaces(len(movers), seed=5))
    for _ in range(3):
        st.apply_movers(DT)
    st.update(DT)
    live = {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}
    assert SWEEP_TAGS <= live and st.mover_sweep_info()["passes"] == 4
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    st.set_movers(np.zeros(0, M.MOVER_DTYPE))
    live = {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}
    assert SWEEP_TAGS <= live and not any(t.startswith("grid.mover_") for t in live)
    _end(st)
