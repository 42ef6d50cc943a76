"""GPU (-m gpu): moving colliders (gpe_set_movers / _get_movers / _get_mover_poses / _set_mover_poses / _apply_movers /
_get_movers_info, csrc/k_movers.hip, csrc/gpe_movers.hip).

The motion and the pass are binary32 functions: every comparison is bit for bit against the numpy model
(tests/_movers_model.py: the motion in numpy float32, the push tests/_colliders_model.apply on the posed capsules, brute
force, no grid), and the steps against the CPU oracle with the model's passes behind every step (movers, then static
colliders).  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _movers_model as M
from tests.test_gpu_colliders import _scene_colliders, _scene_particles

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = M.RUN_DT
NAN, INF = float("nan"), float("inf")
WORLD = (200.0, 200.0)
RUN_STEPS = 60
MOVER_TAGS = {"grid.mover_def", "grid.mover_pose", "grid.mover_rec", "grid.mover_pushed", "grid.mover_masks"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_rows(a, b):
    """two structured arrays (movers, poses), word for word"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _state(gpe, pos, rad, world=WORLD, mode=None, prev=None, gravity=(0.0, 0.0), flags=0, **kw):
    return gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=gpe.MODE_NATIVE if mode is None else mode,
                     flags=gpe._lib.FLAG_GUARD_ALLOCS | flags, **kw)


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


def _run_state(gpe, mode=None, flags=0, movers=True, n=1500, **kw):
    pos, rad = CM.floor_scene(n)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD, mode=mode, gravity=M.RUN_GRAVITY, flags=flags, **kw)
    st.set_colliders(M.RUN_FLOOR)
    if movers:
        st.set_movers(M.run_movers())
    return st


# ---- references, computed once --------------------------------------------------------------------------------------
VARYING = [DT if s % 3 else DT / 2 for s in range(RUN_STEPS)]


@pytest.fixture(scope="module")
def run(oracle):
    """oracle step + the model's passes (movers, then the floor), 60 steps, no re-sort"""
    return M.run_reference(oracle, [DT] * RUN_STEPS)


@pytest.fixture(scope="module")
def run_resorted(oracle):
    return M.run_reference(oracle, [DT] * RUN_STEPS, resort_every=16, resort_first=True)


@pytest.fixture(scope="module")
def run_varying(oracle):
    return M.run_reference(oracle, VARYING)


# ---- 1. one pass equals the model -----------------------------------------------------------------------------------
def _scene_movers():
    """40 movers over the capsules of the static colliders' scene: both kinds, discs, thin walls, a pivot on an end
    point and one far from the capsule, omega = 0, v = 0, one reaching outside the world, one whose |b - a|^2
    overflows, one beyond 2^17 cells"""
    cs = _scene_colliders()
    rng = np.random.default_rng(17)
    out = []
    for j in range(30):
        a, b, R = cs[j, 0:2], cs[j, 2:4], cs[j, 4]
        if j % 2:
            pivot = a if j % 4 == 1 else a + rng.uniform(-20, 20, 2)
            out.append(M.rotor(a, b, R, pivot, rng.uniform(-20, 20)))
        else:
            out.append(M.linear(a, b, R, v=rng.uniform(-20, 20, 2), travel=0.0 if j % 4 else rng.uniform(2, 9)))
    s = cs[30:]
    out += [M.linear(s[0, 0:2], s[0, 2:4], s[0, 4], v=(0, 0), travel=3.0),           # the floor past both walls: v = 0
            M.rotor(s[1, 0:2], s[1, 2:4], s[1, 4], s[1, 0:2], 12.0),                 # a disc turning about its centre
            M.rotor(s[2, 0:2], s[2, 2:4], s[2, 4], s[2, 0:2], -9.0),                 # a wall, the pivot on its end a
            M.rotor(s[3, 0:2], s[3, 2:4], s[3, 4], (400.0, -300.0), 0.5),            # the pivot far from the capsule
            M.rotor(s[4, 0:2], s[4, 2:4], s[4, 4], (25.0, 70.0), 0.0),               # omega = 0
            M.linear(s[5, 0:2], s[5, 2:4], s[5, 4], v=(3.0, -4.0), travel=2.0),      # a point, R = 0
            M.rotor(s[6, 0:2], s[6, 2:4], s[6, 4], s[6, 0:2], 12.0),                 # the disc again: a tie on depth
            M.linear(s[7, 0:2], s[7, 2:4], s[7, 4], v=(6.0, 6.0), travel=0.0),       # from inside to far outside the world
            M.linear(s[8, 0:2], s[8, 2:4], s[8, 4]),                                 # |b - a|^2 overflows
            M.linear(s[9, 0:2], s[9, 2:4], s[9, 4], v=(0.0, 1.0), travel=2.0)]       # beyond 2^17 cells
    return M.rows(*out)


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("n", [4000, 3999, 1, 2, 3, 511, 512, 513])
def test_one_pass_equals_the_model(gpe, n, mode):
    """apply_movers(dt) on 40 movers, checked after 1, 2 and 7 advances with the particles placed around the POSED
    surfaces: pos bit for bit as the model, prev and radius untouched, pushed the model's count, the poses the model's.
    Even n, odd n and the tail alone; the edges of the pair loop (2, 3, 511, 512, 513); then particles that walk every
    mover: a radius above the bound, outside the grid."""
    movers = _scene_movers()
    assert len(movers) == 40 and M.dt_allowed(movers, DT)
    mv = M.Movers(movers)
    pos, rad = _scene_particles(n, mv.capsules(), seed=n)
    st = _state(gpe, pos, rad, mode=_mode(gpe, mode))
    st.set_movers(movers)
    assert same_rows(st.movers(), movers) and same_rows(st.mover_poses(), mv.poses())
    advances = pushed = 0
    for upto in (1, 2, 7):
        while advances < upto - 1:                                     # passes in between: wherever they leave things
            st.apply_movers(DT)
            pos, moved = mv.apply(pos, rad, WORLD, DT)
            pushed += int(moved.sum())
            advances += 1
        ahead = M.Movers(movers)
        ahead.set_poses(mv.poses())
        ahead.q0, ahead.q1 = M.advance(movers, ahead.q0, ahead.q1, DT)
        pos, rad = _scene_particles(n, ahead.capsules(), seed=n + upto)  # around the surfaces as the pass will see them
        prev = (pos + F32(0.125)).astype(F32)
        _set(st, pos, prev, rad)
        st.apply_movers(DT)
        want, moved = mv.apply(pos, rad, WORLD, DT)
        advances += 1
        pushed += int(moved.sum())
        got, got_prev, got_rad = _arrays(st)
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (upto, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert same_bits(got_prev, prev) and same_bits(got_rad, rad)
        assert same_rows(st.mover_poses(), mv.poses()), upto
        info = st.movers_info()
        print("n %d after %d advances: moved %d, grid %d x %d, %d bits listed" % (n, upto, moved.sum(), info["grid_x"], info["grid_y"], info["listed"]))
        assert (info["k"], info["passes"], info["pushed"], info["mask_words"]) == (40, advances, pushed, 1)
        assert info["grid_x"] == 101 and info["grid_y"] == 101         # cells of max(4 * 0.5, 200 / 128) = 2
        assert 2 * 101 * 101 <= info["listed"] < 101 * 101 * 40 // 4   # (two movers are listed everywhere)
        if n >= 2000:
            assert 300 < moved.sum() < n - 300                         # the scene exercises both outcomes
        elif n >= 511:
            assert 0 < moved.sum() < n                                 # both outcomes among the few
        elif n > 1:
            assert moved.any()                                         # (not the empty-cell path alone)
        pos = want
    # |r| = 3 > rb = 0.5 (add_particles keeps fmaxf(0.5, -3) = 0.5) and a particle outside the grid: every mover is walked
    caps = mv.capsules()
    disc = caps[31]
    extra = np.array([disc[0:2] + (0.0, 6.0), [30.0, 30.0], [201.0, 150.0], [210.0, 150.0]], F32)
    extra_rad = np.array([-3.0, -3.0, 0.5, 0.5], F32)
    st.add_particles(extra, extra_rad)
    assert abs(st.particles.get_max_radius()) == 0.5
    all_pos, all_rad = np.concatenate([pos, extra]), np.concatenate([rad, extra_rad])
    want, moved = mv.apply(all_pos, all_rad, WORLD, 0.0)               # dt = 0: the poses stay, the pass runs
    # the disc from 6 away; the floor from outside the world, inside the grid and (beyond 101 cells of 2) outside it
    assert moved[len(pos)] and moved[len(pos) + 2] and moved[len(pos) + 3]
    st.apply_movers(0.0)
    assert same_bits(st.positions(), want) and same_rows(st.mover_poses(), mv.poses())
    assert st.movers_info()["pushed"] == pushed + int(moved.sum())
    tags = _end(st)
    assert MOVER_TAGS <= tags


# ---- 2. word boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 65, 1024])
def test_mask_word_boundaries(gpe, k):
    """Small discs on a lattice, each turning about a pivot beside it: one mask word, exactly one, one bit into the
    second, all sixteen."""
    n = 4000
    j = np.arange(k)
    centre = np.stack([(j % 32) * 6.0 + 5.0, (j // 32) * 6.0 + 5.0], axis=1)
    movers = M.rows(*[M.rotor(c, c, 0.75, c + (1.0, 0.5), 3.0 + (i % 7)) for i, c in enumerate(centre)])
    rng = np.random.default_rng(k)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    which = rng.integers(0, k, 1500)
    pos[:1500] = (centre[which] + rng.uniform(-2.5, 2.5, (1500, 2))).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad)
    st.set_movers(movers)
    mv = M.Movers(movers)
    for s in range(3):
        pos, moved = mv.apply(pos, rad, WORLD, DT)
        st.apply_movers(DT)
        assert same_bits(st.positions(), pos), s
        assert moved.sum() > (10 if k == 1 else 100)
    assert same_rows(st.mover_poses(), mv.poses())
    info = st.movers_info()
    print("k %d: %d bits listed in %d x %d cells" % (k, info["listed"], info["grid_x"], info["grid_y"]))
    assert info["mask_words"] == (k + 63) // 64 and info["k"] == k and info["pushed"] == mv.pushed
    assert 0 < info["listed"] < k * info["grid_x"] * info["grid_y"]    # culling happens
    assert info["listed"] < 40 * k
    if k == 1024:                                                      # one too many is refused; the set stays
        with pytest.raises(gpe.GpeError) as e:
            st.set_movers(np.concatenate([movers, movers[:1]]))
        assert e.value.status == gpe._lib.GPE_ERR_INVALID_ARG and len(st.movers()) == 1024
    _end(st)


# ---- 3. at rest it is the static pass -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4000, 3999])
def test_movers_at_rest_are_static_colliders(gpe, n):
    cs = _scene_colliders()
    movers = M.rows(*[M.linear(c[0:2], c[2:4], c[4]) for c in cs])
    pos, rad = _scene_particles(n, cs, seed=n)
    moving = _state(gpe, pos, rad)
    static = _state(gpe, pos, rad)
    moving.set_movers(movers)
    static.set_colliders(cs)
    for s in range(2):
        moving.apply_movers(DT)
        static.apply_colliders()
        assert same_bits(moving.positions(), static.positions()), s
        assert moving.movers_info()["pushed"] == static.colliders_info()["pushed"] > 300
    poses = moving.mover_poses()
    assert same_bits(np.stack([poses[f] for f in ("ax", "ay", "bx", "by")], axis=1), cs[:, 0:4])
    assert not same_bits(moving.positions(), pos)
    _end(moving)
    _end(static)


# ---- 4. a run -------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("resorted", [False, True], ids=["no_resort", "resort_every_16"])
def test_run_steps_and_module_calls_equal_the_oracle_plus_the_model(gpe, run, run_resorted, mode, resorted):
    """The floor scene with a piston that turns within the run and a paddle: 60 steps by gpe_run, by gpe_step and by the
    per-module calls with the apply hooks; all three are the oracle's step with the model's passes behind it."""
    frames, pushed_movers, pushed_floor = run_resorted if resorted else run
    every, first = (16, True) if resorted else (0, False)
    m = _mode(gpe, mode)
    runner, stepper, modular = (_run_state(gpe, mode=m) for _ in range(3))
    runner.run(DT, RUN_STEPS, resort_every=every, resort_first=first)
    for s in range(RUN_STEPS):
        resort = (s == 0 and first) or bool(every and s > 0 and s % every == 0)
        stepper.update(DT, resort=resort)
        _module_step(modular, DT, resort)
        for st in (stepper, modular):
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
        assert same_rows(stepper.mover_poses(), frames[s][2]), s
    assert frames[-1][2]["q1"][0] == -1.0 or frames[-1][2]["q1"][0] == 1.0
    assert -1.0 in [float(f[2]["q1"][0]) for f in frames]              # the piston reversed within the run
    for st in (runner, stepper, modular):
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
        assert same_rows(st.mover_poses(), frames[-1][2])
        info = st.movers_info()
        assert (info["k"], info["passes"], info["pushed"]) == (2, RUN_STEPS, pushed_movers)
        assert st.colliders_info()["pushed"] == pushed_floor
        _end(st)
    assert pushed_movers > 200


def test_a_dt_that_changes_between_steps(gpe, run_varying):
    frames, pushed_movers, _ = run_varying
    stepper, modular = _run_state(gpe), _run_state(gpe, mode=gpe.MODE_COMPAT)
    for s, dt in enumerate(VARYING):
        stepper.update(dt)
        _module_step(modular, dt, False)
        for st in (stepper, modular):
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
            assert same_rows(st.mover_poses(), frames[s][2]), s
    assert stepper.movers_info()["pushed"] == modular.movers_info()["pushed"] == pushed_movers
    _end(stepper)
    _end(modular)


# ---- 5. unarmed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_movers_nothing_changes_and_nothing_is_launched(gpe, run, mode):
    m = _mode(gpe, mode)
    never = _run_state(gpe, mode=m, movers=False, profiling=True)
    cleared = _run_state(gpe, mode=m, profiling=True)
    cleared.clear_movers()
    assert len(cleared.movers()) == 0 and len(cleared.mover_poses()) == 0
    assert cleared.movers_info() == dict(k=0, passes=0, pushed=0, grid_x=0, grid_y=0, mask_words=0, listed=0)
    results = []
    for st in (never, cleared):
        st.apply_movers(DT)                                            # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        results.append(_arrays(st))
        assert "Movers" not in st.ctx.timings() and st.ctx.timings()["Colliders"][1] == 20
        assert not any(t.startswith("grid.mover_") for t, _, _, state in st.ctx.guard_registry() if state == "live")
    assert all(same_bits(a, b) for a, b in zip(*results))
    assert not same_bits(results[0][0], run[0][19][0])                 # (the movers do change this scene)
    _end(never)
    _end(cleared)
    armed = _run_state(gpe, mode=m, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), run[0][19][0])
    assert armed.ctx.timings()["Movers"][1] == 20
    _end(armed)


# ---- 6. step state --------------------------------------------------------------------------------------------------
def _same_as_twin(st, tw, what):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    assert same_bits(got[0], pos) and same_bits(got[1], prev) and same_bits(got[2], rad), what
    assert same_rows(st.movers(), tw.m.movers) and same_rows(st.mover_poses(), tw.m.poses()), what


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_and_the_poses_survive_everything_but_set_movers(gpe, oracle, mode):
    world = (100.0, 100.0)
    cs = np.array([[-5, 80, 105, 80, 5]], F32)
    movers = M.rows(M.linear((10, 50), (10, 76), 2.0, v=(24.0, 0.0), travel=30.0),
                    M.rotor((60, 55), (72, 55), 1.5, (60, 55), -5.0),
                    M.linear((150, 150), (150, 150), 8.0, v=(0.0, 0.0)))
    rng = np.random.default_rng(12)
    n = 3999
    pos = rng.uniform(1, 99, (n, 2)).astype(F32)
    pos[:, 1] = pos[:, 1] * F32(0.7)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=(0.0, 60.0), mode=_mode(gpe, mode))
    tw = M.Twin(oracle, pos, rad, world=world, gravity=(0.0, 60.0))
    st.set_colliders(cs); tw.set_colliders(cs)
    st.set_movers(movers); tw.set_movers(movers)

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what)
        info = st.movers_info()
        assert (info["passes"], info["pushed"]) == (tw.m.passes, tw.m.pushed), what
        return info

    steps("start")
    pos2 = rng.uniform(1, 99, (n - 500, 2)).astype(F32)
    _set(st, pos2, pos2, rad[:n - 500]); tw.set_particles(pos2, pos2, rad[:n - 500])
    steps("set_particles")
    add = rng.uniform(5, 95, (300, 2)).astype(F32)
    st.add_particles(add, np.full(300, 0.5, F32)); tw.add(add, np.full(300, 0.5, F32))
    steps("add")
    assert st.remove_particles_in_circle((50, 40), 12.0) == tw.remove_circle(50, 40, 12.0) > 0
    steps("remove")
    who = np.arange(0, 400, 2, dtype=U32)
    where = (rng.uniform(-4, 4, (200, 2)) + (66.0, 55.0)).astype(F32)  # onto the paddle
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    grow = rng.uniform(5, 95, (6000, 2)).astype(F32)                   # past the capacity
    grow[:, 1] *= F32(0.5)
    st.add_particles(grow, np.full(6000, 0.5, F32)); tw.add(grow, np.full(6000, 0.5, F32))
    before = steps("growth")
    # a larger radius: the next build takes the new bound
    st.edit_particles(indices=[7], radii=[1.5]); tw.edit([7], "index", radius=[1.5])
    after = steps("radius edit")
    assert (before["grid_x"], after["grid_x"]) == (51, 17)             # cells of 2 -> cells of 6
    # gpe_set_world: the view follows without a rebuild on the host; the mover at (150, 150) in the new part acts
    st.ctx.call("gpe_set_world", 200.0, 200.0); tw.set_world(200.0, 200.0)
    who = np.array([3, 4], U32)
    where = np.array([[153.0, 150.0], [150.0, 144.0]], F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    pushed = tw.m.pushed
    st.apply_movers(DT); tw.apply_movers(DT)
    _same_as_twin(st, tw, "set_world")
    assert tw.m.pushed >= pushed + 2 and st.movers_info()["pushed"] == tw.m.pushed
    assert st.movers_info()["grid_x"] == 34
    assert tuple(st.positions()[3]) == (158.5, 150.0)                  # from 3 away to R + r = 8.5 away
    steps("after set_world")
    # set_mover_poses(mover_poses()) is the identity; a rewound state replays
    poses = st.mover_poses()
    st.set_mover_poses(poses)
    assert same_rows(st.mover_poses(), poses)
    steps("poses set to themselves")
    junk = poses.copy()
    junk["ax"] = 1e9                                                   # ax .. by of the input are ignored
    st.set_mover_poses(junk); tw.m.set_poses(poses)
    _same_as_twin(st, tw, "rewound")
    steps("after the rewind")
    # a new set replaces the old one, starts fresh and zeroes the counters
    st.set_movers(movers[:2]); tw.set_movers(movers[:2])
    info = st.movers_info()
    assert (info["k"], info["passes"], info["pushed"]) == (2, 0, 0)
    _same_as_twin(st, tw, "new set")
    steps("new set, stepped")
    tw.close()
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_continue_on_the_same_bits(gpe, run, tmp_path, mode):
    L = gpe._lib
    m = _mode(gpe, mode)
    frames = run[0]
    st = _run_state(gpe, mode=m)
    st.run(DT, 30, resort_every=0, resort_first=False)
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert same_rows(d["movers"].astype(gpe.MOVER_DTYPE), M.run_movers())
        assert same_rows(d["mover_poses"].astype(gpe.MOVER_POSE_DTYPE), frames[29][2])
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    assert same_rows(back.movers(), st.movers()) and same_rows(back.mover_poses(), st.mover_poses())
    for s in (st, back):
        s.run(DT, 30, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(s)
        assert same_bits(pos, frames[59][0]) and same_bits(prev, frames[59][1])
        assert same_rows(s.mover_poses(), frames[59][2])
    assert back.movers_info()["passes"] == 30 and st.movers_info()["passes"] == 60
    _end(back)
    st.clear_movers()                                                  # a context without movers writes none and loads none
    st.save(path)
    with np.load(path) as d:
        assert "movers" not in d.files and "mover_poses" not in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    assert len(back.movers()) == 0
    _end(back)
    _end(st)


def test_tracer_and_monitor_frames_show_the_state_behind_the_movers(gpe, run):
    frames = run[0]
    st = _run_state(gpe)
    st.enable_uids()
    uids = np.array([0, 7, 100, 1499, 731], U32)
    st.tracers_begin(uids, every=1, frames=32, prev=True)
    st.monitor_begin(every=1, frames=32)
    st.run(DT, 25, resort_every=0, resort_first=False)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 25 and recorded == 25
    for s in range(25):
        pos, prev, _ = frames[s]
        assert same_bits(tr.pos[s], pos[uids]) and same_bits(tr.prev[s], prev[uids]), s
        assert rec["max_x"][s] == pos[:, 0].max() and rec["min_x"][s] == pos[:, 0].min() and rec["n"][s] == 1500
    st.tracers_end(); st.monitor_end()
    _end(st)


def test_movers_before_there_are_particles(gpe):
    L = gpe._lib
    ctx = gpe.Context(world=M.RUN_WORLD, gravity=M.RUN_GRAVITY, flags=L.FLAG_GUARD_ALLOCS)
    ps = gpe.ParticleSystem(ctx)
    ps.set_movers(M.run_movers())
    ps.apply_movers(DT)                                                # no particles: GPE_OK, nothing done, nothing advanced
    mv = M.Movers(M.run_movers())
    assert ps.movers_info() == dict(k=2, passes=0, pushed=0, grid_x=0, grid_y=0, mask_words=1, listed=0)
    assert same_rows(ps.mover_poses(), mv.poses())
    pos, rad = CM.floor_scene(200)
    pos[:100] = (np.random.default_rng(3).uniform(-3, 3, (100, 2)) + (5.0, 35.0)).astype(F32)   # onto the piston
    f = C.POINTER(C.c_float)
    ctx.call("gpe_set_particles", pos.ctypes.data_as(f), None, rad.ctypes.data_as(f), 200)
    ps.apply_movers(DT)
    want, moved = mv.apply(pos, rad, M.RUN_WORLD, DT)
    assert same_bits(ctx.download(L.POS, F32, (-1, 2)), want) and moved.sum() > 20
    assert ps.movers_info()["pushed"] == int(moved.sum()) and same_rows(ps.mover_poses(), mv.poses())
    ctx.guard_check()
    assert ctx.guard_damaged == 0
    ctx.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_the_poses_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    pos, rad = CM.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD, gravity=M.RUN_GRAVITY)
    tw = M.Twin(oracle, pos, rad, world=M.RUN_WORLD, gravity=M.RUN_GRAVITY)
    movers = M.run_movers()                                            # |omega| 6; speed 30 over a travel of 10
    st.set_movers(movers); tw.set_movers(movers)                       # (no static colliders: their refusals come first)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info, poses = st.movers_info(), st.mover_poses()
    assert info["passes"] == 5

    def untouched(what):
        assert same_rows(st.movers(), movers) and same_rows(st.mover_poses(), poses), what
        assert st.movers_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    def rows(*ms):
        out = (L.GpeMover * len(ms))()
        for o, m in zip(out, ms):
            for name, value in zip(M.FIELDS, m):
                setattr(o, name, value)
        return out

    def pose_rows(*ps):
        out = (L.GpeMoverPose * len(ps))()
        for o, (q0, q1) in zip(out, ps):
            o.q0, o.q1 = q0, q1
        return out

    #        ax ay bx by R    kind vx vy travel px py omega flags reserved
    ok = (1.0, 2.0, 3.0, 4.0, 0.5, 0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0, 0, 0)

    def but(**kw):
        return tuple(kw.get(name, value) for name, value in zip(M.FIELDS, ok))

    h = st.ctx.h
    k = C.c_uint64()
    minfo = L.GpeMoversInfo(struct_size=C.sizeof(L.GpeMoversInfo))
    assert lib.gpe_set_movers(None, rows(ok), 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_movers(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_mover_poses(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_set_mover_poses(None, pose_rows((0, 1)), 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_movers(None, DT) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_movers_info(None, C.byref(minfo)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    bad = {
        "NULL movers with k > 0": lambda: lib.gpe_set_movers(h, None, 2),
        "k > GPE_MOVERS_MAX": lambda: lib.gpe_set_movers(h, rows(*([ok] * (L.MOVERS_MAX + 1))), L.MOVERS_MAX + 1),
        "NaN ax": lambda: lib.gpe_set_movers(h, rows(ok, but(ax=NAN)), 2),
        "inf ay": lambda: lib.gpe_set_movers(h, rows(ok, but(ay=INF)), 2),
        "-inf bx": lambda: lib.gpe_set_movers(h, rows(ok, but(bx=-INF)), 2),
        "NaN by": lambda: lib.gpe_set_movers(h, rows(but(by=NAN), ok), 2),
        "NaN radius": lambda: lib.gpe_set_movers(h, rows(ok, but(radius=NAN)), 2),
        "inf radius": lambda: lib.gpe_set_movers(h, rows(ok, but(radius=INF)), 2),
        "negative radius": lambda: lib.gpe_set_movers(h, rows(ok, but(radius=-0.25)), 2),
        "NaN vx": lambda: lib.gpe_set_movers(h, rows(ok, but(vx=NAN)), 2),
        "inf vy": lambda: lib.gpe_set_movers(h, rows(ok, but(vy=INF)), 2),
        "a speed that overflows": lambda: lib.gpe_set_movers(h, rows(ok, but(vx=3e38, vy=3e38)), 2),
        "NaN travel": lambda: lib.gpe_set_movers(h, rows(ok, but(travel=NAN)), 2),
        "negative travel": lambda: lib.gpe_set_movers(h, rows(ok, but(travel=-1.0)), 2),
        "inf px": lambda: lib.gpe_set_movers(h, rows(ok, but(kind=1, px=INF)), 2),
        "NaN py": lambda: lib.gpe_set_movers(h, rows(ok, but(kind=1, py=NAN)), 2),
        "inf omega": lambda: lib.gpe_set_movers(h, rows(ok, but(kind=1, omega=INF)), 2),
        "NaN omega on a LINEAR mover": lambda: lib.gpe_set_movers(h, rows(ok, but(omega=NAN)), 2),
        "unknown kind": lambda: lib.gpe_set_movers(h, rows(ok, but(kind=2)), 2),
        "flags": lambda: lib.gpe_set_movers(h, rows(ok, but(flags=1)), 2),
        "reserved": lambda: lib.gpe_set_movers(h, rows(ok, but(reserved=7)), 2),
        "info struct_size": lambda: lib.gpe_get_movers_info(h, C.byref(L.GpeMoversInfo(struct_size=C.sizeof(L.GpeMoversInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_movers_info(h, None),
        "get NULL k": lambda: lib.gpe_get_movers(h, None, 0, None),
        "get NULL out": lambda: lib.gpe_get_movers(h, None, 3, C.byref(k)),
        "poses NULL k": lambda: lib.gpe_get_mover_poses(h, None, 0, None),
        "poses NULL out": lambda: lib.gpe_get_mover_poses(h, None, 2, C.byref(k)),
        "set poses: k is not the set's size": lambda: lib.gpe_set_mover_poses(h, pose_rows((0, 1)), 1),
        "set poses: NULL": lambda: lib.gpe_set_mover_poses(h, None, 2),
        "set poses: NaN state": lambda: lib.gpe_set_mover_poses(h, pose_rows((0, 1), (NAN, 0)), 2),
        "set poses: inf state": lambda: lib.gpe_set_mover_poses(h, pose_rows((INF, 1), (1, 0)), 2),
        "set poses: sgn not +-1": lambda: lib.gpe_set_mover_poses(h, pose_rows((1, 0.5), (1, 0)), 2),
        "set poses: g above travel": lambda: lib.gpe_set_mover_poses(h, pose_rows((10.5, 1), (1, 0)), 2),
        "set poses: g below 0": lambda: lib.gpe_set_mover_poses(h, pose_rows((-0.5, -1), (1, 0)), 2),
        # the dt contract: |6 * dt| <= 0.5 and 30 * |dt| <= 10
        "step: omega * dt": lambda: lib.gpe_step(h, 0.09, 0),
        "step: speed * dt": lambda: lib.gpe_step(h, -0.4, 0),
        "step: NaN dt": lambda: lib.gpe_step(h, NAN, 0),
        "run: omega * dt": lambda: lib.gpe_run(h, 0.09, 3, 0, 0),
        "run: inf dt": lambda: lib.gpe_run(h, INF, 3, 0, 1),
        "apply: omega * dt": lambda: lib.gpe_apply_movers(h, -0.09),
        "apply: NaN dt": lambda: lib.gpe_apply_movers(h, NAN),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        untouched(what)
    assert L.MOVERS_MAX == 1024 and not M.dt_allowed(movers, 0.09) and M.dt_allowed(movers, 0.08)
    # the other way round: sharding a context that holds movers
    keys = np.arange(600, dtype=U32)
    sharding = {
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, 600, 500),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), 600, 0),
    }
    for what, call in sharding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"moving colliders" in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK                    # switching them off is no sharding
    # the largest steps the contract admits are taken, and the context goes on as the twin does
    for dt in (0.08, -0.08, 0.0):
        st.update(dt); tw.step(dt)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 is accepted as 0; a partial read delivers the first rows
    assert lib.gpe_set_movers(h, rows(but(radius=-0.0), ok), 2) == L.GPE_OK
    out = rows(ok, ok, ok)
    assert lib.gpe_get_movers(h, out, 1, C.byref(k)) == L.GPE_OK and k.value == 2
    assert bits([out[0].radius]).tolist() == [0] and out[0].by == 4.0
    assert (out[1].radius, out[2].radius) == (0.5, 0.5)               # past the capacity: left as they were
    got = pose_rows((9, 9), (9, 9))
    assert lib.gpe_get_mover_poses(h, got, 1, C.byref(k)) == L.GPE_OK and k.value == 2
    assert (got[0].q0, got[0].q1, got[0].ax, got[1].q0) == (0.0, 1.0, 1.0, 9.0)
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_movers(gpe, how):
    L = gpe._lib
    pos, rad = CM.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_movers(M.run_movers())
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.movers()) == 0 and st.movers_info()["k"] == 0
    st.apply_movers(DT)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)
