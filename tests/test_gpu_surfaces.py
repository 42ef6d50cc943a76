"""GPU (-m gpu): surface materials (gpe_set_surfaces / gpe_get_surfaces; csrc/k_surface.h, the surface forms of the passes
in csrc/k_colliders.hip and csrc/k_movers.hip, csrc/gpe_surfaces.hip).

The rule is a binary32 function: every comparison is bit for bit (uint32 views; a NaN of the model must be a NaN on the
device) against the numpy model (tests/_surfaces_model.py: brute force, no grid), and the steps against the CPU oracle
with the model's passes behind every step (movers, then static colliders, each with its surfaces).  Every context runs
under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _movers_model as M
from tests import _surfaces_model as S

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = M.RUN_DT
DTS = M.TABLE_DTS                                                      # 40 steps; a zero and a negative dt among them
NAN, INF = float("nan"), float("inf")
WORLD = S.ONE_PASS_WORLD
SURFACE_TAGS = {"grid.collider_surf", "grid.mover_surf", "grid.mover_old"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    """the same bits; where the model has a NaN the device has a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_rows(a, b):
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


def _live(st):
    return {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}


def _arrays(st):
    return st.positions(), st.previous_positions(), st.radii()


def _set(st, pos, prev, rad):
    f = C.POINTER(C.c_float)
    pos, prev, rad = (np.ascontiguousarray(a, F32) for a in (pos, prev, rad))
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), prev.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else None


def _differ(got, want):
    return np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]


# ---- 1. one pass equals the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("n", [4000, 3999, 1, 2, 3, 511, 512, 513])
def test_one_pass_equals_the_model(gpe, n, mode):
    """The static colliders' scene and the movers' scene with mixed surfaces, every fourth row PLAIN, velocities of every
    kind (approaching, separating, tiny, not finite): pos and prev bit for bit as the model through apply_colliders, then
    through apply_movers(dt).  Even n, odd n and the tail alone; the edges of the pair loop (2, 3, 511, 512, 513: all
    their particles near surfaces, the branch counts asked of the large scenes only); then the particles that walk every
    obstacle."""
    cs, surf, pos, prev, rad = S.collider_scene(n)
    st = _state(gpe, pos, rad, prev=prev, mode=_mode(gpe, mode))
    st.set_colliders(cs)
    st.set_surfaces("colliders", surf)
    assert same_rows(st.surfaces("colliders"), S.stored(surf)) and len(st.surfaces("movers")) == 0
    pushed = 0
    for turn in range(2):                                              # the second pass starts from the first one's result
        want, want_prev, moved, br = S.apply(pos, prev, rad, cs, surf, WORLD)
        if n >= 2000 and turn == 0:
            print("n %d colliders: %s" % (n, S.coverage(moved, br, n)))
        elif n > 1 and turn == 0:
            assert moved.any()                                         # (not the empty-cell path alone)
        st.apply_colliders()
        got, got_prev, got_rad = _arrays(st)
        bad = _differ(got, want)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        bad = _differ(got_prev, want_prev)
        assert bad.size == 0, (turn, bad[:5], prev[bad[:5]], got_prev[bad[:5]], want_prev[bad[:5]])
        assert np.array_equal(bits(got_rad), bits(rad))
        pushed += int(moved.sum())
        assert st.colliders_info()["pushed"] == pushed
        pos, prev = want, want_prev
    # |r| = 3 > rb = 0.5 and a particle outside the grid: every collider is walked
    extra = np.array([[100.0, 106.0], [60.0, 62.75], [30.0, 30.0], [201.0, 150.0], [210.0, 150.0]], F32)
    extra_rad = np.array([-3.0, -3.0, -3.0, 0.5, 0.5], F32)
    st.add_particles(extra, extra_rad)
    assert abs(st.particles.get_max_radius()) == 0.5
    all_pos, all_prev, all_rad = np.concatenate([pos, extra]), np.concatenate([prev, extra]), np.concatenate([rad, extra_rad])
    st.edit_particles(indices=np.arange(n, n + 5, dtype=U32), previous=(extra - F32(0.25)).astype(F32))
    all_prev[n:] = (extra - F32(0.25)).astype(F32)
    want, want_prev, moved, _ = S.apply(all_pos, all_prev, all_rad, cs, surf, WORLD)
    assert moved[n] and moved[n + 1] and moved[n + 3] and moved[n + 4]
    st.apply_colliders()
    got, got_prev, _ = _arrays(st)
    assert same_bits(got, want) and same_bits(got_prev, want_prev)
    tags = _end(st)
    assert "grid.collider_surf" in tags and not {"grid.mover_surf", "grid.mover_old"} & tags

    # the movers
    movers, msurf = S.mover_scene_set()
    mv = S.Movers(movers)
    mv.set_surfaces(msurf)
    pos, prev, rad = S.mover_scene_particles(n, mv, DT, seed=n)
    st = _state(gpe, pos, rad, prev=prev, mode=_mode(gpe, mode))
    st.set_movers(movers)
    st.set_surfaces("movers", msurf)
    assert same_rows(st.surfaces("movers"), S.stored(msurf)) and len(st.surfaces("colliders")) == 0
    for turn in range(3):
        if turn:
            pos, prev, rad = S.mover_scene_particles(n, mv, DT, seed=n + turn)
            _set(st, pos, prev, rad)
        want, want_prev, moved, br = mv.apply_surface(pos, prev, rad, WORLD, DT)
        if n >= 2000 and turn == 0:
            print("n %d movers: %s" % (n, S.coverage(moved, br, n, movers=True)))
        elif n > 1 and turn == 0:
            assert moved.any()
        st.apply_movers(DT)
        got, got_prev, got_rad = _arrays(st)
        bad = _differ(got, want)
        assert bad.size == 0, (turn, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        bad = _differ(got_prev, want_prev)
        assert bad.size == 0, (turn, bad[:5], prev[bad[:5]], got_prev[bad[:5]], want_prev[bad[:5]])
        assert np.array_equal(bits(got_rad), bits(rad)) and same_rows(st.mover_poses(), mv.poses())
        assert st.movers_info()["pushed"] == mv.pushed
    pos, prev = want, want_prev
    caps = mv.capsules()
    extra = np.array([caps[31, 0:2] + (0.0, 6.0), [30.0, 30.0], [201.0, 150.0], [210.0, 150.0]], F32)
    extra_rad = np.array([-3.0, -3.0, 0.5, 0.5], F32)
    st.add_particles(extra, extra_rad)
    st.edit_particles(indices=np.arange(n, n + 4, dtype=U32), previous=(extra + F32(0.125)).astype(F32))
    all_pos, all_rad = np.concatenate([pos, extra]), np.concatenate([rad, extra_rad])
    all_prev = np.concatenate([prev, (extra + F32(0.125)).astype(F32)])
    want, want_prev, moved, br = mv.apply_surface(all_pos, all_prev, all_rad, WORLD, 0.0)   # dt = 0: the walls stand still
    assert moved[n] and moved[n + 2] and moved[n + 3] and not br["wall_moved"].any()
    st.apply_movers(0.0)
    got, got_prev, _ = _arrays(st)
    assert same_bits(got, want) and same_bits(got_prev, want_prev) and same_rows(st.mover_poses(), mv.poses())
    tags = _end(st)
    assert {"grid.mover_surf", "grid.mover_old"} <= tags and "grid.collider_surf" not in tags


# ---- 2. the movers' mask-word boundaries ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 65, 1024])
def test_mask_word_boundaries_with_surfaces(gpe, k):
    """Small discs on a lattice, each turning about a pivot beside it, each with its own surface: one mask word, exactly
    one, one bit into the second, all sixteen."""
    n = 4000
    j = np.arange(k)
    centre = np.stack([(j % 32) * 6.0 + 5.0, (j // 32) * 6.0 + 5.0], axis=1)
    movers = M.rows(*[M.rotor(c, c, 0.75, c + (1.0, 0.5), 3.0 + (i % 7)) for i, c in enumerate(centre)])
    surf = S.scene_surfaces(k, seed=k)
    rng = np.random.default_rng(k)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    which = rng.integers(0, k, 1500)
    pos[:1500] = (centre[which] + rng.uniform(-2.5, 2.5, (1500, 2))).astype(F32)
    prev = S.scene_prev(pos, k + 1)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=prev)
    st.set_movers(movers)
    st.set_surfaces("movers", surf)
    mv = S.Movers(movers)
    mv.set_surfaces(surf)
    for s in range(3):
        pos, prev, moved, br = mv.apply_surface(pos, prev, rad, WORLD, DT)
        st.apply_movers(DT)
        got, got_prev, _ = _arrays(st)
        assert same_bits(got, pos) and same_bits(got_prev, prev), s
        assert moved.sum() > (10 if k == 1 else 100) and br["wall_moved"].sum() > (0 if k == 1 else 50)
    assert same_rows(st.mover_poses(), mv.poses()) and same_rows(st.surfaces("movers"), surf)
    info = st.movers_info()
    assert info["mask_words"] == (k + 63) // 64 and info["k"] == k and info["pushed"] == mv.pushed
    _end(st)


# ---- 3. runs --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(oracle):
    """oracle step + the model's passes with surfaces (movers, then the floor), 40 steps of varying dt, no re-sort"""
    return S.run_reference(oracle, DTS)


@pytest.fixture(scope="module")
def run_resorted(oracle):
    return S.run_reference(oracle, DTS, resort_every=16, resort_first=True)


@pytest.fixture(scope="module")
def run_plain(oracle):
    """the same run without surfaces: the movers' reference"""
    return M.run_reference(oracle, DTS)


def _run_state(gpe, mode=None, flags=0, surfaces=True, n=1500, **kw):
    pos, rad = CM.floor_scene(n)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD, mode=mode, gravity=M.RUN_GRAVITY, flags=flags, **kw)
    st.set_colliders(M.RUN_FLOOR)
    st.set_movers(M.run_movers())
    if surfaces:
        st.set_surfaces("colliders", S.RUN_COLLIDER_SURFACES)
        st.set_surfaces("movers", S.RUN_MOVER_SURFACES)
    return st


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


def _resort_at(s, every, first):
    return (s == 0 and first) or bool(every and s > 0 and s % every == 0)


def _segments(dts, every, first):
    """the runs of gpe_run that take the steps of dts: a new one where dt changes or a re-sort is due -> (start, count,
    dt, resort_first)"""
    out = []
    for s, dt in enumerate(dts):
        due = _resort_at(s, every, first)
        if out and out[-1][2] == dt and not due:
            out[-1][1] += 1
        else:
            out.append([s, 1, dt, due])
    return out


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("resorted", [False, True], ids=["no_resort", "resort_every_16"])
def test_runs_steps_and_module_calls_equal_the_oracle_plus_the_model(gpe, run, run_resorted, run_plain, mode, resorted):
    """The floor with (0.5, 0.3), a piston and a paddle with surfaces of their own, 40 steps whose dt is also zero and
    negative (the walls stand still, the walls move back): by gpe_run, by gpe_step and by the per-module calls with the
    two hooks; all three are the oracle's step with the model's passes behind it."""
    frames, pushed_movers, pushed_floor = run_resorted if resorted else run
    every, first = (16, True) if resorted else (0, False)
    m = _mode(gpe, mode)
    runner, stepper, modular = (_run_state(gpe, mode=m) for _ in range(3))
    for start, count, dt, due in _segments(DTS, every, first):
        runner.run(dt, count, resort_every=0, resort_first=due)
        last = start + count - 1
        pos, prev, _ = _arrays(runner)
        assert same_bits(pos, frames[last][0]) and same_bits(prev, frames[last][1]), last
    for s, dt in enumerate(DTS):
        resort = _resort_at(s, every, first)
        stepper.update(dt, resort=resort)
        _module_step(modular, dt, resort)
        for st in (stepper, modular):
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
        assert same_rows(stepper.mover_poses(), frames[s][2]), s
    for st in (runner, stepper, modular):
        assert same_rows(st.mover_poses(), frames[-1][2])
        assert st.movers_info()["pushed"] == pushed_movers and st.colliders_info()["pushed"] == pushed_floor
        _end(st)
    assert pushed_movers > 100 and pushed_floor > 1000
    if not resorted:                                                   # (the surfaces do change this scene)
        assert not same_bits(frames[-1][0], run_plain[0][-1][0]) and not same_bits(frames[-1][1], run_plain[0][-1][1])


# ---- 4. PLAIN everywhere, and no surfaces at all --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_all_plain_surfaces_and_no_surfaces_are_the_plain_passes(gpe, run_plain, mode):
    """All-PLAIN surfaces run the surface kernels and give the bits of the run without surfaces; a context that never set
    a surface, and one that cleared them, launch the scopes and hold the allocations they did before."""
    m = _mode(gpe, mode)
    frames = run_plain[0]
    plain = _run_state(gpe, mode=m, surfaces=False)
    plain.set_surfaces("colliders", S.uniform(1, 0.9, 0.7, S.PLAIN))
    plain.set_surfaces("movers", S.uniform(2, 0.9, 0.7, S.PLAIN))
    assert SURFACE_TAGS <= _live(plain)
    never = _run_state(gpe, mode=m, surfaces=False, profiling=True)
    cleared = _run_state(gpe, mode=m, profiling=True)
    cleared.clear_surfaces("colliders")
    cleared.clear_surfaces("movers")
    assert len(cleared.surfaces("colliders")) == 0 and len(cleared.surfaces("movers")) == 0
    for s, dt in enumerate(DTS):
        for st in (plain, never, cleared):
            st.update(dt)
            pos, prev, _ = _arrays(st)
            assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    for st in (never, cleared):
        st.run(DT, 10, resort_every=0, resort_first=False)
        t = st.ctx.timings()
        assert t["Movers"][1] == len(DTS) + 10 and t["Colliders"][1] == len(DTS) + 10
        assert not any("surf" in name.lower() for name in t)           # no scope of its own
        assert not SURFACE_TAGS & _live(st)
    assert not SURFACE_TAGS & {t for t, _, _, _ in never.ctx.guard_registry()}   # never allocated, not only released
    for st in (plain, never, cleared):
        _end(st)


# ---- 5. step state --------------------------------------------------------------------------------------------------
def _same_as_twin(st, tw, what):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    assert same_bits(got[0], pos) and same_bits(got[1], prev) and same_bits(got[2], rad), what
    assert same_rows(st.mover_poses(), tw.m.poses()), what
    for target in ("colliders", "movers"):
        assert same_rows(st.surfaces(target), tw.surfaces(target)), (what, target)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_surfaces_survive_everything_but_a_new_set(gpe, oracle, mode):
    world = (100.0, 100.0)
    cs = np.array([[-5, 80, 105, 80, 5], [50, 40, 50, 40, 3]], F32)
    movers = M.rows(M.linear((10, 50), (10, 76), 2.0, v=(24.0, 0.0), travel=30.0),
                    M.rotor((60, 55), (72, 55), 1.5, (60, 55), -5.0))
    csurf, msurf = S.rows((0.6, 0.4), (1.0, 0.0, S.PLAIN)), S.rows((0.2, 0.9), (0.9, 0.1))
    rng = np.random.default_rng(12)
    n = 2999
    pos = rng.uniform(1, 99, (n, 2)).astype(F32)
    pos[:, 1] = pos[:, 1] * F32(0.7)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=(0.0, 60.0), mode=_mode(gpe, mode))
    tw = S.Twin(oracle, pos, rad, world=world, gravity=(0.0, 60.0))
    for h in (st, tw):
        h.set_colliders(cs)
        h.set_movers(movers)
        h.set_surfaces("colliders", csurf)
        h.set_surfaces("movers", msurf)

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what)
        assert st.movers_info()["pushed"] == tw.m.pushed and st.colliders_info()["pushed"] == tw.pushed, what

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
    st.enable_uids(); tw.enable_uids()
    steps("uids on")
    st.enable_uids(False); tw.enable_uids(False)
    steps("uids off")
    grow = rng.uniform(5, 95, (5000, 2)).astype(F32)                   # past the capacity
    grow[:, 1] *= F32(0.5)
    st.add_particles(grow, np.full(5000, 0.5, F32)); tw.add(grow, np.full(5000, 0.5, F32))
    steps("growth")
    st.ctx.call("gpe_set_world", 120.0, 100.0); tw.set_world(120.0, 100.0)
    steps("set_world")
    # a new set drops its own surfaces and leaves the other set's
    st.set_colliders(cs[:1]); tw.set_colliders(cs[:1])
    assert len(st.surfaces("colliders")) == 0 and same_rows(st.surfaces("movers"), msurf)
    assert "grid.collider_surf" not in _live(st) and "grid.mover_surf" in _live(st)
    steps("new colliders")
    st.set_movers(movers[:1]); tw.set_movers(movers[:1])
    assert len(st.surfaces("movers")) == 0 and not SURFACE_TAGS & _live(st)
    steps("new movers")
    st.set_surfaces("colliders", csurf[:1]); tw.set_surfaces("colliders", csurf[:1])
    st.clear_colliders(); tw.set_colliders(np.zeros((0, 5), F32))      # k == 0 drops them too
    assert len(st.surfaces("colliders")) == 0 and not SURFACE_TAGS & _live(st)
    steps("no colliders")
    tw.close()
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_continue_on_the_same_bits(gpe, tmp_path, mode):
    L = gpe._lib
    m = _mode(gpe, mode)
    st = _run_state(gpe, mode=m)
    st.run(DT, 20, resort_every=0, resort_first=False)
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert same_rows(d["collider_surfaces"].astype(gpe.SURFACE_DTYPE), S.RUN_COLLIDER_SURFACES)
        assert same_rows(d["mover_surfaces"].astype(gpe.SURFACE_DTYPE), S.RUN_MOVER_SURFACES)
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    for target in ("colliders", "movers"):
        assert same_rows(back.surfaces(target), st.surfaces(target)) and len(back.surfaces(target))
    results = []
    for s in (st, back):
        s.run(DT, 20, resort_every=0, resort_first=False)
        results.append(_arrays(s) + (s.mover_poses(),))
    assert all(same_bits(a, b) for a, b in zip(results[0][:3], results[1][:3])) and same_rows(results[0][3], results[1][3])
    _end(back)
    st.clear_surfaces("movers")                                        # what is absent is not written
    st.save(path)
    with np.load(path) as d:
        assert "mover_surfaces" not in d.files and "collider_surfaces" in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    assert len(back.surfaces("movers")) == 0 and len(back.surfaces("colliders")) == 1
    _end(back)
    _end(st)


# ---- 6. the observers -----------------------------------------------------------------------------------------------
def test_tracer_and_monitor_frames_show_the_state_behind_the_surface_passes(gpe, run):
    frames = run[0]
    st = _run_state(gpe)
    st.enable_uids()
    uids = np.array([0, 7, 100, 1499, 731], U32)
    st.tracers_begin(uids, every=1, frames=32, prev=True)
    st.monitor_begin(every=1, frames=32)
    st.run(DTS[0], 2, resort_every=0, resort_first=False)             # the first two steps share their dt
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 2 and recorded == 2
    for s in range(2):
        pos, prev, _ = frames[s]
        assert same_bits(tr.pos[s], pos[uids]) and same_bits(tr.prev[s], prev[uids]), s
        assert rec["max_x"][s] == pos[:, 0].max() and rec["min_x"][s] == pos[:, 0].min() and rec["n"][s] == 1500
    st.tracers_end(); st.monitor_end()
    _end(st)


def test_tracer_frames_over_a_longer_run(gpe, oracle):
    """25 steps of one dt, by then the floor and both movers have acted: every frame is the state behind the passes"""
    frames, pushed_movers, pushed_floor = S.run_reference(oracle, [DT] * 25)
    assert pushed_movers > 50 and pushed_floor > 500
    st = _run_state(gpe)
    st.enable_uids()
    uids = np.arange(0, 1500, 37, dtype=U32)
    st.tracers_begin(uids, every=1, frames=32, prev=True)
    st.monitor_begin(every=1, frames=32)
    st.run(DT, 25, resort_every=0, resort_first=False)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 25 and recorded == 25
    for s in range(25):
        pos, prev, _ = frames[s]
        assert same_bits(tr.pos[s], pos[uids]) and same_bits(tr.prev[s], prev[uids]), s
        assert rec["max_x"][s] == pos[:, 0].max() and rec["min_x"][s] == pos[:, 0].min()
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_surfaces_the_sets_and_the_next_step_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    pos, rad = CM.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD, gravity=M.RUN_GRAVITY)
    tw = S.Twin(oracle, pos, rad, world=M.RUN_WORLD, gravity=M.RUN_GRAVITY)
    for h in (st, tw):
        h.set_colliders(M.RUN_FLOOR)
        h.set_movers(M.run_movers())
        h.set_surfaces("colliders", S.RUN_COLLIDER_SURFACES)
        h.set_surfaces("movers", S.RUN_MOVER_SURFACES)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    sets = st.colliders(), st.movers(), st.mover_poses()
    infos = st.colliders_info(), st.movers_info()

    def untouched(what):
        assert same_rows(st.surfaces("colliders"), S.RUN_COLLIDER_SURFACES), what
        assert same_rows(st.surfaces("movers"), S.RUN_MOVER_SURFACES), what
        assert same_bits(st.colliders(), sets[0]) and same_rows(st.movers(), sets[1]) and same_rows(st.mover_poses(), sets[2]), what
        assert (st.colliders_info(), st.movers_info()) == infos, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    def rows(*rs):
        out = (L.GpeSurface * len(rs))()
        for o, (e, mu, flags, reserved) in zip(out, rs):
            o.restitution, o.friction, o.flags, o.reserved = e, mu, flags, reserved
        return out

    ok = (0.5, 0.5, 0, 0)
    h = st.ctx.h
    k = C.c_uint64()
    assert lib.gpe_set_surfaces(None, 0, rows(ok), 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_surfaces(None, 0, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    bad = {
        "NULL rows with k > 0": lambda: lib.gpe_set_surfaces(h, 0, None, 1),
        "unknown target": lambda: lib.gpe_set_surfaces(h, 2, rows(ok), 1),
        "unknown target, k = 0": lambda: lib.gpe_set_surfaces(h, 7, None, 0),
        "k above the colliders": lambda: lib.gpe_set_surfaces(h, 0, rows(ok, ok), 2),
        "k below the movers": lambda: lib.gpe_set_surfaces(h, 1, rows(ok), 1),
        "k above the movers": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, ok, ok), 3),
        "NaN restitution": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, (NAN, 0.5, 0, 0)), 2),
        "negative restitution": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, (-0.125, 0.5, 0, 0)), 2),
        "restitution above 1": lambda: lib.gpe_set_surfaces(h, 1, rows((1.0000001, 0.5, 0, 0), ok), 2),
        "inf restitution": lambda: lib.gpe_set_surfaces(h, 0, rows((INF, 0.5, 0, 0)), 1),
        "NaN friction": lambda: lib.gpe_set_surfaces(h, 0, rows((0.5, NAN, 0, 0)), 1),
        "inf friction": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, (0.5, INF, 0, 0)), 2),
        "negative friction": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, (0.5, -1.0, 0, 0)), 2),
        "unknown flag": lambda: lib.gpe_set_surfaces(h, 0, rows((0.5, 0.5, 2, 0)), 1),
        "unknown flag beside PLAIN": lambda: lib.gpe_set_surfaces(h, 0, rows((0.5, 0.5, 0x80000001, 0)), 1),
        "reserved": lambda: lib.gpe_set_surfaces(h, 1, rows(ok, (0.5, 0.5, 0, 9)), 2),
        "get: unknown target": lambda: lib.gpe_get_surfaces(h, 2, None, 0, C.byref(k)),
        "get: NULL k": lambda: lib.gpe_get_surfaces(h, 0, None, 0, None),
        "get: NULL out": lambda: lib.gpe_get_surfaces(h, 1, None, 2, C.byref(k)),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        untouched(what)
    for _ in range(3):                                                 # the context goes on as the twin does
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 is accepted and reads back as +0; a partial read delivers the first rows; the ends of both ranges are taken
    assert lib.gpe_set_surfaces(h, 1, rows((-0.0, -0.0, 1, 0), (1.0, 3e38, 0, 0)), 2) == L.GPE_OK
    out = rows(ok, ok, ok)
    assert lib.gpe_get_surfaces(h, 1, out, 1, C.byref(k)) == L.GPE_OK and k.value == 2
    assert bits([out[0].restitution, out[0].friction]).tolist() == [0, 0] and out[0].flags == 1
    assert (out[1].restitution, out[2].restitution) == (0.5, 0.5)      # past the capacity: left as they were
    # a context without a set takes k = 0 only
    assert lib.gpe_set_surfaces(h, 1, None, 0) == L.GPE_OK and len(st.surfaces("movers")) == 0
    st.clear_movers()
    assert lib.gpe_set_surfaces(h, 1, rows(ok), 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_set_surfaces(h, 1, None, 0) == L.GPE_OK
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_surfaces(gpe, how):
    L = gpe._lib
    pos, rad = CM.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.RUN_WORLD)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    for target in ("colliders", "movers"):
        with pytest.raises(gpe.GpeError) as e:
            st.set_surfaces(target, S.rows((0.5, 0.5)))
        assert e.value.status == L.GPE_ERR_UNSUPPORTED
        st.clear_surfaces(target)                                      # k == 0 is no surface
        assert len(st.surfaces(target)) == 0
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    assert not SURFACE_TAGS & _live(st)
    _end(st)
