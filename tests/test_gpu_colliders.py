"""GPU (-m gpu): static colliders (gpe_set_colliders / _get_colliders / _apply_colliders / _get_colliders_info,
csrc/k_colliders.hip, csrc/gpe_colliders.hip).

The pass is a binary32 function of (p, r, colliders): every comparison is bit for bit against the numpy model
(tests/_colliders_model.py: brute force, no grid), and the steps against the CPU oracle with the model's pass behind
every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _colliders_model as M

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = M.FLOOR_DT
NAN, INF = float("nan"), float("inf")
WORLD = (200.0, 200.0)
FLOOR_STEPS = 60


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


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


def _floor_state(gpe, mode=None, flags=0, colliders=M.FLOOR_COLLIDERS, **kw):
    pos, rad = M.floor_scene()
    st = _state(gpe, pos, rad, world=M.FLOOR_WORLD, mode=mode, gravity=M.FLOOR_GRAVITY, flags=flags, **kw)
    if colliders is not None:
        st.set_colliders(colliders)
    return st


# ---- references, computed once --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor(oracle):
    """the CPU test's reference: oracle step + model pass, 60 steps, no re-sort"""
    return M.floor_reference(oracle, FLOOR_STEPS)


@pytest.fixture(scope="module")
def floor_resorted(oracle):
    return M.floor_reference(oracle, FLOOR_STEPS, resort_every=16, resort_first=True)


@pytest.fixture(scope="module")
def floor_plain(oracle):
    """the same scene without colliders: the oracle alone"""
    return M.floor_reference(oracle, 20, colliders=None)


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
def _scene_colliders(seed=3):
    """about 40: random capsules, discs and thin walls, the CPU test's special shapes, one reaching outside the world"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(5, 195, (30, 2))
    b = a + rng.uniform(-30, 30, (30, 2))
    R = np.where(rng.random(30) < 0.25, 0.0, rng.uniform(0.0, 3.0, 30))
    cs = np.concatenate([a, b, R[:, None]], axis=1)
    cs[::7, 2:4] = cs[::7, 0:2]                                        # discs
    special = [[-5, 150, 205, 150, 9.5],                               # a floor reaching past both walls
               [100, 100, 100, 100, 4], [50, 60, 150, 60, 2], [150, 40, 50, 40, 2], [20, 20, 20, 120, 1],
               [60, 80, 60, 80, 0], [100, 100, 100, 100, 4],           # a point; a duplicate of the disc (a tie on depth)
               [180, 10, 260, -40, 1.5],                               # from inside to far outside the world
               [1e30, 100, -1e30, 100, 1],                             # |b - a|^2 overflows: listed everywhere, touches nothing
               [-3e9, 170, 3e9, 171, 0.5]]                             # far: its rounding exceeds a cell
    return np.concatenate([cs, np.array(special)], axis=0).astype(F32)


def _scene_particles(n, cs, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    rad = np.full(n, 0.5, F32)
    m = min(n, 1500)
    if n > 1:
        # near the colliders' surfaces, on both sides of "touched"
        j = rng.integers(0, len(cs) - 2, m)
        u = rng.random(m)[:, None]
        on = cs[j, 0:2] + u * (cs[j, 2:4] - cs[j, 0:2])
        pos[:m] = (on + rng.uniform(-1.1, 1.1, (m, 2)) * (cs[j, 4] + 0.5)[:, None]).astype(F32)
    if n >= 2000:                                                      # (the fixed rows below need 1955; a smaller n is all near surfaces)
        # exactly on axes (u = 0.25, 0.5, 0.75 and the end points), on discs' centres, on cell borders (cells of 2.0)
        k = 0
        for c in cs[30:37]:
            for u in (0.0, 0.25, 0.5, 0.75, 1.0):
                pos[m + k] = c[0:2] + F32(u) * (c[2:4] - c[0:2])
                k += 1
        grid = (rng.integers(0, 100, (200, 2)) * 2).astype(F32)
        pos[m + k:m + k + 200] = grid
        pos[m + k + 200:m + k + 300, 0] = grid[:100, 0]                # on a vertical border only
        pos[m + k + 300:m + k + 400] = np.nextafter(grid[:100], F32(0)) # one ulp below a corner
        pos[m + k + 400] = (NAN, 100.0)
        pos[m + k + 401] = (100.5, NAN)
        pos[m + k + 402] = (INF, 100.0)
        pos[m + k + 403] = (-INF, -INF)
        pos[m + k + 404] = (1e30, 100.0)
        pos[m + k + 405] = (250.0, 100.0)                              # outside the world and the grid, untouched
        pos[m + k + 406] = (201.0, 150.0)                              # outside the world, inside the floor's reach
        pos[m + k + 407] = (-0.0, 150.0)
        rad[m + k + 410:m + k + 420] = -0.5                            # negative radii
        pos[m + k + 410:m + k + 420] = pos[:10] + F32(0.25)
    if n == 1:
        pos[0] = (100.0, 103.0)                                        # inside the disc
    return pos, rad


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("n", [4000, 3999, 1, 2, 3, 511, 512, 513])
def test_one_pass_equals_the_model(gpe, n, mode):
    """apply_colliders() alone on ~40 colliders: pos bit for bit as the model, prev and radius untouched, pushed the
    model's count.  Even n, odd n (the single-particle tail) and the tail alone; the edges of the pair loop (one pair
    without and with the tail, one workgroup of pairs less one, exactly one, one and the tail); then a radius above the grid's bound
    (a particle of radius -3 added afterwards: max_radius keeps 0.5), which takes the walk over every collider."""
    cs = _scene_colliders()
    assert len(cs) == 40
    pos, rad = _scene_particles(n, cs, seed=n)
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=gpe.MODE_COMPAT if mode == "compat" else None)
    st.set_colliders(cs)
    assert same_bits(st.colliders(), cs)
    want, moved = M.apply(pos, rad, cs, WORLD)
    st.apply_colliders()
    got, got_prev, got_rad = _arrays(st)
    info = st.colliders_info()
    print("n %d: moved %d, grid %d x %d, %d list entries" % (n, moved.sum(), info["grid_x"], info["grid_y"], info["list_entries"]))
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert same_bits(got_prev, prev) and same_bits(got_rad, rad)
    assert info["k"] == 40 and info["passes"] == 1 and info["pushed"] == int(moved.sum())
    assert info["grid_x"] == 101 and info["grid_y"] == 101             # cells of max(4 * 0.5, 200 / 1024) = 2
    assert 0 < info["list_entries"] < 101 * 101 * 40 // 4
    if n >= 2000:
        assert 300 < moved.sum() < n - 300                             # the scene exercises both outcomes
        assert not same_bits(got, pos)
    elif n >= 511:
        assert 0 < moved.sum() < n                                 # both outcomes among the few
    elif n > 1:
        assert moved.any()                                         # (not the empty-cell path alone)
    # a second pass starts from the first one's result
    want2, moved2 = M.apply(want, rad, cs, WORLD)
    st.apply_colliders()
    assert same_bits(st.positions(), want2)
    assert st.colliders_info()["pushed"] == int(moved.sum() + moved2.sum())
    # |r| = 3 > rb = 0.5: add_particles keeps fmaxf(0.5, -3) = 0.5, so the grid is not rebuilt for it
    extra = np.array([[100.0, 106.0], [60.0, 62.75], [30.0, 30.0]], F32)  # the disc (R 4) from 6 away, the point, nothing
    st.add_particles(extra, np.full(3, -3.0, F32))
    assert abs(st.particles.get_max_radius()) == 0.5
    all_pos, all_rad = np.concatenate([want2, extra]), np.concatenate([rad, np.full(3, -3.0, F32)])
    want3, moved3 = M.apply(all_pos, all_rad, cs, WORLD)
    assert moved3[-3] and moved3[-2]                                   # only reachable with |r| = 3
    st.apply_colliders()
    assert same_bits(st.positions(), want3)
    assert st.colliders_info()["grid_x"] == 101
    tags = _end(st)
    assert {"grid.collider_rec", "grid.collider_pushed", "grid.collider_cell_start", "grid.collider_items"} <= tags


def test_4096_discs(gpe):
    n = 4000
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    c = np.stack([gx.ravel(), gy.ravel()], axis=1) * 3.125 + 1.5
    cs = np.concatenate([c, c, np.full((4096, 1), 0.75)], axis=1).astype(F32)
    rng = np.random.default_rng(40)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    pos[:64] = cs[rng.integers(0, 4096, 64), 0:2]                      # on discs' centres: the (1, 0) normal
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad)
    st.set_colliders(cs)
    want, moved = M.apply(pos, rad, cs, WORLD)
    st.apply_colliders()
    assert same_bits(st.positions(), want)
    info = st.colliders_info()
    assert info["k"] == 4096 and info["pushed"] == int(moved.sum()) and 1000 < moved.sum() < n
    assert info["list_entries"] < 4096 * 64
    with pytest.raises(gpe.GpeError) as e:                             # 4097 is one too many; the set stays
        st.set_colliders(np.concatenate([cs, cs[:1]]))
    assert e.value.status == gpe._lib.GPE_ERR_INVALID_ARG and len(st.colliders()) == 4096
    _end(st)


def test_the_grid_strides_a_second_trip(gpe):
    """2048 workgroups x 256 lanes x 2 particles: from 1 048 577 particles on a lane takes a second pair"""
    n = 2048 * 256 * 2 + 3
    cs = np.array([[0, 100, 200, 100, 2], [100, 0, 100, 200, 0], [50, 50, 50, 50, 10], [150, 150, 170, 130, 1]], F32)
    rng = np.random.default_rng(9)
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, mode=gpe.MODE_COMPAT)
    st.set_colliders(cs)
    want, moved = M.apply(pos, rad, cs, WORLD)
    st.apply_colliders()
    assert same_bits(st.positions(), want)
    assert st.colliders_info()["pushed"] == int(moved.sum())
    assert moved[:1000].any() and moved[-100000:].any()
    _end(st)


@pytest.mark.parametrize("world,rb_radius", [((200.0, INF), 0.5), ((200.0, 200.0), INF), ((200.0, 200.0), NAN),
                                             ((2.5, 2.5), 0.75), ((1e-3, 1e-3), 0.5)])
def test_worlds_and_radius_bounds_that_leave_one_cell(gpe, world, rb_radius):
    """A world or a largest radius that no grid can be cut for: one cell that lists everything, the same function.
    (COMPAT: such particles are outside any box the native step takes.)"""
    cs = _scene_colliders()[30:38]
    pos = np.array([[100.0, 103.0], [60.0, 60.5], [1.0, 1.0], [NAN, 1.0], [150.0, 39.0], [2.0, 2.0]], F32)
    rad = np.array([0.5, 0.5, 0.5, 0.5, 0.5, rb_radius], F32)
    st = _state(gpe, pos, rad, world=world, mode=gpe.MODE_COMPAT)
    st.set_colliders(cs)
    want, moved = M.apply(pos, rad, cs, world)
    st.apply_colliders()
    assert same_bits(st.positions(), want)
    info = st.colliders_info()
    assert (info["grid_x"], info["grid_y"], info["list_entries"]) == (1, 1, 8) and info["pushed"] == int(moved.sum())
    _end(st)


# ---- 2. the hook ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_oracle_plus_the_model(gpe, floor, mode):
    frames, pushes = floor
    L = gpe._lib
    st = _floor_state(gpe, mode=L.MODE_COMPAT if mode == "compat" else None)
    for s in range(FLOOR_STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    assert not (pos[:, 1] >= 50).any() and pos[:, 1].max() > 39        # the floor is reached and never crossed
    info, pipe = st.colliders_info(), st.ctx.pipeline_info()
    assert info["passes"] == FLOOR_STEPS and info["pushed"] == pushes and info["k"] == 3
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == FLOOR_STEPS
        print("native sorts in %d steps: %d" % (FLOOR_STEPS, pipe["native_sorts"]))
    else:
        assert pipe["compat_steps"] == FLOOR_STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_and_sort_every_step_end_on_the_same_bits(gpe, floor, floor_resorted, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else None
    frames, pushes = floor
    for flags in (0, L.FLAG_SORT_EVERY_STEP):
        st = _floor_state(gpe, mode=m, flags=flags)
        st.run(DT, FLOOR_STEPS, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1]), flags
        info, pipe = st.colliders_info(), st.ctx.pipeline_info()
        assert info["passes"] == FLOOR_STEPS and info["pushed"] == pushes
        if mode == "native":
            assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == FLOOR_STEPS
            print("flags %d: native sorts in %d steps: %d" % (flags, FLOOR_STEPS, pipe["native_sorts"]))
        _end(st)
    # resort_every = 16: the reference re-sorts at the same steps
    frames, pushes = floor_resorted
    st = _floor_state(gpe, mode=m)
    st.run(DT, FLOOR_STEPS, resort_every=16, resort_first=True)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
    assert st.colliders_info()["pushed"] == pushes
    _end(st)


def test_the_kept_block_table_survives_positions_moved_behind_its_back(gpe, oracle):
    """The floor scene's world is small enough for its block keys to sort in one radix pass, which never keeps its
    table.  Here 220 x 220 (625 blocks: two passes): most native steps reuse the kept table, the rosters and the
    straggler lists, with the pass moving particles between them.  Every step as the twin, by gpe_step and by gpe_run."""
    L = gpe._lib
    world, gravity, n, steps = (220.0, 220.0), (0.0, 40.0), 4000, 40
    rng = np.random.default_rng(8)
    pos = np.stack([rng.uniform(1, 219, n), rng.uniform(1, 150, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    pegs = [[20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 3.0]
            for i in range(11) for j in range(4)]
    cs = np.array([[-5, 185, 225, 185, 10], [30, 40, 110, 70, 1], [200, 30, 120, 75, 0]] + pegs, F32)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.set_colliders(cs)
    st = _state(gpe, pos, rad, world=world, gravity=gravity)
    st.set_colliders(cs)
    runner = _state(gpe, pos, rad, world=world, gravity=gravity)
    runner.set_colliders(cs)
    for s in range(steps):
        st.update(DT, resort=(s == 0)); tw.step(DT, resort=(s == 0))
        _same_as_twin(st, tw, s)
    runner.run(DT, steps, resort_every=0, resort_first=True)
    _same_as_twin(runner, tw, "gpe_run")
    assert tw.pushed > 2000
    for ctx in (st, runner):
        info, pipe = ctx.colliders_info(), ctx.ctx.pipeline_info()
        print("native sorts in %d steps: %d, pushed %d" % (steps, pipe["native_sorts"], info["pushed"]))
        assert (info["passes"], info["pushed"]) == (steps, tw.pushed)
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == steps and pipe["sort_passes"] >= 2
        assert pipe["native_sorts"] < steps, "every step sorted: the kept table was never used"
        _end(ctx)
    tw.close()


# ---- 3. no colliders, no trace --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_colliders_nothing_changes_and_nothing_is_launched(gpe, floor, floor_plain, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else None
    plain, _ = floor_plain
    never = _floor_state(gpe, mode=m, colliders=None, profiling=True)
    cleared = _floor_state(gpe, mode=m, profiling=True)
    cleared.clear_colliders()
    assert len(cleared.colliders()) == 0 and cleared.colliders_info() == dict(k=0, passes=0, pushed=0, grid_x=0, grid_y=0,
                                                                               list_entries=0)
    for st in (never, cleared):
        st.apply_colliders()                                           # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, plain[19][0]) and same_bits(prev, plain[19][1])
        assert "Colliders" not in st.ctx.timings()
        assert not any(t.startswith("grid.collider_") for t, _, _, state in st.ctx.guard_registry() if state == "live")
        _end(st)
    armed = _floor_state(gpe, mode=m, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), floor[0][19][0])
    assert armed.ctx.timings()["Colliders"][1] == 20
    _end(armed)


# ---- 4. lifecycle ---------------------------------------------------------------------------------------------------
def _same_as_twin(st, tw, what):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    assert same_bits(got[0], pos) and same_bits(got[1], prev) and same_bits(got[2], rad), what
    assert same_bits(st.colliders(), tw.colliders), what


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_survives_everything_but_set_colliders(gpe, oracle, mode):
    L = gpe._lib
    world = (100.0, 100.0)
    cs = np.array([[-5, 80, 105, 80, 5], [50, 40, 50, 40, 6], [20, 20, 45, 30, 1], [150, 150, 150, 150, 8]], F32)
    rng = np.random.default_rng(12)
    n = 3999
    pos = rng.uniform(1, 99, (n, 2)).astype(F32)
    pos[:, 1] = pos[:, 1] * F32(0.7)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=(0.0, 60.0), mode=L.MODE_COMPAT if mode == "compat" else None)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=(0.0, 60.0))
    st.set_colliders(cs); tw.set_colliders(cs)

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what)
        info = st.colliders_info()
        assert (info["passes"], info["pushed"]) == (tw.passes, tw.pushed), what
        return info

    steps("start")
    # gpe_set_particles on the live context
    pos2 = rng.uniform(1, 99, (n - 500, 2)).astype(F32)
    _set(st, pos2, pos2, rad[:n - 500]); tw.set_particles(pos2, pos2, rad[:n - 500])
    steps("set_particles")
    add = rng.uniform(5, 95, (300, 2)).astype(F32)
    st.add_particles(add, np.full(300, 0.5, F32)); tw.add(add, np.full(300, 0.5, F32))
    steps("add")
    assert st.remove_particles_in_circle((50, 40), 12.0) == tw.remove_circle(50, 40, 12.0) > 0
    steps("remove")
    who = np.arange(0, 400, 2, dtype=U32)
    where = rng.uniform(40, 60, (200, 2)).astype(F32)                  # into the disc
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    grow = rng.uniform(5, 95, (6000, 2)).astype(F32)                   # past the capacity
    grow[:, 1] *= F32(0.5)
    st.add_particles(grow, np.full(6000, 0.5, F32)); tw.add(grow, np.full(6000, 0.5, F32))
    steps("growth")
    st.enable_uids(); tw.enable_uids()
    steps("uids on")
    st.enable_uids(False); tw.enable_uids(False)
    # a larger radius: the grid is rebuilt for the new bound
    before = steps("uids off")
    st.edit_particles(indices=[7], radii=[1.5]); tw.edit([7], "index", radius=[1.5])
    after = steps("radius edit")
    assert (before["grid_x"], after["grid_x"]) == (51, 17)             # cells of 2 -> cells of 6
    # gpe_set_world: the grid follows, the collider at (150, 150) in the newly uncovered part acts
    st.ctx.call("gpe_set_world", 200.0, 200.0); tw.set_world(200.0, 200.0)
    who = np.array([3, 4], U32)
    where = np.array([[153.0, 150.0], [150.0, 144.0]], F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    pushed = tw.pushed
    st.apply_colliders(); tw.apply_colliders()
    _same_as_twin(st, tw, "set_world")
    assert tw.pushed >= pushed + 2 and st.colliders_info()["pushed"] == tw.pushed
    assert st.colliders_info()["grid_x"] == 34
    assert tuple(st.positions()[3]) == (158.5, 150.0)                  # from 3 away to R + r = 8.5 away
    steps("after set_world")
    # a new set replaces the old one and zeroes the counters
    st.set_colliders(cs[:2]); tw.set_colliders(cs[:2])
    assert st.colliders_info()["passes"] == 0 and st.colliders_info()["pushed"] == 0
    steps("new set")
    tw.close()
    _end(st)


# ---- 5. observers ---------------------------------------------------------------------------------------------------
def test_tracer_and_monitor_frames_show_the_projected_positions(gpe, floor):
    frames, _ = floor
    st = _floor_state(gpe)
    st.enable_uids()
    uids = np.array([0, 7, 100, 1499, 731], U32)
    st.tracers_begin(uids, every=1, frames=32, prev=True)
    st.monitor_begin(every=1, frames=32)
    st.run(DT, 25, resort_every=0, resort_first=False)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 25 and recorded == 25
    touched_somewhere = False
    for s in range(25):
        pos, prev = frames[s]
        assert same_bits(tr.pos[s], pos[uids]) and same_bits(tr.prev[s], prev[uids]), s
        assert rec["max_y"][s] == pos[:, 1].max() and rec["min_y"][s] == pos[:, 1].min() and rec["n"][s] == 1500
        assert rec["sum_y"][s] == pytest.approx(float(pos[:, 1].astype(np.float64).sum()), rel=1e-12)
        touched_somewhere |= bool((pos[:, 1] > 39.9).any())
    assert touched_somewhere                                           # frames were taken behind the pass, on the floor
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 6. save / load -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_continue_on_the_same_bits(gpe, floor, tmp_path, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else None
    frames, _ = floor
    st = _floor_state(gpe, mode=m)
    st.run(DT, 30, resort_every=0, resort_first=False)
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert same_bits(d["colliders"], M.FLOOR_COLLIDERS)
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    assert same_bits(back.colliders(), st.colliders()) and same_bits(back.colliders(), M.FLOOR_COLLIDERS)
    for s in (st, back):
        s.run(DT, 30, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(s)
        assert same_bits(pos, frames[59][0]) and same_bits(prev, frames[59][1])
    assert back.colliders_info()["passes"] == 30 and st.colliders_info()["passes"] == 60
    _end(back)
    # a context without colliders writes none and loads none
    st.clear_colliders()
    st.save(path)
    with np.load(path) as d:
        assert "colliders" not in d.files
    back = gpe.State.load(path, mode=L.MODE_NATIVE if m is None else m, flags=L.FLAG_GUARD_ALLOCS)
    assert len(back.colliders()) == 0
    _end(back)
    _end(st)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    pos, rad = M.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.FLOOR_WORLD, gravity=M.FLOOR_GRAVITY)
    tw = M.Twin(oracle, pos, rad, world=M.FLOOR_WORLD, gravity=M.FLOOR_GRAVITY)
    st.set_colliders(M.FLOOR_COLLIDERS); tw.set_colliders(M.FLOOR_COLLIDERS)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.colliders_info()

    def untouched(what):
        assert same_bits(st.colliders(), M.FLOOR_COLLIDERS), what
        assert st.colliders_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    def rows(*cs):
        out = (L.GpeCollider * len(cs))()
        for o, c in zip(out, cs):
            o.ax, o.ay, o.bx, o.by, o.radius, o.flags = c
        return out

    ok = (1.0, 2.0, 3.0, 4.0, 0.5, 0)
    h = st.ctx.h
    # a NULL ctx, everywhere
    k = C.c_uint64()
    cinfo = L.GpeCollidersInfo(struct_size=C.sizeof(L.GpeCollidersInfo))
    assert lib.gpe_set_colliders(None, rows(ok), 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_colliders(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_colliders(None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_colliders_info(None, C.byref(cinfo)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    bad = {
        "NULL colliders with k > 0": lambda: lib.gpe_set_colliders(h, None, 2),
        "k > GPE_COLLIDERS_MAX": lambda: lib.gpe_set_colliders(h, rows(*([ok] * (L.COLLIDERS_MAX + 1))), L.COLLIDERS_MAX + 1),
        "NaN ax": lambda: lib.gpe_set_colliders(h, rows(ok, (NAN, 2, 3, 4, 0.5, 0)), 2),
        "inf ay": lambda: lib.gpe_set_colliders(h, rows(ok, (1, INF, 3, 4, 0.5, 0)), 2),
        "-inf bx": lambda: lib.gpe_set_colliders(h, rows(ok, (1, 2, -INF, 4, 0.5, 0)), 2),
        "NaN by": lambda: lib.gpe_set_colliders(h, rows((1, 2, 3, NAN, 0.5, 0), ok), 2),
        "NaN radius": lambda: lib.gpe_set_colliders(h, rows(ok, (1, 2, 3, 4, NAN, 0)), 2),
        "inf radius": lambda: lib.gpe_set_colliders(h, rows(ok, (1, 2, 3, 4, INF, 0)), 2),
        "negative radius": lambda: lib.gpe_set_colliders(h, rows(ok, (1, 2, 3, 4, -0.25, 0)), 2),
        "flags": lambda: lib.gpe_set_colliders(h, rows(ok, (1, 2, 3, 4, 0.5, 1)), 2),
        "info struct_size": lambda: lib.gpe_get_colliders_info(h, C.byref(L.GpeCollidersInfo(struct_size=C.sizeof(L.GpeCollidersInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_colliders_info(h, None),
        "get NULL k": lambda: lib.gpe_get_colliders(h, None, 0, None),
        "get NULL out": lambda: lib.gpe_get_colliders(h, None, 3, C.byref(k)),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        untouched(what)
    assert L.COLLIDERS_MAX == 4096
    # the other way round: sharding a context that holds colliders
    keys = np.arange(600, dtype=U32)
    sharding = {
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, 600, 500),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), 600, 0),
    }
    for what, call in sharding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"colliders" in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK                    # switching them off is no sharding
    # -0.0 is accepted as 0; a partial read delivers the first rows
    assert lib.gpe_set_colliders(h, rows((1, 2, 3, 4, -0.0, 0), ok), 2) == L.GPE_OK
    out = rows(ok, ok, ok)
    assert lib.gpe_get_colliders(h, out, 1, C.byref(k)) == L.GPE_OK and k.value == 2
    assert bits([out[0].radius]).tolist() == [0] and out[0].by == 4.0
    assert (out[1].radius, out[2].radius) == (0.5, 0.5)               # past the capacity: left as they were
    # the context goes on as the twin does
    st.set_colliders(M.FLOOR_COLLIDERS)
    tw.passes = tw.pushed = 0
    for _ in range(5):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_colliders(gpe, how):
    L = gpe._lib
    pos, rad = M.floor_scene(600)
    st = _state(gpe, pos, rad, world=M.FLOOR_WORLD)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_colliders(M.FLOOR_COLLIDERS)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.colliders()) == 0 and st.colliders_info()["k"] == 0
    st.apply_colliders()
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)


def test_colliders_before_there_are_particles(gpe):
    L = gpe._lib
    ctx = gpe.Context(world=M.FLOOR_WORLD, gravity=M.FLOOR_GRAVITY, flags=L.FLAG_GUARD_ALLOCS)
    ps = gpe.ParticleSystem(ctx)
    ps.set_colliders(M.FLOOR_COLLIDERS)
    ps.apply_colliders()                                               # no particles: GPE_OK, nothing done
    assert ps.colliders_info() == dict(k=3, passes=0, pushed=0, grid_x=0, grid_y=0, list_entries=0)
    pos, rad = M.floor_scene(100)
    pos[:, 1] += F32(3.0)                                              # some start inside the floor's reach
    f = C.POINTER(C.c_float)
    ctx.call("gpe_set_particles", pos.ctypes.data_as(f), None, rad.ctypes.data_as(f), 100)
    ps.apply_colliders()
    want, moved = M.apply(pos, rad, M.FLOOR_COLLIDERS, M.FLOOR_WORLD)
    assert same_bits(ctx.download(L.POS, F32, (-1, 2)), want) and moved.any()
    assert ps.colliders_info()["pushed"] == int(moved.sum())
    ctx.guard_check()
    assert ctx.guard_damaged == 0
    ctx.close()


# ---- 8. a seeded random interleaving --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_random_interleaving_against_the_twin(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else L.MODE_NATIVE
    rng = np.random.default_rng(2024 if mode == "native" else 2025)
    world, gravity = M.FLOOR_WORLD, (0.0, 80.0)
    pos, rad = M.floor_scene(600)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, mode=m)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)

    def random_set():
        k = int(rng.integers(1, 9))
        a = rng.uniform(0, 60, (k, 2))
        b = a + rng.uniform(-25, 25, (k, 2)) * (rng.random((k, 1)) < 0.7)
        cs = np.concatenate([a, b, rng.uniform(0, 3, (k, 1))], axis=1)
        cs[0] = (-5, 52, 65, 52, 8)                                    # always a floor
        return cs.astype(F32)

    ops = ["set", "clear", "step", "run", "add", "remove", "edit", "resort", "saveload", "apply"]
    weights = np.array([3, 1, 5, 4, 2, 2, 2, 2, 2, 1], float)
    log, most_pushed = [], 0
    cs = random_set()
    st.set_colliders(cs); tw.set_colliders(cs)
    for i in range(30):
        op = str(rng.choice(ops, p=weights / weights.sum()))
        log.append(op)
        if op == "set":
            cs = random_set()
            st.set_colliders(cs); tw.set_colliders(cs)
        elif op == "clear":
            st.clear_colliders(); tw.set_colliders(np.zeros((0, 5), F32))
        elif op == "step":
            for _ in range(int(rng.integers(1, 4))):
                st.update(DT); tw.step(DT)
        elif op == "run":
            k, every, first = int(rng.integers(2, 9)), int(rng.integers(0, 4)), bool(rng.integers(0, 2))
            st.run(DT, k, resort_every=every, resort_first=first); tw.run(DT, k, resort_every=every, resort_first=first)
        elif op == "add":
            k = int(rng.integers(1, 40))
            p = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 30, k)], axis=1).astype(F32)
            st.add_particles(p, np.full(k, 0.5, F32)); tw.add(p, np.full(k, 0.5, F32))
        elif op == "remove":
            c, r = rng.uniform(10, 50, 2), float(rng.uniform(1, 5))
            if 0 < int(_circle_count(tw, c, r)) < len(tw):
                assert st.remove_particles_in_circle(c, r) == tw.remove_circle(c[0], c[1], r)
        elif op == "edit":
            k = int(rng.integers(1, 30))
            who = rng.choice(len(tw), k, replace=False).astype(U32)
            where = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 45, k)], axis=1).astype(F32)
            st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
        elif op == "resort":
            st.particles.sort_by_cell_id(); tw.morton_resort()
        elif op == "saveload":
            path = str(tmp_path / ("s%d.npz" % i))
            st.save(path)
            _end(st)
            st = gpe.State.load(path, mode=m, flags=L.FLAG_GUARD_ALLOCS)
            tw.passes = tw.pushed = 0                                  # (load sets the colliders anew)
        else:
            st.apply_colliders(); tw.apply_colliders()
        _same_as_twin(st, tw, (i, log))
        info = st.colliders_info()
        assert (info["k"], info["passes"], info["pushed"]) == (len(tw.colliders), tw.passes, tw.pushed), (i, log)
        most_pushed = max(most_pushed, tw.pushed)
    print(" ".join(log), "| most pushes under one set:", most_pushed)
    assert {"set", "step", "run"} <= set(log) and most_pushed > 100
    tw.close()
    _end(st)


def _circle_count(tw, c, r):
    """how many particles of the twin the circle would remove"""
    from tests._oracle_model import circle_mask
    return circle_mask(tw.arrays()[0], c[0], c[1], r).sum()
