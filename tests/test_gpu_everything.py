"""GPU (-m gpu): every pass behind a step armed at once -- bends -> areas -> bonds (the coloured solver) -> bodies ->
movers (surfaces, swept) -> static colliders (surfaces, swept) -> fields -> observers, the order of gpe_step / gpe_run
-- against the one composed twin of tests/_everything_model.py, which is made of nothing but the model functions each
feature's own tests pin against the device (tests/test_everything_cpu.py ties it to the five existing twins).

The bonds' solver is the twelfth arm: `no_bond_solver` is the eleven arms under Jacobi, `all` runs the coloured pass in
its one-workgroup form (the scene's bonds name fewer particles than lds_nodes_max), `all_wide` over
tests/_everything_model.wide_scene in its per-colour form.  The model does not know the form: both must give its bits
inside a full step.

Every comparison is bit for bit on uint32 views, a NaN for a NaN.  Every context runs under GPE_FLAG_GUARD_ALLOCS and
ends with no damaged red zone.  A mismatch that goes away when one arm is left out (test_every_step_equals_the_twin's
leave-one-out cases) points at the library's hook -- the order of the passes, a stale grid, a stale pointer after a
growth, the order of restoration in State.load -- not at a model."""
import numpy as np
import pytest

from tests import _areas_model as AM
from tests import _bends_model as NM
from tests import _bond_solver_model as BS
from tests import _bonds_model as BM
from tests import _colliders_model as CM
from tests import _everything_model as E
from tests import _fields_model as FM

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = E.DT
STEPS = E.STEPS
CASES = ["all"] + ["no_" + a for a in E.ARMS] + ["none", "all_wide"]
# pendulum, bricks (the brittle one), the blob's loop, loose, a ring in each sense, shots
TRACKED = np.array([0, 4, 9, 30, 33, 60, 100, 500, E.RING_FIRST + 3, E.RING_FIRST + E.RING + 5, 1017, 1024], U32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    """the same bits; where the twin has a NaN the device has a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_rows(a, b):
    """two structured arrays of one layout, byte for byte"""
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and a.tobytes() == b.tobytes()


def _differ(got, want):
    if got.shape != want.shape:
        return "shapes %r %r" % (got.shape, want.shape)
    bad = np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
    return bad[:5], got[bad[:5]], want[bad[:5]]


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE


def _arms(case):
    return {"all": E.ARMS, "all_wide": E.ARMS, "none": ()}.get(case, tuple(a for a in E.ARMS if "no_" + a != case))


def _form(st, tw_info, what):
    """the launch form the last coloured pass took (the device's alone): 0 where none ran since the mode was set, else 2
    (one workgroup) while the set held names at most lds_nodes_max uids, 1 (a launch per colour) past that"""
    info = st.bond_solver_info()
    nodes = st.bonds_info()["nodes"]
    want = 0 if tw_info["passes"] == 0 else (2 if nodes <= info["lds_nodes_max"] else 1)
    assert info["form"] == want, (what, info, nodes)
    return info["form"]


def _state(gpe, mode, arms=E.ARMS, sc=None):
    sc = E.scene() if sc is None else sc
    st = gpe.State(sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev, mode=_mode(gpe, mode),
                   flags=gpe._lib.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    return E.arm(st, sc, arms)


def _end(st):
    """every context ends here: no red zone of a live or a released buffer is damaged"""
    zones = st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0, zones
    st.close()


def _ran_native(gpe, st, mode, steps):
    pipe = st.ctx.pipeline_info()
    if mode == "native":
        assert pipe["pipeline"] == gpe._lib.PIPELINE_NATIVE and pipe["native_steps"] == steps and pipe["compat_steps"] == 0, pipe
    else:
        assert pipe["compat_steps"] == steps and pipe["native_steps"] == 0, pipe


def _same_particles(st, tw, what):
    pos, prev, rad = tw.arrays()
    got = st.positions(), st.previous_positions(), st.radii()
    assert same_bits(got[0], pos), (what, "pos", _differ(got[0], pos))
    assert same_bits(got[1], prev), (what, "prev", _differ(got[1], prev))
    assert same_bits(got[2], rad) and np.array_equal(st.uids(), tw.uids), what


def _same_flags_and_poses(st, f, what):
    """f: a Frame of the twin -- the bodies' poses, the broken flags, the movers' poses and the loops' (area, lambda)
    rows as of the last relaxation (NaNs for a loop that was inert in it, and before the first pass)"""
    assert same_bits(st.body_poses(), f.body_poses), (what, "body poses")
    assert np.array_equal(st.bodies()[1], f.bodies_broken) and np.array_equal(st.bonds()[1], f.bonds_broken), (what, "broken flags")
    assert same_rows(st.mover_poses(), f.mover_poses), (what, "mover poses", st.mover_poses(), f.mover_poses)
    assert same_bits(st.area_values(), f.area_value), (what, "area values", st.area_values(), f.area_value)


def _same_as_twin(st, tw, what):
    """the particles, every stored set read back, the poses, the flags, the loops' values and the counters"""
    _same_particles(st, tw, what)
    assert same_bits(st.colliders(), tw.colliders) and same_rows(st.movers(), tw.m.movers), (what, "colliders / movers")
    for target in ("colliders", "movers"):
        assert same_rows(st.surfaces(target), tw.surfaces(target)), (what, target, "surfaces")
    assert same_rows(st.fields(), tw.fields) and st.collider_sweep() is tw.sweep, (what, "fields / sweep")
    assert st.mover_sweep() is tw.m.sweep, (what, "the movers' sweep")
    assert same_rows(st.bends(), tw.bends), (what, "bends")
    rec, uid = st.areas()                                              # (a pump that did not land shows in rest_area)
    assert same_rows(rec, tw.areas) and np.array_equal(uid, tw.area_member_uid), (what, "areas")
    rec, _ = st.bonds()
    assert same_rows(rec, tw.bonds), (what, "bonds")
    rec, _, uid, rest = st.bodies()
    assert same_rows(rec, tw.bodies) and np.array_equal(uid, tw.member_uid) and same_bits(rest, tw.member_rest), (what, "bodies")
    _same_flags_and_poses(st, E.frame(tw), what)
    got, want = E.state_counters(st), tw.counters()
    assert got == want, (what, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    assert st.bond_solver() == ("coloured" if tw.bond_solver == BS.COLOURED else "jacobi"), (what, "the bonds' solver")
    _form(st, want["bond_solver"], what)


# ---- the references: the twin alone, once per configuration ---------------------------------------------------------
@pytest.fixture(scope="module")
def lds_nodes_max(gpe):
    """the most particles a set may name for the coloured pass's one-workgroup form, as the library reports it"""
    probe = gpe.State(np.full((1, 2), 5.0, F32), np.full(1, 0.5, F32), world=E.WORLD, mode=gpe.MODE_NATIVE,
                      flags=gpe._lib.FLAG_GUARD_ALLOCS)
    lds = probe.bond_solver_info()["lds_nodes_max"]
    _end(probe)
    return lds


@pytest.fixture(scope="module")
def reference(oracle, lds_nodes_max):
    """reference(case) -> (the scene, frames after each of the 40 steps, counters at the end) of the twin armed as the
    case says; `all_wide` over wide_scene(lds_nodes_max), every other case over scene()"""
    done = {}

    def get(case):
        if case not in done:
            arms = _arms(case)
            sc = E.wide_scene(lds_nodes_max) if case == "all_wide" else E.scene()
            tw = E.twin(oracle, arms, sc)
            # (no set, no surfaces; the movers' sweep and the bonds' solver are the context's modes: on with no movers
            # and no bonds held, off with thin movers and with bonds)
            assert tw.armed() == tuple(a for a in arms if a.split("_")[0] + "s" in arms or "_" not in a
                                       or a in ("mover_sweep", "bond_solver"))
            done[case] = (sc, E.frames(tw), tw.counters())
            tw.close()
        return done[case]
    return get


@pytest.fixture(scope="module")
def resorted(oracle):
    """all arms, the re-sorts of gpe_run(40, resort_every = 16, resort_first)"""
    tw = E.twin(oracle)
    out = E.frames(tw, resort_every=16, resort_first=True), tw.counters()
    tw.close()
    return out


# ---- 1, 2. every step equals the twin: all arms, each one left out, none ---------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("case", CASES)
def test_every_step_equals_the_twin(gpe, reference, lds_nodes_max, case, mode):
    """40 gpe_step calls over scene(): pos and prev after each, the poses, the broken flags and the loops' values after
    every tenth, every counter at the end.  `all` pins the order of the seven passes in the forms the twelve arms give
    them (the bonds' coloured, the movers' and the static colliders' with surfaces and swept) and of the observers behind
    them; the other cases are bit-identical to the twin configured the same way and bisect a failure of `all`.
    `no_movers` keeps the movers' sweep on with no movers held and `no_bonds` the coloured solver with no bonds held;
    under `no_mover_sweep` the thin movers run the plain pass, and `no_bond_solver` is the eleven arms under Jacobi.
    The coloured pass of `all` takes the one-workgroup form; `all_wide`, whose bonds name more than lds_nodes_max
    particles, the per-colour one from its first step on."""
    sc, frames, counters = reference(case)
    solver = counters["bond_solver"]
    if case in ("all", "all_wide"):
        assert counters["sweep"]["stopped"] > 0 and counters["bodies"]["broken"] > 0 and counters["movers"]["pushed"] > 0
        assert counters["mover_sweep"]["stopped"] > 0
        assert counters["bends"]["passes"] == counters["areas"]["passes"] == STEPS
        assert solver["mode"] == BS.COLOURED and solver["passes"] == STEPS and counters["bonds"]["broken"] > 0
    if case == "all_wide":
        assert counters["bonds"]["nodes"] > lds_nodes_max and solver["colours"] <= BS.COLOURS_MAX
        assert counters["bonds"]["broken"] > 1                         # (the tie, and ties along the fill)
    if case in ("no_bonds", "no_bond_solver", "none"):
        assert solver["passes"] == 0 and solver["mode"] == (BS.JACOBI if case != "no_bonds" else BS.COLOURED)
    st = _state(gpe, mode, _arms(case), sc)
    assert _form(st, dict(passes=0), (case, "before the first step")) == 0
    for s in range(STEPS):
        st.update(DT)
        f = frames[s]
        pos, prev = st.positions(), st.previous_positions()
        assert same_bits(pos, f.pos), (case, s, "pos", _differ(pos, f.pos))
        assert same_bits(prev, f.prev), (case, s, "prev", _differ(prev, f.prev))
        if s == 0 and case == "all_wide":
            assert st.bond_solver_info()["form"] == 1
        if s % 10 == 9:
            _same_flags_and_poses(st, f, (case, s))
    got = E.state_counters(st)
    assert got == counters, {k: (got[k], counters[k]) for k in got if got[k] != counters[k]}
    form = _form(st, solver, (case, "at the end"))
    assert form == {"all": 2, "all_wide": 1}.get(case, form) and (form == 0) == (solver["passes"] == 0)
    print("case %s (%s): form %d, %d colours, %d nodes" % (case, mode, form, solver["colours"], counters["bonds"]["nodes"]))
    _ran_native(gpe, st, mode, STEPS)
    _end(st)


# ---- 3. one run equals the loop, and the observers see the end of the chain -------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_loop_and_the_observers_see_the_end_of_the_chain(gpe, resorted, mode):
    frames, counters = resorted
    st = _state(gpe, mode)
    st.tracers_begin(TRACKED, every=1, frames=64, prev=True, index=True)
    st.monitor_begin(every=1, frames=64)
    st.run(DT, STEPS, resort_every=16, resort_first=True)
    last = frames[-1]
    pos, prev = st.positions(), st.previous_positions()
    assert same_bits(pos, last.pos), _differ(pos, last.pos)
    assert same_bits(prev, last.prev), _differ(prev, last.prev)
    assert np.array_equal(st.uids(), last.uids) and not np.array_equal(last.uids, np.arange(E.N))
    _same_flags_and_poses(st, last, "run")
    got = E.state_counters(st)
    assert got == counters, {k: (got[k], counters[k]) for k in got if got[k] != counters[k]}
    assert st.bonds_info()["resolves"] == st.bodies_info()["resolves"] == 3          # before steps 0, 16, 32
    assert st.bends_info()["resolves"] == st.areas_info()["resolves"] == 3
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == STEPS and recorded == STEPS
    for s, f in enumerate(frames):                                     # frames taken behind every pass, the swept ones too
        slot = BM.slots_of(f.uids, TRACKED)
        assert (slot >= 0).all() and np.array_equal(tr.index[s], slot), s
        assert same_bits(tr.pos[s], f.pos[slot]) and same_bits(tr.prev[s], f.prev[slot]), s
        assert rec["min_y"][s] == f.pos[:, 1].min() and rec["max_y"][s] == f.pos[:, 1].max() and rec["n"][s] == E.N, s
    st.tracers_end(); st.monitor_end()
    _ran_native(gpe, st, mode, STEPS)
    _end(st)


# ---- 4. one event, every structure ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_event_invalidates_every_structure(gpe, oracle, mode):
    """Fully armed and stepping: a radius edit to three times the largest and back, gpe_set_world to twice the size and
    back, an add past the capacity, the removal of a body member, of a bonded uid, of a loop's member and of a bend's
    hinge, a re-sort (all four uid-named sets look their slots up again), a spell in the other mode; three steps and a
    full comparison (the movers' sweep and the bonds' solver with their counters in it) behind each.  A grid of the
    movers that is cut anew must not drop the swept form: its pass counter goes on behind the radius edit and the new
    world.  The bonds' coloured pass, in its one-workgroup form, reads node_slot again and writes every present node
    back behind each event: its pass counter goes on as well, and the colours stay the set's."""
    from tests.test_gpu_fields import grid_dims
    L = gpe._lib
    st = _state(gpe, mode)
    tw = E.twin(oracle)
    rng = np.random.default_rng(5)
    total = [0]
    colours = BS.colour_info(tw.bonds)
    assert colours[0] >= 3

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        total[0] += k
        _same_as_twin(st, tw, what)
        assert tw.fully_armed(), what
        return st.colliders_info(), st.movers_info(), st.fields_info()

    def grids(infos):
        return [(i["grid_x"], i["grid_y"]) for i in infos]

    def still_swept(what):
        """the mode is on and every step so far ran the movers' pass in its swept form"""
        info = st.mover_sweep_info()
        assert st.mover_sweep() is True and info["mode"] == L.SWEEP_ON and info["passes"] == total[0], (what, info, total[0])
        info = st.bond_solver_info()
        assert st.bond_solver() == "coloured" and (info["passes"], info["form"]) == (total[0], 2), (what, info, total[0])
        assert (info["colours"], info["largest_colour"]) == colours, (what, info, colours)

    start = steps("start", 6)
    assert grids(start)[2] == grid_dims(E.WORLD)[1:]
    still_swept("start")
    # a new largest radius: the particle grid, the colliders' and the movers' grids are cut anew in one step
    who = np.array([700], U32)
    st.edit_particles(indices=who, radii=np.array([1.5], F32)); tw.edit(who, "index", radius=np.array([1.5], F32))
    up = steps("radius up")
    assert grids(up)[0] != grids(start)[0] and grids(up)[1] != grids(start)[1], (grids(start), grids(up))
    assert grids(up)[2] == grid_dims(E.WORLD)[1:]                       # (the fields' grid follows the world alone)
    still_swept("radius up")
    st.edit_particles(indices=who, radii=np.array([0.5], F32)); tw.edit(who, "index", radius=np.array([0.5], F32))
    down = steps("radius down")
    assert grids(down) == grids(start)
    # the world doubles: one particle put on the floor's end and one into the well, both in the newly covered part
    big = (2 * E.WORLD[0], 2 * E.WORLD[1])
    st.ctx.call("gpe_set_world", *big); tw.set_world(*big)
    who, where = np.array([300, 301], U32), np.array([[63.0, 39.75], [85.0, 45.0]], F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    half = np.full(1, 0.5, F32)
    assert (where[:, 0] > E.WORLD[0]).all() and CM.touch(where[:1], half, tw.colliders[0])[0][0] and FM.matches(where[1:], tw.fields[1])[0]
    wide = steps("world grown")
    assert grids(wide)[0] != grids(start)[0] and grids(wide)[1] != grids(start)[1], (grids(start), grids(wide))
    assert grids(wide)[2] == grid_dims(big)[1:]
    still_swept("world grown")
    home = np.array([[30.0, 20.0], [32.0, 20.0]], F32)
    st.edit_particles(indices=who, positions=home); tw.edit(who, "index", pos=home)
    st.ctx.call("gpe_set_world", *E.WORLD); tw.set_world(*E.WORLD)
    back = steps("world back")
    assert grids(back) == grids(start)
    # an add past the capacity: every particle buffer moves
    k = 1100
    grow = np.stack([rng.uniform(2, 58, k), rng.uniform(2, 28, k)], axis=1).astype(F32)
    st.add_particles(grow, np.full(k, 0.25, F32)); tw.add(grow, np.full(k, 0.25, F32))
    steps("growth")
    # a member of a live body, a bonded particle, a member of a ring's loop and the middle node of a bend leave
    ring = E.RING_FIRST                                                # (the first ring: loop 0, bends 0 .. 15)
    # of the first brick; the pair bond's end; the anchored one; the loop's member; the bend's hinge
    gone = np.array([10, 17, 1, ring + 3, ring + 4], U32)
    # (no bond is broken but the tie of the ring over the paddle, which names none of them)
    assert tw.broken.tolist() == [False] * (len(tw.bonds) - 1) + [True] and tw.bonds["uid_a"][-1] == E.FALLER not in gone
    assert not tw.bodies_broken[1] and not np.isnan(tw.area_value).any()
    assert tw.area_member_uid[3] == ring + 3 and tw.bends["uid_b"][4] == ring + 4
    assert st.remove_particles_by_uid(gone) == tw.remove_uids(gone) == 5
    steps("removal")
    assert not np.isnan(tw.poses[1]).any()                             # the brick goes on with seven members
    # the loop without its members is inert (tests/_areas_model.loop_phase: NaNs in its row), the other three act
    assert np.isnan(tw.area_value[0]).all() and not np.isnan(tw.area_value[1:]).any()
    names = ("bonds", "bodies", "bends", "areas")
    resolves = {name: getattr(st, name + "_info")()["resolves"] for name in names}
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("sort_by_cell_id")
    for name in names:
        assert getattr(st, name + "_info")()["resolves"] > resolves[name], name
    other = L.MODE_NATIVE if mode == "compat" else L.MODE_COMPAT
    st.ctx.call("gpe_set_mode", other)
    steps("the other mode")
    st.ctx.call("gpe_set_mode", _mode(gpe, mode))
    steps("the mode back")
    still_swept("the end")
    # (a native step that finds particles outside a world that shrank back is the compat pipeline's: no exact split)
    pipe = st.ctx.pipeline_info()
    print(pipe)
    assert pipe["native_steps"] + pipe["compat_steps"] == total[0], pipe
    assert pipe["compat_steps" if mode == "native" else "native_steps"] >= 3 and pipe["native_steps"] > 0, pipe
    tw.close()
    _end(st)


# ---- 5. save and load with everything ---------------------------------------------------------------------------------
PUMPED = 2                                                             # the loop the save / load test pumps before it saves


@pytest.fixture(scope="module")
def pumped(oracle):
    """all arms, 15 steps, loop PUMPED pumped to 1.25 times its rest area, 15 more steps without interruption ->
    (frames, the areas' rows from the pump on)"""
    tw = E.twin(oracle)
    frames = E.frames(tw, 15)
    tw.set_area_targets(PUMPED, F32(1.25) * tw.areas["rest_area"][PUMPED:PUMPED + 1])
    rows = tw.areas.copy()
    frames += E.frames(tw, 15)
    tw.close()
    return frames, rows


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_with_all_thirteen_groups(gpe, pumped, tmp_path, mode):
    """one loop pumped and the context saved after 15 steps, with the coloured solver on and the tie broken, loaded
    into a fresh context of each mode, 15 more steps: the bits of the uninterrupted twin.  The loaded contexts hold the
    mode, the colours of the loaded set and its broken flags whichever of the two was restored first."""
    L = gpe._lib
    frames, rows = pumped
    sc = E.scene()
    colours = BS.colour_info(sc.bonds)
    st = _state(gpe, mode, sc=sc)
    for s in range(15):
        st.update(DT)
    assert frames[14].bodies_broken.any() and not frames[14].bodies_broken.all()
    assert frames[14].bonds_broken.any() and not frames[14].bonds_broken.all() and colours[0] >= 3
    st.set_area_targets(PUMPED, F32(1.25) * sc.areas["rest_area"][PUMPED:PUMPED + 1])
    assert same_rows(st.areas()[0], rows) and not same_rows(rows, AM.stored(sc.areas))
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert set(E.GROUPS) <= set(d.files), sorted(d.files)
        assert np.array_equal(d["bodies_broken"], frames[14].bodies_broken) and d["collider_sweep"].tolist() == [1]
        assert same_rows(d["mover_poses"], frames[14].mover_poses) and d["mover_sweep"].tolist() == [1]
        assert d["bond_solver"].tolist() == [L.BOND_SOLVER_COLOURED]
        assert np.array_equal(d["bonds_broken"], frames[14].bonds_broken)
        assert same_rows(d["areas"], rows) and np.array_equal(d["area_member_uid"], sc.area_member_uid)
        assert same_rows(d["bends"], NM.stored(sc.bends))
        assert (d["bend_iterations"].tolist(), d["area_iterations"].tolist()) == ([sc.bend_iterations], [sc.area_iterations])
    backs = [gpe.State.load(path, mode=m, flags=L.FLAG_GUARD_ALLOCS) for m in (_mode(gpe, mode), _mode(gpe, "compat" if mode == "native" else "native"))]
    assert same_bits(st.area_values(), frames[14].area_value) and not np.isnan(st.area_values()).any()
    for h in backs:
        assert h.collider_sweep() is True and np.array_equal(h.bodies()[1], frames[14].bodies_broken)
        assert h.mover_sweep() is True and h.mover_sweep_info()["passes"] == 0     # (its counters start anew)
        info = h.bond_solver_info()
        assert h.bond_solver() == "coloured" and (info["colours"], info["largest_colour"]) == colours, info
        assert (info["mode"], info["passes"], info["form"]) == (L.BOND_SOLVER_COLOURED, 0, 0), info
        assert np.array_equal(h.bonds()[1], frames[14].bonds_broken)
        assert same_rows(h.mover_poses(), frames[14].mover_poses)
        for target in ("colliders", "movers"):
            assert same_rows(h.surfaces(target), st.surfaces(target)) and len(h.surfaces(target)) > 0
        got, member = h.areas()
        assert same_rows(got, rows) and np.array_equal(member, sc.area_member_uid) and same_rows(h.bends(), NM.stored(sc.bends))
        assert h.area_values().shape == (len(rows), 2) and np.isnan(h.area_values()).all()     # no pass yet
        assert h.bends_info()["passes"] == h.areas_info()["passes"] == 0
    for s in range(15, 30):
        for h in [st] + backs:
            h.update(DT)
            pos, prev = h.positions(), h.previous_positions()
            assert same_bits(pos, frames[s].pos), (s, h is st, "pos", _differ(pos, frames[s].pos))
            assert same_bits(prev, frames[s].prev), (s, h is st, "prev", _differ(prev, frames[s].prev))
    f = frames[29]
    for h in [st] + backs:
        _same_flags_and_poses(h, f, "after load")
        assert h.mover_sweep_info()["passes"] == (30 if h is st else 15)
        assert h.bends_info()["passes"] == h.areas_info()["passes"] == (30 if h is st else 15)
        info = h.bond_solver_info()
        assert (info["passes"], info["form"]) == (30 if h is st else 15, 2), info
        assert (info["colours"], info["largest_colour"]) == colours, info
        assert same_rows(h.areas()[0], rows)
    _ran_native(gpe, st, mode, 30)
    _ran_native(gpe, backs[0], mode, 15)
    _ran_native(gpe, backs[1], "compat" if mode == "native" else "native", 15)
    for h in [st] + backs:
        _end(h)


# ---- 6. the random interleaving ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("seed", E.SEEDS)
def test_a_random_interleaving_against_the_twin(gpe, oracle, seed, mode):
    """plan(seed) against a State and the twin: after every operation the particles, every stored set read back, the
    two sweeps' modes, the bonds' solver with its colours and launch form, the poses, the broken flags and the
    counters.  The solver is switched with a set and a broken bond held, set again while on, and offered a set of 65
    colours; every other block runs under the coloured mode."""
    seq = E.Sequence(E.plan(seed), oracle, gpe=gpe, mode_name=mode, compare=_same_as_twin, end=_end)
    try:
        seq.run()
    finally:
        print("\n".join(seq.log))
        print(dict(seq.cov))
        seq.close()
    seq.cov.check()
    # (no exact split: the spell in the other mode apart, a native step that finds particles outside a world that shrank
    # back is the compat pipeline's)
    print("native steps %d, compat steps %d, in the other mode %d" % (seq.native_steps, seq.compat_steps, seq.other_steps))
    assert seq.native_steps + seq.compat_steps == seq.steps and seq.native_steps > 0
    if mode == "compat":
        assert seq.native_steps <= seq.other_steps
