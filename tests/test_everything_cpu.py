"""CPU: the composed twin of tests/_everything_model.py (bends, areas, bonds under either solver, bodies, movers with
surfaces and their sweep, static colliders with surfaces and the sweep, fields, all behind one step) before any GPU time
is spent on it: it is no new oracle (bit for bit the four existing twins where only their features are set, and the
solver's twin with the coloured solver on), its scene acts and tells every arm apart, and its random plans reach what
tests/test_gpu_everything.py needs them to reach."""
import numpy as np
import pytest

from tests import _areas_model as AM
from tests import _bodies_model as BD
from tests import _bond_solver_model as BS
from tests import _bonds_model as BM
from tests import _everything_model as E
from tests import _mover_sweep_model as MS
from tests import _sweep_model as SW

F32 = np.float32
U32 = np.uint32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def full(oracle):
    """scene(), all arms, 40 steps -> (frames, counters, the step after which a body was first broken, field_changed)"""
    tw = E.twin(oracle)
    frames = E.frames(tw)
    out = frames, tw.counters(), next(s for s, f in enumerate(frames) if f.bodies_broken.any()), tw.field_changed
    tw.close()
    return out


def test_with_the_yards_features_alone_it_is_the_bodies_twin(oracle):
    """bonds, bodies and the yard's colliders: the frames of tests/_bodies_model.Twin over the yard's 60 steps"""
    from tests.test_gpu_bodies import STEPS, YARD_COLLIDERS, YARD_GRAVITY, YARD_WORLD, yard_scene
    pos, rad, bodies, member_uid, member_rest, bonds = yard_scene()
    twins = []
    for cls in (BD.Twin, E.Everything):
        tw = cls(oracle, pos, rad, world=YARD_WORLD, gravity=YARD_GRAVITY)
        tw.enable_uids()
        tw.set_bonds(bonds, 2); tw.set_bodies(bodies, member_uid, member_rest); tw.set_colliders(YARD_COLLIDERS)
        twins.append(tw)
    old, new = twins
    for s in range(STEPS):
        old.step(E.DT); new.step(E.DT)
        for a, b in zip(old.arrays(), new.arrays()):
            assert same_bits(a, b), s
        assert same_bits(old.poses, new.poses) and np.array_equal(old.bodies_broken, new.bodies_broken), s
    assert old.bodies_broken.any() and old.pushed == new.pushed > 0
    assert old.bonds_info() == new.bonds_info() and old.bodies_info() == new.bodies_info()
    assert new.armed() == ("bonds", "bodies", "colliders")
    old.close(); new.close()


def test_with_the_yards_features_and_the_coloured_solver_it_is_the_solvers_twin(oracle):
    """bonds under the coloured solver, bodies and the yard's colliders: the frames, the broken flags and the solver's
    info of tests/_bond_solver_model.Twin chained as the bodies' twin (its pass in the bonds' place of
    tests/_bodies_model.Twin.step) over the yard's 60 steps; the mode set before the set on one pair, behind it on the
    other"""
    from tests.test_gpu_bodies import STEPS, YARD_COLLIDERS, YARD_GRAVITY, YARD_WORLD, yard_scene

    class Chained(BD.Twin, BS.Twin):
        pass
    assert Chained.__mro__[1:4] == (BD.Twin, BS.Twin, BS.Mixin) and Chained.apply_bonds is BS.Mixin.apply_bonds
    pos, rad, bodies, member_uid, member_rest, bonds = yard_scene()
    bonds = bonds.copy()
    bonds["max_length"][-1] = F32(1.01) * bonds["rest_length"][-1]     # (a bond that breaks on the way)
    for first in (True, False):
        twins = []
        for cls in (Chained, E.Everything):
            tw = cls(oracle, pos, rad, world=YARD_WORLD, gravity=YARD_GRAVITY)
            tw.enable_uids()
            if first:
                tw.set_bond_solver("coloured")
            tw.set_bonds(bonds, 2); tw.set_bodies(bodies, member_uid, member_rest); tw.set_colliders(YARD_COLLIDERS)
            if not first:
                tw.set_bond_solver("coloured")
            twins.append(tw)
        old, new = twins
        for s in range(STEPS):
            old.step(E.DT); new.step(E.DT)
            for a, b in zip(old.arrays(), new.arrays()):
                assert same_bits(a, b), s
            assert same_bits(old.poses, new.poses) and np.array_equal(old.bodies_broken, new.bodies_broken), s
            assert np.array_equal(old.broken, new.broken), s
        assert old.bodies_broken.any() and old.pushed == new.pushed > 0 and new.coloured_changed > 0
        assert old.broken.any() and not old.broken.all()
        assert old.bonds_info() == new.bonds_info() and old.bodies_info() == new.bodies_info()
        assert old.bond_solver_info() == new.bond_solver_info() and new.bond_solver_info()["passes"] == STEPS
        print(new.bonds_info(), new.bond_solver_info())
        assert new.armed() == ("bonds", "bond_solver", "bodies", "colliders")
        old.close(); new.close()


def test_with_the_sweeps_features_alone_it_is_the_sweep_twin(oracle):
    """movers, colliders, both surfaces, the sweep and fields over scene(): the frames of tests/_sweep_model.Twin (which
    has no movers' sweep: the thin movers run the plain pass)"""
    sc = E.scene()
    arms = tuple(a for a in E.ARMS if a not in ("bends", "areas", "bonds", "bond_solver", "bodies", "mover_sweep"))
    twins = []
    for cls in (SW.Twin, E.Everything):
        tw = cls(oracle, sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev)
        tw.enable_uids()
        twins.append(E.arm(tw, sc, arms))
    old, new = twins
    for s in range(E.STEPS):
        resort = s % 16 == 0
        old.step(E.DT, resort=resort); new.step(E.DT, resort=resort)
        for a, b in zip(old.arrays(), new.arrays()):
            assert same_bits(a, b), s
        assert old.m.poses().tobytes() == new.m.poses().tobytes() and np.array_equal(old.uids, new.uids), s
    assert (old.pushed, old.m.pushed, old.swept, old.stopped) == (new.pushed, new.m.pushed, new.swept, new.stopped)
    assert old.swept > 0 and old.stopped > 0 and old.m.pushed > 0 and new.field_changed > 0 and new.armed() == arms
    old.close(); new.close()


def test_with_both_sweeps_and_no_bonds_or_bodies_it_is_the_mover_sweep_twin(oracle):
    """movers, both surfaces, colliders, both sweeps and fields over scene(): the frames, the mover poses and the swept
    pass's counters of tests/_mover_sweep_model.Twin"""
    sc = E.scene()
    arms = tuple(a for a in E.ARMS if a not in ("bends", "areas", "bonds", "bond_solver", "bodies"))
    twins = []
    for cls in (MS.Twin, E.Everything):
        tw = cls(oracle, sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev)
        tw.enable_uids()
        twins.append(E.arm(tw, sc, arms))
    old, new = twins
    for s in range(E.STEPS):
        resort = s % 16 == 0
        old.step(E.DT, resort=resort); new.step(E.DT, resort=resort)
        for a, b in zip(old.arrays(), new.arrays()):
            assert same_bits(a, b), s
        assert old.m.poses().tobytes() == new.m.poses().tobytes() and np.array_equal(old.uids, new.uids), s
        assert old.mover_sweep_info() == new.mover_sweep_info(), s
    assert (old.pushed, old.m.pushed, old.swept, old.stopped) == (new.pushed, new.m.pushed, new.swept, new.stopped)
    info = new.mover_sweep_info()
    assert info["mode"] == 1 and info["passes"] == E.STEPS and info["swept"] > 0 and info["stopped"] > 0
    assert old.swept > 0 and old.stopped > 0 and new.field_changed > 0 and new.armed() == arms
    old.close(); new.close()


def test_with_the_rings_features_alone_it_is_the_areas_twin(oracle):
    """areas, bends, bonds and the floor over test_gpu_areas' rings: the frames, the (area, lambda) rows and the
    counters of tests/_areas_model.Twin over that file's 50 steps"""
    from tests import test_gpu_areas as TA
    pos, rad, bonds, bends, rows, member = TA.ring_scene()
    twins = []
    for cls in (AM.Twin, E.Everything):
        tw = cls(oracle, pos, rad, world=TA.RING_WORLD, gravity=TA.RING_GRAVITY)
        tw.enable_uids()
        tw.set_areas(rows, member, TA.AREA_ITERATIONS); tw.set_bends(bends, TA.BEND_ITERATIONS)
        tw.set_bonds(bonds, TA.BOND_ITERATIONS); tw.set_colliders(TA.RING_COLLIDERS)
        twins.append(tw)
    old, new = twins
    for s in range(TA.STEPS):
        old.step(E.DT); new.step(E.DT)
        for a, b in zip(old.arrays(), new.arrays()):
            assert same_bits(a, b), s
        assert same_bits(old.area_value, new.area_value) and not np.isnan(new.area_value).any(), s
    assert old.pushed == new.pushed > 0 and new.bend_changed > 0 and new.area_changed > 0
    assert old.bends_info() == new.bends_info() and old.areas_info() == new.areas_info() and old.bonds_info() == new.bonds_info()
    assert new.bends_info()["passes"] == new.areas_info()["passes"] == TA.STEPS
    assert new.armed() == ("bends", "areas", "bonds", "colliders")
    old.close(); new.close()


def test_the_scene_acts(full):
    frames, counters, first_break, field_changed = full
    sc = E.scene()
    assert len(sc.rad) == E.N == 1025 and (sc.collider_surfaces["flags"] == 1).any()
    assert len(E.ARMS) == 12 and len(sc.movers) == 4 and (sc.movers["radius"] == 0).sum() == 2
    # four loops, either sense among the rings; a particle that is a bend node, a loop's member, a bond's end and a
    # member of a body at once, and its body live at the end
    loops = E.scene_loops(sc.bodies)
    assert len(sc.areas) == len(loops) == 4 and (sc.areas["rest_area"][:3] > 0).tolist() == [True, False, True]
    multi = set(sc.bends["uid_b"]) & set(sc.area_member_uid) & set(sc.bonds["uid_a"]) & set(sc.member_uid)
    first = int(sc.bodies["first"][E.BLOB])
    assert multi == set(sc.member_uid[first + 1:first + 1 + E.RING]) and multi == set(loops[3])
    assert not frames[-1].bodies_broken[E.BLOB] and not np.isnan(frames[-1].body_poses[E.BLOB]).any()
    assert counters["bends"]["passes"] == counters["areas"]["passes"] == E.STEPS
    assert all(np.isfinite(f.area_value).all() for f in frames) and frames[-1].area_value.shape == (4, 2)
    assert all(np.isfinite(f.pos).all() and np.isfinite(f.prev).all() for f in frames)
    print(counters, "first break after step", first_break)
    assert counters["colliders"]["pushed"] > 0 and counters["movers"]["pushed"] > 0
    assert counters["sweep"]["swept"] > 0 and counters["sweep"]["stopped"] > 0 and field_changed > 0
    assert counters["mover_sweep"]["swept"] > 0 and counters["mover_sweep"]["stopped"] > 0
    assert counters["bodies"]["broken"] >= 1 and first_break < 15       # (test_gpu_everything saves after 15 steps)
    assert counters["bodies"]["broken"] < counters["bodies"]["k"]      # (... and needs a body that is not broken)
    # a bond breaks under the coloured pass, before the save as well: the tie, and nothing else
    first_snap = next(s for s, f in enumerate(frames) if f.bonds_broken.any())
    assert counters["bond_solver"]["mode"] == BS.COLOURED and counters["bond_solver"]["passes"] == E.STEPS
    assert 0 < first_snap < 15 and frames[first_snap].bonds_broken[-1] and counters["bonds"]["broken"] >= 1
    assert counters["bond_solver"]["colours"] >= 3 and counters["bonds"]["nodes"] <= 1024
    assert counters["bonds"]["passes"] == counters["bodies"]["passes"] == counters["sweep"]["passes"] == E.STEPS
    assert counters["movers"]["passes"] == counters["fields"]["passes"] == counters["mover_sweep"]["passes"] == E.STEPS


def test_the_wide_scene_names_more_particles_than_one_workgroup_takes(oracle, full):
    """wide_scene(limit): more nodes than the limit (the library's policy constant here; the GPU test asks the device),
    within GPE_BOND_MAX_DEGREE and 64 colours.  Its ties have stiffness 0 and follow the scene's bonds, whose colours
    they leave alone: the particles' bits are the scene's, some ties break on the way."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    internal = open(os.path.join(root, "gpu-physics-engine_amd", "csrc", "gpe_internal.h")).read()
    policy = int(re.search(r"#define GPE_BOND_LDS_NODES_MAX (\d+)", internal).group(1))
    base = E.scene()
    for limit in (policy, E.N - 1, E.N + 41):                          # (past the particles: uids nobody has)
        sc = E.wide_scene(limit)
        assert BM.node_count(sc.bonds) > limit and sc.bonds[:len(base.bonds)].tobytes() == base.bonds.tobytes()
        assert np.array_equal(BS.colours(sc.bonds)[:len(base.bonds)], BS.colours(base.bonds))
        assert BS.colour_info(sc.bonds)[0] <= BS.COLOURS_MAX
    tw = E.twin(oracle, sc=E.wide_scene(policy))
    frames = E.frames(tw)
    counters = tw.counters()
    tw.close()
    for s, (f, g) in enumerate(zip(frames, full[0])):
        assert same_bits(f.pos, g.pos) and same_bits(f.prev, g.prev), s
    print(counters["bonds"], counters["bond_solver"])
    assert counters["bonds"]["broken"] > full[1]["bonds"]["broken"] >= 1
    assert counters["bond_solver"]["passes"] == E.STEPS


def test_the_thin_movers_skip_particles_under_the_plain_pass(oracle, full):
    """the composed scene with the movers' sweep off: the gate and the blade jump across particles the swept form
    pushes, so `pushed` of the movers differs (and the swept form's counters stay 0)"""
    tw = E.twin(oracle, tuple(a for a in E.ARMS if a != "mover_sweep"))
    E.frames(tw)
    off, on = tw.counters(), full[1]
    tw.close()
    print("movers pushed: swept", on["movers"]["pushed"], "plain", off["movers"]["pushed"])
    assert off["mover_sweep"] == dict(mode=0, passes=0, swept=0, stopped=0) and off["movers"]["passes"] == E.STEPS
    assert off["movers"]["pushed"] != on["movers"]["pushed"]


@pytest.mark.parametrize("out", E.ARMS)
def test_every_arm_matters(oracle, full, out):
    """leaving one arm out changes the bits after 40 steps: the leave-one-out cases on the GPU can tell the arms apart"""
    tw = E.twin(oracle, tuple(a for a in E.ARMS if a != out))
    assert out not in tw.armed()
    last = E.frames(tw)[-1]
    tw.close()
    assert not (same_bits(last.pos, full[0][-1].pos) and same_bits(last.prev, full[0][-1].prev))


PASSES = ("bends", "areas", "bonds", "bodies", "movers", "colliders", "fields")


def _swapped(oracle, full, a, b):
    """passes a and b of PASSES swapped behind every step: other bits after 40 steps"""
    order = list(PASSES)
    order[a], order[b] = order[b], order[a]

    class Swapped(E.Everything):
        def step(self, dt, resort=False):
            E.OracleModel.step(self, dt, resort=resort)
            for name in order:
                getattr(self, "apply_" + name)(*((dt,) if name in ("movers", "fields") else ()))

    sc = E.scene()
    tw = Swapped(oracle, sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev)
    tw.enable_uids()
    last = E.frames(E.arm(tw, sc))[-1]
    tw.close()
    assert not (same_bits(last.pos, full[0][-1].pos) and same_bits(last.prev, full[0][-1].prev)), order


@pytest.mark.parametrize("first", range(len(PASSES) - 1))
def test_the_order_of_the_passes_matters(oracle, full, first):
    """two neighbouring passes swapped behind every step change the bits after 40 steps: the all-arms case on the GPU
    pins the order of gpe_step, not only the presence of every pass"""
    _swapped(oracle, full, first, first + 1)


def test_the_areas_behind_the_bodies_give_other_bits(oracle, full):
    """the areas' pass swapped with the bodies' (two sets of the uid sets' table, two apart in it): the blob's loop and
    the blob's shape matching touch the same particles, so the all-arms case tells the two orders apart"""
    _swapped(oracle, full, PASSES.index("areas"), PASSES.index("bodies"))


@pytest.mark.parametrize("seed", E.SEEDS)
def test_the_plans_reach_what_they_are_for(oracle, seed):
    plan = E.plan(seed)
    assert 60 <= len(plan.ops) == 105 and plan.ops == E.plan(seed).ops
    seq = E.Sequence(plan, oracle)
    try:
        seq.run()
        print("\n".join(seq.log))
        print(dict(seq.cov))
        seq.cov.check()
        for k in ("op_solver_jacobi", "op_solver_coloured", "op_solver_coloured_again", "op_refuse_65_colours",
                  "solver_switched_with_a_broken_bond_held", "armed_bond_broke_under_coloured", "armed_coloured_changed",
                  "save_load_with_the_mode_and_a_broken_bond", "growth_under_coloured", "removal_of_bonded_under_coloured"):
            assert seq.cov[k] >= 1, k
        print("fully armed steps: %d of %d" % (seq.cov["armed_steps"], seq.steps))
        assert np.isfinite(seq.tw.arrays()[0]).all()
    finally:
        seq.close()
