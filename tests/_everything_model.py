"""Every pass behind a step armed at once: bends -> areas -> bonds (Jacobi / coloured) -> bodies -> movers (plain /
surfaces / swept) -> static colliders (plain / surfaces / swept) -> fields, the order of gpe_step and gpe_run
(csrc/gpe_api.hip).  TEST INFRASTRUCTURE ONLY.

Everything is one twin over the three chains of twins the features' own tests use (tests/_bodies_model.Twin: bonds,
bodies, plain colliders; tests/_areas_model.Twin: bends, areas, bonds, plain colliders; tests/_sweep_model.Twin: movers,
surfaces, sweep, fields) with the movers' sweep of tests/_mover_sweep_model.Mixin and the bonds' solver of
tests/_bond_solver_model.Mixin in front.  It writes no physics: every pass is the model function its feature's tests
pin against the device, and tests/test_everything_cpu.py ties it bit for bit to the five existing twins.  THE NEXT PASS
BEHIND A STEP IS ADDED HERE: its twin into the bases, its call into step(), its arm into ARMS, arm(), armed(),
counters(), state_counters() and reloaded(), its blocks into BLOCKS and what they must reach into Coverage.check().

scene() is the staged scene of the CPU and GPU tests, arm() sets its features on a twin or on a State (their methods
share names), plan(seed) a list of operations and Sequence the thing that applies them to a twin and, when it has one, to
a State.  Every draw comes from one generator and depends on nothing but the twin's state, so a plan runs with the twin
alone on a CPU, where Coverage.check() is met before any GPU time is spent."""
import collections
import ctypes as C
import os
import tempfile

import numpy as np

from tests import _areas_model as AM
from tests import _bends_model as NM
from tests import _bodies_model as BD
from tests import _bond_solver_model as BS
from tests import _bonds_model as BM
from tests import _fields_model as FM
from tests import _mover_sweep_model as MS
from tests import _movers_model as MM
from tests import _surfaces_model as SM
from tests import _sweep_model as SW
from tests._oracle_model import OracleModel, VEL_ADD, VEL_SET, circle_mask

F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
DTS = (1.0 / 60.0, 1.0 / 120.0)
STEPS = 40
SEEDS = (1, 2, 3)
ARMS = ("bends", "areas", "bonds", "bond_solver", "bodies", "movers", "mover_surfaces", "mover_sweep", "colliders",
        "collider_surfaces", "sweep", "fields")
# the arrays of a snapshot that holds all thirteen optional groups (State.save; the movers' poses belong to the movers'
# group, the relaxation counts and the loops' members to the bends' and the areas'; the bonds' solver is written where
# bonds are held and it is the coloured one)
GROUPS = ("colliders", "collider_surfaces", "collider_sweep", "bonds", "bond_solver", "bends", "bend_iterations", "areas",
          "area_member_uid", "area_iterations", "bodies", "fields", "movers", "mover_poses", "mover_surfaces", "mover_sweep",
          "uids")


class Everything(BS.Mixin, MS.Mixin, BD.Twin, AM.Twin, SW.Twin):
    """One context with all eleven features: the MRO runs through the three chains once, every constructor is
    cooperative; the movers' mixin makes self.m a set that holds the movers' sweep, the solver's mixin in front keeps
    the bonds' solver and the colours of the set held (both modes of the context, not of a set)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.field_passes = self.field_touched = self.field_changed = 0
        self.bend_changed = self.area_changed = self.coloured_changed = 0

    def _changed_by(self, apply):
        """run a pass of a twin below -> the rows whose pos bits it changed"""
        before = np.ascontiguousarray(self.arrays()[0], F32).view(U32).copy()
        apply()
        return int((np.ascontiguousarray(self.arrays()[0], F32).view(U32) != before).any(axis=1).sum())

    def apply_bends(self):
        """gpe_apply_bends: the bends' twin's pass (tests/_bends_model.apply); bend_changed counts the rows it changed"""
        self.bend_changed += self._changed_by(super().apply_bends)

    def apply_areas(self):
        """gpe_apply_areas: the areas' twin's pass (tests/_areas_model.apply); area_changed counts the rows it changed"""
        self.area_changed += self._changed_by(super().apply_areas)

    def apply_bonds(self):
        """gpe_apply_bonds: the bonds' twin's pass, or the solver's coloured one; coloured_changed counts the rows a
        coloured pass changed"""
        coloured = self.bond_solver == BS.COLOURED
        changed = self._changed_by(super().apply_bonds)
        if coloured:
            self.coloured_changed += changed

    def set_fields(self, fields):
        super().set_fields(fields)
        self.field_passes = self.field_touched = 0

    def apply_fields(self, dt):
        """gpe_apply_fields: tests/_fields_model.apply on prev; field_changed counts the rows whose prev bits changed"""
        if len(self.fields) == 0:
            return
        self._pull()
        new, touched = FM.apply(self.pos, self.prev, self.fields, dt)
        self.field_changed += int((np.ascontiguousarray(new).view(U32) != np.ascontiguousarray(self.prev, F32).view(U32))
                                  .any(axis=1).sum())
        self.prev = new
        self.field_passes += 1
        self.field_touched += int(touched.sum())

    def step(self, dt, resort=False):
        OracleModel.step(self, dt, resort=resort)
        self.apply_bends()
        self.apply_areas()
        self.apply_bonds()
        self.apply_bodies()
        self.apply_movers(dt)
        self.apply_colliders()
        self.apply_fields(dt)

    def armed(self):
        """-> the arms that are set"""
        on = dict(bends=len(self.bends) > 0, areas=len(self.areas) > 0,
                  bonds=len(self.bonds) > 0, bond_solver=self.bond_solver == BS.COLOURED,
                  bodies=len(self.bodies) > 0, movers=len(self.m) > 0,
                  mover_surfaces=self.m.surfaces is not None, mover_sweep=self.m.sweep, colliders=len(self.colliders) > 0,
                  collider_surfaces=self.collider_surfaces is not None, sweep=self.sweep, fields=len(self.fields) > 0)
        return tuple(a for a in ARMS if on[a])

    def fully_armed(self):
        return self.armed() == ARMS and self.uids is not None

    def reloaded(self):
        """State.save() / State.load(): every set is set anew (its counters start again, the body poses are unknown
        until a pass), the broken flags, the movers' states, the two sweeps' modes and the bonds' solver with the
        colours of its set are kept.  (A coloured mode over no bonds is not written: it comes back as Jacobi.)"""
        self.passes = self.pushed = 0
        self.solver_passes = 0
        if len(self.bonds) == 0:
            self.bond_solver, self.bond_colour = BS.JACOBI, np.zeros(0, np.int64)
        self.bend_passes = self.area_passes = 0
        self.area_value = np.full((len(self.areas), 2), np.nan, F32)   # (as set_areas leaves it: no pass yet)
        self.bond_passes = self.body_passes = 0
        self.poses = np.full((len(self.bodies), 4), np.nan, F32)
        self.m.passes = self.m.pushed = 0
        self.m.sweep_passes = self.m.swept = self.m.stopped = 0
        self.sweep_passes = self.swept = self.stopped = 0
        self.field_passes = self.field_touched = 0

    def counters(self):
        """what the info calls of a context report, as far as the model knows it"""
        return dict(colliders=dict(k=len(self.colliders), passes=self.passes, pushed=self.pushed),
                    movers=dict(k=len(self.m), passes=self.m.passes, pushed=self.m.pushed),
                    sweep=dict(mode=int(self.sweep), passes=self.sweep_passes, swept=self.swept, stopped=self.stopped),
                    mover_sweep=self.mover_sweep_info(),
                    bends=self.bends_info(), areas=self.areas_info(), bonds=self.bonds_info(), bodies=self.bodies_info(),
                    bond_solver=self.bond_solver_info(),
                    fields=dict(k=len(self.fields), passes=self.field_passes if len(self.fields) else 0,
                                touched=self.field_touched if len(self.fields) else 0))


def state_counters(st):
    """the same dict from a State (the grids' sizes, the uid lookups and the solver's launch form and LDS limit, which
    the model does not have, left out)"""
    pick = lambda info, names: {k: info[k] for k in names}
    bends, areas, bonds, bodies = st.bends_info(), st.areas_info(), st.bonds_info(), st.bodies_info()
    for info in (bends, areas, bonds, bodies):
        info.pop("resolves")
    return dict(colliders=pick(st.colliders_info(), ("k", "passes", "pushed")),
                movers=pick(st.movers_info(), ("k", "passes", "pushed")), sweep=st.sweep_info(),
                mover_sweep=st.mover_sweep_info(), bends=bends, areas=areas, bonds=bonds, bodies=bodies,
                bond_solver=pick(st.bond_solver_info(), ("mode", "colours", "largest_colour", "passes")),
                fields=pick(st.fields_info(), ("k", "passes", "touched")))


# ---- the scene: test_gpu_bodies' yard filled up to 1025 particles, with a piston, a paddle, a thin gate, a thin blade,
# ---- a corner and a field set ------------------------------------------------------------------------------------------
WORLD, GRAVITY = (60.0, 60.0), (0.0, 100.0)
N = 1025                                                               # odd, past two blocks of 512
CORNER = np.array([[50, 31, 57, 31, 0], [57, 31, 57, 38, 0]], F32)     # two zero-radius capsules: apex (57, 31), open to the lower left
SHOTS = 8
SHOT_SPEED = 6.0                                                       # units per step: thinner walls than a step's path
# thinner than one step's displacement, where the plain pass skips particles: an R = 0 gate at 2 units per step through the
# lattice on the floor, an R = 0 blade at 0.4 rad per step that reaches the bricks' band
THIN_MOVERS = MM.rows(MM.linear((14, 30), (14, 39.4), 0.0, v=(120.0, 0.0), travel=12.0),
                      MM.rotor((30, 36), (36, 36), 0.0, (30, 36), 24.0))
# rings of RING members (centre, clockwise): one in the bricks' band in front of the piston, under the lattice's upper
# rows; two above the lattice, over the paddle and over the bricks, inside the vortex once they have fallen
RING = 16
RINGS = (((11.5, 29.0), False), ((42.0, 13.0), True), ((22.5, 13.0), False))
RING_PRESSURE = (1.0, 1.1, 0.9)
RING_FIRST = N - SHOTS - RING * len(RINGS)                             # the rings' uids: behind the fill, before the shots
FALLER, TIE_LENGTH = RING_FIRST + RING + 2, 1.5                        # a member of the second ring and the tie that lets it go
BLOB = 7                                                               # the yard's soft body: its 16 outer members carry a loop
BEND_STIFFNESS, AREA_STIFFNESS, EDGE_STIFFNESS = 0.1, 0.8, 0.25
Scene = collections.namedtuple("Scene", "pos prev rad bonds iterations bodies member_uid member_rest colliders "
                                        "collider_surfaces movers mover_surfaces fields bends bend_iterations areas "
                                        "area_member_uid area_iterations")


def scene_loops(bodies):
    """-> the uids of the scene's four loops, in order around each: the three rings, then the blob's outer members"""
    first = int(bodies["first"][BLOB])
    assert bodies["count"][BLOB] == 1 + RING
    return ([np.arange(RING_FIRST + RING * q, RING_FIRST + RING * (q + 1), dtype=U32) for q in range(len(RINGS))]
            + [np.arange(first + 1, first + 1 + RING, dtype=U32)])


def scene():
    """uid = storage index at the start.  The yard (a pendulum, six bricks of which one is brittle, a soft blob, 120
    loose particles; a floor and a peg; two bonds relaxed twice), 775 more loose particles on a jittered lattice above
    the floor, three RINGS, and eight shots: particles below the corner that leave for its apex at 6 units per step.
    Every ring, and the ring of the blob's 16 outer members, carries bonds along its edge, a bend at every member (one
    relaxation) and one area constraint (two): a member of the blob's ring is a bend node, an area member, a bond end
    and a body member at once.  The last bond is a tie that breaks when FALLER has fallen TIE_LENGTH.  The movers are
    tests/_movers_model.run_movers' thick piston and paddle, then THIN_MOVERS."""
    from tests.test_gpu_areas import ring
    from tests.test_gpu_bodies import YARD_COLLIDERS, yard_scene
    pos, rad, bodies, member_uid, member_rest, bonds = yard_scene()
    bodies["break_distance"][3] = 0.05                                 # the brittle brick breaks well before the 15th step
    rng = np.random.default_rng(31)
    k = RING_FIRST - len(pos)
    i = np.arange(56 * 29)
    x, y = 2.5 + 1.0 * (i % 56), 39.4 - 1.02 * (i // 56)               # rows from the floor (centres rest at 39.5) upward
    far = lambda cx, cy, r: (x - cx) ** 2 + (y - cy) ** 2 > r * r
    free = ((y < 25.5) | (y > 32.5)) & far(30, 15, 3.8) & far(40, 30, 3.8)          # the bricks' band, the blob, the peg
    free &= ~((x > 8.5) & (x < 13.5) & (y < 16.0))                     # the pendulum
    free &= ~((x < 7.8) & (y > 25.0)) & ~((x > 37.5) & (x < 50.5) & (y > 29.5) & (y < 34.5))     # the piston, the paddle
    free &= ~((x > 48.5) & (y > 30.0) & (y < 39.0))                    # the corner and the lane of the shots
    rings = [ring(RING, c, seed=40 + q, wobble=0.05, clockwise=cw) for q, (c, cw) in enumerate(RINGS)]
    for c, _ in RINGS:
        free &= far(c[0], c[1], 3.9)
    assert free.sum() >= k
    fill = np.stack([x, y], axis=1)[free][:k] + rng.uniform(-0.08, 0.08, (k, 2))
    j = np.arange(SHOTS)
    shots = np.stack([50.5 + 1.1 * (j % 4), 36.0 + 1.1 * (j // 4)], axis=1)
    pos = np.concatenate([pos, fill] + rings + [shots]).astype(F32)
    prev = pos.copy()
    d = np.array([57.0, 31.0]) - shots                                 # toward the apex
    d /= np.linalg.norm(d, axis=1)[:, None]
    prev[-SHOTS:] = (shots - SHOT_SPEED * d).astype(F32)
    assert len(pos) == N
    loops = scene_loops(bodies)
    uid = np.stack(loops)
    nxt, prv = np.roll(uid, -1, axis=1), np.roll(uid, 1, axis=1)
    rest = np.repeat([1.1] * len(RINGS) + [1.05], RING)                # a little over the spacing the loops start with
    # ... and a tie of stiffness 0 from a member of the ring that falls over the paddle to where it starts: it moves
    # nothing and breaks once the member is TIE_LENGTH away, under either solver
    bonds = np.concatenate([bonds, BM.pairs(uid.ravel(), nxt.ravel(), rest, EDGE_STIFFNESS),
                            BM.anchors([FALLER], [pos[FALLER]], 0.0, 0.0, TIE_LENGTH)])
    start = np.arange(N, dtype=U32)
    bends = NM.captured(pos, start, np.stack([prv.ravel(), uid.ravel(), nxt.ravel()], axis=1), BEND_STIFFNESS)
    areas, area_member_uid = AM.captured(pos, start, loops, AREA_STIFFNESS, RING_PRESSURE + (1.0,))
    assert sorted(np.sign(areas["rest_area"][:len(RINGS)]).tolist()) == [-1, 1, 1]    # either sense of rotation
    colliders = np.concatenate([YARD_COLLIDERS, CORNER]).astype(F32)
    movers = np.concatenate([MM.run_movers(), THIN_MOVERS])
    assert all(MM.dt_allowed(movers, dt) for dt in DTS)
    return Scene(pos, prev, np.full(N, 0.5, F32), bonds, 2, bodies, member_uid, member_rest, colliders,
                 SM.scene_surfaces(len(colliders)), movers, SM.scene_surfaces(len(movers), seed=5), FM.POOL_FIELDS,
                 bends, 1, areas, area_member_uid, 2)


def wide_scene(lds_nodes_max):
    """scene() with ties of stiffness 0 along the fill until the bonds name more than lds_nodes_max uids
    (gpe_get_bond_solver_info): a coloured pass over it takes the per-colour launch form.  Neighbouring uids no bond of
    the scene names are tied in disjoint pairs, every third tie with a max_length a shove breaks; a uid left over gets
    an anchor where it starts; past the scene's particles the ties name uids nobody has (nodes all the same)."""
    sc = scene()
    named = np.zeros(N, bool)
    named[np.concatenate([sc.bonds["uid_a"], sc.bonds["uid_b"][(sc.bonds["flags"] & BM.BOND_ANCHOR) == 0]])] = True
    loose = np.nonzero(~named)[0].astype(U32)
    a, b = loose[0:len(loose) - 1:2], loose[1::2]
    ties = [BM.pairs(a, b, 1.0, 0.0, np.where(np.arange(len(a)) % 3 == 0, 1.6, 0.0).astype(F32))]
    if len(loose) % 2:
        ties.append(BM.anchors(loose[-1:], sc.pos[loose[-1:]], 0.0, 0.0))
    short = lds_nodes_max + 1 - N
    if short > 0:
        absent = N + 7 + np.arange(short + short % 2, dtype=U32)
        ties.append(BM.pairs(absent[0::2], absent[1::2], 1.0, 0.0))
    bonds = np.concatenate([sc.bonds] + ties)
    assert BM.node_count(bonds) > lds_nodes_max and BS.colour_info(bonds)[0] <= BS.COLOURS_MAX
    ends = np.concatenate([bonds["uid_a"], bonds["uid_b"][(bonds["flags"] & BM.BOND_ANCHOR) == 0]])
    assert np.unique(ends, return_counts=True)[1].max() <= BM.BOND_MAX_DEGREE
    return sc._replace(bonds=bonds)


def arm(h, sc, arms=ARMS):
    """set the features of `arms` on a twin or a State (uids on already); a set left out leaves its surfaces out, but
    not the movers' sweep nor the bonds' solver: the modes are the context's, on with no movers and no bonds held as
    well.  The solver is set in front of its set (the plans cover the other order)."""
    if "bends" in arms:
        h.set_bends(sc.bends, sc.bend_iterations)
    if "areas" in arms:
        h.set_areas(sc.areas, sc.area_member_uid, sc.area_iterations)
    if "bond_solver" in arms:
        h.set_bond_solver("coloured")
    if "bonds" in arms:
        h.set_bonds(sc.bonds, sc.iterations)
    if "bodies" in arms:
        h.set_bodies(sc.bodies, sc.member_uid, sc.member_rest)
    if "colliders" in arms:
        h.set_colliders(sc.colliders)
        if "collider_surfaces" in arms:
            h.set_surfaces("colliders", sc.collider_surfaces)
    if "sweep" in arms:
        h.set_collider_sweep(True)
    if "movers" in arms:
        h.set_movers(sc.movers)
        if "mover_surfaces" in arms:
            h.set_surfaces("movers", sc.mover_surfaces)
    if "mover_sweep" in arms:
        h.set_mover_sweep(True)
    if "fields" in arms:
        h.set_fields(sc.fields)
    return h


def twin(oracle, arms=ARMS, sc=None):
    sc = scene() if sc is None else sc
    tw = Everything(oracle, sc.pos, sc.rad, world=WORLD, gravity=GRAVITY, prev=sc.prev)
    tw.enable_uids()
    return arm(tw, sc, arms)


Frame = collections.namedtuple("Frame", "pos prev uids body_poses bodies_broken bonds_broken mover_poses area_value")


def frame(tw):
    pos, prev, _ = tw.arrays()
    return Frame(pos.copy(), prev.copy(), tw.uids.copy(), tw.poses.copy(), tw.bodies_broken.copy(), tw.broken.copy(),
                 tw.m.poses(), tw.area_value.copy())


def frames(tw, steps=STEPS, dt=DT, resort_every=0, resort_first=False):
    """-> the frames after every step, the re-sorts taken as gpe_run(steps, resort_every, resort_first) takes them"""
    out = []
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(dt, resort=bool(resort))
        out.append(frame(tw))
    return out


# ---- the random interleaving -------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "seed ops")
SETS = ("bends", "areas", "bonds", "bodies", "fields", "collider_surfaces", "mover_surfaces")
BLOCKS = ([["set_" + s, "step", "clear_" + s, "step", "set_" + s] for s in SETS] + [
    ["set_colliders", "set_collider_surfaces", "step", "clear_colliders", "step", "set_colliders", "set_collider_surfaces"],
    ["set_movers", "set_mover_surfaces", "step", "clear_movers", "step", "set_movers", "set_mover_surfaces"],
    ["sweep_off", "step", "sweep_on"], ["mover_sweep_off", "step", "mover_sweep_on"], ["set_mover_poses", "step"],
    ["run"], ["run"], ["run_resort_mid"], ["resort", "step"], ["add_few", "step"], ["add_grow", "step"],
    ["remove_circle", "step"], ["remove_members", "step"], ["remove_uid"], ["edit_pos", "step"],
    ["radius_up", "step", "radius_down", "step"], ["kick", "step"], ["world_grow", "step", "world_back", "step"], ["gravity"],
    ["other_mode"], ["save_load", "step"], ["pump", "step"], ["apply_bends"], ["apply_areas"], ["apply_bonds"],
    ["apply_bodies"], ["apply_movers"], ["apply_colliders"], ["apply_fields"],
    # the bonds' solver: switched with the set held, set while already on, and a set it cannot take
    ["solver_jacobi", "step", "solver_coloured", "step"], ["solver_coloured_again", "step"], ["refuse_65_colours", "step"]])
REPLACING = (["set_" + s for s in SETS + ("colliders", "movers", "mover_poses")] + ["clear_" + s for s in SETS + ("colliders", "movers")]
             + ["sweep_off", "sweep_on", "mover_sweep_off", "mover_sweep_on"]
             + ["solver_jacobi", "solver_coloured", "solver_coloured_again", "refuse_65_colours"])


def plan(seed):
    """BLOCKS in a random order behind a run of the scene as it starts (its shots and the brittle brick act there).  A
    block leaves every arm set, so every block starts fully armed; what its operations draw when they run comes from
    Sequence.rng."""
    rng = np.random.default_rng(7100 + seed)
    order = rng.permutation(len(BLOCKS))
    ops = ["run_start"] + [op for i in order for op in BLOCKS[i]]
    # the opening run and every block once: seven sets of 5, two of 7, 2 x 3 + 2 for the modes and the poses, 3 runs,
    # 9 blocks of 2 (the pump's among them), 2 of 4, 3 single operations, the 7 passes and the solver's 4 + 2 + 2
    assert len(ops) == 1 + 7 * 5 + 2 * 7 + 8 + 3 + 9 * 2 + 2 * 4 + 3 + 7 + 8 == 105
    return Plan(seed, ops)


class Coverage(collections.Counter):
    """What a sequence reached, counted on the twin's side."""

    def check(self):
        need = (["armed_" + k for k in ("colliders_pushed", "movers_pushed", "swept", "stopped", "mover_swept", "mover_stopped",
                                        "body_broke", "field_changed", "bend_changed", "area_changed", "resort", "growth",
                                        "removal_of_member_and_bonded", "loop_lost_a_member", "pump", "radius_up",
                                        "bond_broke_under_coloured", "coloured_changed")]
                + ["set_world_with_grids", "save_load_every_group", "run_resorts_in_its_middle"] + ["op_" + op for op in REPLACING]
                + ["solver_switched_with_a_broken_bond_held", "save_load_with_the_mode_and_a_broken_bond",
                   "growth_under_coloured", "removal_of_bonded_under_coloured"])
        missing = [k for k in need if self[k] == 0]
        assert not missing, "the sequence never reached: %s\n%s" % (", ".join(missing), dict(self))
        assert self["armed_steps"] >= 30, "only %d steps with all twelve arms set" % self["armed_steps"]


class Sequence:
    """One plan applied to the twin and (gpe given) to a State under GPE_FLAG_GUARD_ALLOCS.  compare(st, twin, where) is
    called after every operation, end(st) with every State that leaves."""

    def __init__(self, plan_, oracle, gpe=None, mode_name="native", compare=None, end=None):
        self.plan, self.gpe, self.compare, self.end, self.mode_name = plan_, gpe, compare, end, mode_name
        self.rng = np.random.default_rng(7200 + plan_.seed)
        self.sc = scene()
        self.tw = twin(oracle, sc=self.sc)
        self.world = WORLD
        self.cov = Coverage()
        self.log = []
        self.cap = len(self.tw)
        self.steps = 0
        self.native_steps = self.compat_steps = self.other_steps = 0
        self.st = self.L = None
        self.tmp = tempfile.TemporaryDirectory()
        if gpe is not None:
            self.L = gpe._lib
            self.mode = self.L.MODE_NATIVE if mode_name == "native" else self.L.MODE_COMPAT
            self.other = self.L.MODE_COMPAT if mode_name == "native" else self.L.MODE_NATIVE
            self.st = gpe.State(self.sc.pos, self.sc.rad, world=WORLD, gravity=GRAVITY, prev=self.sc.prev, mode=self.mode,
                                flags=self.L.FLAG_GUARD_ALLOCS)
            self.st.enable_uids()
            arm(self.st, self.sc)

    # ---- plumbing -----------------------------------------------------------------------------------------------------
    def where(self, i, op):
        return "seed %d %s op #%d (%s)\n  %s" % (self.plan.seed, self.mode_name, i, op, "\n  ".join(self.log))

    def both(self):
        return [h for h in (self.st, self.tw) if h is not None]

    def retire(self):
        info = self.st.ctx.pipeline_info()
        self.native_steps += info["native_steps"]
        self.compat_steps += info["compat_steps"]

    def close(self):
        if self.st is not None:
            self.retire()
            self.end(self.st)
            self.st = None
        self.tw.close()
        self.tmp.cleanup()

    def run(self):
        for i, op in enumerate(self.plan.ops):
            self.cov["op_" + op] += 1
            getattr(self, "op_" + op)()
            if self.st is not None:
                cap = C.c_uint64()
                self.st.ctx.call("gpe_capacity", C.byref(cap))
                assert cap.value == self.cap, "capacity %d, expected %d\n%s" % (cap.value, self.cap, self.where(i, op))
                self.compare(self.st, self.tw, self.where(i, op))

    def _a_particle(self):
        p = self.tw.arrays()[0]
        return p[int(self.rng.integers(0, len(p)))]

    def _inside(self, k, y1=35.0):
        return np.stack([self.rng.uniform(2, 58, k), self.rng.uniform(2, y1, k)], axis=1).astype(F32)

    # ---- steps --------------------------------------------------------------------------------------------------------
    def _watch(self):
        tw = self.tw
        return dict(colliders_pushed=tw.pushed, movers_pushed=tw.m.pushed, swept=tw.swept, stopped=tw.stopped,
                    mover_swept=tw.m.swept, mover_stopped=tw.m.stopped,
                    body_broke=int(tw.bodies_broken.sum()), field_changed=tw.field_changed,
                    bend_changed=tw.bend_changed, area_changed=tw.area_changed,
                    # (counted over fully armed steps, where the solver is the coloured one)
                    bond_broke_under_coloured=int(tw.broken.sum()), coloured_changed=tw.coloured_changed)

    def _twin_step(self, dt, resort):
        armed = self.tw.fully_armed()
        before = self._watch()
        self.tw.step(dt, resort=resort)
        self.steps += 1
        if armed:
            self.cov["armed_steps"] += 1
            for k, v in self._watch().items():
                self.cov["armed_" + k] += v - before[k]
            if resort:
                self.cov["armed_resort"] += 1

    def _dt(self):
        dt = DTS[int(self.rng.integers(0, 2))]
        assert MM.dt_allowed(self.tw.m.movers, dt)
        return dt

    def _steps(self, k, dt=None):
        for s in range(k):
            d = self._dt() if dt is None else dt
            resort = bool(self.rng.integers(0, 4) == 0)
            if self.st is not None:
                self.st.update(d, resort=resort)
            self._twin_step(d, resort)
            self.log.append("step dt 1/%d%s" % (round(1 / d), " resort" if resort else ""))

    def op_step(self):
        self._steps(int(self.rng.integers(1, 4)))

    def _run(self, k, every, first, dt):
        if self.st is not None:
            self.st.run(dt, k, resort_every=every, resort_first=first)
        for s in range(k):
            self._twin_step(dt, bool((s == 0 and first) or (every and s > 0 and s % every == 0)))
        if every and k > every:
            self.cov["run_resorts_in_its_middle"] += 1
        self.log.append("run %d dt 1/%d every %d first %s" % (k, round(1 / dt), every, first))

    def op_run_start(self):
        self._run(16, 0, False, DT)

    def op_run(self):
        self._run(int(self.rng.integers(5, 13)), int(self.rng.choice([0, 4])), bool(self.rng.integers(0, 2)), self._dt())

    def op_run_resort_mid(self):
        self._run(int(self.rng.integers(9, 14)), 4, bool(self.rng.integers(0, 2)), self._dt())

    def op_resort(self):
        if self.st is not None:
            self.st.particles.sort_by_cell_id()
        self.tw.morton_resort()
        if self.tw.fully_armed():
            self.cov["armed_resort"] += 1
        self.log.append("morton resort")

    def op_other_mode(self):
        k = int(self.rng.integers(1, 4))
        if self.st is not None:
            self.st.ctx.call("gpe_set_mode", self.other)
        self._steps(k)
        self.other_steps += k
        if self.st is not None:
            self.st.ctx.call("gpe_set_mode", self.mode)
        self.log.append("(%d steps in the other mode)" % k)

    # ---- particles come and go, and are edited ------------------------------------------------------------------------
    def _add(self, p, r, what):
        n = len(self.tw)
        for h in self.both():
            (h.add_particles if h is self.st else h.add)(p, r)
        grew = n + len(r) > self.cap
        if grew:
            self.cap = max(n + len(r), 2 * self.cap)
            if self.tw.fully_armed():
                self.cov["armed_growth"] += 1
                self.cov["growth_under_coloured"] += 1
        self.log.append("%s %d%s" % (what, len(r), " (grew to %d)" % self.cap if grew else ""))

    def op_add_few(self):
        k = int(self.rng.integers(1, 20))
        self._add(self._inside(k, 25.0), np.full(k, 0.5, F32), "add")

    def op_add_grow(self):
        k = self.cap - len(self.tw) + 30
        self._add(self._inside(k, 30.0), np.full(k, 0.25, F32), "add past the capacity")

    def op_remove_circle(self):
        c = self._a_particle()
        c, r = (float(c[0]), float(c[1])), float(F32(self.rng.uniform(1.0, 3.0)))
        if circle_mask(self.tw.arrays()[0], c[0], c[1], r).all():
            r = 0.0
        want = self.tw.remove_circle(c[0], c[1], r)
        if self.st is not None:
            assert self.st.remove_particles_in_circle(c, r) == want
        self.log.append("remove circle %s r %g: %d" % (c, r, want))

    def _remove_uids(self, q, what):
        want = self.tw.remove_uids(q)
        if self.st is not None:
            assert self.st.remove_particles_by_uid(q) == want
        self.log.append("%s: %d of %d uids" % (what, want, len(q)))

    def op_remove_members(self):
        """a live member of a body, a live bonded particle, a live member of a loop (the loop is inert from here on), a
        live node of a bend, two more and one nobody has"""
        tw, rng = self.tw, self.rng
        armed = tw.fully_armed()
        live = lambda u: u[np.isin(u, tw.uids)]
        member, bonded = live(tw.member_uid), live(np.concatenate([tw.bonds["uid_a"], tw.bonds["uid_b"]]))
        looped = live(tw.area_member_uid)
        node = live(np.concatenate([tw.bends["uid_a"], tw.bends["uid_b"], tw.bends["uid_c"]]))
        q = [rng.choice(member)] if len(member) else []
        q += [rng.choice(bonded)] if len(bonded) else []
        q += [rng.choice(looped)] if len(looped) else []
        q += [rng.choice(node)] if len(node) else []
        if armed and len(member) and len(bonded):
            self.cov["armed_removal_of_member_and_bonded"] += 1
        if armed and len(bonded):
            self.cov["removal_of_bonded_under_coloured"] += 1
        if armed and len(looped) and len(node):
            self.cov["armed_loop_lost_a_member"] += 1
        q = np.unique(np.concatenate([q, rng.choice(tw.uids, 2, replace=False), [tw.next_uid + 3]]).astype(U32))
        self._remove_uids(q, "remove a member, a bonded uid, a loop's member and a bend's node")

    def op_remove_uid(self):
        q = np.unique(np.append(self.rng.choice(self.tw.uids, 3, replace=False), 0xFFFFFFF0).astype(U32))
        self._remove_uids(q, "remove uids")

    def _edit(self, who, what, **kw):
        want = self.tw.edit(who, "index", **kw)
        if self.st is not None:
            got = self.st.edit_particles(indices=who, positions=kw.get("pos"), previous=kw.get("prev"), radii=kw.get("radius"))
            assert got == want
        self.log.append("%s: %d" % (what, want))

    def op_edit_pos(self):
        k = int(self.rng.integers(1, 30))
        who = self.rng.choice(len(self.tw), k, replace=False).astype(U32)
        self._edit(who, "edit positions", pos=self._inside(k))

    def op_radius_up(self):
        """one particle gets a new largest radius: every grid that depends on the radius bound is stale"""
        tw = self.tw
        armed = tw.fully_armed()
        who = int(self.rng.integers(0, len(tw)))
        new = F32(F32(abs(tw.max_radius)) * F32(2.0))
        self._edit(np.array([who], U32), "radius up to %g" % new, radius=np.array([new], F32))
        assert tw.max_radius == new
        if armed:
            self.cov["armed_radius_up"] += 1

    def op_radius_down(self):
        tw = self.tw
        r = tw.arrays()[2]
        who = int(np.nonzero(np.abs(r) == abs(tw.max_radius))[0][-1])
        self._edit(np.array([who], U32), "radius down", radius=np.array([0.5], F32))

    def op_kick(self):
        """a kick of a random disc, and a volley at the corner: the particles below it leave for its apex at SHOT_SPEED"""
        rng, tw = self.rng, self.tw
        c = self._a_particle()
        c, r = (float(c[0]), float(c[1])), float(F32(rng.uniform(2.0, 8.0)))
        a = (float(F32(rng.uniform(-2, 2))), float(F32(rng.uniform(-2, 2))))
        s = float(F32(SHOT_SPEED / np.sqrt(2.0)))
        for centre, radius, op, acc in ((c, r, VEL_ADD, a), ((53.5, 34.5), 2.5, VEL_SET, (s, -s))):
            want = tw.kick(circle_mask(tw.arrays()[0], centre[0], centre[1], radius), op, *acc)
            if self.st is not None:
                assert self.st.kick_circle(centre, radius, op, acc) == want
            self.log.append("kick %s r %g op %d %s: %d" % (centre, radius, op, acc, want))

    # ---- constants ----------------------------------------------------------------------------------------------------
    def _world(self, w):
        tw = self.tw
        if len(tw.colliders) and len(tw.m) and len(tw.fields):
            self.cov["set_world_with_grids"] += 1
        if self.st is not None:
            self.st.ctx.call("gpe_set_world", w[0], w[1])
        tw.set_world(*w)
        self.world = w
        self.log.append("world %s" % (w,))

    def op_world_grow(self):
        """twice the size; one particle put on the floor's end and one into the well, both in the newly covered part"""
        self._world((2 * WORLD[0], 2 * WORLD[1]))
        who = self.rng.choice(len(self.tw), 2, replace=False).astype(U32)
        self._edit(who, "edit into the new part", pos=np.array([[63.0, 39.75], [85.0, 45.0]], F32))

    def op_world_back(self):
        self._world(WORLD)

    def op_gravity(self):
        g = (float(self.rng.choice([0.0, 20.0, -20.0])), float(self.rng.choice([100.0, 60.0, 140.0])))
        if self.st is not None:
            self.st.ctx.call("gpe_set_gravity", g[0], g[1])
        self.tw.set_gravity(*g)
        self.log.append("gravity %s" % (g,))

    def op_save_load(self):
        tw = self.tw
        every = tw.fully_armed()
        if every:
            self.cov["save_load_every_group"] += 1
        if every and tw.broken.any():
            self.cov["save_load_with_the_mode_and_a_broken_bond"] += 1
        if self.st is not None:
            path = os.path.join(self.tmp.name, "snap_%d.npz" % len(self.log))
            self.st.save(path)
            with np.load(path) as d:
                if every:
                    assert set(GROUPS) <= set(d.files), sorted(d.files)
            self.retire()
            self.end(self.st)
            self.st = self.gpe.State.load(path, mode=self.mode, flags=self.L.FLAG_GUARD_ALLOCS)
        tw.reloaded()
        self.cap = len(tw)
        self.log.append("save / load%s" % (" (every group)" if every else ""))

    def op_pump(self):
        """gpe_set_area_targets between two steps: new rest areas for a sub-range of the loops, the set's slots and
        counters kept"""
        tw, rng = self.tw, self.rng
        k = len(tw.areas)
        assert k > 0                                                   # (every block leaves the areas set)
        first = int(rng.integers(0, k))
        count = int(rng.integers(1, max(k - first, 2)))                # (less than the whole set where it has two loops)
        t = (tw.areas["rest_area"][first:first + count] * rng.uniform(0.7, 1.4, count)).astype(F32)
        for h in self.both():
            h.set_area_targets(first, t)
        if tw.fully_armed():
            self.cov["armed_pump"] += 1
        self.log.append("pump loops %d .. %d of %d" % (first, first + count - 1, k))

    # ---- the passes called directly -----------------------------------------------------------------------------------
    def _apply(self, name, *args):
        for h in self.both():
            getattr(h, name)(*args)
        self.log.append("%s%s" % (name, args if args else ""))

    def op_apply_bends(self):
        self._apply("apply_bends")

    def op_apply_areas(self):
        self._apply("apply_areas")

    def op_apply_bonds(self):
        self._apply("apply_bonds")

    def op_apply_bodies(self):
        self._apply("apply_bodies")

    def op_apply_movers(self):
        self._apply("apply_movers", self._dt())

    def op_apply_colliders(self):
        self._apply("apply_colliders")

    def op_apply_fields(self):
        self._apply("apply_fields", self._dt())

    # ---- the sets: replaced, cleared, set again -----------------------------------------------------------------------
    def _set(self, name, *args, what=None):
        for h in self.both():
            getattr(h, name)(*args)
        self.log.append(what or name)

    def _near(self, seed, count, free):
        p = self.tw.arrays()[0]
        near = np.argsort(((p - p[seed]) ** 2).sum(axis=1), kind="stable")
        return near[free[near]][:count]

    def op_set_bends(self):
        """chains of particles that are neighbours now, bent towards angles they do not hold (a chain's inner particles
        are hinge of one bend and arm of the next), and one bend with a uid nobody has"""
        rng, tw = self.rng, self.tw
        rows = []
        for _ in range(int(rng.integers(4, 9))):
            chain = self._near(int(rng.integers(0, len(tw))), int(rng.choice([3, 4, 6])), np.ones(len(tw), bool))
            u = tw.uids[chain]
            rows.append(NM.bends(u[:-2], u[1:-1], u[2:], rng.uniform(-np.pi, np.pi, len(u) - 2), float(rng.choice([0.1, 0.5]))))
        rows.append(NM.bends([u[0]], [tw.next_uid + 5], [u[1]], 1.0, 0.5))
        self._set("set_bends", np.concatenate(rows), int(rng.integers(1, 4)))

    def op_clear_bends(self):
        self._set("set_bends", np.zeros(0, NM.BEND_DTYPE), 1, what="clear bends")

    def op_set_areas(self):
        """loops round groups of particles that are close now, in either sense, pumped a little off the area they hold;
        some share members with a later loop; one uid nobody has"""
        rng, tw = self.rng, self.tw
        p = tw.arrays()[0]
        free = np.ones(len(tw), bool)
        loops = []
        for _ in range(int(rng.integers(3, 8))):
            g = self._near(int(rng.integers(0, len(tw))), int(rng.choice([3, 4, 5, 8, 17])), free)
            if len(g) >= 3:
                if rng.integers(0, 2):
                    free[g] = False
                c = p[g].astype(np.float64).mean(axis=0)
                g = g[np.argsort(np.arctan2(p[g, 1] - c[1], p[g, 0] - c[0]), kind="stable")]     # round their centre
                loops.append(tw.uids[g[::-1] if rng.integers(0, 2) else g])
        rows, member = AM.captured(p, tw.uids, loops, rng.choice([0.25, 0.8, 1.0], len(loops)), rng.uniform(0.8, 1.3, len(loops)))
        member[int(rng.integers(0, len(member)))] = tw.next_uid + 9
        self._set("set_areas", rows, member, int(rng.integers(1, 4)))

    def op_clear_areas(self):
        self._set("set_areas", np.zeros(0, AM.AREA_DTYPE), np.zeros(0, U32), 1, what="clear areas")

    def op_set_bonds(self):
        """anchors that hold particles where they are, a tie of stiffness 0 between two of them that breaks in its first
        relaxation unless they touch, pairs of neighbours (some that snap), one uid nobody has"""
        rng, tw = self.rng, self.tw
        p = tw.arrays()[0]
        pins = rng.choice(len(tw), 4, replace=False)
        rows = [BM.anchors(tw.uids[pins], p[pins], 0.0, 0.5), BM.pairs([tw.uids[pins[1]]], [tw.uids[pins[2]]], 1.0, 0.0, 1.0)]
        for _ in range(5):
            a = int(rng.integers(0, len(tw)))
            near = self._near(a, 3, np.ones(len(tw), bool))
            b = int(near[near != a][0])
            rows.append(BM.pairs([tw.uids[a]], [tw.uids[b]], 1.0, float(rng.choice([0.25, 1.0])), float(rng.choice([0.0, 1.6]))))
        rows.append(BM.pairs([tw.uids[pins[0]]], [tw.next_uid + 7], 1.0))
        self._set("set_bonds", np.concatenate(rows), int(rng.integers(1, 4)))

    def op_clear_bonds(self):
        self._set("set_bonds", np.zeros(0, BM.BOND_DTYPE), 1, what="clear bonds")

    def op_set_bodies(self):
        """bodies over particles that are close now, their shape a little off; some brittle; one uid nobody has"""
        rng, tw = self.rng, self.tw
        p = tw.arrays()[0]
        free = np.ones(len(tw), bool)
        groups = []
        for _ in range(int(rng.integers(4, 10))):
            g = self._near(int(rng.integers(0, len(tw))), int(rng.choice([2, 3, 4, 5, 9, 17, 33])), free)
            if len(g) >= 2:
                free[g] = False
                groups.append(g)
        counts = [len(g) for g in groups]
        slot = np.concatenate(groups)
        member_uid = tw.uids[slot].copy()
        member_uid[int(rng.integers(0, len(slot)))] = tw.next_uid + 11
        rest = (p[slot] + rng.uniform(-0.15, 0.15, (len(slot), 2))).astype(F32)
        bodies = BD.rows(counts, rng.choice(np.array([1.0, 0.5, 0.25], F32), len(counts)),
                         np.where(np.arange(len(counts)) % 2 == 0, 0.3, 0.0).astype(F32))
        self._set("set_bodies", bodies, member_uid, rest)

    def op_clear_bodies(self):
        self._set("set_bodies", np.zeros(0, BD.BODY_DTYPE), np.zeros(0, U32), np.zeros((0, 2), F32), what="clear bodies")

    def op_set_colliders(self):
        """the floor, a peg somewhere, the corner, and sometimes a thin shelf"""
        rng = self.rng
        x, y = float(rng.uniform(15, 45)), float(rng.uniform(28, 34))
        rows = [[-5, 45, 65, 45, 5], [x, y, x, y, float(rng.uniform(1, 3))]] + CORNER.tolist()
        if rng.integers(0, 2):
            rows.append([float(rng.uniform(5, 25)), 36.0, float(rng.uniform(26, 40)), 37.0, 0.0])
        self._set("set_colliders", np.array(rows, F32))

    def op_clear_colliders(self):
        self._set("set_colliders", np.zeros((0, 5), F32), what="clear colliders")

    def op_set_collider_surfaces(self):
        self._set("set_surfaces", "colliders", SM.scene_surfaces(len(self.tw.colliders), seed=int(self.rng.integers(0, 1000))),
                  what="set collider surfaces")

    def op_clear_collider_surfaces(self):
        self._set("set_surfaces", "colliders", np.zeros(0, SM.SURFACE_DTYPE), what="clear collider surfaces")

    def op_set_movers(self):
        """a thick piston and a thick paddle, and thinner than a step's displacement a gate near the piston and a blade
        near the paddle, either way round"""
        rng = self.rng
        x, y = float(rng.uniform(4, 8)), float(rng.uniform(26, 30))
        px, py = float(rng.uniform(30, 46)), float(rng.uniform(30, 36))
        gx, bx = x + float(rng.uniform(6, 12)), px - float(rng.uniform(4, 10))
        movers = MM.rows(MM.linear((x, y), (x, y + 13), 2.0, v=(float(rng.uniform(15, 30)), 0.0), travel=float(rng.uniform(6, 12))),
                         MM.rotor((px, py), (px + 7, py), 1.5, (px, py), float(rng.choice([-6.0, 4.0, 6.0]))),
                         MM.linear((gx, y + 2), (gx, 39.4), 0.0, v=(float(rng.choice([-150.0, -90.0, 90.0, 120.0])), 0.0),
                                   travel=float(rng.uniform(8, 12))),
                         MM.rotor((bx, py + 2), (bx + 6, py + 2), 0.0, (bx, py + 2), float(rng.choice([-24.0, -18.0, 18.0, 24.0]))))
        assert all(MM.dt_allowed(movers, dt) for dt in DTS)
        self._set("set_movers", movers)

    def op_clear_movers(self):
        self._set("set_movers", np.zeros(0, MM.MOVER_DTYPE), what="clear movers")

    def op_set_mover_surfaces(self):
        self._set("set_surfaces", "movers", SM.scene_surfaces(len(self.tw.m), seed=int(self.rng.integers(0, 1000))),
                  what="set mover surfaces")

    def op_clear_mover_surfaces(self):
        self._set("set_surfaces", "movers", np.zeros(0, SM.SURFACE_DTYPE), what="clear mover surfaces")

    def op_set_mover_poses(self):
        """the states a fresh copy of the set reaches after a few steps: valid ones, other than those held"""
        ahead = MM.Movers(self.tw.m.movers)
        for _ in range(int(self.rng.integers(3, 30))):
            ahead.q0, ahead.q1 = MM.advance(ahead.movers, ahead.q0, ahead.q1, DT)
        poses = ahead.poses()
        if self.st is not None:
            self.st.set_mover_poses(poses)
        self.tw.m.set_poses(poses)
        self.log.append("set mover poses")

    def op_set_fields(self):
        """a vortex, a well and a wind inside the yard, the drag pool over the floor, and the pool scene's own set behind
        them (it acts once the world has grown)"""
        rng = self.rng
        at = lambda: (float(rng.uniform(10, 50)), float(rng.uniform(25, 38)))
        v, w = at(), at()
        rows = FM.rows(FM.field(FM.CIRCLE, FM.VORTEX, FM.NONE, (v[0], v[1], 9.0, 0), pole=v, strength=float(rng.uniform(40, 120))),
                       FM.field(FM.CIRCLE, FM.RADIAL, FM.LINEAR, (w[0], w[1], 8.0, 0), pole=w, strength=150.0, reach=8.0),
                       FM.field(FM.BOX, FM.DRAG, FM.NONE, (5, 36, 55, 41), strength=float(rng.choice([0.9, 0.98]))),
                       FM.field(FM.BOX, FM.UNIFORM, FM.NONE, (0, 0, 60, 30), f=(float(rng.uniform(-30, 30)), -10.0)),
                       FM.POOL_FIELDS)
        self._set("set_fields", rows)

    def op_clear_fields(self):
        self._set("set_fields", np.zeros(0, FM.DTYPE), what="clear fields")

    def op_sweep_off(self):
        self._set("set_collider_sweep", False, what="sweep off")

    def op_sweep_on(self):
        self._set("set_collider_sweep", True, what="sweep on")

    # the movers' sweep goes off through the C entry point and on through the module class, neither through State: with
    # arm() and State.load, which use State, a later save_load covers every way in
    def op_mover_sweep_off(self):
        if self.st is not None:
            self.st.ctx.call("gpe_set_mover_sweep", self.L.SWEEP_OFF)
        self.tw.set_mover_sweep(False)
        self.log.append("mover sweep off (ctx.call)")

    def op_mover_sweep_on(self):
        if self.st is not None:
            self.st.particles.set_mover_sweep(True)
        self.tw.set_mover_sweep(True)
        self.log.append("mover sweep on (ParticleSystem)")

    # ---- the bonds' solver --------------------------------------------------------------------------------------------
    def _solver(self, solver, what):
        tw = self.tw
        held = len(tw.bonds) > 0
        if solver == "coloured" and tw.bond_solver == BS.JACOBI and held and tw.broken.any():
            self.cov["solver_switched_with_a_broken_bond_held"] += 1   # (the tables are built from the kept set)
        self._set("set_bond_solver", solver, what="%s (%d bonds held, %d broken)" % (what, len(tw.bonds), int(tw.broken.sum())))

    def op_solver_jacobi(self):
        assert self.tw.bond_solver == BS.COLOURED and len(self.tw.bonds) > 0
        self._solver("jacobi", "solver: jacobi")

    def op_solver_coloured(self):
        assert self.tw.bond_solver == BS.JACOBI and len(self.tw.bonds) > 0
        self._solver("coloured", "solver: coloured")

    def op_solver_coloured_again(self):
        """the mode set while it is on: the tables are kept, the solver's counters start again"""
        colour = self.tw.bond_colour.copy()
        assert self.tw.bond_solver == BS.COLOURED and len(colour) > 0
        self._solver("coloured", "solver: coloured again")
        assert np.array_equal(self.tw.bond_colour, colour) and self.tw.solver_passes == 0

    def op_refuse_65_colours(self):
        """a star of 65 bonds on one live uid needs 65 colours: refused, the set held stays"""
        tw, rng = self.tw, self.rng
        assert tw.bond_solver == BS.COLOURED
        hub = int(rng.choice(tw.uids))
        star = BM.pairs(np.full(65, hub), rng.choice(tw.uids[tw.uids != hub], 65, replace=False), 3.0, 0.01)
        held = tw.bonds.copy()
        try:
            tw.set_bonds(star, 1)
            raise AssertionError("the twin took a set of 65 colours")
        except BS.Refused:
            pass
        assert tw.bonds.tobytes() == held.tobytes()
        if self.st is not None:
            try:
                self.st.set_bonds(star, 1)
                raise AssertionError("the context took a set of 65 colours")
            except self.gpe.GpeError as e:
                assert e.status == self.L.GPE_ERR_INVALID_ARG, e
        self.log.append("a star of 65 on uid %d: refused" % hub)
