"""GPU (-m gpu): the bonds' coloured solver (gpe_set_bond_solver / _get_bond_solver / _get_bond_solver_info,
csrc/k_bonds.hip k_bonds_colour and k_bonds_coloured, csrc/gpe_bonds.hip, csrc/bond_colours.h).

A coloured pass is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy
model (tests/_bond_solver_model.py: greedy colours in plain Python, the uids looked up afresh), the steps against the
composed twin of tests/_everything_model.py with the model's pass in the bonds' place.  Both launch forms are reached:
the info says which one a pass took.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red
zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _bond_solver_model as S
from tests import _bonds_model as BM
from tests import _everything_model as E

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
WORLD = S.WORLD
COLOUR_TAGS = {"uid.bond_order", "uid.bond_colour_start"}
# what a Jacobi context holds (tests/test_gpu_bonds.py BOND_TAGS)
BOND_TAGS = {"uid.bond_rec", "uid.bond_node_uid", "uid.bond_node_slot", "uid.bond_row_start", "uid.bond_inc",
             "uid.bond_corr", "uid.bond_state", "uid.bond_broken"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    """the same bits; where the model has a NaN the device has a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE


def _state(gpe, pos, rad, world=WORLD, mode="native", prev=None, gravity=(0.0, 0.0), solver="coloured"):
    st = gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=_mode(gpe, mode),
                   flags=gpe._lib.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    if solver:
        st.set_bond_solver(solver)
    return st


def _end(st):
    """every context ends here: no red zone of a live or a released buffer is damaged -> the live tags"""
    zones = st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0, zones
    tags = {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}
    st.close()
    return tags


def _rows(gpe, bonds):
    assert gpe.BOND_DTYPE == BM.BOND_DTYPE
    return np.ascontiguousarray(bonds, gpe.BOND_DTYPE)


def _passes(st, pos, rad, uids, bonds, iterations, passes, form=None):
    """`passes` calls of apply_bonds against the model: pos, the broken flags, bonds_info and the solver's info"""
    col = S.colours(bonds)
    colours, largest = S.colour_info(bonds)
    lds = st.bond_solver_info()["lds_nodes_max"]
    nodes = BM.node_count(bonds)
    want, broken = pos, np.zeros(len(bonds), bool)
    for p in range(passes):
        want, broken = S.apply(want, rad, uids, bonds, broken, iterations, WORLD, col)
        st.apply_bonds()
        got = st.positions()
        bad = np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(st.bonds()[1], broken), (p, np.nonzero(st.bonds()[1] != broken)[0][:10])
        assert st.bonds_info() == dict(iterations=iterations, k=len(bonds), nodes=nodes, passes=p + 1,
                                       live=len(bonds) - int(broken.sum()), broken=int(broken.sum()), resolves=1)
        info = st.bond_solver_info()
        assert info == dict(mode=S.COLOURED, colours=colours, largest_colour=largest, form=2 if nodes <= lds else 1,
                            lds_nodes_max=lds, passes=p + 1)
        assert form is None or info["form"] == form
    return want, broken


# ---- 1. the pass alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("n", [4000, 3999])
def test_one_pass_equals_the_model(gpe, n, iterations, mode):
    """apply_bonds() alone on the hostile scene, three passes: pos bit for bit as the model, prev and radius untouched,
    the broken flags, the counters and the colours the model's."""
    pos, rad, uids, bonds, third = S.hostile_scene(n)
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bonds(_rows(gpe, bonds), iterations)
    info = st.bond_solver_info()
    assert (info["mode"], info["form"], info["passes"]) == (S.COLOURED, 0, 0)
    assert S.HUB_DEGREE <= info["colours"] <= 64 and (info["colours"], info["largest_colour"]) == S.colour_info(bonds)
    want, broken = _passes(st, pos, rad, uids, bonds, iterations, 3)
    assert broken[third - 2] and broken[third] and 50 < broken.sum() < 1500      # the early break and the late one
    moved = (bits(want) != bits(pos)).any(axis=1)
    assert 1000 < moved.sum() < n - 20                                 # both outcomes
    assert same_bits(st.previous_positions(), prev) and same_bits(st.radii(), rad)
    assert st.bonds()[0].tobytes() == bonds.tobytes()
    tags = _end(st)
    assert BOND_TAGS | COLOUR_TAGS | {"uid.bond_max_length", "uid.bond_anchors"} <= tags


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 1025])
def test_the_tails_of_a_colour(gpe, k):
    """k bonds of the hostile scene: fewer than a wave, one wave exactly, one more, a block and one more (the
    one-workgroup form while they name at most lds_nodes_max particles), and 1025, which name more and take the
    per-colour form.  With lds_nodes_max = 1024 no colour of a one-workgroup pass exceeds its 1024 lanes: the second
    trip of that kernel's stride loop is reached by timing builds only and is not checked here."""
    pos, rad, uids, bonds, _ = S.hostile_scene(4000)
    bonds = bonds[np.random.default_rng(k).permutation(len(bonds))[:k]]
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_bonds(_rows(gpe, bonds), 2)
    want, _ = _passes(st, pos, rad, uids, bonds, 2, 1)
    assert not same_bits(want, pos)
    _end(st)


# ---- 2. both launch forms at the threshold -----------------------------------------------------------------------------
def chain_scene(m):
    """m particles along a serpentine of rows of 150, spacing 1.2 with a jitter, uid = 3 * index + 1; an anchor on the
    first and a bond of rest 1 and stiffness 1 between neighbours: m nodes, two colours"""
    rng = np.random.default_rng(m)
    i = np.arange(m)
    row, col = i // 150, i % 150
    col = np.where(row % 2 == 0, col, 149 - col)
    pos = (np.stack([5.0 + 1.2 * col, 5.0 + 1.2 * row], axis=1) + rng.uniform(-0.2, 0.2, (m, 2))).astype(F32)
    uids = (3 * i + 1).astype(U32)
    bonds = np.concatenate([BM.anchors([uids[0]], [(4.0, 4.0)], 1.0), BM.pairs(uids[:-1], uids[1:], 1.0, 1.0)])
    bonds["max_length"][5::97] = 1.25                                  # some break at once, some later, most never
    return pos, np.full(m, 0.5, F32), uids, bonds


def test_both_forms_at_the_threshold_give_the_models_bits(gpe):
    probe = _state(gpe, np.full((1, 2), 5.0, F32), np.full(1, 0.5, F32))
    lds = probe.bond_solver_info()["lds_nodes_max"]
    _end(probe)
    assert lds <= 8192
    sizes = [(lds, 2), (lds + 1, 1)] if lds >= 2 else [(2, 1)]
    for m, form in sizes:
        pos, rad, uids, bonds = chain_scene(m)
        assert BM.node_count(bonds) == m
        st = _state(gpe, pos, rad, prev=pos)
        st.set_uids(uids)
        st.set_bonds(_rows(gpe, bonds), 3)
        want, broken = _passes(st, pos, rad, uids, bonds, 3, 2, form=form)
        assert st.bond_solver_info()["colours"] == 2 and 0 < broken.sum() < len(bonds) // 50
        assert (bits(want) != bits(pos)).any(axis=1).sum() > m // 2
        _end(st)


def test_a_sheet_of_four_colours_on_the_per_colour_form(gpe):
    side = 96
    rng = np.random.default_rng(96)
    j, i = np.meshgrid(np.arange(side), np.arange(side))
    pos = (np.stack([10.0 + 1.25 * j.ravel(), 10.0 + 1.25 * i.ravel()], axis=1) + rng.uniform(-0.3, 0.3, (side * side, 2))).astype(F32)
    uid = (i * side + j).astype(U32)
    bonds = np.concatenate([BM.pairs(uid[:, :-1].ravel(), uid[:, 1:].ravel(), 1.25, 1.0),
                            BM.pairs(uid[:-1, :].ravel(), uid[1:, :].ravel(), 1.25, 1.0)])
    st = _state(gpe, pos, np.full(side * side, 0.5, F32), prev=pos)
    assert st.bond_solver_info()["lds_nodes_max"] < side * side
    st.set_bonds(_rows(gpe, bonds), 2)
    _passes(st, pos, np.full(side * side, 0.5, F32), np.arange(side * side, dtype=U32), bonds, 2, 2, form=1)
    assert st.bond_solver_info()["colours"] == 4
    _end(st)


# ---- 3. steps against the twin -----------------------------------------------------------------------------------------
ARMS = ("bends", "bonds", "bodies", "colliders")
STEPS_A, STEPS_B, STEPS_C = 15, 5, 40                                  # gpe_step, gpe_step after the edits, gpe_run
FALLER = E.RING_FIRST + E.RING + 2                                     # a member of the ring that starts above the lattice


def step_scene():
    """the composed twin's scene with one more bond: a tie of stiffness 0 from a falling ring member to where it
    starts, which breaks once the member is 1.5 away"""
    sc = E.scene()
    tie = BM.anchors([FALLER], [sc.pos[FALLER]], 0.0, 0.0, 1.5)
    return sc._replace(bonds=np.concatenate([sc.bonds, tie]))


def _edits(h, is_state):
    """a forced re-sort, a removal by circle, an add: the same calls on the State and on the twin"""
    add = np.stack([20.0 + 1.1 * np.arange(6), np.full(6, 3.0)], axis=1).astype(F32)
    if is_state:
        h.particles.sort_by_cell_id()
        gone = h.remove_particles_in_circle((22.5, 13.0), 1.2)         # inside the third ring: some of its members
        h.add_particles(add, np.full(6, 0.5, F32))
    else:
        h.morton_resort()
        gone = h.remove_circle(22.5, 13.0, 1.2)
        h.add(add, np.full(6, 0.5, F32))
    return gone


@pytest.fixture(scope="module")
def stepped(oracle):
    """the twin's particles and flags after every gpe_step, and after the run"""
    sc = step_scene()
    tw = S.everything_class()(oracle, sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev)
    tw.enable_uids()
    tw.set_bond_solver("coloured")
    E.arm(tw, sc, ARMS)
    frames = []

    def keep():
        pos, prev, _ = tw.arrays()
        frames.append((pos.copy(), prev.copy(), tw.uids.copy(), tw.broken.copy(), tw.bodies_broken.copy(), tw.bonds_info(),
                       tw.bond_solver_info()))
    for _ in range(STEPS_A):
        tw.step(DT)
        keep()
    tie_at_edits = bool(tw.broken[-1])
    gone = _edits(tw, False)
    for _ in range(STEPS_B):
        tw.step(DT)
        keep()
    tw.run(DT, STEPS_C, resort_every=16, resort_first=False)
    keep()
    assert gone > 0 and tw.broken[-1] and tw.broken.sum() >= 1
    tw.close()
    return sc, frames, gone, tie_at_edits


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_sixty_steps_equal_the_twin(gpe, stepped, mode):
    """gpe_step and gpe_run under gravity over the yard's floor with bends and bodies armed too (bends -> bonds ->
    bodies -> colliders), a re-sort, a removal and an add in between: the slots go stale and are resolved again, the
    tie breaks on the way."""
    sc, frames, gone, _ = stepped
    st = gpe.State(sc.pos, sc.rad, world=E.WORLD, gravity=E.GRAVITY, prev=sc.prev, mode=_mode(gpe, mode),
                   flags=gpe._lib.FLAG_GUARD_ALLOCS)
    st.enable_uids()
    st.set_bond_solver("coloured")
    E.arm(st, sc, ARMS)

    def same(f, what):
        pos, prev, uids, broken, bodies_broken, info, solver = f
        assert np.array_equal(st.uids(), uids), what
        assert same_bits(st.positions(), pos) and same_bits(st.previous_positions(), prev), what
        assert np.array_equal(st.bonds()[1], broken) and np.array_equal(st.bodies()[1], bodies_broken), what
        got = st.bonds_info()
        got.pop("resolves")
        assert got == info, what
        got = st.bond_solver_info()
        assert {k: got[k] for k in solver} == solver and got["form"] in (1, 2), what
    for s in range(STEPS_A):
        st.update(DT)
        same(frames[s], s)
    assert _edits(st, True) == gone
    for s in range(STEPS_A, STEPS_A + STEPS_B):
        st.update(DT)
        same(frames[s], s)
    st.run(DT, STEPS_C, resort_every=16, resort_first=False)
    same(frames[-1], "run")
    assert st.bonds_info()["resolves"] >= 3 and st.bonds()[1][-1]
    _end(st)


# ---- 4. off means off --------------------------------------------------------------------------------------------------
def test_back_to_jacobi_is_a_context_that_never_heard_of_the_mode(gpe):
    pos, rad, b = __import__("tests.test_gpu_bonds", fromlist=["cloth_scene"]).cloth_scene()
    b["stiffness"] = np.where(b["flags"] == 0, 0.25, b["stiffness"])
    world, gravity = (60.0, 60.0), (0.0, 100.0)
    plain = _state(gpe, pos, rad, world=world, gravity=gravity, solver=None)
    there = _state(gpe, pos, rad, world=world, gravity=gravity, solver="coloured")
    for st in (plain, there):
        st.set_bonds(_rows(gpe, b), 2)
        st.run(DT, 4, resort_every=0, resort_first=False)               # (the same history but for the solver)
    assert there.bond_solver_info()["passes"] == 4 and COLOUR_TAGS <= {t for t, _, _, s in there.ctx.guard_registry() if s == "live"}
    # back to Jacobi, the set given anew over the same particles: from here on the two contexts are one
    there.set_bond_solver("jacobi")
    assert there.bond_solver() == "jacobi" and there.bond_solver_info() == dict(
        mode=0, colours=0, largest_colour=0, form=0, lds_nodes_max=plain.bond_solver_info()["lds_nodes_max"], passes=0)
    assert np.array_equal(plain.uids(), there.uids())
    p, q = plain.positions(), plain.previous_positions()
    assert not same_bits(there.positions(), p)
    there.edit_particles(indices=np.arange(len(p), dtype=U32), positions=p, previous=q)
    for st in (plain, there):
        st.set_bonds(_rows(gpe, b), 2)
        st.ctx.set_profiling(True)
        st.ctx.reset_timings()
        st.run(DT, 10, resort_every=0, resort_first=False)
        st.update(DT)
        st.apply_bonds()
    for a, c in zip((plain.positions(), plain.previous_positions()), (there.positions(), there.previous_positions())):
        assert same_bits(a, c)
    for st in (plain, there):
        scopes = {name for name in st.ctx.timings() if name.startswith("bonds/")}
        assert scopes - {"bonds/resolve"} == {"bonds/bond", "bonds/node"}, scopes       # (the lookup after set_bonds)
    live = lambda st: {t for t, _, _, s in st.ctx.guard_registry() if s == "live"}
    assert not (COLOUR_TAGS & live(there)) and not (COLOUR_TAGS & live(plain))
    assert {t for t in live(there) if t.startswith("uid.bond_")} == {t for t in live(plain) if t.startswith("uid.bond_")}
    assert not any(t in COLOUR_TAGS for t, _, _, _ in plain.ctx.guard_registry())     # never allocated at all
    _end(plain)
    _end(there)


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------
def _rope(m=40):
    pos = np.stack([np.full(m, 30.0), 10.0 + 1.5 * np.arange(m)], axis=1).astype(F32)
    uid = np.arange(m, dtype=U32)
    bonds = np.concatenate([BM.anchors([0], [(30.0, 8.5)], 1.5), BM.pairs(uid[:-1], uid[1:], 1.5, 1.0)])
    return pos, np.full(m, 0.5, F32), bonds


def test_the_mode_is_step_state(gpe, tmp_path):
    L = gpe._lib
    pos, rad, bonds = _rope()
    world, gravity = (60.0, 120.0), (0.0, 100.0)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, solver=None)
    assert st.bond_solver() == "jacobi" and st.bond_solver_info()["colours"] == 0
    st.set_bond_solver("coloured")                                     # allowed with no set
    assert st.bond_solver() == "coloured" and st.bond_solver_info()["colours"] == 0
    assert not (COLOUR_TAGS & {t for t, _, _, _ in st.ctx.guard_registry()})
    st.set_bonds(_rows(gpe, bonds), 1)
    assert (st.bond_solver_info()["colours"], st.bond_solver_info()["largest_colour"]) == (2, 20)
    st.set_bonds(_rows(gpe, bonds[:-2]), 2)                            # survives gpe_set_bonds, the tables follow the set
    assert st.bond_solver() == "coloured" and st.bond_solver_info()["largest_colour"] == 19
    st.clear_bonds()
    assert st.bond_solver() == "coloured" and st.bond_solver_info()["colours"] == 0
    # ... and the other way round: the mode over a set held builds the tables from the kept set
    st.set_bond_solver("jacobi")
    st.set_bonds(_rows(gpe, bonds), 1)
    st.set_bond_solver("coloured")
    assert st.bond_solver_info()["colours"] == 2
    st.run(DT, 5, resort_every=0, resort_first=False)
    st.ctx.call("gpe_set_world", 70.0, 130.0)
    assert st.bond_solver() == "coloured"
    st.update(DT)
    assert st.bond_solver_info()["passes"] == 6
    # save / load: the key is there, the loaded context goes on with the same bits
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["bond_solver"].tolist() == [1]
        stripped = {k: d[k] for k in d.files if k != "bond_solver"}
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.bond_solver() == "coloured" and back.bond_solver_info()["colours"] == 2
    old = str(tmp_path / "old.npz")
    np.savez(old, **stripped)                                          # a file without the key: Jacobi
    jac = gpe.State.load(old, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert jac.bond_solver() == "jacobi" and len(jac.bonds()[0]) == len(bonds)
    for h in (st, back, jac):
        h.run(DT, 5, resort_every=0, resort_first=False)
    assert same_bits(st.positions(), back.positions()) and same_bits(st.previous_positions(), back.previous_positions())
    assert not same_bits(st.positions(), jac.positions())
    st.set_bond_solver("jacobi")
    st.save(path)
    with np.load(path) as d:
        assert "bond_solver" not in d.files
    for h in (st, back, jac):
        _end(h)


def test_every_refusal_leaves_the_set_the_mode_and_the_bits_untouched(gpe):
    L = gpe._lib
    lib = L.load()
    pos, rad, bonds = _rope()
    extra = np.stack([10.0 + 1.2 * (np.arange(70) % 35), 100.0 + 1.2 * (np.arange(70) // 35)], axis=1).astype(F32)
    pos, rad = np.concatenate([pos, extra]), np.concatenate([rad, np.full(70, 0.5, F32)])
    star = lambda d: BM.pairs(np.full(d, 40), 41 + np.arange(d), 3.0, 0.01)
    uids = np.arange(len(pos), dtype=U32)
    for held in ("coloured", "jacobi"):
        st = _state(gpe, pos, rad, world=(60.0, 120.0), solver=held)
        st.set_bonds(_rows(gpe, bonds), 2)
        info, solver = st.bonds_info(), st.bond_solver_info()

        def untouched(what):
            assert st.bond_solver() == held and st.bond_solver_info() == solver and st.bonds_info() == info, what
            assert st.bonds()[0].tobytes() == bonds.tobytes(), what
        h = st.ctx.h
        mode = C.c_uint32(7)
        short = L.GpeBondSolverInfo(struct_size=C.sizeof(L.GpeBondSolverInfo) - 8)
        assert lib.gpe_set_bond_solver(None, 1) == L.GPE_ERR_INVALID_ARG
        assert lib.gpe_get_bond_solver(None, C.byref(mode)) == L.GPE_ERR_INVALID_ARG and mode.value == 7
        for what, call in {"mode 2": lambda: lib.gpe_set_bond_solver(h, 2),
                           "mode 0xFFFFFFFF": lambda: lib.gpe_set_bond_solver(h, 0xFFFFFFFF),
                           "get: NULL mode": lambda: lib.gpe_get_bond_solver(h, None),
                           "info: NULL": lambda: lib.gpe_get_bond_solver_info(h, None),
                           "info: short struct_size": lambda: lib.gpe_get_bond_solver_info(h, C.byref(short))}.items():
            assert call() == L.GPE_ERR_INVALID_ARG, what
            untouched(what)
        # a star of 65 needs 65 colours: refused from gpe_set_bonds under the mode, and from the mode over the set
        if held == "coloured":
            st.set_bonds(_rows(gpe, np.concatenate([bonds[:3], star(64)])), 2)       # 64 fit
            assert st.bond_solver_info()["colours"] == 64
            st.set_bonds(_rows(gpe, bonds), 2)
            with pytest.raises(gpe.GpeError) as e:
                st.set_bonds(_rows(gpe, star(65)), 1)
        else:
            st.set_bonds(_rows(gpe, star(65)), 2)                      # Jacobi takes it
            bonds_held, info = star(65), st.bonds_info()
            with pytest.raises(gpe.GpeError) as e:
                st.set_bond_solver("coloured")
            assert st.bonds()[0].tobytes() == bonds_held.tobytes() and st.bond_solver() == "jacobi" and st.bonds_info() == info
            st.set_bonds(_rows(gpe, bonds), 2)
            info = st.bonds_info()
        assert e.value.status == L.GPE_ERR_INVALID_ARG and "65 colours" in str(e.value)
        untouched("65 colours")
        # the next pass is the model's for the set and the mode held
        st.apply_bonds()
        apply = S.apply if held == "coloured" else BM.apply
        want, _ = apply(pos, rad, uids, bonds, np.zeros(len(bonds), bool), 2, (60.0, 120.0))
        assert same_bits(st.positions(), want)
        tags = _end(st)
        assert (COLOUR_TAGS <= tags) if held == "coloured" else not (COLOUR_TAGS & tags)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_solver(gpe, how):
    L = gpe._lib
    pos, rad, _ = _rope()
    st = _state(gpe, pos, rad, world=(60.0, 120.0), solver=None)
    st.enable_uids(False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    for solver in ("coloured", "jacobi"):
        with pytest.raises(gpe.GpeError) as e:
            st.set_bond_solver(solver)
        assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert st.bond_solver() == "jacobi" and st.bond_solver_info()["passes"] == 0
    assert same_bits(st.positions(), pos)
    assert not (COLOUR_TAGS & _end(st))
