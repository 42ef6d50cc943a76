"""GPU (-m gpu): the bends' coloured solver (gpe_set_bend_solver / _get_bend_solver / _get_bend_solver_info,
csrc/k_bends.hip k_bends_colour and k_bends_coloured, csrc/gpe_bends.hip, csrc/bend_colours.h).

A coloured pass is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy
model (tests/_bend_solver_model.py: greedy colours in plain Python, the uids looked up afresh), the steps against the
bends' twin with the model's pass in the bends' place.  Both launch forms are reached: the info says which one a pass
took.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red zone."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _bend_solver_model as S
from tests import _bends_model as M
from tests import _bonds_model as BM

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
PI = math.pi
WORLD = S.WORLD
COLOUR_TAGS = {"uid.bend_order", "uid.bend_colour_start"}
# what a Jacobi context holds (tests/test_gpu_bends.py BEND_TAGS)
BEND_TAGS = {"uid.bend_rec", "uid.bend_node_uid", "uid.bend_node_slot", "uid.bend_row_start", "uid.bend_inc",
             "uid.bend_corr", "uid.bend_state"}


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
        st.set_bend_solver(solver)
    return st


def _live(st):
    return {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}


def _end(st):
    """every context ends here: no red zone of a live or a released buffer is damaged -> the live tags"""
    zones = st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0, zones
    tags = _live(st)
    st.close()
    return tags


def _rows(gpe, bends):
    assert gpe.BEND_DTYPE == M.BEND_DTYPE
    return np.ascontiguousarray(bends, gpe.BEND_DTYPE)


def _passes(st, pos, rad, uids, bends, iterations, passes, form=None):
    """`passes` calls of apply_bends against the model: pos, bends_info and the solver's info"""
    col = S.colours(bends)
    colours, largest = S.colour_info(bends)
    lds = st.bend_solver_info()["lds_nodes_max"]
    nodes = M.node_count(bends)
    want = pos
    for p in range(passes):
        want = S.apply(want, rad, uids, bends, iterations, WORLD, col)
        st.apply_bends()
        got = st.positions()
        bad = np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert st.bends_info() == dict(iterations=iterations, k=len(bends), nodes=nodes, passes=p + 1, resolves=1)
        info = st.bend_solver_info()
        assert info == dict(mode=S.COLOURED, colours=colours, largest_colour=largest, form=2 if nodes <= lds else 1,
                            lds_nodes_max=lds, passes=p + 1)
        assert form is None or info["form"] == form
    return want


# ---- 1. the pass alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostile():
    """the hostile scene and what three passes of the model make of it, per (n, iterations): computed once"""
    out = {}
    for n in (4000, 3999):
        scene = S.hostile_scene(n)
        col = S.colours(scene[3])
        for iterations in (1, 3):
            want, frames = scene[0], []
            for _ in range(3):
                want = S.apply(want, scene[1], scene[2], scene[3], iterations, WORLD, col)
                frames.append(want)
            out[n, iterations] = scene, frames
    return out


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("n", [4000, 3999])
def test_one_pass_equals_the_model(gpe, hostile, n, iterations, mode):
    """apply_bends() alone on the hostile scene, three passes on the per-colour form: pos bit for bit as the model, prev
    and radius untouched, the counters and the colours the model's."""
    (pos, rad, uids, bends), frames = hostile[n, iterations]
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), iterations)
    info = st.bend_solver_info()
    assert (info["mode"], info["form"], info["passes"]) == (S.COLOURED, 0, 0)
    assert S.HUB_DEGREE <= info["colours"] <= 64 and (info["colours"], info["largest_colour"]) == S.colour_info(bends)
    assert M.node_count(bends) > info["lds_nodes_max"]
    for p, want in enumerate(frames):
        st.apply_bends()
        got = st.positions()
        bad = np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert st.bend_solver_info()["form"] == 1 and st.bend_solver_info()["passes"] == p + 1
    assert st.bends_info() == dict(iterations=iterations, k=len(bends), nodes=M.node_count(bends), passes=3, resolves=1)
    moved = (bits(frames[-1]) != bits(pos)).any(axis=1)
    assert 1500 < moved.sum() < n - 20                                 # both outcomes
    assert same_bits(st.previous_positions(), prev) and same_bits(st.radii(), rad)
    assert st.bends().tobytes() == M.stored(bends).tobytes()
    assert BEND_TAGS | COLOUR_TAGS <= _end(st)


def triples_scene(k):
    """k bends over k disjoint triples (3 k particles, one colour): jittered corners on a 63-wide lattice of spacing 3,
    uids that are no storage indices, mixed rest angles and stiffnesses"""
    rng = np.random.default_rng(k)
    n = 3 * k
    i = np.arange(n)
    pos = (np.stack([5.0 + 3.0 * (i % 63), 5.0 + 3.0 * (i // 63)], axis=1) + rng.uniform(-0.5, 0.5, (n, 2))).astype(F32)
    uids = (rng.permutation(n).astype(np.uint64) * 13 + 5).astype(U32)
    t = rng.permutation(n).reshape(k, 3) if k < 64 else i.reshape(k, 3)
    bends = M.bends(uids[t[:, 0]], uids[t[:, 1]], uids[t[:, 2]], rng.choice(S.RESTS, k), rng.choice([0.25, 0.5, 1.0], k))
    return pos, np.full(n, 0.5, F32), uids, bends


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 342])
def test_the_tails_of_a_colour(gpe, k):
    """k bends over disjoint triples, all of one colour: fewer than a wave, one wave exactly, one more, a block and one
    more -- the one-workgroup form while they name at most lds_nodes_max particles -- and 342, which name 1026
    particles and take the per-colour form when the limit is 1024."""
    pos, rad, uids, bends = triples_scene(k)
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), 2)
    lds = st.bend_solver_info()["lds_nodes_max"]
    want = _passes(st, pos, rad, uids, bends, 2, 1, form=2 if 3 * k <= lds else 1)
    assert st.bend_solver_info()["colours"] == 1 and st.bend_solver_info()["largest_colour"] == k
    assert (bits(want) != bits(pos)).any(axis=1).sum() > 2 * k
    _end(st)


# ---- 2. both launch forms at the threshold -----------------------------------------------------------------------------
def chain_scene(m):
    """m particles along a serpentine of rows of 150, spacing 1.2 with a jitter, uid = 3 * index + 1; a bend of a
    straight rest and stiffness 1 at every inner particle, listed in order: m nodes, three colours"""
    rng = np.random.default_rng(m)
    i = np.arange(m)
    row, col = i // 150, i % 150
    col = np.where(row % 2 == 0, col, 149 - col)
    pos = (np.stack([5.0 + 1.2 * col, 5.0 + 1.2 * row], axis=1) + rng.uniform(-0.2, 0.2, (m, 2))).astype(F32)
    uids = (3 * i + 1).astype(U32)
    return pos, np.full(m, 0.5, F32), uids, M.bends(uids[:-2], uids[1:-1], uids[2:], PI, 1.0)


def test_both_forms_at_the_threshold_give_the_models_bits(gpe):
    probe = _state(gpe, np.full((1, 2), 5.0, F32), np.full(1, 0.5, F32))
    lds = probe.bend_solver_info()["lds_nodes_max"]
    _end(probe)
    assert lds <= 8192
    sizes = [(lds, 2), (lds + 1, 1)] if lds >= 3 else [(3, 1)]
    for m, form in sizes:
        pos, rad, uids, bends = chain_scene(m)
        assert M.node_count(bends) == m
        st = _state(gpe, pos, rad, prev=pos)
        st.set_uids(uids)
        st.set_bends(_rows(gpe, bends), 3)
        want = _passes(st, pos, rad, uids, bends, 3, 2, form=form)
        assert st.bend_solver_info()["colours"] == 3
        assert (bits(want) != bits(pos)).any(axis=1).sum() > m // 2
        _end(st)


def test_a_sheet_on_the_per_colour_form(gpe):
    side = 40
    rng = np.random.default_rng(side)
    j, i = np.meshgrid(np.arange(side), np.arange(side))
    pos = (np.stack([10.0 + 1.25 * j.ravel(), 10.0 + 1.25 * i.ravel()], axis=1) + rng.uniform(-0.3, 0.3, (side * side, 2))).astype(F32)
    uid = (i * side + j).astype(U32)
    t = np.concatenate([np.stack([uid[:, :-2].ravel(), uid[:, 1:-1].ravel(), uid[:, 2:].ravel()], axis=1),
                        np.stack([uid[:-2, :].ravel(), uid[1:-1, :].ravel(), uid[2:, :].ravel()], axis=1)])
    bends = M.bends(t[:, 0], t[:, 1], t[:, 2], PI, 1.0)
    rad = np.full(side * side, 0.5, F32)
    st = _state(gpe, pos, rad, prev=pos)
    assert st.bend_solver_info()["lds_nodes_max"] < side * side
    st.set_bends(_rows(gpe, bends), 2)
    _passes(st, pos, rad, np.arange(side * side, dtype=U32), bends, 2, 2, form=1)      # (colours, largest_colour: the model's)
    assert 3 <= st.bend_solver_info()["colours"] <= 16                 # (a particle sits in at most 6 bends: 3 * (6 - 1) + 1)
    _end(st)


# ---- 3. steps against the twin -----------------------------------------------------------------------------------------
SHEET, SHEET_REST = 16, 1.25
SHEET_WORLD, SHEET_GRAVITY = (60.0, 60.0), (0.0, 100.0)
STEPS_A, STEPS_B, STEPS_C = 15, 5, 40                                  # gpe_step, gpe_step after the edits, gpe_run


def sheet_scene():
    """a 16 x 16 sheet hanging from its two upper corners: bonds (Jacobi 0.25 x 4) and straight bends of stiffness 1
    along rows and columns; uid = row * 16 + column"""
    j, i = np.meshgrid(np.arange(SHEET), np.arange(SHEET))
    pos = np.stack([10.0 + SHEET_REST * j.ravel(), 4.0 + SHEET_REST * i.ravel()], axis=1).astype(F32)
    uid = (i * SHEET + j).astype(U32)
    bonds = np.concatenate([BM.anchors([0, SHEET - 1], pos[[0, SHEET - 1]], 0.0, 1.0),
                            BM.pairs(uid[:, :-1].ravel(), uid[:, 1:].ravel(), SHEET_REST, 0.25),
                            BM.pairs(uid[:-1, :].ravel(), uid[1:, :].ravel(), SHEET_REST, 0.25)])
    t = np.concatenate([np.stack([uid[:, :-2].ravel(), uid[:, 1:-1].ravel(), uid[:, 2:].ravel()], axis=1),
                        np.stack([uid[:-2, :].ravel(), uid[1:-1, :].ravel(), uid[2:, :].ravel()], axis=1)])
    return pos, np.full(SHEET * SHEET, 0.5, F32), bonds, M.bends(t[:, 0], t[:, 1], t[:, 2], PI, 1.0)


def _arm(h, rows_bends, rows_bonds):
    h.set_bend_solver("coloured")
    h.set_bends(rows_bends, 2)
    h.set_bonds(rows_bonds, 4)


def _edits(h, is_state):
    """a forced re-sort, a removal by circle, an add, an edit by uid: the same calls on the State and on the twin"""
    add = np.stack([40.0 + 1.1 * np.arange(6), np.full(6, 3.0)], axis=1).astype(F32)
    who = np.array([SHEET * SHEET - 1, SHEET * SHEET - 2, 999999], U32)    # the lower right corner, its neighbour, nobody
    where = np.array([[35.0, 20.0], [34.0, 21.0], [1.0, 1.0]], F32)
    if is_state:
        h.particles.sort_by_cell_id()
        gone = h.remove_particles_in_circle((20.0, 14.0), 1.5)         # a hole in the sheet: its bends go inert
        h.add_particles(add, np.full(6, 0.5, F32))
        assert h.edit_particles(uids=who, positions=where) == 2
    else:
        h.morton_resort()
        gone = h.remove_circle(20.0, 14.0, 1.5)
        h.add(add, np.full(6, 0.5, F32))
        assert h.edit(who, "uid", pos=where) == 2
    return gone


@pytest.fixture(scope="module")
def stepped(oracle):
    """the twin's particles after every gpe_step, and after the run"""
    pos, rad, bonds, bends = sheet_scene()
    tw = S.Twin(oracle, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY)
    tw.enable_uids()
    _arm(tw, bends, bonds)
    frames = []

    def keep():
        p, q, _ = tw.arrays()
        frames.append((p.copy(), q.copy(), tw.uids.copy(), tw.bends_info(), tw.bend_solver_info()))
    for _ in range(STEPS_A):
        tw.step(DT)
        keep()
    gone = _edits(tw, False)
    for _ in range(STEPS_B):
        tw.step(DT)
        keep()
    tw.run(DT, STEPS_C, resort_every=16, resort_first=False)
    keep()
    assert gone > 0
    tw.close()
    return frames, gone


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_sixty_steps_equal_the_twin(gpe, stepped, mode):
    """gpe_step and gpe_run under gravity with bonds behind the bends (bends -> bonds), a re-sort, a removal, an add and
    an edit in between: the slots go stale and are resolved again, the bends of removed particles go inert."""
    frames, gone = stepped
    pos, rad, bonds, bends = sheet_scene()
    st = _state(gpe, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY, mode=mode, solver=None)
    _arm(st, _rows(gpe, bends), np.ascontiguousarray(bonds, gpe.BOND_DTYPE))

    def same(f, what):
        p, q, uids, info, solver = f
        assert np.array_equal(st.uids(), uids), what
        assert same_bits(st.positions(), p) and same_bits(st.previous_positions(), q), what
        got = st.bends_info()
        got.pop("resolves")
        assert got == info, what
        got = st.bend_solver_info()
        assert {k: got[k] for k in solver} == solver and got["form"] == 2, what
    for s in range(STEPS_A):
        st.update(DT)
        same(frames[s], s)
    assert _edits(st, True) == gone
    for s in range(STEPS_A, STEPS_A + STEPS_B):
        st.update(DT)
        same(frames[s], s)
    st.run(DT, STEPS_C, resort_every=16, resort_first=False)
    same(frames[-1], "run")
    assert st.bends_info()["resolves"] >= 3 and st.bond_solver() == "jacobi"
    _end(st)


# ---- 4. off means off --------------------------------------------------------------------------------------------------
def test_back_to_jacobi_is_a_context_that_never_heard_of_the_mode(gpe):
    pos, rad, bonds, bends = sheet_scene()
    bends["stiffness"] = 0.3                                           # (a stiffness Jacobi holds)
    plain = _state(gpe, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY, solver=None)
    there = _state(gpe, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY, solver="coloured")
    for st in (plain, there):
        st.set_bends(_rows(gpe, bends), 2)
        st.set_bonds(np.ascontiguousarray(bonds, gpe.BOND_DTYPE), 4)
        st.run(DT, 4, resort_every=0, resort_first=False)               # (the same history but for the solver)
    assert there.bend_solver_info()["passes"] == 4 and COLOUR_TAGS <= _live(there)
    # back to Jacobi, the set given anew over the same particles: from here on the two contexts are one
    there.set_bend_solver("jacobi")
    assert there.bend_solver() == "jacobi" and there.bend_solver_info() == dict(
        mode=0, colours=0, largest_colour=0, form=0, lds_nodes_max=plain.bend_solver_info()["lds_nodes_max"], passes=0)
    assert there.bend_solver_info() == plain.bend_solver_info()
    assert not (COLOUR_TAGS & _live(there))                            # the colour tables are freed
    assert np.array_equal(plain.uids(), there.uids())
    p, q = plain.positions(), plain.previous_positions()
    assert not same_bits(there.positions(), p)
    there.edit_particles(indices=np.arange(len(p), dtype=U32), positions=p, previous=q)
    for st in (plain, there):
        st.set_bends(_rows(gpe, bends), 2)
        st.ctx.set_profiling(True)
        st.ctx.reset_timings()
        st.run(DT, 10, resort_every=0, resort_first=False)
        st.update(DT)
        st.apply_bends()
    for a, c in zip((plain.positions(), plain.previous_positions()), (there.positions(), there.previous_positions())):
        assert same_bits(a, c)
    for st in (plain, there):
        scopes = {name for name in st.ctx.timings() if name.startswith("bends/")}
        assert scopes - {"bends/resolve"} == {"bends/bend", "bends/node"}, scopes       # (the lookup after set_bends)
    assert there.bends_info() == plain.bends_info() and there.bend_solver_info() == plain.bend_solver_info()
    assert not (COLOUR_TAGS & _live(there)) and not (COLOUR_TAGS & _live(plain))
    assert {t for t in _live(there) if t.startswith("uid.bend_")} == {t for t in _live(plain) if t.startswith("uid.bend_")}
    assert not any(t in COLOUR_TAGS for t, _, _, _ in plain.ctx.guard_registry())     # never allocated at all
    _end(plain)
    _end(there)


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------
def _blade(m=40):
    """a blade of m particles standing on the floor of a 60 x 120 world, bent a little"""
    i = np.arange(m)
    pos = np.stack([30.0 + 0.01 * i * i, 110.0 - 1.5 * i], axis=1).astype(F32)
    uid = np.arange(m, dtype=U32)
    return pos, np.full(m, 0.5, F32), M.bends(uid[:-2], uid[1:-1], uid[2:], PI, 1.0)


def _hub(d, first=41):
    """a hinge (uid 40) shared by d bends with otherwise distinct ends"""
    return M.bends(first + 2 * np.arange(d), np.full(d, 40), first + 1 + 2 * np.arange(d), PI, 0.01)


def test_the_mode_is_step_state(gpe, tmp_path):
    L = gpe._lib
    pos, rad, bends = _blade()
    world, gravity = (60.0, 120.0), (0.0, 100.0)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, solver=None)
    assert st.bend_solver() == "jacobi" and st.bend_solver_info()["colours"] == 0
    st.set_bend_solver("coloured")                                     # allowed with no set
    assert st.bend_solver() == "coloured" and st.bend_solver_info()["colours"] == 0
    assert not (COLOUR_TAGS & {t for t, _, _, _ in st.ctx.guard_registry()})
    st.set_bends(_rows(gpe, bends), 1)
    assert (st.bend_solver_info()["colours"], st.bend_solver_info()["largest_colour"]) == (3, 13)
    st.set_bends(_rows(gpe, bends[:-2]), 2)                            # survives gpe_set_bends, the tables follow the set
    assert st.bend_solver() == "coloured" and st.bend_solver_info()["largest_colour"] == 12
    st.clear_bends()
    assert st.bend_solver() == "coloured" and st.bend_solver_info()["colours"] == 0
    # ... and the other way round: the mode over a set held builds the tables from the kept set
    st.set_bend_solver("jacobi")
    st.set_bends(_rows(gpe, bends), 1)
    st.set_bend_solver("coloured")
    assert st.bend_solver_info()["colours"] == 3 and st.bond_solver() == "jacobi"    # (the bonds' mode is another one)
    st.run(DT, 5, resort_every=0, resort_first=False)
    st.ctx.call("gpe_set_world", 70.0, 130.0)
    assert st.bend_solver() == "coloured"
    st.update(DT)
    assert st.bend_solver_info()["passes"] == 6
    # save / load: the key is there, the loaded context goes on with the same bits
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["bend_solver"].tolist() == [1] and "bond_solver" not in d.files
        stripped = {k: d[k] for k in d.files if k != "bend_solver"}
    back = gpe.State.load(path, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert back.bend_solver() == "coloured" and back.bend_solver_info()["colours"] == 3
    old = str(tmp_path / "old.npz")
    np.savez(old, **stripped)                                          # a file without the key: Jacobi
    jac = gpe.State.load(old, mode=L.MODE_NATIVE, flags=L.FLAG_GUARD_ALLOCS)
    assert jac.bend_solver() == "jacobi" and len(jac.bends()) == len(bends)
    for h in (st, back, jac):
        h.run(DT, 5, resort_every=0, resort_first=False)
    assert same_bits(st.positions(), back.positions()) and same_bits(st.previous_positions(), back.previous_positions())
    assert not same_bits(st.positions(), jac.positions())
    st.set_bend_solver("jacobi")
    st.save(path)
    with np.load(path) as d:
        assert "bend_solver" not in d.files
    st.set_bend_solver("coloured")                                     # a coloured mode without bends is not written
    st.clear_bends()
    st.save(path)
    with np.load(path) as d:
        assert "bend_solver" not in d.files and "bends" not in d.files
    for h in (st, back, jac):
        _end(h)


def test_every_refusal_leaves_the_set_the_mode_and_the_bits_untouched(gpe):
    L = gpe._lib
    lib = L.load()
    pos, rad, bends = _blade()
    extra = np.stack([5.0 + 1.2 * (np.arange(140) % 40), 10.0 + 1.2 * (np.arange(140) // 40)], axis=1).astype(F32)
    pos, rad = np.concatenate([pos, extra]), np.concatenate([rad, np.full(140, 0.5, F32)])
    uids = np.arange(len(pos), dtype=U32)
    for held in ("coloured", "jacobi"):
        st = _state(gpe, pos, rad, world=(60.0, 120.0), solver=held)
        st.set_bends(_rows(gpe, bends), 2)
        info, solver = st.bends_info(), st.bend_solver_info()

        def untouched(what):
            assert st.bend_solver() == held and st.bend_solver_info() == solver and st.bends_info() == info, what
            assert st.bends().tobytes() == bends.tobytes(), what
            assert same_bits(st.positions(), pos), what
        h = st.ctx.h
        mode = C.c_uint32(7)
        short = L.GpeBendSolverInfo(struct_size=C.sizeof(L.GpeBendSolverInfo) - 8)
        assert lib.gpe_set_bend_solver(None, 1) == L.GPE_ERR_INVALID_ARG
        assert lib.gpe_get_bend_solver(None, C.byref(mode)) == L.GPE_ERR_INVALID_ARG and mode.value == 7
        for what, call in {"mode 2": lambda: lib.gpe_set_bend_solver(h, 2),
                           "mode 0xFFFFFFFF": lambda: lib.gpe_set_bend_solver(h, 0xFFFFFFFF),
                           "get: NULL mode": lambda: lib.gpe_get_bend_solver(h, None),
                           "info: NULL": lambda: lib.gpe_get_bend_solver_info(h, None),
                           "info: short struct_size": lambda: lib.gpe_get_bend_solver_info(h, C.byref(short))}.items():
            assert call() == L.GPE_ERR_INVALID_ARG, what
            untouched(what)
        with pytest.raises(ValueError):
            st.set_bend_solver("gauss")
        # a hinge of 65 bends needs 65 colours: refused from gpe_set_bends under the mode, and from the mode over the set
        if held == "coloured":
            st.set_bends(_rows(gpe, np.concatenate([bends[:3], _hub(64)])), 2)       # 64 fit
            assert st.bend_solver_info()["colours"] == 64
            st.set_bends(_rows(gpe, bends), 2)
            with pytest.raises(gpe.GpeError) as e:
                st.set_bends(_rows(gpe, _hub(65)), 1)
        else:
            st.set_bends(_rows(gpe, _hub(65)), 2)                      # Jacobi takes it
            held_info = st.bends_info()
            with pytest.raises(gpe.GpeError) as e:
                st.set_bend_solver("coloured")
            assert st.bends().tobytes() == _hub(65).tobytes() and st.bend_solver() == "jacobi" and st.bends_info() == held_info
            assert not (COLOUR_TAGS & _live(st))
            st.set_bends(_rows(gpe, bends), 2)
        assert e.value.status == L.GPE_ERR_INVALID_ARG and "65 colours" in str(e.value)
        untouched("65 colours")
        # the next pass is the model's for the set and the mode held
        st.apply_bends()
        if held == "coloured":
            want = S.apply(pos, rad, uids, bends, 2, (60.0, 120.0))
        else:
            want = M.apply(pos, rad, uids, bends, 2, (60.0, 120.0))
        assert same_bits(st.positions(), want) and not same_bits(want, pos)
        tags = _end(st)
        assert (COLOUR_TAGS <= tags) if held == "coloured" else not (COLOUR_TAGS & tags)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_solver(gpe, how):
    L = gpe._lib
    pos, rad, _ = _blade()
    st = _state(gpe, pos, rad, world=(60.0, 120.0), solver=None)
    st.enable_uids(False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    for solver in ("coloured", "jacobi"):
        with pytest.raises(gpe.GpeError) as e:
            st.set_bend_solver(solver)
        assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert st.bend_solver() == "jacobi" and st.bend_solver_info()["passes"] == 0
    assert same_bits(st.positions(), pos)
    assert not (COLOUR_TAGS & _end(st))
