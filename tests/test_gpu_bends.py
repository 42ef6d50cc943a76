"""GPU (-m gpu): bend constraints (gpe_set_bends / _get_bends / _apply_bends / _get_bends_info, csrc/k_bends.hip,
csrc/gpe_bends.hip, csrc/bend_graph.h).

A relaxation is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy
model (tests/_bends_model.py: no graph, the uids looked up afresh), and the steps against the CPU oracle with the
model's bends, bonds and colliders passes behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends
with no damaged red zone."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _bends_model as M
from tests import _bonds_model as BM
from tests._oracle_model import circle_mask

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
NAN, INF = float("nan"), float("inf")
PI = math.pi
WORLD = (200.0, 200.0)
ABSENT = M.UID_ABSENT
BEND_TAGS = {"uid.bend_rec", "uid.bend_node_uid", "uid.bend_node_slot", "uid.bend_row_start", "uid.bend_inc",
             "uid.bend_corr", "uid.bend_state"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE


def _state(gpe, pos, rad, world=WORLD, mode="native", prev=None, gravity=(0.0, 0.0), flags=0, uids=True, **kw):
    st = gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=_mode(gpe, mode),
                   flags=gpe._lib.FLAG_GUARD_ALLOCS | flags, **kw)
    if uids:
        st.enable_uids()
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


def _rows(gpe, bends):
    """the model's rows as the engine's (the same layout)"""
    assert gpe.BEND_DTYPE == M.BEND_DTYPE
    return np.ascontiguousarray(bends, gpe.BEND_DTYPE)


def _bond_rows(gpe, bonds):
    return np.ascontiguousarray(bonds, gpe.BOND_DTYPE)


def _info(st):
    info = st.bends_info()
    info.pop("resolves")
    return info


def _same_as_twin(st, tw, what, by_uid=False):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    if by_uid:
        a, b = np.argsort(st.uids()), np.argsort(tw.uids)
        assert np.array_equal(st.uids()[a], tw.uids[b]), what
        got, (pos, prev, rad) = [x[a] for x in got], [x[b] for x in (pos, prev, rad)]
    elif tw.uids is not None:
        assert np.array_equal(st.uids(), tw.uids), what
    bad = np.nonzero((bits(got[0]) != bits(pos)).any(axis=1))[0] if got[0].shape == pos.shape else "shape"
    assert same_bits(got[0], pos), (what, bad[:5], got[0][bad[:5]], pos[bad[:5]])
    assert same_bits(got[1], prev) and same_bits(got[2], rad), what
    assert st.bends().tobytes() == tw.bends.tobytes(), what
    assert _info(st) == tw.bends_info(), what
    rec, broken = st.bonds()
    assert rec.tobytes() == tw.bonds.tobytes() and np.array_equal(broken, tw.broken), what


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
RESTS = np.array([PI, -PI, PI / 2, -PI / 2, 0.3, -2.5, 0.0, 3.0])


def _pass_scene(n):
    """n particles on a jittered 64-wide lattice of spacing 3 with uids that are no storage indices, and about 2 n
    bends: triples along rows and columns and round corners with mixed rest angles (most are more than 90 degrees off
    theirs), a triple listed twice, uids no particle has, a NaN particle, a coincident pair, inf and 1e20 positions, a
    corner that opens across the world's edge.  The last 40 storage slots hold the particles with a special role."""
    rng = np.random.default_rng(n)
    full = 4000
    i = np.arange(full)
    pos = np.stack([4.0 + 3.0 * (i % 64), 4.0 + 3.0 * (i // 64)], axis=1) + rng.uniform(-0.4, 0.4, (full, 2))
    pos = pos.astype(F32)
    rad = np.full(full, 0.5, F32)
    uids = (rng.permutation(full).astype(np.uint64) * 7919 + 11).astype(U32)     # distinct, far above n, unordered
    s = full - 40
    u = lambda slot: uids[np.asarray(slot)]
    parts = []

    def triples(a, b, c, stiffness=None):
        k = len(a)
        st = rng.choice([0.0, 0.1, 0.25, 0.5, 1.0], k) if stiffness is None else stiffness
        return M.bends(u(a), u(b), u(c), rng.choice(RESTS, k), st)

    a = rng.integers(0, s - 130, 7600)
    a = a[(a % 64) < 62]
    kind = rng.integers(0, 3, len(a))
    b = np.where(kind == 0, a + 1, np.where(kind == 1, a + 64, a))
    c = np.where(kind == 0, a + 2, np.where(kind == 1, a + 128, a + 64))
    a2 = np.where(kind == 2, a + 1, a)
    parts.append(triples(a2, b, c))
    parts.append(np.repeat(triples([s + 0], [s + 1], [s + 2], 0.25), 2))            # the same bend twice
    parts.append(M.bends([u(7), 0xFFFFFFF0, u(3)], [0xFFFFFFF0, u(8), u(5)], [u(9), u(10), 0xFFFFFFF1], PI, 1.0))
    pos[s + 4] = (NAN, 100.0)
    pos[s + 6] = pos[s + 5]                                                        # coincident centres
    pos[s + 7], pos[s + 8] = (INF, 50.0), (1e20, 50.0)
    parts.append(triples([s + 4, 20, 21, s + 5, 22, s + 7, 23], [24, s + 4, 25, s + 6, s + 5, 26, s + 8],
                         [27, 28, s + 4, 29, s + 6, 30, 31], 1.0))
    # a right angle at the world's corner with a straight rest: a and c are pushed out across the edge, and clamped
    pos[s + 10], pos[s + 11], pos[s + 12] = (2.75, 199.25), (0.75, 199.25), (0.75, 197.25)
    flat = M.bends([u(s + 10)], [u(s + 11)], [u(s + 12)], PI, 1.0)
    flat["rest_sin"] = -0.0                                                        # (the exact (-1, 0); -0.0 is stored as +0)
    parts.append(flat)
    parts.append(triples([full - 1], [40], [41], 0.5))                              # (absent when n = 3999)
    bends = np.concatenate(parts)
    return pos[:n], rad[:n], uids[:n], bends


def _check_passes(st, pos, prev, rad, uids, bends, iterations, passes, k_resolves=1):
    want = pos
    for p in range(passes):
        want = M.apply(want, rad, uids, bends, iterations, WORLD)
        st.apply_bends()
        got, got_prev, got_rad = _arrays(st)
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert same_bits(got_prev, prev) and same_bits(got_rad, rad)
        assert st.bends_info() == dict(iterations=iterations, k=len(bends), nodes=M.node_count(bends), passes=p + 1,
                                       resolves=k_resolves)
    return want


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("n", [4000, 3999])
def test_one_pass_equals_the_model(gpe, n, iterations, mode):
    """apply_bends() alone, two passes: pos bit for bit as the model, prev and radius untouched, the counters the model's"""
    pos, rad, uids, bends = _pass_scene(n)
    assert 1.7 * n < len(bends) < 2.1 * n
    acts, s = M.corrections(pos, uids, bends)[:2]
    assert (np.abs(s[acts]) == 1).sum() > 1000 and (np.abs(s[acts]) < 1).sum() > 1000 and 10 <= (~acts).sum() < 40
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), iterations)
    assert st.bends().tobytes() == M.stored(bends).tobytes()
    want = _check_passes(st, pos, prev, rad, uids, bends, iterations, 2)
    moved = (bits(want) != bits(pos)).any(axis=1)
    assert 2000 < moved.sum() < n - 5                                  # both outcomes
    assert same_bits(want[3964:3969], pos[3964:3969])                  # NaN, coincident, inf, 1e20: every bit kept
    first = M.relax(pos, rad, uids, bends, WORLD)[0]
    assert first[3970, 1] == 199.5 and first[3972, 0] == 0.5           # across the edge: clamped
    tags = _end(st)
    assert BEND_TAGS <= tags


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
def test_one_pass_on_three_particles_with_one_bend(gpe, iterations, mode):
    pos = np.array([[12.0, 10.0], [10.0, 10.0], [10.5, 12.0]], F32)
    rad = np.array([0.5, 0.75, 0.25], F32)
    uids = np.array([40, 7, 1000000], U32)
    bends = M.bends([40], [7], [1000000], 2.0, 0.5)
    prev = (pos + F32(1)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), iterations)
    want = _check_passes(st, pos, prev, rad, uids, bends, iterations, 2)
    assert (bits(want) != bits(pos)).any(axis=1).all()
    _end(st)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_the_tails_of_both_phases(gpe, k):
    """k bends on 4000 particles: fewer than a wave, one wave exactly, one more, a block and one more"""
    pos, rad, uids, bends = _pass_scene(4000)
    bends = bends[np.random.default_rng(k).permutation(len(bends))[:k]]
    bends["stiffness"][0] = 0.5                                        # (the first one moves its particles for sure)
    assert M.corrections(pos, uids, bends)[0][0]
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), 2)
    want = _check_passes(st, pos, pos, rad, uids, bends, 2, 1)
    assert not same_bits(want, pos)
    _end(st)


def test_a_hub_of_the_largest_degree(gpe):
    """one particle in GPE_BEND_MAX_DEGREE bends, in every role: one lane adds 1024 shares in ascending bend index"""
    L = gpe._lib
    pos, rad, uids, _ = _pass_scene(4000)
    d = L.BEND_MAX_DEGREE
    rng = np.random.default_rng(4)
    others = rng.permutation(np.arange(1, 3900))[:2 * d].reshape(d, 2)
    t = np.zeros((d, 3), np.int64)
    for j in range(d):
        t[j] = np.insert(others[j], j % 3, 0)                          # the hub is a, then the hinge, then c
    bends = M.bends(uids[t[:, 0]], uids[t[:, 1]], uids[t[:, 2]], rng.choice(RESTS, d), 0.01)
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_bends(_rows(gpe, bends), 2)
    want = _check_passes(st, pos, pos, rad, uids, bends, 2, 1)
    assert not same_bits(want[0], pos[0]) and st.bends_info()["nodes"] == 2 * d + 1
    _end(st)


# ---- 2. the hook: a sheet above a floor -----------------------------------------------------------------------------
SHEET, SHEET_REST = 32, 1.25
SHEET_WORLD, SHEET_GRAVITY = (60.0, 60.0), (0.0, 100.0)
SHEET_COLLIDERS = np.array([[-5, 52, 65, 52, 5], [30, 30, 30, 30, 4]], F32)    # a floor and a disc in the sheet's way
BOND_ITERATIONS, BEND_ITERATIONS = 4, 2
STEPS = 40


def sheet_scene():
    """a 32 x 32 sheet hanging from its two upper corners, bonds and bends along rows and columns; uid = row * 32 + column"""
    j, i = np.meshgrid(np.arange(SHEET), np.arange(SHEET))
    pos = np.stack([10.0 + SHEET_REST * j.ravel(), 4.0 + SHEET_REST * i.ravel()], axis=1).astype(F32)
    uid = (i * SHEET + j)
    right = BM.pairs(uid[:, :-1].ravel(), uid[:, 1:].ravel(), SHEET_REST, 0.25)
    down = BM.pairs(uid[:-1, :].ravel(), uid[1:, :].ravel(), SHEET_REST, 0.25)
    pins = BM.anchors([0, SHEET - 1], pos[[0, SHEET - 1]], 0.0, 1.0)
    triples = np.concatenate([np.stack([uid[:, :-2].ravel(), uid[:, 1:-1].ravel(), uid[:, 2:].ravel()], axis=1),
                              np.stack([uid[:-2, :].ravel(), uid[1:-1, :].ravel(), uid[2:, :].ravel()], axis=1)])
    bends = M.captured(pos, np.arange(SHEET * SHEET, dtype=U32), triples, 0.3)
    return pos, np.full(SHEET * SHEET, 0.5, F32), np.concatenate([pins, right, down]), bends, triples


def sheet_twin(oracle, bends=True, bonds=True, colliders=True):
    pos, rad, b, bd, _ = sheet_scene()
    tw = M.Twin(oracle, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY)
    tw.enable_uids()
    if bends:
        tw.set_bends(bd, BEND_ITERATIONS)
    if bonds:
        tw.set_bonds(b, BOND_ITERATIONS)
    if colliders:
        tw.set_colliders(SHEET_COLLIDERS)
    return tw


def sheet_state(gpe, mode="native", bends=True, bonds=True, colliders=True, shuffle=None, **kw):
    pos, rad, b, bd, _ = sheet_scene()
    if shuffle is not None:
        st = _state(gpe, pos[shuffle], rad[shuffle], world=SHEET_WORLD, gravity=SHEET_GRAVITY, mode=mode, **kw)
        st.set_uids(shuffle.astype(U32))
    else:
        st = _state(gpe, pos, rad, world=SHEET_WORLD, gravity=SHEET_GRAVITY, mode=mode, **kw)
    if bends:
        st.set_bends(_rows(gpe, bd), BEND_ITERATIONS)
    if bonds:
        st.set_bonds(_bond_rows(gpe, b), BOND_ITERATIONS)
    if colliders:
        st.set_colliders(SHEET_COLLIDERS)
    return st


def _frames(tw, steps, resort_every=0, resort_first=False):
    frames = []
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(DT, resort=bool(resort))
        pos, prev, _ = tw.arrays()
        frames.append((pos.copy(), prev.copy(), tw.uids.copy()))
    return frames


@pytest.fixture(scope="module")
def sheet(oracle):
    """the reference of the hook tests: oracle step -> model bends -> model bonds -> model colliders, 40 steps"""
    tw = sheet_twin(oracle)
    frames = _frames(tw, STEPS)
    info, pushed = tw.bends_info(), tw.pushed
    tw.close()
    assert pushed > 0 and np.isfinite(frames[-1][0]).all()
    return frames, info, pushed


@pytest.fixture(scope="module")
def sheet_resorted(oracle):
    tw = sheet_twin(oracle)
    frames = _frames(tw, STEPS, resort_every=16, resort_first=True)
    info = tw.bends_info()
    tw.close()
    return frames, info


@pytest.fixture(scope="module")
def sheet_without_bends(oracle):
    tw = sheet_twin(oracle, bends=False)
    frames = _frames(tw, 20)
    tw.close()
    return frames


def test_the_sheets_bends_are_the_angles_it_holds(gpe, sheet, sheet_without_bends):
    """State.bends_from_positions captures what the model captures; and the bends do change the run"""
    pos, rad, _, bd, triples = sheet_scene()
    st = _state(gpe, pos, rad, world=SHEET_WORLD)
    rows = st.bends_from_positions(triples, 0.3)
    assert rows.tobytes() == bd.tobytes()
    assert np.array_equal(rows["rest_cos"], np.full(len(rows), -1, F32)) and (np.abs(rows["rest_sin"]) < 1e-6).all()
    by_angle = gpe.bends_from_angles(triples[:, 0], triples[:, 1], triples[:, 2], PI, 0.3)
    assert by_angle.tobytes() == M.bends(triples[:, 0], triples[:, 1], triples[:, 2], PI, 0.3).tobytes()
    with pytest.raises(ValueError):
        st.bends_from_positions([[0, 1, 5000]], 0.3)
    _end(st)
    assert not same_bits(sheet[0][19][0], sheet_without_bends[19][0])


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_twin(gpe, sheet, mode):
    frames, info, pushed = sheet
    L = gpe._lib
    st = sheet_state(gpe, mode)
    for s in range(STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    assert _info(st) == info and st.bends_info()["resolves"] == 1 and st.colliders_info()["pushed"] == pushed
    pipe = st.ctx.pipeline_info()
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == STEPS
    else:
        assert pipe["compat_steps"] == STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_twin_and_the_observers_see_the_result(gpe, sheet, mode):
    frames, info, pushed = sheet
    st = sheet_state(gpe, mode)
    uids = np.array([0, 31, 300, 1023, 12], U32)
    st.tracers_begin(uids, every=1, frames=64, prev=True)
    st.monitor_begin(every=1, frames=64)
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
    assert _info(st) == info and st.colliders_info()["pushed"] == pushed
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == STEPS and recorded == STEPS
    for s in range(STEPS):                                             # frames taken behind all three passes
        p, q = frames[s][0], frames[s][1]
        assert same_bits(tr.pos[s], p[uids]) and same_bits(tr.prev[s], q[uids]), s
        assert rec["max_y"][s] == p[:, 1].max() and rec["min_y"][s] == p[:, 1].min() and rec["n"][s] == SHEET * SHEET
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 3. re-sorts and storage order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_resorts_and_shuffled_storage_keep_the_bends_on_their_particles(gpe, sheet, sheet_resorted, mode):
    frames, info = sheet_resorted

    def by_uid(st, want):
        a, b = np.argsort(st.uids()), np.argsort(want[2])
        pos, prev, _ = _arrays(st)
        assert same_bits(pos[a], want[0][b]) and same_bits(prev[a], want[1][b])

    st = sheet_state(gpe, mode)
    st.run(DT, STEPS, resort_every=16, resort_first=True)
    by_uid(st, frames[STEPS - 1])
    assert not np.array_equal(st.uids(), np.arange(SHEET * SHEET))     # the re-sorts did move the particles
    assert _info(st) == info and st.bends_info()["resolves"] == 3      # before steps 0, 16, 32
    _end(st)
    # a re-sort in the middle, step by step: the uids are looked up again only on the step after it
    st = sheet_state(gpe, mode)
    for s in range(20):
        st.update(DT, resort=(s % 16 == 0))
        assert st.bends_info()["resolves"] == 1 + s // 16, s
        if s in (0, 15, 16, 17, 19):
            by_uid(st, frames[s])
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_particles_shuffled_in_storage_keep_their_bends(gpe, oracle, sheet, mode):
    """the uids kept, the storage order not.  The passes depend on the uids alone: per uid they give the bits of the
    unshuffled sheet.  (The collision solve of the step visits particles in storage order, so whole steps are compared
    with a twin that is shuffled the same way.)"""
    shuffle = np.random.default_rng(9).permutation(SHEET * SHEET)
    st, plain = sheet_state(gpe, mode, shuffle=shuffle), sheet_state(gpe, mode)
    for ctx in (st, plain):
        ctx.run(DT, 5, resort_every=0, resort_first=False)             # (bent by now)
    where, prev = plain.positions(), plain.previous_positions()
    st.edit_particles(uids=np.arange(SHEET * SHEET, dtype=U32), positions=where, previous=prev)
    for ctx in (st, plain):
        ctx.apply_bends(); ctx.apply_colliders(); ctx.apply_bends()
    a = np.argsort(st.uids())
    assert np.array_equal(st.uids()[a], plain.uids())
    assert same_bits(st.positions()[a], plain.positions()) and not same_bits(plain.positions(), where)
    _end(st); _end(plain)
    pos, rad, b, bd, _ = sheet_scene()
    tw = M.Twin(oracle, pos[shuffle], rad[shuffle], world=SHEET_WORLD, gravity=SHEET_GRAVITY)
    tw.enable_uids(); tw.set_uids(shuffle.astype(U32))
    tw.set_bends(bd, BEND_ITERATIONS); tw.set_bonds(b, BOND_ITERATIONS); tw.set_colliders(SHEET_COLLIDERS)
    st = sheet_state(gpe, mode, shuffle=shuffle)
    for s in range(12):
        st.update(DT, resort=(s == 6)); tw.step(DT, resort=(s == 6))
        _same_as_twin(st, tw, s)
    tw.close()
    _end(st)


# ---- 4. the order of the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_step_is_the_module_calls_then_bends_then_bonds_then_colliders(gpe, sheet, mode):
    frames = sheet[0]
    st = sheet_state(gpe, mode)
    for s in range(6):
        st.grid.build_cell_ids(); st.grid.sort_map(); st.collision_system.solve_collisions()
        st.particles.update_positions(DT)
        before = st.positions()
        st.apply_bends()
        bent = st.positions()
        st.apply_bonds()
        st.apply_colliders()
        assert same_bits(st.positions(), frames[s][0]) and same_bits(st.previous_positions(), frames[s][1]), s
        assert not same_bits(before, bent) or s == 0
    assert st.bends_info()["passes"] == 6
    # ... and in no other order: bonds in front of the bends gives other bits
    other = sheet_state(gpe, mode)
    for s in range(6):
        other.grid.build_cell_ids(); other.grid.sort_map(); other.collision_system.solve_collisions()
        other.particles.update_positions(DT)
        other.apply_bonds(); other.apply_bends(); other.apply_colliders()
    assert not same_bits(other.positions(), frames[5][0])
    _end(st); _end(other)


# ---- 5. no bends, no trace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_bends_nothing_changes_and_nothing_is_launched(gpe, sheet, sheet_without_bends, mode):
    never = sheet_state(gpe, mode, bends=False, profiling=True)
    cleared = sheet_state(gpe, mode, profiling=True)
    cleared.clear_bends()
    empty = dict(iterations=0, k=0, nodes=0, passes=0, resolves=0)
    for st in (never, cleared):
        assert len(st.bends()) == 0 and st.bends_info() == empty
        st.ctx.reset_timings()
        st.apply_bends()                                               # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, sheet_without_bends[19][0]) and same_bits(prev, sheet_without_bends[19][1])
        assert not any(name == "Bends" or name.startswith("bends/") for name in st.ctx.timings())
        assert not any(t.startswith("uid.bend_") for t, _, _, state in st.ctx.guard_registry() if state == "live")
        _end(st)
    armed = sheet_state(gpe, mode, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), sheet[0][19][0])
    t = armed.ctx.timings()
    assert t["Bends"][1] == 20 and t["bends/bend"][1] == t["bends/node"][1] == 20 * BEND_ITERATIONS
    assert t["bends/resolve"][1] == 1 and t["Bonds"][1] == 20
    _end(armed)


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_survives_everything_but_set_bends(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    st = sheet_state(gpe, mode)
    tw = sheet_twin(oracle)
    rng = np.random.default_rng(21)

    def steps(what, k=2, by_uid=False):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what, by_uid=by_uid)

    steps("start", 4)
    band = circle_mask(tw.arrays()[0], 22.0, 18.0, 3.0)
    assert st.kick_circle((22.0, 18.0), 3.0, L.VEL_ADD, (0.0, 2.0)) == tw.kick(band, L.VEL_ADD, 0.0, 2.0) > 0
    steps("kick")
    add = rng.uniform(2, 8, (100, 2)).astype(F32)
    st.add_particles(add, np.full(100, 0.5, F32)); tw.add(add, np.full(100, 0.5, F32))
    steps("add")
    # removals: a corner by circle (its bends go inert), two particles by mask, two by uid
    corner = (10.0 + 31 * 1.25, 4.0)
    assert st.remove_particles_in_circle(corner, 1.0) == tw.remove_circle(corner[0], corner[1], 1.0) > 0
    steps("remove circle")
    mask = np.zeros(len(tw), np.uint8); mask[[3, 200]] = 1
    gone = tw.uids[[3, 200]].copy()
    assert st.remove_particles(mask) == tw.remove_mask(mask) == 2
    steps("remove mask")
    acts = M.corrections(tw.arrays()[0], tw.uids, tw.bends)[0]
    assert not acts[(tw.bends["uid_b"] == gone[0]) | (tw.bends["uid_a"] == gone[1])].any() and acts.sum() > 1500
    assert st.remove_particles_by_uid([100, 101, 4000000]) == tw.remove_uids([100, 101, 4000000]) == 2
    steps("remove uid")
    who = np.arange(0, 60, 2, dtype=U32)
    where = (tw.arrays()[0][who] + F32(0.25)).astype(F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit by index")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    resolves = st.bends_info()["resolves"]
    steps("quiet steps")
    assert st.bends_info()["resolves"] == resolves                     # nothing moved the particles: no new lookup
    grow = np.stack([rng.uniform(2, 58, 1500), rng.uniform(54, 59, 1500)], axis=1).astype(F32)   # past the capacity
    st.add_particles(grow, np.full(1500, 0.2, F32)); tw.add(grow, np.full(1500, 0.2, F32))
    steps("growth")
    other = L.MODE_NATIVE if mode == "compat" else L.MODE_COMPAT
    st.ctx.call("gpe_set_mode", other); tw.set_mode(other)
    steps("set_mode")
    st.ctx.call("gpe_set_world", 64.0, 60.0); tw.set_world(64.0, 60.0)
    steps("set_world")
    # the removed uids come back on two other particles, put where the old ones would hang: their bends act again
    u = tw.uids.copy()
    assert not np.isin(gone, u).any() and np.isin(gone + 1, u).all()
    last = np.array([len(u) - 1, len(u) - 2], U32)
    where = (tw.arrays()[0][M.slots_of(u, gone + 1)] + np.array([-1.0, 0.3], F32)).astype(F32)
    st.edit_particles(indices=last, positions=where); tw.edit(last, "index", pos=where)
    u[last] = gone
    before = tw.arrays()[0].copy()
    st.set_uids(u); tw.set_uids(u)
    st.apply_bends(); tw.apply_bends()
    _same_as_twin(st, tw, "set_uids")
    moved = (bits(tw.arrays()[0]) != bits(before)).any(axis=1)
    assert moved[len(u) - 1] and moved[len(u) - 2]
    # save / load: the set and its relaxation count travel, the counters start anew
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["bends"].tobytes() == tw.bends.tobytes() and int(d["bend_iterations"][0]) == BEND_ITERATIONS
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    assert back.bends().tobytes() == tw.bends.tobytes()
    assert back.bends_info() == dict(iterations=BEND_ITERATIONS, k=len(tw.bends), nodes=SHEET * SHEET, passes=0, resolves=0)
    passes, bond_passes, pushes = tw.bend_passes, tw.bond_passes, (tw.passes, tw.pushed)
    tw.run(DT, 6, resort_every=4, resort_first=False)
    for s in (st, back):
        s.run(DT, 6, resort_every=4, resort_first=False)
        tw.bend_passes = passes + 6 if s is st else 6
        _same_as_twin(s, tw, "after load")
    _end(back)
    # gpe_set_particles renumbers the uids from 0: the bends name the new particles
    pos, rad = sheet_scene()[:2]
    pos = (pos + F32(3.0)).astype(F32)
    f = C.POINTER(C.c_float)
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), pos.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))
    tw.set_particles(pos, pos, rad)
    tw.bend_passes = passes + 6
    steps("set_particles")
    # a new set zeroes the counters; a context without bends writes none and loads none
    st.set_bends(_rows(gpe, tw.bends[:100]), 3); tw.set_bends(tw.bends[:100], 3)
    assert st.bends_info() == dict(iterations=3, k=100, nodes=M.node_count(tw.bends), passes=0, resolves=0)
    steps("new set")
    st.clear_bends()
    st.save(path)
    with np.load(path) as d:
        assert "bends" not in d.files and "bend_iterations" not in d.files and "bonds" in d.files
    tw.close()
    _end(st)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    st = sheet_state(gpe, bonds=False)
    tw = sheet_twin(oracle, bonds=False)
    for _ in range(3):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.bends_info()
    held = st.bends()

    def untouched(what):
        assert st.bends().tobytes() == held.tobytes() and st.bends_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    names = ["uid_a", "uid_b", "uid_c", "rest_cos", "rest_sin", "stiffness", "flags", "reserved"]

    def rows(*bs):
        out = (L.GpeBend * len(bs))()
        for o, b in zip(out, bs):
            for name, v in zip(names, b):
                setattr(o, name, v)
        return out

    ok = (1, 2, 3, 0.6, 0.8, 0.5, 0, 0)
    h = st.ctx.h
    k = C.c_uint64()
    binfo = L.GpeBendsInfo(struct_size=C.sizeof(L.GpeBendsInfo))
    assert C.sizeof(L.GpeBend) == 32 and C.sizeof(L.GpeBendsInfo) == 40
    assert lib.gpe_set_bends(None, rows(ok), 1, 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bends(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_bends(None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bends_info(None, C.byref(binfo)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bends(h, None, 0, None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bends(h, None, 2, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL arguments")

    def one(**change):
        base = list(ok)
        for name, v in change.items():
            base[names.index(name)] = v
        return lambda: lib.gpe_set_bends(h, rows(ok, tuple(base)), 2, 1)

    d = L.BEND_MAX_DEGREE
    hub = rows(*[(0, 2 * j + 1, 2 * j + 2, -1.0, 0.0, 0.5, 0, 0) for j in range(d + 1)])
    bad = {
        "NULL bends with k > 0": lambda: lib.gpe_set_bends(h, None, 2, 1),
        "k > GPE_BENDS_MAX": lambda: lib.gpe_set_bends(h, rows(ok), L.BENDS_MAX + 1, 1),
        "iterations 0": lambda: lib.gpe_set_bends(h, rows(ok), 1, 0),
        "iterations 33": lambda: lib.gpe_set_bends(h, rows(ok), 1, L.BEND_ITER_MAX + 1),
        "a == b": one(uid_a=2), "b == c": one(uid_c=2), "a == c": one(uid_c=1),
        "uid_a absent": one(uid_a=ABSENT), "uid_b absent": one(uid_b=ABSENT), "uid_c absent": one(uid_c=ABSENT),
        "NaN cos": one(rest_cos=NAN), "inf sin": one(rest_sin=INF), "not a unit vector": one(rest_cos=0.7),
        "zero vector": one(rest_cos=0.0, rest_sin=0.0), "4e-6 off": one(rest_cos=1.0, rest_sin=0.002),
        "NaN stiffness": one(stiffness=NAN), "stiffness > 1": one(stiffness=1.5), "stiffness < 0": one(stiffness=-0.25),
        "flags": one(flags=1), "reserved": one(reserved=7),
        "degree 1025": lambda: lib.gpe_set_bends(h, hub, d + 1, 1),
        "info struct_size": lambda: lib.gpe_get_bends_info(h, C.byref(L.GpeBendsInfo(struct_size=C.sizeof(L.GpeBendsInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_bends_info(h, None),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        assert b"gpe_" in lib.gpe_last_error(h), what                  # the message names the call
        untouched(what)
    assert (L.BENDS_MAX, L.BEND_MAX_DEGREE, L.BEND_ITER_MAX) == (4194304, 1024, 32)
    # while the set is held: the uids stay on, and the context cannot be sharded
    pos, rad = sheet_scene()[:2]
    keys = np.arange(len(rad), dtype=U32)
    holding = {
        "gpe_enable_uids": lambda: lib.gpe_enable_uids(h, 0),
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, len(rad), len(rad) - 10),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), len(rad), 0),
    }
    for what, call in holding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"bends" in lib.gpe_last_error(h) and what.encode() in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK and lib.gpe_enable_uids(h, 1) == L.GPE_OK     # no change: allowed
    untouched("allowed calls")
    # a partial read delivers the first rows
    out = rows(ok, ok, ok)
    assert lib.gpe_get_bends(h, out, 2, C.byref(k)) == L.GPE_OK and k.value == len(held)
    assert (out[0].uid_a, out[0].uid_b, out[0].uid_c, out[1].uid_a, out[2].uid_a) == (0, 1, 2, 1, 1)
    # the context goes on as the twin does
    for _ in range(3):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 is accepted and stored as +0; a vector within 2^-20 of unit length, the degree cap itself and duplicates are
    z = rows((1, 2, 3, -0.0, -1.0, -0.0, 0, 0), (1, 2, 3, 1.0, 0.0009, 1.0, 0, 0), ok, ok)
    assert lib.gpe_set_bends(h, z, 4, L.BEND_ITER_MAX) == L.GPE_OK
    rec = st.bends()
    assert bits(rec["rest_cos"][:1]).tolist() == [0] and bits(rec["stiffness"][:1]).tolist() == [0]
    assert lib.gpe_set_bends(h, hub, d, 1) == L.GPE_OK
    assert st.bends_info()["nodes"] == 2 * d + 1
    st.update(DT)
    # without uids: GPE_ERR_STATE, and nothing is held
    st.clear_bends()
    st.enable_uids(False)
    assert lib.gpe_set_bends(h, rows(ok), 1, 1) == L.GPE_ERR_STATE and b"gpe_set_bends" in lib.gpe_last_error(h)
    assert st.bends_info()["k"] == 0
    assert lib.gpe_set_bends(h, None, 0, 1) == L.GPE_OK                # clearing nothing needs no uids
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_bends(gpe, how):
    L = gpe._lib
    pos, rad, _, bd, _ = sheet_scene()
    st = _state(gpe, pos, rad, world=SHEET_WORLD, uids=False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_bends(_rows(gpe, bd), 1)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.bends()) == 0 and st.bends_info()["k"] == 0
    st.apply_bends()
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)


# ---- 8. the guarded allocations over the sheet ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_guarded_run_of_the_sheet_reports_nothing(gpe, mode):
    """every table of the set sits between red zones, allocated with no slack: steps, a run with re-sorts, a pass on
    its own, a smaller and a larger set in place of the first, and the clearing leave every zone whole"""
    st = sheet_state(gpe, mode)
    st.run(DT, 8, resort_every=3, resort_first=True)
    st.update(DT); st.apply_bends()
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    live = {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}
    assert BEND_TAGS <= live
    bd = sheet_scene()[3]
    st.set_bends(_rows(gpe, bd[:65]), 1)
    st.run(DT, 4, resort_every=0, resort_first=False)
    st.set_bends(_rows(gpe, np.concatenate([bd, bd[::-1]])), 3)
    st.run(DT, 4, resort_every=2, resort_first=False)
    st.clear_bends()
    st.update(DT)
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    _end(st)


# ---- 9. a seeded random interleaving --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_random_interleaving_against_the_twin(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    rng = np.random.default_rng(177 if mode == "native" else 178)
    world, gravity = (60.0, 60.0), (0.0, 80.0)
    n = 600
    pos = np.stack([rng.uniform(2, 58, n), rng.uniform(2, 40, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, mode=mode)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids()

    def nearest_two():
        p, uids = tw.arrays()[0], tw.uids
        k = int(rng.integers(20, 300))
        b = rng.integers(0, len(uids), k)
        d2 = ((p[b, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(k), b] = np.inf
        near = np.argsort(d2, axis=1)[:, :2]
        return p, uids, b, near[:, 0], near[:, 1]

    def random_bends():
        """hinges with their two nearest particles as arms, a few uids nobody has"""
        p, uids, b, a, c = nearest_two()
        k = len(b)
        held = M.captured(p, uids, np.stack([uids[a], uids[b], uids[c]], axis=1), rng.uniform(0.05, 0.5, k).astype(F32))
        turned = M.bends(uids[a], uids[b], uids[c], rng.uniform(-PI, PI, k), rng.uniform(0.05, 0.3, k).astype(F32))
        ghosts = M.bends(uids[a[:5]], np.arange(5) + 3000000000, uids[c[:5]], PI, 0.5)
        held = held[np.isfinite(held["rest_cos"]) & np.isfinite(held["rest_sin"])]    # (two particles on one spot)
        return np.concatenate([held[::2], turned[1::2], ghosts]), int(rng.integers(1, 5))

    def random_bonds():
        p, uids, b, a, _ = nearest_two()
        return BM.pairs(uids[a], uids[b], rng.uniform(1.0, 2.0, len(b)).astype(F32), 0.3), int(rng.integers(1, 4))

    ops = ["set_bends", "clear", "step", "run", "add", "remove", "edit", "kick", "resort", "apply", "bonds", "colliders",
           "saveload"]
    weights = np.array([4, 1, 6, 5, 2, 3, 2, 2, 2, 2, 2, 2, 2], float)
    log, most_passes = [], 0
    b, it = random_bends()
    st.set_bends(_rows(gpe, b), it); tw.set_bends(b, it)
    for i in range(36):
        op = str(rng.choice(ops, p=weights / weights.sum()))
        log.append(op)
        if op == "set_bends":
            b, it = random_bends()
            st.set_bends(_rows(gpe, b), it); tw.set_bends(b, it)
        elif op == "clear":
            st.clear_bends(); tw.set_bends(np.zeros(0, M.BEND_DTYPE), 1)
        elif op == "step":
            for _ in range(int(rng.integers(1, 4))):
                resort = bool(rng.integers(0, 4) == 0)
                st.update(DT, resort=resort); tw.step(DT, resort=resort)
        elif op == "run":
            k, every, first = int(rng.integers(2, 9)), int(rng.integers(0, 4)), bool(rng.integers(0, 2))
            st.run(DT, k, resort_every=every, resort_first=first); tw.run(DT, k, resort_every=every, resort_first=first)
        elif op == "add":
            k = int(rng.integers(1, 40))
            p = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 30, k)], axis=1).astype(F32)
            st.add_particles(p, np.full(k, 0.5, F32)); tw.add(p, np.full(k, 0.5, F32))
        elif op == "remove":
            if rng.integers(0, 2):
                c, r = rng.uniform(10, 50, 2), float(rng.uniform(1, 5))
                if 0 < int(circle_mask(tw.arrays()[0], c[0], c[1], r).sum()) < len(tw):
                    assert st.remove_particles_in_circle(c, r) == tw.remove_circle(c[0], c[1], r)
            else:
                gone = rng.choice(tw.uids, 6, replace=False)
                assert st.remove_particles_by_uid(gone) == tw.remove_uids(gone) == 6
        elif op == "edit":
            k = int(rng.integers(1, 30))
            who = rng.choice(len(tw), k, replace=False).astype(U32)
            where = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 45, k)], axis=1).astype(F32)
            st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
        elif op == "kick":
            c, r = rng.uniform(10, 50, 2), float(rng.uniform(3, 10))
            a = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
            mask = circle_mask(tw.arrays()[0], c[0], c[1], r)
            assert st.kick_circle(c, r, L.VEL_ADD, a) == tw.kick(mask, 0, a[0], a[1])
        elif op == "resort":
            st.particles.sort_by_cell_id(); tw.morton_resort()
        elif op == "apply":
            st.apply_bends(); tw.apply_bends()
        elif op == "bonds":
            bo, bit = random_bonds() if rng.integers(0, 3) else (np.zeros(0, BM.BOND_DTYPE), 1)
            st.set_bonds(_bond_rows(gpe, bo), bit); tw.set_bonds(bo, bit)
        elif op == "colliders":
            cs = (np.array([[-5, 52, 65, 52, 8], [rng.uniform(10, 50), 35, rng.uniform(10, 50), 38, rng.uniform(0, 3)]], F32)
                  if rng.integers(0, 3) else np.zeros((0, 5), F32))
            st.set_colliders(cs); tw.set_colliders(cs)
        else:
            path = str(tmp_path / ("s%d.npz" % i))
            st.save(path)
            _end(st)
            st = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
            tw.bend_passes = tw.bond_passes = 0                        # (load sets the sets anew)
            tw.passes = tw.pushed = 0
        _same_as_twin(st, tw, (i, log))
        assert same_bits(st.colliders(), tw.colliders), (i, log)
        most_passes = max(most_passes, tw.bend_passes)
    print(" ".join(log), "| most passes under one set:", most_passes)
    assert {"set_bends", "step", "run"} <= set(log) and most_passes > 5
    tw.close()
    _end(st)
