"""GPU (-m gpu): area constraints (gpe_set_areas / _get_areas / _apply_areas / _get_areas_info / _get_area_values /
_set_area_targets, csrc/k_areas.hip, csrc/gpe_areas.hip, csrc/area_table.h).

A relaxation is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy
model (tests/_areas_model.py: no tables, the uids looked up afresh), and the steps against the CPU oracle with the
model's bends, areas, bonds and colliders passes behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and
ends with no damaged red zone."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _areas_model as M
from tests import _bends_model as NM
from tests import _bonds_model as BM
from tests._oracle_model import circle_mask

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
NAN, INF = float("nan"), float("inf")
PI = math.pi
WORLD = (400.0, 300.0)
ABSENT = M.UID_ABSENT
AREA_TAGS = {"uid.area_rec", "uid.area_order", "uid.area_member_node", "uid.area_member_slot", "uid.area_node_uid",
             "uid.area_node_slot", "uid.area_row_start", "uid.area_inc", "uid.area_corr", "uid.area_state",
             "uid.area_value"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def same_values(got, want):
    """(area, lambda) per loop: the model's bits where a loop acted, NaNs where it was inert"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    inert = np.isnan(want).all(axis=1)
    return got.shape == want.shape and np.isnan(got[inert]).all() and same_bits(got[~inert], want[~inert])


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


def _rows(gpe, areas):
    """the model's rows as the engine's (the same layout)"""
    assert gpe.AREA_DTYPE == M.AREA_DTYPE
    return np.ascontiguousarray(areas, gpe.AREA_DTYPE)


def _info(st):
    info = st.areas_info()
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
    rows, member = st.areas()
    assert rows.tobytes() == tw.areas.tobytes() and np.array_equal(member, tw.area_member_uid), what
    assert _info(st) == tw.areas_info(), what
    assert st.bends().tobytes() == tw.bends.tobytes(), what
    rec, broken = st.bonds()
    assert rec.tobytes() == tw.bonds.tobytes() and np.array_equal(broken, tw.broken), what


def ring(n, centre, radius=None, seed=None, wobble=0.0, clockwise=False):
    radius = max(2.0, 1.1 * n / (2 * math.pi)) if radius is None else radius
    a = 2 * math.pi * np.arange(n) / n * (-1 if clockwise else 1)
    p = np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)
    if wobble:
        p = p + np.random.default_rng(seed).uniform(-wobble, wobble, (n, 2))
    return p.astype(F32)


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
COUNTS = [3, 4, 5, 8, 9, 33, 63, 64, 65, 129, 513, 4096]


def _pass_scene():
    """One wobbly ring per count of COUNTS (every class; the last register-path count 64, the first looping count 65,
    a partial gather batch 129, a second partial batch 513, all 64 rounds 4096), then loops that share members with
    the first rings, a loop with a uid nobody has, a NaN member, a loop whose members coincide, a loop across the
    world's edge.  Uids are no storage indices."""
    rng = np.random.default_rng(12)
    pos, loops, at = [], [], 0
    for c in COUNTS:
        r = min(max(2.0, 1.1 * c / (2 * math.pi)), 120.0)
        pos.append(ring(c, (rng.uniform(r + 2, 398 - r), rng.uniform(r + 2, 298 - r)), r, seed=c, wobble=0.3))
        loops.append(np.arange(at, at + c))
        at += c
    n = 6000
    rings = at
    pos = np.concatenate(pos + [rng.uniform(3, 397, (n - at, 2)).astype(F32)])
    rad = rng.uniform(0.25, 0.75, n).astype(F32)
    uids = (rng.permutation(n).astype(np.uint64) * 7919 + 11).astype(U32)
    f = rings                                                          # the first free particle
    pos[f:f + 3] = [[1.0, 10.0], [-2.0, 14.0], [3.0, 18.0]]            # across the left edge: the clamp works
    pos[f + 3:f + 7] = pos[f + 3]                                      # four on one spot
    pos[f + 7] = (NAN, 50.0)
    loops += [np.array([0, 1, 2, f + 10]), np.array([1, 0, f + 11, f + 12]),       # share the triangle's edge 0 - 1
              np.array([f, f + 1, f + 2]), np.array([f + 3, f + 4, f + 5, f + 6]),
              np.array([f + 7, f + 13, f + 14, f + 15, f + 16]), np.array([f + 20, f + 21, f + 22, f + 23, f + 24][::-1])]
    member = np.concatenate([uids[g] for g in loops] + [np.array([uids[f + 30], 0xFFFFFFF0, uids[f + 31]], U32)])
    counts = [len(g) for g in loops] + [3]
    rows = M.rows_for(counts, 0.0, rng.choice([0.25, 0.5, 1.0], len(counts)))
    with np.errstate(all="ignore"):
        area = np.array([M.shoelace64(pos[g]) for g in loops] + [5.0])
    rows["rest_area"] = np.where(np.isfinite(area), area, 7.0) * rng.uniform(0.5, 1.5, len(counts))
    rows["stiffness"][12] = 0.0                                        # (a zero correction still counts)
    rows["rest_area"][13] = -0.0
    order = rng.permutation(len(rows))                                 # the ranges tile [0, members) in any order
    return pos, rad, uids, rows[order], member, len(COUNTS)


def _check_passes(st, pos, prev, rad, uids, rows, member, iterations, passes, world=WORLD, k_resolves=1):
    want = pos
    for p in range(passes):
        want, value = M.apply(want, rad, uids, rows, member, iterations, world, values=True)
        st.apply_areas()
        got, got_prev, got_rad = _arrays(st)
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert same_bits(got_prev, prev) and same_bits(got_rad, rad)
        assert same_values(st.area_values(), value), p
        assert st.areas_info() == dict(iterations=iterations, k=len(rows), members=len(member), nodes=M.node_count(member),
                                       passes=p + 1, resolves=k_resolves)
    return want


@pytest.fixture(scope="module")
def pass_scene():
    return _pass_scene()


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
def test_one_pass_equals_the_model(gpe, pass_scene, iterations, mode):
    """apply_areas() alone, two passes over a set mixing every class: pos bit for bit as the model, prev and radius
    untouched, (area, lambda) and the counters the model's"""
    pos, rad, uids, rows, member, rings = pass_scene
    acts, value, _, _ = M.loop_phase(pos, uids, rows, member)
    assert sorted(rows["count"][acts].tolist()) == sorted(COUNTS + [3, 4, 4, 5]) and (~acts).sum() == 3
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, iterations)
    got_rows, got_member = st.areas()
    assert got_rows.tobytes() == M.stored(rows).tobytes() and np.array_equal(got_member, member)
    assert np.isnan(st.area_values()).all() and len(st.area_values()) == len(rows)     # no pass yet
    want = _check_passes(st, pos, prev, rad, uids, rows, member, iterations, 2)
    f = int(sum(COUNTS))
    assert same_bits(want[f + 3:f + 8], pos[f + 3:f + 8])              # coincident, NaN: every bit kept
    assert same_bits(want[f + 30:f + 32], pos[f + 30:f + 32])          # a loop with an absent uid: its others too
    assert want[f + 1, 0] == rad[f + 1]                                # across the edge: clamped
    moved = (bits(want) != bits(pos)).any(axis=1)
    assert moved[:f].all() and not moved[f + 40:].any()
    tags = _end(st)
    assert AREA_TAGS <= tags


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
def test_one_pass_on_three_particles_with_one_triangle(gpe, iterations, mode):
    pos = np.array([[12.0, 10.0], [10.0, 10.0], [10.5, 12.0]], F32)
    rad = np.array([0.5, 0.75, 0.25], F32)
    uids = np.array([40, 7, 1000000], U32)
    rows = M.rows_for([3], 3.5, 0.5)
    prev = (pos + F32(1)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), uids, iterations)
    want = _check_passes(st, pos, prev, rad, uids, rows, uids, iterations, 2)
    assert (bits(want) != bits(pos)).any(axis=1).all()
    _end(st)


def _quads(cols, rows_):
    """the quads of a (cols + 1) x (rows_ + 1) lattice of spacing 2 at (10, 10), counter-clockwise: uid = row * (cols + 1) + column"""
    j, i = np.meshgrid(np.arange(cols + 1), np.arange(rows_ + 1))
    pos = np.stack([10.0 + 2.0 * j.ravel(), 10.0 + 2.0 * i.ravel()], axis=1)
    v = lambda r, c: r * (cols + 1) + c
    loops = [np.array([v(r, c), v(r, c + 1), v(r + 1, c + 1), v(r + 1, c)]) for r in range(rows_) for c in range(cols)]
    return pos, loops


@pytest.mark.parametrize("k", [15, 16, 17])
def test_the_tail_of_the_loop_phase(gpe, k):
    """k separate quads: a wave of class 4 not full, full, and one over"""
    rng = np.random.default_rng(k)
    pos = np.concatenate([ring(4, (10.0 + 6 * (q % 8), 10.0 + 6 * (q // 8)), 2.0, seed=q, wobble=0.3) for q in range(k)])
    rad = np.full(len(pos), 0.5, F32)
    uids = (rng.permutation(len(pos)) + 100).astype(U32)
    loops = [uids[4 * q:4 * q + 4] for q in range(k)]
    rows, member = M.captured(pos, uids, loops, 0.5, rng.uniform(0.5, 1.5, k))
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, 2)
    want = _check_passes(st, pos, pos, rad, uids, rows, member, 2, 1)
    assert (bits(want) != bits(pos)).any(axis=1).all()
    _end(st)


@pytest.mark.parametrize("m", [63, 64, 65, 257])
def test_the_tail_of_the_node_phase(gpe, m):
    """a strip of m - 2 triangles over m nodes (a loop has at least three, so the smallest node count is the single
    triangle's above): fewer than a wave, one wave exactly, one more, a block and one more"""
    rng = np.random.default_rng(m)
    i = np.arange(m)
    pos = (np.stack([5.0 + 1.5 * i, 20.0 + 2.0 * (i % 2)], axis=1) + rng.uniform(-0.2, 0.2, (m, 2))).astype(F32)
    rad = np.full(m, 0.5, F32)
    uids = (rng.permutation(m) * 3 + 5).astype(U32)
    loops = [uids[[t, t + 1, t + 2]] if t % 2 == 0 else uids[[t + 1, t, t + 2]] for t in range(m - 2)]
    rows, member = M.captured(pos, uids, loops, 0.3, 1.2)
    world = (420.0, 60.0)
    st = _state(gpe, pos, rad, prev=pos, world=world)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, 2)
    want = _check_passes(st, pos, pos, rad, uids, rows, member, 2, 1, world=world)
    assert (bits(want) != bits(pos)).any(axis=1).all() and st.areas_info()["nodes"] == m
    _end(st)


@pytest.mark.parametrize("count", [40, 200])
def test_the_wrap_around_with_neighbours_far_apart_in_storage(gpe, count):
    """members 0 and count - 1, and for the looping path members 63 and 64, lie at opposite ends of the storage, with
    filler between them; per uid the model's bits"""
    rng = np.random.default_rng(count)
    n = 3000
    p = ring(count, (100.0, 100.0), seed=count, wobble=0.3)
    slots = rng.permutation(np.arange(10, n - 10))[:count]
    slots[0], slots[count - 1] = 0, n - 1
    if count > 64:
        slots[63], slots[64] = 1, n - 2
    pos = rng.uniform(150, 390, (n, 2)).astype(F32)
    pos[slots] = p
    rad = np.full(n, 0.5, F32)
    uids = (rng.permutation(n) + 7).astype(U32)
    rows, member = M.captured(pos, uids, [uids[slots]], 0.8, 1.3)
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, 3)
    want = _check_passes(st, pos, pos, rad, uids, rows, member, 3, 1)
    assert (bits(want[slots]) != bits(pos[slots])).any(axis=1).all()
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_shared_vertices_a_sheet_of_quads_and_a_hub_in_64_triangles(gpe, mode):
    L = gpe._lib
    rng = np.random.default_rng(6)
    sheet, loops = _quads(6, 6)                                        # 49 vertices, the 25 inner ones in 4 quads each
    d = L.AREA_MAX_DEGREE
    a = 2 * PI * np.arange(d) / d
    fan = np.concatenate([[[100.0, 100.0]], np.stack([100 + 20 * np.cos(a), 100 + 20 * np.sin(a)], axis=1)])
    pos = (np.concatenate([sheet, fan]) + rng.uniform(-0.3, 0.3, (49 + 1 + d, 2))).astype(F32)
    hub = 49
    loops += [np.array([hub, hub + 1 + j, hub + 1 + (j + 1) % d]) for j in range(d)]
    n = len(pos)
    uids = (rng.permutation(n) * 11 + 3).astype(U32)
    rows, member = M.captured(pos, uids, [uids[g] for g in loops], 0.2, rng.uniform(0.7, 1.3, len(loops)))
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=pos, mode=mode)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, 2)
    degree = np.bincount(M.slots_of(uids, member), minlength=n)
    assert degree[hub] == d and (degree[:49] == 4).sum() == 25 and degree[hub + 1:].tolist() == [2] * d
    want = _check_passes(st, pos, pos, rad, uids, rows, member, 2, 2)
    assert (bits(want) != bits(pos)).any(axis=1).all()
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_inert_loops_leave_their_members_alone_and_act_again(gpe, mode):
    """a loop with one member removed is inert while the other loops act, and acts again once the uid is back; a NaN
    member makes its loop inert; area_values reads NaN for the inert loops"""
    rng = np.random.default_rng(8)
    counts = [5, 70, 12, 4]
    pos = np.concatenate([ring(c, (30.0 + 60 * q, 60.0), seed=q, wobble=0.3) for q, c in enumerate(counts)])
    n = len(pos)
    rad = np.full(n, 0.5, F32)
    first = np.concatenate([[0], np.cumsum(counts)])
    loops = [np.arange(first[q], first[q + 1]) for q in range(4)]
    rows, member = M.captured(pos, np.arange(n, dtype=U32), loops, 0.5, 1.25)
    st = _state(gpe, pos, rad, prev=pos, mode=mode)
    st.set_areas(_rows(gpe, rows), member, 1)
    gone = np.array([first[1] + 66, 2], U32)                           # a member of the looping ring, one of the pentagon
    assert st.remove_particles_by_uid(gone) == 2
    uids = st.uids()
    p = st.positions()
    acts, value, _, _ = M.loop_phase(p, uids, rows, member)
    assert acts.tolist() == [False, False, True, True]
    st.apply_areas()
    want = M.apply(p, rad[:n - 2], uids, rows, member, 1, WORLD)
    assert same_bits(st.positions(), want) and same_values(st.area_values(), value)
    untouched = np.isin(uids, np.concatenate(loops[:2]))
    assert same_bits(want[untouched], p[untouched]) and (bits(want[~untouched]) != bits(p[~untouched])).any(axis=1).all()
    # the uids come back on two new particles where the old ones were: both loops act again
    st.add_particles(pos[gone], rad[gone])
    uids = np.concatenate([uids, gone])
    st.set_uids(uids)
    p = st.positions()
    acts, value, _, _ = M.loop_phase(p, uids, rows, member)
    assert acts.all()
    st.apply_areas()
    want = M.apply(p, rad, uids, rows, member, 1, WORLD)
    assert same_bits(st.positions(), want) and same_values(st.area_values(), value) and not np.isnan(st.area_values()).any()
    assert (bits(want) != bits(p)).any(axis=1).all()
    # a NaN member
    who = np.array([int(M.slots_of(uids, [first[2] + 3])[0])], U32)
    st.edit_particles(indices=who, positions=np.array([[NAN, 60.0]], F32))
    p = st.positions()
    st.apply_areas()
    want, value = M.apply(p, rad, uids, rows, member, 1, WORLD, values=True)
    assert same_bits(st.positions(), want) and same_values(st.area_values(), value)
    assert np.isnan(value[2]).all() and not np.isnan(value[[0, 1, 3]]).any()
    # (one lookup before the first pass, one after the add and set_uids; an edit in place moves no slot)
    assert st.areas_info()["passes"] == 3 and st.areas_info()["resolves"] == 2
    _end(st)


def test_a_clockwise_and_a_counter_clockwise_copy(gpe):
    pos = np.concatenate([ring(9, (50.0, 50.0), seed=1, wobble=0.3), ring(9, (90.0, 50.0), seed=1, wobble=0.3, clockwise=True),
                          ring(80, (200.0, 100.0), seed=2, wobble=0.3), ring(80, (300.0, 100.0), seed=2, wobble=0.3, clockwise=True)])
    n = len(pos)
    uids = np.arange(n, dtype=U32)
    loops = [np.arange(0, 9), np.arange(9, 18), np.arange(18, 98), np.arange(98, 178)]
    rows, member = M.captured(pos, uids, loops, 1.0, 1.5)
    assert (rows["rest_area"] > 0).tolist() == [True, False, True, False]
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=pos)
    st.set_areas(_rows(gpe, rows), member, 2)
    want = _check_passes(st, pos, pos, rad, uids, rows, member, 2, 1)
    grown = [abs(M.shoelace64(want[g])) / abs(M.shoelace64(pos[g])) for g in loops]
    assert all(1.45 < g < 1.55 for g in grown), grown                  # both senses grow towards 1.5 times their area
    v = st.area_values()
    assert (v[:, 0] > 0).tolist() == [True, False, True, False]
    _end(st)


# ---- 2. the hook: bonded rings above a floor ------------------------------------------------------------------------
RINGS, RING = 64, 16
RING_WORLD, RING_GRAVITY = (72.0, 72.0), (0.0, 100.0)
RING_COLLIDERS = np.array([[-5, 68, 80, 68, 4]], F32)                  # a floor
BOND_ITERATIONS, BEND_ITERATIONS, AREA_ITERATIONS = 3, 1, 2
STEPS = 50


def ring_scene():
    """64 rings of 16 on an 8 x 8 grid, each ring bonded along its edge, with a bend at every member and one area
    constraint; uid = ring * 16 + member"""
    pos = np.concatenate([ring(RING, (6.0 + 8.5 * (q % 8), 5.0 + 7.5 * (q // 8)), seed=q, wobble=0.05) for q in range(RINGS)])
    n = RINGS * RING
    uid = np.arange(n, dtype=U32).reshape(RINGS, RING)
    nxt, prv = np.roll(uid, -1, axis=1), np.roll(uid, 1, axis=1)
    bonds = BM.pairs(uid.ravel(), nxt.ravel(), 1.1, 0.25)
    bends = NM.captured(pos, np.arange(n, dtype=U32), np.stack([prv.ravel(), uid.ravel(), nxt.ravel()], axis=1), 0.1)
    rows, member = M.captured(pos, np.arange(n, dtype=U32), list(uid), 0.8, 1.0)
    return pos, np.full(n, 0.5, F32), bonds, bends, rows, member


def ring_twin(oracle, areas=True, bends=True, bonds=True, colliders=True):
    pos, rad, b, bd, rows, member = ring_scene()
    tw = M.Twin(oracle, pos, rad, world=RING_WORLD, gravity=RING_GRAVITY)
    tw.enable_uids()
    if areas:
        tw.set_areas(rows, member, AREA_ITERATIONS)
    if bends:
        tw.set_bends(bd, BEND_ITERATIONS)
    if bonds:
        tw.set_bonds(b, BOND_ITERATIONS)
    if colliders:
        tw.set_colliders(RING_COLLIDERS)
    return tw


def ring_state(gpe, mode="native", areas=True, bends=True, bonds=True, colliders=True, shuffle=None, **kw):
    pos, rad, b, bd, rows, member = ring_scene()
    if shuffle is not None:
        st = _state(gpe, pos[shuffle], rad[shuffle], world=RING_WORLD, gravity=RING_GRAVITY, mode=mode, **kw)
        st.set_uids(shuffle.astype(U32))
    else:
        st = _state(gpe, pos, rad, world=RING_WORLD, gravity=RING_GRAVITY, mode=mode, **kw)
    if areas:
        st.set_areas(_rows(gpe, rows), member, AREA_ITERATIONS)
    if bends:
        st.set_bends(np.ascontiguousarray(bd, gpe.BEND_DTYPE), BEND_ITERATIONS)
    if bonds:
        st.set_bonds(np.ascontiguousarray(b, gpe.BOND_DTYPE), BOND_ITERATIONS)
    if colliders:
        st.set_colliders(RING_COLLIDERS)
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
def rings(oracle):
    """the reference of the hook tests: oracle step -> model bends -> model areas -> model bonds -> model colliders"""
    tw = ring_twin(oracle)
    frames = _frames(tw, STEPS)
    info, pushed, value = tw.areas_info(), tw.pushed, tw.area_value.copy()
    tw.close()
    assert pushed > 0 and np.isfinite(frames[-1][0]).all()
    return frames, info, pushed, value


@pytest.fixture(scope="module")
def rings_without_areas(oracle):
    tw = ring_twin(oracle, areas=False)
    frames = _frames(tw, 20)
    tw.close()
    return frames


def test_the_rings_areas_are_the_areas_they_hold(gpe, rings, rings_without_areas):
    """State.areas_from_loops captures what the model captures; and the areas do change the run"""
    pos, rad, _, _, rows, member = ring_scene()
    st = _state(gpe, pos, rad, world=RING_WORLD)
    uid = np.arange(RINGS * RING, dtype=U32).reshape(RINGS, RING)
    got_rows, got_member = st.areas_from_loops(list(uid), 0.8)
    assert got_rows.tobytes() == rows.tobytes() and np.array_equal(got_member, member)
    pumped = st.areas_from_loops([uid[3], uid[5][::-1]], stiffness=[0.5, 1.0], pressure=[2.0, 0.5])[0]
    assert pumped["rest_area"][0] == F32(2.0 * M.shoelace64(pos[uid[3]])) and pumped["rest_area"][1] < 0
    assert pumped["first"].tolist() == [0, 16] and pumped["stiffness"].tolist() == [0.5, 1.0]
    with pytest.raises(ValueError):
        st.areas_from_loops([[0, 1, 5000]])
    _end(st)
    assert not same_bits(rings[0][19][0], rings_without_areas[19][0])


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_twin(gpe, rings, mode):
    frames, info, pushed, value = rings
    L = gpe._lib
    st = ring_state(gpe, mode)
    for s in range(STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    assert _info(st) == info and st.areas_info()["resolves"] == 1 and st.colliders_info()["pushed"] == pushed
    assert same_values(st.area_values(), value)
    pipe = st.ctx.pipeline_info()
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == STEPS
    else:
        assert pipe["compat_steps"] == STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_twin_and_the_observers_see_the_result(gpe, rings, mode):
    frames, info, pushed, value = rings
    st = ring_state(gpe, mode)
    uids = np.array([0, 31, 300, 1023, 12], U32)
    st.tracers_begin(uids, every=1, frames=64, prev=True)
    st.monitor_begin(every=1, frames=64)
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
    assert _info(st) == info and st.colliders_info()["pushed"] == pushed and same_values(st.area_values(), value)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == STEPS and recorded == STEPS
    for s in range(STEPS):                                             # frames taken behind all four passes
        p, q = frames[s][0], frames[s][1]
        assert same_bits(tr.pos[s], p[uids]) and same_bits(tr.prev[s], q[uids]), s
        assert rec["max_y"][s] == p[:, 1].max() and rec["min_y"][s] == p[:, 1].min() and rec["n"][s] == RINGS * RING
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 3. re-sorts and storage order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_particles_shuffled_in_storage_and_a_forced_resort_keep_the_bits_per_uid(gpe, oracle, mode):
    """the uids kept, the storage order not: the passes depend on the uids alone, so per uid they give the bits of the
    unshuffled rings; so does the pass after a forced re-sort, when `resolves` counts up by one.  (The collision solve
    of the step visits particles in storage order, so whole steps are compared with a twin shuffled the same way.)"""
    n = RINGS * RING
    shuffle = np.random.default_rng(9).permutation(n)
    st, plain = ring_state(gpe, mode, shuffle=shuffle), ring_state(gpe, mode)
    for ctx in (st, plain):
        ctx.run(DT, 5, resort_every=0, resort_first=False)             # (squashed a little by now)
    where, prev = plain.positions(), plain.previous_positions()
    st.edit_particles(uids=np.arange(n, dtype=U32), positions=where, previous=prev)
    for ctx in (st, plain):
        ctx.apply_areas(); ctx.apply_colliders(); ctx.apply_areas()
    a = np.argsort(st.uids())
    assert np.array_equal(st.uids()[a], plain.uids())
    assert same_bits(st.positions()[a], plain.positions()) and not same_bits(plain.positions(), where)
    assert same_bits(st.area_values(), plain.area_values())
    resolves = st.areas_info()["resolves"]
    st.particles.sort_by_cell_id()                                     # a forced re-sort
    assert not np.array_equal(st.uids()[a], plain.uids())
    for ctx in (st, plain):
        ctx.apply_areas()
    a = np.argsort(st.uids())
    assert same_bits(st.positions()[a], plain.positions()) and same_bits(st.area_values(), plain.area_values())
    assert st.areas_info()["resolves"] == resolves + 1
    st.apply_areas()
    assert st.areas_info()["resolves"] == resolves + 1                 # nothing moved the particles: no new lookup
    _end(st); _end(plain)
    pos, rad, b, bd, rows, member = ring_scene()
    tw = M.Twin(oracle, pos[shuffle], rad[shuffle], world=RING_WORLD, gravity=RING_GRAVITY)
    tw.enable_uids(); tw.set_uids(shuffle.astype(U32))
    tw.set_areas(rows, member, AREA_ITERATIONS); tw.set_bends(bd, BEND_ITERATIONS); tw.set_bonds(b, BOND_ITERATIONS)
    tw.set_colliders(RING_COLLIDERS)
    st = ring_state(gpe, mode, shuffle=shuffle)
    for s in range(12):
        st.update(DT, resort=(s == 6)); tw.step(DT, resort=(s == 6))
        _same_as_twin(st, tw, s)
    assert st.areas_info()["resolves"] == 2
    tw.close()
    _end(st)


# ---- 4. the order of the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_step_is_the_module_calls_then_bends_then_areas_then_bonds_then_colliders(gpe, rings, mode):
    frames = rings[0]
    st = ring_state(gpe, mode)
    for s in range(6):
        st.grid.build_cell_ids(); st.grid.sort_map(); st.collision_system.solve_collisions()
        st.particles.update_positions(DT)
        st.apply_bends()
        before = st.positions()
        st.apply_areas()
        after = st.positions()
        st.apply_bonds()
        st.apply_colliders()
        assert same_bits(st.positions(), frames[s][0]) and same_bits(st.previous_positions(), frames[s][1]), s
        assert not same_bits(before, after)
    assert st.areas_info()["passes"] == 6
    # ... and in no other order: the areas in front of the bends, or behind the bonds, give other bits
    for order in (("areas", "bends", "bonds"), ("bends", "bonds", "areas")):
        other = ring_state(gpe, mode)
        for s in range(6):
            other.grid.build_cell_ids(); other.grid.sort_map(); other.collision_system.solve_collisions()
            other.particles.update_positions(DT)
            for name in order:
                getattr(other, "apply_" + name)()
            other.apply_colliders()
        assert not same_bits(other.positions(), frames[5][0]), order
        _end(other)
    _end(st)


# ---- 5. no areas, no trace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_areas_nothing_changes_and_nothing_is_launched(gpe, rings, rings_without_areas, mode):
    never = ring_state(gpe, mode, areas=False, profiling=True)
    cleared = ring_state(gpe, mode, profiling=True)
    cleared.clear_areas()
    empty = dict(iterations=0, k=0, members=0, nodes=0, passes=0, resolves=0)
    for st in (never, cleared):
        rows, member = st.areas()
        assert len(rows) == 0 and len(member) == 0 and st.areas_info() == empty and len(st.area_values()) == 0
        st.ctx.reset_timings()
        st.apply_areas()                                               # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, rings_without_areas[19][0]) and same_bits(prev, rings_without_areas[19][1])
        assert not any(name == "Areas" or name.startswith("areas/") for name in st.ctx.timings())
        assert not any(t.startswith("uid.area_") for t, _, _, state in st.ctx.guard_registry() if state == "live")
        _end(st)
    armed = ring_state(gpe, mode, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), rings[0][19][0])
    t = armed.ctx.timings()
    assert t["Areas"][1] == 20 and t["areas/loop"][1] == t["areas/node"][1] == 20 * AREA_ITERATIONS    # one class: 16
    assert t["areas/resolve"][1] == 1 and t["Bonds"][1] == 20 and t["Bends"][1] == 20
    _end(armed)


# ---- 6. the pump ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_set_area_targets_pumps_a_ring_up(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    st, tw = ring_state(gpe, mode), ring_twin(oracle)
    rest = tw.areas["rest_area"].copy()
    for s in range(20):                                                # ring 27 doubles over 20 steps, ring 28 and 29 shrink
        t = np.array([rest[27] * (1 + (s + 1) / 20), rest[28] * (1 - (s + 1) / 40), rest[29] * 0.9], F32)
        st.set_area_targets(27, t); tw.set_area_targets(27, t)
        st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, s)
    assert st.areas_info()["resolves"] == 1 and st.areas_info()["passes"] == 20       # slots and counters kept
    rows, member = st.areas()
    assert rows["rest_area"][27] == F32(2) * rest[27] and rows["rest_area"][26] == rest[26] and rows["rest_area"][30] == rest[30]
    uid = np.arange(RINGS * RING).reshape(RINGS, RING)
    p = st.positions()
    assert M.shoelace64(p[uid[27]]) > 1.5 * rest[27] and same_values(st.area_values(), tw.area_value)
    st.set_area_targets(5, np.array([-0.0], F32)); tw.set_area_targets(5, [-0.0])
    assert bits(st.areas()[0]["rest_area"][5:6]).tolist() == [0]
    st.set_area_targets(64, np.zeros(0, F32))                          # an empty range at the end: allowed
    path = str(tmp_path / "pumped.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["areas"].tobytes() == tw.areas.tobytes() and np.array_equal(d["area_member_uid"], member)
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    assert back.areas()[0].tobytes() == tw.areas.tobytes()
    _end(back)
    # a range past the set, a NaN target, NULL: refused, nothing changes
    held = st.areas()[0].tobytes()
    lib, h = L.load(), st.ctx.h
    two = (C.c_float * 2)(1.0, 2.0)
    bad = (C.c_float * 2)(1.0, NAN)
    for call in (lambda: lib.gpe_set_area_targets(h, 63, 2, two), lambda: lib.gpe_set_area_targets(h, 65, 0, two),
                 lambda: lib.gpe_set_area_targets(h, 0, 2**64 - 1, two), lambda: lib.gpe_set_area_targets(h, 3, 2, bad),
                 lambda: lib.gpe_set_area_targets(h, 3, 2, None)):
        assert call() == L.GPE_ERR_INVALID_ARG and b"gpe_set_area_targets" in lib.gpe_last_error(h)
        assert st.areas()[0].tobytes() == held
    assert lib.gpe_set_area_targets(None, 0, 2, two) == L.GPE_ERR_INVALID_ARG
    st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    tw.close()
    _end(st)


# ---- 7. lifecycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_survives_everything_but_set_areas(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    st = ring_state(gpe, mode)
    tw = ring_twin(oracle)
    rng = np.random.default_rng(21)

    def steps(what, k=2, by_uid=False):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what, by_uid=by_uid)

    steps("start", 4)
    band = circle_mask(tw.arrays()[0], 22.0, 18.0, 5.0)
    assert st.kick_circle((22.0, 18.0), 5.0, L.VEL_ADD, (0.0, 2.0)) == tw.kick(band, L.VEL_ADD, 0.0, 2.0) > 0
    steps("kick")
    add = np.stack([rng.uniform(2, 70, 100), rng.uniform(1, 2, 100)], axis=1).astype(F32)
    st.add_particles(add, np.full(100, 0.3, F32)); tw.add(add, np.full(100, 0.3, F32))
    steps("add")
    # removals: by circle (the rings it hits go inert), two particles by mask, two by uid
    where = tw.arrays()[0][40]
    assert st.remove_particles_in_circle(where, 1.0) == tw.remove_circle(where[0], where[1], 1.0) > 0
    steps("remove circle")
    mask = np.zeros(len(tw), np.uint8); mask[[3, 200]] = 1
    gone = tw.uids[[3, 200]].copy()
    assert st.remove_particles(mask) == tw.remove_mask(mask) == 2
    steps("remove mask")
    acts = M.loop_phase(tw.arrays()[0], tw.uids, tw.areas, tw.area_member_uid)[0]
    assert not acts[[0, 12, 2]].any() and acts.sum() >= RINGS - 5
    assert st.remove_particles_by_uid([100, 101, 4000000]) == tw.remove_uids([100, 101, 4000000]) == 2
    steps("remove uid")
    who = np.arange(300, 360, 2, dtype=U32)
    to = (tw.arrays()[0][who] + F32(0.25)).astype(F32)
    st.edit_particles(indices=who, positions=to); tw.edit(who, "index", pos=to)
    steps("edit by index")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    resolves = st.areas_info()["resolves"]
    steps("quiet steps")
    assert st.areas_info()["resolves"] == resolves                     # nothing moved the particles: no new lookup
    grow = np.stack([rng.uniform(2, 70, 1500), rng.uniform(1, 3, 1500)], axis=1).astype(F32)    # past the capacity
    st.add_particles(grow, np.full(1500, 0.2, F32)); tw.add(grow, np.full(1500, 0.2, F32))
    steps("growth")
    other = L.MODE_NATIVE if mode == "compat" else L.MODE_COMPAT
    st.ctx.call("gpe_set_mode", other); tw.set_mode(other)
    steps("set_mode")
    st.ctx.call("gpe_set_world", 76.0, 72.0); tw.set_world(76.0, 72.0)
    steps("set_world")
    # the removed uids come back on two other particles, put near their old neighbours: their rings act again
    u = tw.uids.copy()
    assert not np.isin(gone, u).any() and np.isin(gone + 1, u).all()
    last = np.array([len(u) - 1, len(u) - 2], U32)
    to = (tw.arrays()[0][M.slots_of(u, gone + 1)] + np.array([-0.5, 0.6], F32)).astype(F32)
    st.edit_particles(indices=last, positions=to); tw.edit(last, "index", pos=to)
    u[last] = gone
    st.set_uids(u); tw.set_uids(u)
    st.apply_areas(); tw.apply_areas()
    _same_as_twin(st, tw, "set_uids")
    acts = M.loop_phase(tw.arrays()[0], tw.uids, tw.areas, tw.area_member_uid)[0]
    assert acts[[0, 12]].all() and same_values(st.area_values(), tw.area_value)
    # save / load: the set, its members and its relaxation count travel, the counters start anew
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["areas"].tobytes() == tw.areas.tobytes() and int(d["area_iterations"][0]) == AREA_ITERATIONS
        assert np.array_equal(d["area_member_uid"], tw.area_member_uid)
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    assert back.areas()[0].tobytes() == tw.areas.tobytes()
    assert back.areas_info() == dict(iterations=AREA_ITERATIONS, k=RINGS, members=RINGS * RING, nodes=RINGS * RING, passes=0, resolves=0)
    passes = tw.area_passes
    tw.run(DT, 6, resort_every=4, resort_first=False)
    for s in (st, back):
        s.run(DT, 6, resort_every=4, resort_first=False)
        tw.area_passes = passes + 6 if s is st else 6
        _same_as_twin(s, tw, "after load")
    _end(back)
    # gpe_set_particles renumbers the uids from 0: the loops name the new particles
    pos, rad = ring_scene()[:2]
    pos = (pos + F32(1.0)).astype(F32)
    f = C.POINTER(C.c_float)
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), pos.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))
    tw.set_particles(pos, pos, rad)
    tw.area_passes = passes + 6
    steps("set_particles")
    # a new set zeroes the counters; a context without areas writes none and loads none
    st.set_areas(_rows(gpe, tw.areas[:10]), tw.area_member_uid[:160], 3); tw.set_areas(tw.areas[:10], tw.area_member_uid[:160], 3)
    assert st.areas_info() == dict(iterations=3, k=10, members=160, nodes=160, passes=0, resolves=0)
    steps("new set")
    st.clear_areas()
    st.save(path)
    with np.load(path) as d:
        assert "areas" not in d.files and "area_member_uid" not in d.files and "area_iterations" not in d.files and "bonds" in d.files
    tw.close()
    _end(st)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    st = ring_state(gpe, bonds=False, bends=False)
    tw = ring_twin(oracle, bonds=False, bends=False)
    for _ in range(3):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.areas_info()
    held = [a.tobytes() for a in st.areas()]

    def untouched(what):
        assert [a.tobytes() for a in st.areas()] == held and st.areas_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    names = ["first", "count", "rest_area", "stiffness", "flags", "reserved"]

    def rows(*bs):
        out = (L.GpeArea * len(bs))()
        for o, b in zip(out, bs):
            for name, v in zip(names, b):
                setattr(o, name, v)
        return out

    def u32(*v):
        return (C.c_uint32 * len(v))(*v)

    ok = [(0, 3, 2.0, 0.5, 0, 0), (3, 4, -1.0, 1.0, 0, 0)]
    uid = [1, 2, 3, 3, 2, 4, 5]
    h = st.ctx.h
    k, m = C.c_uint64(), C.c_uint64()
    ainfo = L.GpeAreasInfo(struct_size=C.sizeof(L.GpeAreasInfo))
    assert C.sizeof(L.GpeArea) == 24 and C.sizeof(L.GpeAreasInfo) == 48
    assert lib.gpe_set_areas(None, rows(*ok), 2, u32(*uid), 7, 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_areas(None, None, 0, C.byref(k), None, 0, C.byref(m)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_areas(None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_areas_info(None, C.byref(ainfo)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_area_values(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_areas(h, None, 0, None, None, 0, C.byref(m)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_areas(h, None, 0, C.byref(k), None, 0, None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_areas(h, None, 2, C.byref(k), None, 0, C.byref(m)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_area_values(h, None, 0, None) == L.GPE_ERR_INVALID_ARG
    untouched("NULL arguments")

    def one(loop=1, uids=None, members=None, iterations=1, **change):
        base = [list(r) for r in ok]
        for name, v in change.items():
            base[loop][names.index(name)] = v
        us = uid if uids is None else uids
        return lambda: lib.gpe_set_areas(h, rows(*[tuple(r) for r in base]), 2, u32(*us), len(us) if members is None else members,
                                         iterations)

    d = L.AREA_MAX_DEGREE
    hub_rows = rows(*[(3 * j, 3, 1.0, 0.5, 0, 0) for j in range(d + 1)])
    hub_uid = u32(*[v for j in range(d + 1) for v in (0, 2 * j + 1, 2 * j + 2)])
    bad = {
        "NULL areas with k > 0": lambda: lib.gpe_set_areas(h, None, 2, u32(*uid), 7, 1),
        "NULL member_uid with k > 0": lambda: lib.gpe_set_areas(h, rows(*ok), 2, None, 7, 1),
        "k > GPE_AREAS_MAX": lambda: lib.gpe_set_areas(h, rows(*ok), L.AREAS_MAX + 1, u32(*uid), 7, 1),
        "members > GPE_AREA_MEMBERS_MAX": lambda: lib.gpe_set_areas(h, rows(*ok), 2, u32(*uid), L.AREA_MEMBERS_MAX + 1, 1),
        "iterations 0": one(iterations=0), "iterations 33": one(iterations=L.AREA_ITER_MAX + 1),
        "count 2": one(count=2, uids=uid[:5]), "count 4097": one(count=L.AREA_MAX_MEMBERS + 1, uids=list(range(10, 10 + 3 + 4097))),
        "ranges overlap": one(first=2), "a gap": one(first=4, uids=uid + [9]), "members left at the end": one(uids=uid + [9]),
        "past members": one(count=5), "first + count wraps": one(first=0xFFFFFFFE),
        "uid absent": one(uids=[1, 2, 3, 3, ABSENT, 4, 5]), "a uid twice in one loop": one(uids=[1, 2, 3, 3, 2, 4, 3]),
        "NaN rest_area": one(rest_area=NAN), "inf rest_area": one(rest_area=-INF),
        "NaN stiffness": one(stiffness=NAN), "stiffness > 1": one(stiffness=1.5), "stiffness < 0": one(stiffness=-0.25),
        "flags": one(flags=1), "reserved": one(loop=0, reserved=7),
        "a uid in 65 loops": lambda: lib.gpe_set_areas(h, hub_rows, d + 1, hub_uid, 3 * (d + 1), 1),
        "info struct_size": lambda: lib.gpe_get_areas_info(h, C.byref(L.GpeAreasInfo(struct_size=C.sizeof(L.GpeAreasInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_areas_info(h, None),
        "targets past the set": lambda: lib.gpe_set_area_targets(h, RINGS - 1, 2, (C.c_float * 2)(1.0, 2.0)),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        assert b"gpe_" in lib.gpe_last_error(h), what                  # the message names the call
        untouched(what)
    assert (L.AREAS_MAX, L.AREA_MAX_MEMBERS, L.AREA_MEMBERS_MAX, L.AREA_MAX_DEGREE, L.AREA_ITER_MAX) == (4194304, 4096, 16777216, 64, 32)
    # while the set is held: the uids stay on, and the context cannot be sharded
    pos, rad = ring_scene()[:2]
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
        assert b"areas" in lib.gpe_last_error(h) and what.encode() in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK and lib.gpe_enable_uids(h, 1) == L.GPE_OK     # no change: allowed
    untouched("allowed calls")
    # a partial read delivers the first rows and members
    out, mu = rows(ok[0], ok[0], ok[0]), u32(9, 9, 9, 9, 9)
    assert lib.gpe_get_areas(h, out, 2, C.byref(k), mu, 4, C.byref(m)) == L.GPE_OK and k.value == RINGS and m.value == RINGS * RING
    assert (out[0].first, out[0].count, out[1].first, out[2].first) == (0, RING, RING, 0) and list(mu) == [0, 1, 2, 3, 9]
    # the context goes on as the twin does
    for _ in range(3):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 is accepted and stored as +0; the degree cap itself and ranges given in any order are
    z = rows((4, 3, -0.0, -0.0, 0, 0), (0, 4, 1.0, 1.0, 0, 0))
    assert lib.gpe_set_areas(h, z, 2, u32(3, 2, 4, 5, 1, 2, 3), 7, L.AREA_ITER_MAX) == L.GPE_OK
    rec = st.areas()[0]
    assert bits(rec["rest_area"][:1]).tolist() == [0] and bits(rec["stiffness"][:1]).tolist() == [0]
    assert st.areas_info() == dict(iterations=32, k=2, members=7, nodes=5, passes=0, resolves=0)
    assert lib.gpe_set_areas(h, hub_rows, d, hub_uid, 3 * d, 1) == L.GPE_OK
    assert st.areas_info()["nodes"] == 2 * d + 1
    st.update(DT)
    # without uids: GPE_ERR_STATE, and nothing is held
    st.clear_areas()
    st.enable_uids(False)
    assert lib.gpe_set_areas(h, rows(*ok), 2, u32(*uid), 7, 1) == L.GPE_ERR_STATE and b"gpe_set_areas" in lib.gpe_last_error(h)
    assert st.areas_info()["k"] == 0
    assert lib.gpe_set_areas(h, None, 0, None, 0, 1) == L.GPE_OK       # clearing nothing needs no uids
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_areas(gpe, how):
    L = gpe._lib
    pos, rad, _, _, rows, member = ring_scene()
    st = _state(gpe, pos, rad, world=RING_WORLD, uids=False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_areas(_rows(gpe, rows), member, 1)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.areas()[0]) == 0 and st.areas_info()["k"] == 0
    st.apply_areas()
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)


# ---- 9. the guarded allocations over the rings ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_guarded_run_of_the_rings_reports_nothing(gpe, pass_scene, mode):
    """every table of the set sits between red zones, allocated with no slack: steps, a run with re-sorts, a pass on
    its own, a smaller set and one of every class in place of the first, targets, and the clearing leave every zone
    whole"""
    st = ring_state(gpe, mode)
    st.run(DT, 8, resort_every=3, resort_first=True)
    st.update(DT); st.apply_areas()
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    live = {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}
    assert AREA_TAGS <= live
    rows, member = ring_scene()[4:]
    st.set_areas(_rows(gpe, rows[:17]), member[:17 * RING], 1)
    st.run(DT, 4, resort_every=0, resort_first=False)
    st.set_area_targets(16, rows["rest_area"][16:17] * F32(1.5))
    st.run(DT, 4, resort_every=2, resort_first=False)
    st.clear_areas()
    st.update(DT)
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    _end(st)
    pos, rad, uids, rows, member, _ = pass_scene                       # every class, 4096 members in one loop
    st = _state(gpe, pos, rad, mode=mode)
    st.set_uids(uids)
    st.set_areas(_rows(gpe, rows), member, 3)
    st.apply_areas()
    st.particles.sort_by_cell_id()
    st.apply_areas()
    st.area_values()
    assert st.ctx.guard_check() == [] and st.ctx.guard_damaged == 0
    _end(st)


# ---- 10. a seeded random interleaving -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_random_interleaving_against_the_twin(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    rng = np.random.default_rng(277 if mode == "native" else 278)
    world, gravity = (60.0, 60.0), (0.0, 80.0)
    n = 400
    pos = np.stack([rng.uniform(2, 58, n), rng.uniform(2, 40, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, mode=mode)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids()

    def random_areas():
        """loops of a seed particle's nearest neighbours sorted by angle around their centroid (shared members come
        about by themselves), one much larger loop, a loop with a uid nobody has"""
        p, uids = tw.arrays()[0], tw.uids
        loops = []
        for _ in range(int(rng.integers(3, 30))):
            c = int(rng.integers(3, 12)) if rng.integers(0, 8) else int(rng.integers(65, 150))
            c = min(c, len(uids))
            near = np.argsort(((p - p[rng.integers(0, len(uids))]) ** 2).sum(axis=1))[:c]
            q = p[near].astype(np.float64)
            q = q - q.mean(axis=0)
            loops.append(uids[near[np.argsort(np.arctan2(q[:, 1], q[:, 0]))]])
        rows, member = M.captured(p, uids, loops, rng.uniform(0.05, 0.4, len(loops)).astype(F32), rng.uniform(0.6, 1.4, len(loops)))
        rows["rest_area"] = np.where(np.isfinite(rows["rest_area"]), rows["rest_area"], F32(1))
        ghost = np.concatenate([loops[0][:2], [3000000000]]).astype(U32)
        rows = M.rows_for(np.concatenate([rows["count"], [3]]), np.concatenate([rows["rest_area"], [2.0]]),
                          np.concatenate([rows["stiffness"], [0.5]]))
        return rows, np.concatenate([member, ghost]), int(rng.integers(1, 4))

    def random_bonds():
        p, uids = tw.arrays()[0], tw.uids
        b = rng.integers(0, len(uids), int(rng.integers(20, 200)))
        d2 = ((p[b, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(len(b)), b] = np.inf
        a = np.argmin(d2, axis=1)
        return BM.pairs(uids[a], uids[b], rng.uniform(1.0, 2.0, len(b)).astype(F32), 0.3), int(rng.integers(1, 4))

    ops = ["set_areas", "clear", "step", "run", "targets", "add", "remove", "edit", "kick", "resort", "apply", "bonds",
           "colliders", "saveload"]
    weights = np.array([4, 1, 8, 5, 4, 2, 3, 2, 2, 2, 2, 2, 2, 2], float)
    log, most_passes, steps = [], 0, 0
    a, mu, it = random_areas()
    st.set_areas(_rows(gpe, a), mu, it); tw.set_areas(a, mu, it)
    for i in range(200):
        op = str(rng.choice(ops, p=weights / weights.sum()))
        log.append(op)
        if op == "set_areas":
            a, mu, it = random_areas()
            st.set_areas(_rows(gpe, a), mu, it); tw.set_areas(a, mu, it)
        elif op == "clear":
            st.clear_areas(); tw.set_areas(np.zeros(0, M.AREA_DTYPE), np.zeros(0, U32), 1)
        elif op == "step":
            for _ in range(int(rng.integers(1, 4))):
                resort = bool(rng.integers(0, 4) == 0)
                st.update(DT, resort=resort); tw.step(DT, resort=resort)
                steps += 1
        elif op == "run":
            k, every, first = int(rng.integers(2, 6)), int(rng.integers(0, 4)), bool(rng.integers(0, 2))
            st.run(DT, k, resort_every=every, resort_first=first); tw.run(DT, k, resort_every=every, resort_first=first)
            steps += k
        elif op == "targets":
            if len(tw.areas):
                first = int(rng.integers(0, len(tw.areas)))
                k = int(rng.integers(0, len(tw.areas) - first + 1))
                t = (tw.areas["rest_area"][first:first + k] * rng.uniform(0.8, 1.25, k)).astype(F32)
                st.set_area_targets(first, t); tw.set_area_targets(first, t)
        elif op == "add":
            k = int(rng.integers(1, 40))
            p = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 30, k)], axis=1).astype(F32)
            st.add_particles(p, np.full(k, 0.5, F32)); tw.add(p, np.full(k, 0.5, F32))
        elif op == "remove":
            if rng.integers(0, 2):
                c, r = rng.uniform(10, 50, 2), float(rng.uniform(1, 4))
                if 0 < int(circle_mask(tw.arrays()[0], c[0], c[1], r).sum()) < len(tw) - 100:
                    assert st.remove_particles_in_circle(c, r) == tw.remove_circle(c[0], c[1], r)
            elif len(tw) > 100:
                gone = rng.choice(tw.uids, 4, replace=False)
                assert st.remove_particles_by_uid(gone) == tw.remove_uids(gone) == 4
        elif op == "edit":
            k = int(rng.integers(1, 30))
            who = rng.choice(len(tw), k, replace=False).astype(U32)
            where = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 45, k)], axis=1).astype(F32)
            st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
        elif op == "kick":
            c, r = rng.uniform(10, 50, 2), float(rng.uniform(3, 10))
            v = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
            mask = circle_mask(tw.arrays()[0], c[0], c[1], r)
            assert st.kick_circle(c, r, L.VEL_ADD, v) == tw.kick(mask, 0, v[0], v[1])
        elif op == "resort":
            st.particles.sort_by_cell_id(); tw.morton_resort()
        elif op == "apply":
            st.apply_areas(); tw.apply_areas()
            assert same_values(st.area_values(), tw.area_value), (i, log)
        elif op == "bonds":
            bo, bit = random_bonds() if rng.integers(0, 3) else (np.zeros(0, BM.BOND_DTYPE), 1)
            st.set_bonds(np.ascontiguousarray(bo, gpe.BOND_DTYPE), bit); tw.set_bonds(bo, bit)
        elif op == "colliders":
            cs = (np.array([[-5, 52, 65, 52, 8], [rng.uniform(10, 50), 35, rng.uniform(10, 50), 38, rng.uniform(0, 3)]], F32)
                  if rng.integers(0, 3) else np.zeros((0, 5), F32))
            st.set_colliders(cs); tw.set_colliders(cs)
        else:
            path = str(tmp_path / ("s%d.npz" % i))
            st.save(path)
            _end(st)
            st = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
            tw.area_passes = tw.bend_passes = tw.bond_passes = 0       # (load sets the sets anew)
            tw.passes = tw.pushed = 0
        _same_as_twin(st, tw, (i, log))
        assert same_bits(st.colliders(), tw.colliders), (i, log)
        most_passes = max(most_passes, tw.area_passes)
    print(" ".join(log), "| steps:", steps, "| most passes under one set:", most_passes)
    assert {"set_areas", "step", "run", "targets", "saveload"} <= set(log) and most_passes > 5 and steps > 100
    tw.close()
    _end(st)
