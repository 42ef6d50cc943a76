"""GPU (-m gpu): nearest-neighbour queries (gpe_query_nearest, csrc/k_nearest.hip).  The contract: count, index, bits(d2),
uid, pos, radius and found of every point equal, bit for bit, what the brute-force numpy float32 model
(tests/_nearest_model.py) gives; for a finite cutoff the neighbours are the circle query's members ordered by
(bits(d2), index); the call leaves no trace on the context.  Every context runs under FLAG_GUARD_ALLOCS and ends with no
damaged red zone."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import _nearest_model as M

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0
F32 = np.float32
U32 = np.uint32
INF, NAN = float("inf"), float("nan")
CANARY = 0xEEEEEEEE
CELL = float(F32(0.5) * F32(2.2))       # gpe_compute_cell_size(0.5): 1.1
BOUND = 131072.0 * CELL                 # 144 179.2
CUTOFFS = (0.0, 0.3, 3.0, 1e9, INF)
RING = [(3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)]


def _gpe():
    return importlib.import_module("gpu-physics-engine_amd")


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


def _state(pos, rad, world=(200.0, 200.0), mode=None, **kw):
    gpe = _gpe()
    return gpe.State(np.asarray(pos, F32).reshape(-1, 2), np.asarray(rad, F32), world=world, mode=mode,
                     flags=gpe._lib.FLAG_GUARD_ALLOCS, **kw)


def _close(st):
    st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0
    st.close()


def _first(want, m):
    """the model's result for m neighbours from its result for more: the first m slots of every row"""
    out = {f: np.ascontiguousarray(want[f][:, :m]) for f in ("index", "dist2", "uid", "pos", "radius")}
    out["count"] = np.minimum(want["count"], U32(m))
    out["found"] = int(out["count"].sum())
    return out


def _same(got, want, uids=False, rows=True):
    """a Neighbours equals the model's dict, bit for bit"""
    assert np.array_equal(got.count, want["count"])
    assert np.array_equal(got.index, want["index"])
    assert np.array_equal(_bits(got.dist2), _bits(want["dist2"]))
    assert got.found == want["found"]
    if rows:
        assert np.array_equal(_bits(got.pos), _bits(want["pos"]))
        assert np.array_equal(_bits(got.radius), _bits(want["radius"]))
    else:
        assert got.pos is None and got.radius is None
    if uids:
        assert np.array_equal(got.uid, want["uid"])
    else:
        assert got.uid is None


def _ask_and_check(st, pts, m, cutoff=INF, uids=False):
    want = M.nearest(pts, st.positions(), m=m, max_distance=cutoff, rad=st.radii(), uids=st.uids() if uids else None)
    _same(st.nearest(pts, m=m, max_distance=cutoff, uids=uids, rows=True), want, uids)
    _same(st.nearest(pts, m=m, max_distance=cutoff), want, rows=False)       # a lean call: the same neighbours
    return want


# ---- the main scene ---------------------------------------------------------------------------------------------------
def _main_scene():
    """n = 4000 of radius 0.5 in a 200 x 200 world (cell 1.1), 300 of them packed into x in [100, 101], y in [50.7, 51.6]:
    one cell holds more than four rounds of a wave; 300 random points in and around the world plus the special ones"""
    rng = np.random.default_rng(2024)
    n = 4000
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    rad = np.full(n, 0.5, F32)
    packed = rng.choice(n, 300, replace=False)
    pos[packed, 0] = rng.uniform(100.0, 101.0, 300).astype(F32)
    pos[packed, 1] = rng.uniform(50.7, 51.6, 300).astype(F32)
    pts = rng.uniform(-5.0, 205.0, (300, 2)).astype(F32)
    special = np.concatenate([np.array([[100.5, 51.15]], F32),                 # the centre of the clump
                              pos[[7, packed[0], 3999]],                       # three particle positions, copied exactly
                              np.array([[-40.0, 90.0], [500.0, 500.0]], F32)]) # outside the world
    pts = np.concatenate([pts, special, pts[:5]])                              # ... and five duplicates
    return pos, rad, pts, [7, int(packed[0]), 3999]


@pytest.fixture(scope="module")
def main_scene():
    pos, rad, pts, copied = _main_scene()
    want = {c: M.nearest(pts, pos, m=64, max_distance=c, rad=rad) for c in CUTOFFS}
    for a in (pos, rad, pts) + tuple(v for w in want.values() for v in w.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return dict(pos=pos, rad=rad, pts=pts, want=want, copied=copied)


def test_the_scene_has_the_cases_it_is_meant_to_have(main_scene):
    s = main_scene
    cell = np.floor(s["pos"] / F32(CELL)).astype(np.int64)
    _, per_cell = np.unique(cell[:, 1] * 65536 + cell[:, 0], return_counts=True)
    assert per_cell.max() == 264 > 4 * 64                         # one cell: more than four rounds of the wave
    c5 = _first(s["want"][3.0], 5)["count"][:300]
    assert ((c5 == 5).sum(), ((c5 > 0) & (c5 < 5)).sum(), (c5 == 0).sum()) == (30, 229, 41)     # full, partial, empty
    assert (s["want"][0.3]["count"][:300] == 0).sum() > 250       # nearly every row is empty
    assert (s["want"][INF]["count"] == 64).all() and (s["want"][1e9]["count"] == 64).all()


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_main_scene_equals_the_model(gpe, main_scene, cutoff):
    s = main_scene
    st = _state(s["pos"], s["rad"])
    for m in (1, 5, 64):
        want = _first(s["want"][cutoff], m)
        _same(st.nearest(s["pts"], m=m, max_distance=cutoff, rows=True), want)
        _same(st.nearest(s["pts"], m=m, max_distance=cutoff), want, rows=False)     # a lean call
    got = st.nearest(s["pts"], m=5, max_distance=cutoff)
    assert np.array_equal(got.index[-5:], got.index[:5]) and np.array_equal(_bits(got.dist2[-5:]), _bits(got.dist2[:5]))
    if cutoff == 0.0:                                            # a copied position finds exactly that particle
        for row, i in zip((301, 302, 303), s["copied"]):
            assert got.count[row] == 1 and got.index[row, 0] == i and _bits(got.dist2[row, :1])[0] == 0
        assert got.found == 3
    _close(st)


def test_main_scene_in_compat_mode(gpe, main_scene):
    s = main_scene
    st = _state(s["pos"], s["rad"], mode=gpe.MODE_COMPAT)
    _same(st.nearest(s["pts"], m=5, max_distance=3.0, rows=True), _first(s["want"][3.0], 5))
    _same(st.nearest(s["pts"], m=64, max_distance=INF, rows=True), s["want"][INF])
    _close(st)


def test_cross_check_with_the_circle_query(gpe, main_scene):
    s = main_scene
    st = _state(s["pos"], s["rad"])
    pick = np.r_[np.arange(34), np.arange(300, 306)]              # 40 points, the special ones among them
    pts = s["pts"][pick]
    got = st.nearest(pts, m=64, max_distance=3.0)
    d2 = M.dist2_matrix(pts, s["pos"])
    some = 0
    for i, p in enumerate(pts):
        members = st.query_circle(p, 3.0).index
        assert got.count[i] == min(64, len(members)) == min(64, st.count_circle(p, 3.0))
        key = (_bits(d2[i, members]).astype(np.uint64) << np.uint64(32)) | members.astype(np.uint64)
        ordered = members[np.argsort(key, kind="stable")][:64]
        assert np.array_equal(got.index[i, :got.count[i]], ordered)
        some += len(members) > 0
    assert some > 20 and got.count[34] == 64                      # the clump's centre has more members than slots
    _close(st)


@pytest.mark.parametrize("k", [1, 3, 257])
def test_batch_sizes_that_the_waves_of_a_workgroup_do_not_divide(gpe, main_scene, k):
    s = main_scene
    st = _state(s["pos"], s["rad"])
    pick = np.arange(k) + 50                                     # includes the special points when k = 257
    want = {f: v[pick] for f, v in _first(s["want"][3.0], 5).items() if f != "found"}
    want["found"] = int(want["count"].sum())
    _same(st.nearest(s["pts"][pick], m=5, max_distance=3.0, rows=True), want)
    _close(st)


# ---- ties -------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_indices(gpe):
    ring = np.array(RING, F32) + F32(40)
    filler = np.array([[150.0, 150.0], [20.0, 170.0]], F32)
    twins = np.array([[90.0, 120.0], [90.0, 120.0]], F32)         # a pair of coincident particles
    rng = np.random.default_rng(5)
    for order in (np.arange(16), np.arange(16)[::-1], rng.permutation(16)):
        pos = np.concatenate([ring, filler, twins])[order]
        st = _state(pos, np.full(16, 0.5, F32))
        pts = np.array([[40, 40], [90, 120], [91, 120]], F32)
        want = _ask_and_check(st, pts, 5)
        on_ring = np.sort(np.nonzero(np.isin(order, np.arange(12)))[0])
        assert want["index"][0].tolist() == on_ring[:5].tolist()              # the lowest storage indices win
        assert (_bits(want["dist2"][0]) == _bits(np.array([25], F32))[0]).all()
        pair = np.sort(np.nonzero(np.isin(order, [14, 15]))[0])
        for row in (1, 2):
            assert want["index"][row, :2].tolist() == pair.tolist()
            assert _bits(want["dist2"][row, :1])[0] == _bits(want["dist2"][row, 1:2])[0]
        assert _bits(want["dist2"][1, :1])[0] == 0
        cut = _ask_and_check(st, pts[:1], 5, cutoff=float(np.nextafter(F32(5), F32(0))))
        assert cut["count"].tolist() == [0]
        assert _ask_and_check(st, pts[:1], 64, cutoff=5.0)["count"].tolist() == [12]
        _close(st)


# ---- mixed radii ------------------------------------------------------------------------------------------------------
def test_mixed_radii_with_one_large_particle_setting_the_cell(gpe):
    rng = np.random.default_rng(77)
    n = 1500
    pos = rng.uniform(0.0, 200.0, (n, 2)).astype(F32)
    rad = rng.uniform(0.5, 3.0, n).astype(F32)
    rad[::7] *= F32(-1.0)
    rad[n // 2] = 9.0                                            # cell 19.8
    pts = rng.uniform(-20.0, 220.0, (120, 2)).astype(F32)
    st = _state(pos, rad)
    before = [_ask_and_check(st, pts, m, cutoff) for m, cutoff in ((1, INF), (9, 7.5), (64, 30.0))]
    st.ctx.call("gpe_grid_set_max_radius", float(0.6 * 20.0))    # the grid's override plays no part
    after = [_ask_and_check(st, pts, m, cutoff) for m, cutoff in ((1, INF), (9, 7.5), (64, 30.0))]
    for a, b in zip(before, after):
        assert np.array_equal(a["index"], b["index"])
    _close(st)


# ---- a sparse scene: tiny radii in a large world -------------------------------------------------------------------------
def test_sparse_scene_with_thousands_of_empty_cells_between_particles(gpe):
    rng = np.random.default_rng(404)
    pos = rng.uniform(0.0, 2800.0, (50, 2)).astype(F32)
    rad = np.full(50, 0.01, F32)
    cell = float(F32(0.01) * F32(2.2))                           # 0.022: the clamp starts at 1441.7, the bound is 2883.6
    assert 1441.0 < 65534 * cell < 1442.0 and 2883.0 < 131072 * cell < 2884.0
    pts = np.array([[10.0, 10.0], [700.0, 650.0], [1400.0, 30.0], [333.3, 1200.0], [-50.0, 900.0], [1441.0, 1441.0],
                    [2000.0, 2500.0], [2880.0, 1.0]], F32)       # the last two lie in the clamped region
    st = _state(pos, rad, world=(2800.0, 2800.0))
    for m in (1, 64):                                            # 64 > 50: the whole table is read
        for cutoff in (1e9, INF):
            want = _ask_and_check(st, pts, m, cutoff)
            assert (want["count"] == min(m, 50)).all()
    _close(st)


# ---- clamped cells and hostile positions ------------------------------------------------------------------------------
def test_clamped_cells_negative_coordinates_and_hostile_positions(gpe):
    rng = np.random.default_rng(31)
    far = np.concatenate([rng.uniform(99990.0, 100010.0, (400, 2)),                      # both cell coordinates past 65 534
                          np.c_[rng.uniform(99990.0, 100010.0, 400), rng.uniform(0.0, 20.0, 400)],
                          rng.uniform(-60.0, -40.0, (400, 2)),                           # negative: column and row 0
                          rng.uniform(0.0, 30.0, (300, 2))])
    hostile = np.array([[NAN, 5.0], [5.0, NAN], [NAN, NAN], [INF, 5.0], [5.0, -INF], [-INF, INF], [1e30, 5.0],
                        [5.0, -1e30], [1e30, 1e30]], F32)
    pos = np.concatenate([far.astype(F32), hostile])
    pos = pos[rng.permutation(len(pos))]
    rad = np.full(len(pos), 0.5, F32)
    assert 72000.0 < 65534 * CELL < 99990.0
    beside = far[rng.integers(0, len(far), 60)] + rng.uniform(-4.0, 4.0, (60, 2))
    edge = BOUND - 1.0
    rim = [[-edge, -edge], [edge, -50.0], [100000.0, -edge], [-100.0, 100000.0], [5.0, edge], [edge, edge], [72100.0, 10.0]]
    pts = np.concatenate([beside, rim]).astype(F32)
    st = _state(pos, rad)
    nan = np.nonzero(np.isnan(pos).any(axis=1))[0]
    bad = np.nonzero(~np.isfinite(pos).all(axis=1) | (np.abs(pos) > 1e29).any(axis=1))[0]
    assert len(bad) == len(hostile) and len(nan) == 3
    for m, cutoff in ((1, 5.0), (8, 5.0), (64, 30.0), (64, 1e9)):
        want = _ask_and_check(st, pts, m, cutoff)
        assert want["found"] > 0 and not np.isin(want["index"], bad).any()            # a finite cutoff: never hostile
    want = _ask_and_check(st, pts, 8, INF)
    assert (want["count"] == 8).all() and not np.isin(want["index"], bad).any()
    n_inf = len(bad) - len(nan)
    assert not np.isin(_ask_and_check(st, pts[:16], 64, INF)["index"], nan).any()
    good = np.setdiff1d(np.arange(len(pos)), bad)[:40]
    small = _state(pos[np.r_[bad, good]], rad[:len(bad) + 40])                        # few enough to reach the end
    want = _ask_and_check(small, pts, 64, INF)
    sp = small.positions()
    s_nan = np.nonzero(np.isnan(sp).any(axis=1))[0]
    assert (want["count"] == len(sp) - len(s_nan)).all() and not np.isin(want["index"], s_nan).any()
    last = want["index"][:, len(sp) - len(s_nan) - n_inf:len(sp) - len(s_nan)]       # d2 = +inf comes last ...
    assert (np.sort(last, axis=1) == np.sort(np.setdiff1d(np.arange(len(bad)), s_nan))).all()
    assert (_bits(want["dist2"][:, len(sp) - len(s_nan) - n_inf:len(sp) - len(s_nan)]) == 0x7F800000).all()
    assert np.array_equal(last, np.sort(last, axis=1))                                # ... ordered by index
    _close(small)
    _close(st)


# ---- the radius-free fallback ---------------------------------------------------------------------------------------------
def test_radius_zero_infinite_radius_and_no_world(gpe, main_scene):
    L = gpe._lib
    s = main_scene
    pts = s["pts"][280:311]
    st = _state(s["pos"][:600], np.zeros(600, F32))               # every radius 0: the cell is world / 1024
    for m, cutoff in ((1, INF), (5, 3.0), (64, 20.0)):
        assert _ask_and_check(st, pts, m, cutoff)["found"] > 0
    _close(st)
    rad = np.full(600, 0.5, F32)
    rad[17] = INF                                                 # one infinite radius: the same
    st = _state(s["pos"][:600], rad)
    for m, cutoff in ((1, INF), (5, 3.0)):
        assert _ask_and_check(st, pts, m, cutoff)["found"] > 0
    _close(st)
    st = _state(s["pos"][:600], np.zeros(600, F32), mode=gpe.MODE_COMPAT)
    st.ctx.call("gpe_set_world", 0.0, 0.0)                        # no radius and no world: no cell size
    status, found, arr = _raw(st, pts, 3)
    assert status == L.GPE_ERR_UNSUPPORTED and found == 0 and _untouched(arr)
    _close(st)


# ---- uids -------------------------------------------------------------------------------------------------------------
def test_uids_after_a_morton_resort(gpe, main_scene):
    s = main_scene
    st = _state(s["pos"], s["rad"])
    st.enable_uids()
    st.run(DT, 2, resort_every=0, resort_first=True)             # the particles change places
    uids = st.uids()
    assert not np.array_equal(uids, np.arange(len(uids), dtype=U32))
    want = _ask_and_check(st, s["pts"], 5, 3.0, uids=True)
    got = st.nearest(s["pts"], m=5, max_distance=3.0, uids=True)
    full = got.index != M.NEAREST_NONE
    assert full.any() and (~full).any() and np.array_equal(got.uid[full], uids[got.index[full]])
    assert (got.uid[~full] == M.UID_ABSENT).all() and np.array_equal(got.uid, want["uid"])
    _close(st)


# ---- read-only --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_nearest_queries_leave_no_trace(gpe, mode):
    n = 20_000
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)
    L = gpe._lib
    m = gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE
    queried, plain = sts = [_state(pos, rad, world=world, mode=m, gravity=(0.0, -9.81)) for _ in range(2)]
    rng = np.random.default_rng(9)
    pts = (rng.uniform(-0.05, 1.05, (64, 2)) * world).astype(F32)
    found = []

    def ask():
        queried.ctx.sync()
        info = queried.ctx.pipeline_info()
        scratch = [queried.ctx.download(w, U32) for w in (L.HOME_CELL_IDS, L.PARTICLE_IDS)]
        want = M.nearest(pts, queried.positions(), m=8, max_distance=2.0, rad=queried.radii())
        _same(queried.nearest(pts, m=8, max_distance=2.0, rows=True), want)
        assert queried.nearest(pts[:3], m=64).found == 3 * 64
        found.append(want["found"])
        after = queried.ctx.pipeline_info()
        for key in ("native_sorts", "roster_stamp", "native_steps", "compat_steps"):
            assert info[key] == after[key], key
        for w, was in zip((L.HOME_CELL_IDS, L.PARTICLE_IDS), scratch):
            assert np.array_equal(queried.ctx.download(w, U32), was)

    for st in sts:
        st.run(DT, 5, resort_every=0, resort_first=True)
    ask()
    for steps, resort in ((6, False), (14, True)):               # 20 further steps, a re-sort among them
        for st in sts:
            st.run(DT, steps, resort_every=0, resort_first=resort)
        ask()
    assert np.array_equal(_bits(queried.positions()), _bits(plain.positions()))
    assert np.array_equal(_bits(queried.previous_positions()), _bits(plain.previous_positions()))
    assert found[-1] > 0
    for st in sts:
        _close(st)


# ---- refusals and edges -----------------------------------------------------------------------------------------------
FIELDS = ("count", "index", "uid", "dist2", "pos_xy", "radius")


def _raw(st, pts, m, cutoff=INF, fields=FIELDS[:2] + FIELDS[3:], struct_cut=0, flags=0, k=None, null_points=False):
    """gpe_query_nearest through ctypes with canary-filled outputs -> (status, found, arrays)"""
    L = _gpe()._lib
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    k = len(pts) if k is None else k
    arr = {f: np.full(2 * max(len(pts), 1) * 65 + 4, CANARY, U32) for f in FIELDS}
    q = L.GpeNearestQuery(struct_size=C.sizeof(L.GpeNearestQuery) - struct_cut, flags=flags, k=k, m=m, max_distance=cutoff,
                          found=12345)
    if not null_points:
        q.point_xy = pts.ctypes.data_as(C.POINTER(C.c_float))
    for f in fields:
        t = C.c_uint32 if f in ("count", "index", "uid") else C.c_float
        setattr(q, f, arr[f].ctypes.data_as(C.POINTER(t)))
    status = st.ctx.lib.gpe_query_nearest(st.ctx.h, C.byref(q))
    return status, q.found, arr


def _untouched(arr):
    return all((a == CANARY).all() for a in arr.values())


def test_refusals(gpe, main_scene):
    L = gpe._lib
    s = main_scene
    st = _state(s["pos"][:500], s["rad"][:500])
    pts = s["pts"][:8].copy()

    def refused(want, m=3, **kw):
        status, found, arr = _raw(st, kw.pop("pts", pts), m, **kw)
        assert status == want and found == 0, (status, found, kw)
        assert _untouched(arr)

    status, found, arr = _raw(st, pts, 3, struct_cut=8)           # a short struct has no found field to clear
    assert status == L.GPE_ERR_INVALID_ARG and found == 12345 and _untouched(arr)
    assert st.ctx.lib.gpe_query_nearest(st.ctx.h, None) == L.GPE_ERR_INVALID_ARG
    refused(L.GPE_ERR_INVALID_ARG, flags=1)
    refused(L.GPE_ERR_INVALID_ARG, m=0)
    refused(L.GPE_ERR_INVALID_ARG, m=65)
    for cutoff in (NAN, -1.0, -INF):
        refused(L.GPE_ERR_INVALID_ARG, cutoff=cutoff)
    refused(L.GPE_ERR_INVALID_ARG, null_points=True)
    refused(L.GPE_ERR_STATE, fields=FIELDS)                       # uid requested while uids are off
    for v in (NAN, INF, -INF, float(np.nextafter(F32(BOUND), F32(INF))), -1.001 * BOUND):
        for axis in (0, 1):
            bad = pts.copy()
            bad[5, axis] = v
            refused(L.GPE_ERR_INVALID_ARG, pts=bad)
    inside = pts.copy()
    inside[5] = [float(np.nextafter(F32(BOUND), F32(0))), -float(np.nextafter(F32(BOUND), F32(0)))]
    status, found, arr = _raw(st, inside, 3)                      # just inside the bound: accepted
    assert status == L.GPE_OK and found == 24 and not _untouched(arr)
    assert (arr["count"][:8] == 3).all() and arr["count"][8] == CANARY and arr["index"][24] == CANARY
    assert (arr["uid"] == CANARY).all()                           # not requested: not written
    status, found, arr = _raw(st, pts, 3, cutoff=-0.0)            # -0.0 is accepted as 0
    assert status == L.GPE_OK and found == 0 and (arr["count"][:8] == 0).all() and (arr["index"][:24] == M.NEAREST_NONE).all()
    status, found, arr = _raw(st, pts, 3, k=0)                    # k == 0
    assert status == L.GPE_OK and found == 0 and _untouched(arr)
    status, found, arr = _raw(st, pts, 3, k=0, null_points=True)
    assert status == L.GPE_OK and found == 0
    _ask_and_check(st, pts, 3)                                    # still usable
    st.ctx.call("gpe_set_active_cells", 0, 0, 10, 10)             # an active cell box: a sharded context
    refused(L.GPE_ERR_UNSUPPORTED)
    _close(st)


def test_a_context_without_particles(gpe, main_scene):
    L = gpe._lib
    pts = main_scene["pts"][299:311]
    empty = gpe.Context(world=(200.0, 200.0), flags=L.FLAG_GUARD_ALLOCS)
    ps = gpe.ParticleSystem(empty)
    got = ps.nearest(pts, m=4, rows=True)
    assert got.found == 0 and (got.count == 0).all() and (got.index == M.NEAREST_NONE).all()
    assert np.isnan(got.dist2).all() and np.isnan(got.pos).all() and np.isnan(got.radius).all()
    assert got.index.shape == (12, 4) and got.pos.shape == (12, 4, 2)
    empty.guard_check()
    assert empty.guard_damaged == 0
    empty.close()


def test_registry_lists_the_nearest_scratch(gpe, main_scene):
    s = main_scene
    st = _state(s["pos"], s["rad"])
    assert not [t for t, _, _, _ in st.ctx.guard_registry() if t.startswith("nearest.")]
    st.nearest(s["pts"][:10], m=2)
    tags = {t: p for t, p, _, state in st.ctx.guard_registry() if state == "live"}
    assert tags["nearest.row_start"] == 4 * 65537 and tags["nearest.points"] == 8 * 10 and tags["nearest.index"] == 4 * 20
    st.nearest(s["pts"][:33], m=7, rows=True)                     # grows on demand
    tags = {t: p for t, p, _, state in st.ctx.guard_registry() if state == "live"}
    assert tags["nearest.row_start"] == 4 * 65537
    for tag, width in (("nearest.points", 8), ("nearest.count", 4)):
        assert tags[tag] == width * 33, tag
    for tag, width in (("nearest.index", 4), ("nearest.uid", 4), ("nearest.dist2", 4), ("nearest.pos", 8),
                       ("nearest.radius", 4)):
        assert tags[tag] == width * 33 * 7, tag
    _close(st)
