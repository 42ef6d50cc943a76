"""GPU (-m gpu): region queries and picking (gpe_query_circle / gpe_query_box / gpe_pick, csrc/k_query.hip).  The
contract: a circle or box query returns exactly the particles the numpy float32 predicate selects on the downloaded
positions, ascending, with their bits; a circle query returns what gpe_remove_particles_in_circle would remove; pick is
the argmin of (bits(d2), index) over the containing discs; and a queried context steps exactly as an unqueried one."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests._oracle_model import box_mask, circle_mask, pick_oracle

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0
F32 = np.float32
MODES = {"native": 1, "compat": 0}
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _status_of(fn):
    gpe = importlib.import_module("gpu-physics-engine_amd")
    with pytest.raises(gpe.GpeError) as e:
        fn()
    return e.value.status


def _check_rows(st, got, want_index, uids_on):
    """got (a QueryResult) holds exactly want_index, ascending, with the downloads' bits at those indices"""
    assert got.index.dtype == np.uint32
    assert np.array_equal(got.index, want_index.astype(np.uint32))
    pos, prev, rad = st.positions(), st.previous_positions(), st.radii()
    assert np.array_equal(_bits(got.pos), _bits(pos[want_index]))
    assert np.array_equal(_bits(got.prev), _bits(prev[want_index]))
    assert np.array_equal(_bits(got.radius), _bits(rad[want_index]))
    if uids_on:
        assert np.array_equal(got.uid, st.uids()[want_index])
    else:
        assert got.uid is None


def _check_regions(st, uids_on):
    pos = st.positions()
    w, h = st.ctx.world()
    p0 = pos[len(pos) // 2]
    circles = [((float(p0[0]), float(p0[1])), 0.0),                 # radius 0 on a particle: at least that one
               ((float(p0[0]), float(p0[1])), 3.7),                 # centre exactly on a particle
               ((w * 0.37, h * 0.61), min(w, h) * 0.12),
               ((-1e6, -1e6), 5.0),                                  # nothing
               ((w / 2, h / 2), 1e7)]                                # everything
    for (cx, cy), r in circles:
        want = np.nonzero(circle_mask(pos, cx, cy, r))[0]
        got = st.query_circle((cx, cy), r)
        _check_rows(st, got, want, uids_on)
        assert st.count_circle((cx, cy), r) == want.size
    assert st.query_circle((float(p0[0]), float(p0[1])), 0.0).index.size >= 1
    boxes = [(w * 0.1, h * 0.2, w * 0.55, h * 0.9),
             (float(p0[0]), float(p0[1]), float(p0[0]), float(p0[1])),   # a degenerate box on a particle
             (w * 0.6, h * 0.5, w * 0.4, h * 0.9),                       # x0 > x1: empty
             (-INF, -INF, w / 3, INF),                                   # half-plane
             (w / 2, -INF, INF, h / 2),
             (-INF, -INF, INF, INF),                                     # everything
             (-1e6, -1e6, -1e5, -1e5)]                                   # nothing
    for x0, y0, x1, y1 in boxes:
        want = np.nonzero(box_mask(pos, x0, y0, x1, y1))[0]
        got = st.query_box((x0, y0), (x1, y1))
        _check_rows(st, got, want, uids_on)
        assert st.count_box((x0, y0), (x1, y1)) == want.size


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 20_000, 200_000])
def test_queries_equal_the_float32_predicate(gpe, mode, n):
    world = gpe.scenes.world_for(max(n, 64), density=0.05)
    pos, rad = gpe.scenes.mixed_radius_cloud(n, world, seed=n + 11)
    st = gpe.State(pos, rad, world=world, mode=MODES[mode])
    uids_on = n % 2 == 0
    if uids_on:
        st.enable_uids()
    st.update(DT, resort=True)
    st.update(DT)
    _check_regions(st, uids_on)
    st.close()


@pytest.mark.parametrize("uids_on", [False, True])
def test_queries_after_100_native_steps(gpe, uids_on):
    n = 200_000
    world = gpe.scenes.world_for(n, density=1.0)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=404)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.8))
    if uids_on:
        st.enable_uids()
    st.run(DT, 100, resort_every=25, resort_first=True)
    assert st.ctx.pipeline_info()["native_steps"] == 100
    _check_regions(st, uids_on)
    st.close()


def _raw(st, name, args, capacity, fields, uid=False, canary=0xA5A5A5A5):
    """gpe_* called through ctypes with canary-filled host arrays of capacity + 8 rows; returns (status, count, arrays)"""
    gpe = importlib.import_module("gpu-physics-engine_amd")
    L = gpe._lib
    rows = capacity + 8
    arr = {"index": np.full(rows, canary, np.uint32), "uid": np.full(rows, canary, np.uint32),
           "pos_xy": np.full(2 * rows, canary, np.uint32), "prev_xy": np.full(2 * rows, canary, np.uint32),
           "radius": np.full(rows, canary, np.uint32)}
    res = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult), capacity=capacity, count=12345)
    for f in fields + (("uid",) if uid else ()):
        t = C.c_uint32 if f in ("index", "uid") else C.c_float
        setattr(res, f, arr[f].ctypes.data_as(C.POINTER(t)))
    status = getattr(st.ctx.lib, name)(st.ctx.h, *args, C.byref(res))
    return status, res.count, arr


ALL = ("index", "pos_xy", "prev_xy", "radius")


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_capacity_below_count_writes_exactly_capacity_rows(gpe, mode):
    n = 60_000
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=61)
    st = gpe.State(pos, rad, world=world, mode=MODES[mode])
    st.enable_uids()
    st.update(DT, resort=True)
    pos, prev, rads, uids = st.positions(), st.previous_positions(), st.radii(), st.uids()
    canary = 0xA5A5A5A5
    for name, args, mask in (("gpe_query_circle", (world[0] / 2, world[1] / 2, world[1] / 3),
                              circle_mask(pos, world[0] / 2, world[1] / 2, world[1] / 3)),
                             ("gpe_query_box", (0.0, 0.0, world[0] / 2, INF), box_mask(pos, 0.0, 0.0, world[0] / 2, INF))):
        want = np.nonzero(mask)[0]
        assert want.size > 5000
        for cap in (0, 1, 63, 64, 2047, 2049, want.size - 1, want.size, want.size + 5):
            status, count, a = _raw(st, name, args, cap, ALL, uid=True)
            assert status == gpe._lib.GPE_OK and count == want.size, (name, cap)
            k = min(cap, want.size)
            w = want[:k]
            assert np.array_equal(a["index"][:k], w)
            assert np.array_equal(a["uid"][:k], uids[w])
            assert np.array_equal(a["pos_xy"][:2 * k], _bits(pos[w]).reshape(-1))
            assert np.array_equal(a["prev_xy"][:2 * k], _bits(prev[w]).reshape(-1))
            assert np.array_equal(a["radius"][:k], _bits(rads[w]))
            for f, width in (("index", 1), ("uid", 1), ("pos_xy", 2), ("prev_xy", 2), ("radius", 1)):
                assert (a[f][width * k:] == canary).all(), (name, cap, f)
        # some fields only: the others stay canaries
        status, count, a = _raw(st, name, args, 100, ("prev_xy",))
        assert status == gpe._lib.GPE_OK and count == want.size
        assert np.array_equal(a["prev_xy"][:200], _bits(prev[want[:100]]).reshape(-1))
        for f in ("index", "uid", "pos_xy", "radius"):
            assert (a[f] == canary).all(), f
    st.close()


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_circle_query_is_what_removal_removes(gpe, mode):
    n = 100_000
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=12)
    a = gpe.State(pos, rad, world=world, mode=MODES[mode])
    b = gpe.State(pos, rad, world=world, mode=MODES[mode])
    for x in (a, b):
        x.run(DT, 20, resort_every=0, resort_first=True)
    rng = np.random.default_rng(3)
    for _ in range(4):
        c = (float(rng.uniform(0, world[0])), float(rng.uniform(0, world[1])))
        r = float(rng.uniform(5.0, 60.0))
        pa, pb = a.positions(), b.positions()
        assert np.array_equal(_bits(pa), _bits(pb))
        q = a.query_circle(c, r)
        assert a.count_circle(c, r) == q.index.size
        removed = b.remove_particles_in_circle(c, r)
        assert removed == q.index.size > 0
        keep = np.ones(pa.shape[0], bool)
        keep[q.index] = False
        assert np.array_equal(_bits(b.positions()), _bits(pa[keep]))
        a.remove_particles(~keep)                       # keep the twins in step
    a.close(); b.close()


def test_queried_run_is_bit_identical_to_an_unqueried_twin(gpe):
    n = 50_000
    world = gpe.scenes.world_for(n, density=1.0)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=200)
    a = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.8))
    b = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, gravity=(0.0, -9.8))
    for x in (a, b):
        x.enable_uids()
    rng = np.random.default_rng(200)
    for s in range(200):
        resort = s % 40 == 0
        c = (float(rng.uniform(0, world[0])), float(rng.uniform(0, world[1])))
        q = a.query_circle(c, 20.0)
        assert q.uid is not None and q.index.size == q.uid.size
        a.query_box((c[0] - 30.0, c[1] - 30.0), (c[0] + 30.0, c[1] + 30.0))
        a.count_box((-INF, -INF), (c[0], INF))
        a.pick(c)
        for x in (a, b):
            x.update(DT, resort=resort)
    assert np.array_equal(_bits(a.positions()), _bits(b.positions()))
    assert np.array_equal(_bits(a.previous_positions()), _bits(b.previous_positions()))
    assert np.array_equal(_bits(a.radii()), _bits(b.radii()))
    assert np.array_equal(a.uids(), b.uids())
    assert a.next_uid() == b.next_uid()
    ia, ib = a.ctx.pipeline_info(), b.ctx.pipeline_info()
    assert ia["native_steps"] == ib["native_steps"] > 0
    assert ia["native_sorts"] == ib["native_sorts"]
    assert np.array_equal(a.find_uids([0, 17, n - 1])[0], b.find_uids([0, 17, n - 1])[0])
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_pick_is_the_nearest_containing_disc(gpe, mode):
    world = (400.0, 300.0)
    pos, rad = gpe.scenes.mixed_radius_cloud(30_000, world, seed=9)
    extra_pos = np.array([[100.0, 100.0], [102.0, 100.0], [98.0, 100.0], [100.0, 102.0],   # equal distances from (100, 100)
                          [250.0, 50.0], [250.5, 50.0],                                   # a negative radius nearer
                          [390.0, 290.0]], F32)
    extra_rad = np.array([-2.5, 2.5, 2.5, 2.5, 3.0, -1.0, 0.25], F32)
    # keep the cloud clear of the planted particles so that the expected winners are theirs
    far = np.ones(len(pos), bool)
    for p in extra_pos:
        far &= ((pos - p) ** 2).sum(axis=1) > 100.0
    pos, rad = np.concatenate([pos[far], extra_pos]).astype(F32), np.concatenate([rad[far], extra_rad]).astype(F32)
    st = gpe.State(pos, rad, world=world, mode=MODES[mode])
    st.particles.sort_by_cell_id()                       # a re-sort without a step: the planted discs stay put
    pos, rad = st.positions(), st.radii()
    points = [(101.0, 100.0), (100.0, 101.0), (99.0, 100.0), (100.0, 100.0), (250.3, 50.0), (250.6, 50.0),
              (390.0, 290.25), (390.0, 290.5), (5.0, 5.0), (-50.0, -50.0)]
    rng = np.random.default_rng(1)
    points += [(float(rng.uniform(0, world[0])), float(rng.uniform(0, world[1]))) for _ in range(40)]
    hits = 0
    for x, y in points:
        want = pick_oracle(pos, rad, x, y)
        got = st.pick((x, y))
        if want is None:
            assert got is None, (x, y)
            continue
        hits += 1
        _check_rows(st, got, np.array([want]), False)
    assert hits >= 7
    # (101, 100) is 1 from both (100, 100) (radius -2.5) and (102, 100): the lower storage index wins
    i100 = int(np.nonzero((pos[:, 0] == F32(100.0)) & (pos[:, 1] == F32(100.0)))[0][0])
    i102 = int(np.nonzero((pos[:, 0] == F32(102.0)) & (pos[:, 1] == F32(100.0)))[0][0])
    assert st.pick((101.0, 100.0)).index[0] == min(i100, i102)
    st.close()


def test_errors_leave_outputs_and_context_untouched(gpe):
    L = gpe._lib
    world = (100.0, 100.0)
    pos, rad = gpe.scenes.uniform_cloud(5000, world, seed=4)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    st.update(DT, resort=True)
    before = (st.positions(), st.previous_positions(), st.radii())
    canary = 0xA5A5A5A5
    bad = [("gpe_query_circle", (50.0, 50.0, -1.0), L.GPE_ERR_INVALID_ARG, False),
           ("gpe_query_circle", (50.0, 50.0, INF), L.GPE_ERR_INVALID_ARG, False),
           ("gpe_query_circle", (50.0, 50.0, float("nan")), L.GPE_ERR_INVALID_ARG, False),
           ("gpe_query_box", (float("nan"), 0.0, 10.0, 10.0), L.GPE_ERR_INVALID_ARG, False),
           ("gpe_query_box", (0.0, 0.0, 10.0, float("nan")), L.GPE_ERR_INVALID_ARG, False),
           ("gpe_query_circle", (50.0, 50.0, 10.0), L.GPE_ERR_STATE, True),       # uid requested, uids off
           ("gpe_query_box", (0.0, 0.0, 50.0, 50.0), L.GPE_ERR_STATE, True),
           ("gpe_pick", (50.0, 50.0), L.GPE_ERR_STATE, True)]
    for name, args, want, uid in bad:
        status, count, a = _raw(st, name, args, 64, ALL, uid=uid)
        assert status == want and count == 0, (name, args, status)
        for f in a:
            assert (a[f] == canary).all(), (name, f)
    for name, args in (("gpe_query_circle", (50.0, 50.0, 10.0)), ("gpe_query_box", (0.0, 0.0, 1.0, 1.0)),
                       ("gpe_pick", (50.0, 50.0))):
        assert getattr(st.ctx.lib, name)(st.ctx.h, *args, None) == L.GPE_ERR_INVALID_ARG
        short = L.GpeQueryResult(struct_size=C.sizeof(L.GpeQueryResult) - 8, capacity=0)
        assert getattr(st.ctx.lib, name)(st.ctx.h, *args, C.byref(short)) == L.GPE_ERR_INVALID_ARG
    assert _status_of(lambda: st.query_circle((1.0, 1.0), -2.0)) == L.GPE_ERR_INVALID_ARG
    for got, want in zip((st.positions(), st.previous_positions(), st.radii()), before):
        assert np.array_equal(_bits(got), _bits(want))
    # still usable
    want = np.nonzero(circle_mask(before[0], 50.0, 50.0, 10.0))[0]
    _check_rows(st, st.query_circle((50.0, 50.0), 10.0), want, False)
    st.update(DT)
    st.close()
    # sharded (order keys on): refused
    sh = gpe.State(pos, rad, world=world)
    sh.ctx.call("gpe_use_order_keys", 1)
    for fn in (lambda: sh.query_circle((1.0, 1.0), 1.0), lambda: sh.query_box((0.0, 0.0), (5.0, 5.0)),
               lambda: sh.pick((1.0, 1.0)), lambda: sh.count_circle((1.0, 1.0), 1.0)):
        assert _status_of(fn) == L.GPE_ERR_UNSUPPORTED
    assert "shard" in sh.ctx.lib.gpe_last_error(sh.ctx.h).decode()
    assert sh.particles.len() == 5000
    sh.close()
    # no particles: GPE_OK, count 0
    ctx = gpe.Context(world=world)
    ps = gpe.ParticleSystem(ctx)
    assert ps.count_circle((1.0, 1.0), 1.0) == 0 and ps.count_box((-INF, -INF), (INF, INF)) == 0
    assert ps.query_circle((1.0, 1.0), 1.0).index.size == 0
    assert ps.query_box((0.0, 0.0), (1.0, 1.0)).index.size == 0
    assert ps.pick((1.0, 1.0)) is None
    ctx.close()


def test_queries_at_16m(gpe):
    """Many workgroups and a multi-level scan of the per-tile counts."""
    n = 16_000_000
    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=16)
    st = gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE)
    st.enable_uids()
    perm = np.random.default_rng(16).permutation(n)       # an unsorted order: matches spread over every tile
    st.set_uids(perm.astype(np.uint32))
    pos = st.positions()
    c, r = (world[0] * 0.4, world[1] * 0.55), world[1] * 0.1
    want = np.nonzero(circle_mask(pos, c[0], c[1], r))[0]
    got = st.query_circle(c, r)
    _check_rows(st, got, want, True)
    assert st.count_circle(c, r) == want.size
    x0, y0, x1, y1 = world[0] * 0.25, -INF, world[0] * 0.75, world[1] * 0.5
    want = np.nonzero(box_mask(pos, x0, y0, x1, y1))[0]
    assert want.size > 3_000_000
    assert st.count_box((x0, y0), (x1, y1)) == want.size
    got = st.query_box((x0, y0), (x1, y1))
    assert np.array_equal(got.index, want.astype(np.uint32))
    assert np.array_equal(_bits(got.pos), _bits(pos[want]))
    assert np.array_equal(got.uid, perm[want].astype(np.uint32))
    p = pos[n // 3]
    assert st.pick((float(p[0]), float(p[1]))).index[0] == pick_oracle(pos, st.radii(), p[0], p[1])
    st.close()
