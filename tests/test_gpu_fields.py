"""GPU (-m gpu): force fields (gpe_set_fields / _get_fields / _apply_fields / _get_fields_info, csrc/k_fields.hip,
csrc/gpe_fields.hip).

The pass is a binary32 function of (pos, prev, fields, dt): every comparison is bit for bit against the numpy model
(tests/_fields_model.py: brute force in ascending field index, no grid), and the steps against the CPU oracle with the
model's pass behind every step.  (A NaN the arithmetic itself produces compares equal to a NaN: its payload is not
specified.)  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends with no damaged red zone."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests import _colliders_model as MC
from tests import _fields_model as M

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = M.POOL_DT
NAN, INF = float("nan"), float("inf")
WORLD = (200.0, 200.0)
POOL_STEPS = 40
TAGS = {"grid.field_rec", "grid.field_touched", "grid.field_cell_start", "grid.field_items"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_prev(got, want):
    """bit for bit, a NaN for a NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def up(x):
    return np.nextafter(F32(x), F32(INF))


def down(x):
    return np.nextafter(F32(x), F32(-INF))


def grid_dims(world):
    """the lookup grid field_grid.h cuts for a world when the entry cap does not bind: (cell, gx, gy)"""
    want = max(world) / 1024.0
    while True:
        cell = 1.0 / float(F32(1) / F32(want))
        nx, ny = math.floor(world[0] / cell) + 1, math.floor(world[1] / cell) + 1
        if nx <= 1024 and ny <= 1024:
            return cell, nx, ny
        want *= 2.0


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


def _live_tags(st):
    return {t for t, _, _, state in st.ctx.guard_registry() if state == "live"}


def _arrays(st):
    return st.positions(), st.previous_positions(), st.radii()


def _set(st, pos, prev, rad):
    f = C.POINTER(C.c_float)
    pos, prev, rad = (np.ascontiguousarray(a, F32) for a in (pos, prev, rad))
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), prev.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))


def _pool_state(gpe, mode=None, flags=0, fields=M.POOL_FIELDS, **kw):
    pos, rad = M.pool_scene()
    st = _state(gpe, pos, rad, world=M.POOL_WORLD, mode=mode, gravity=M.POOL_GRAVITY, flags=flags, **kw)
    if fields is not None:
        st.set_fields(fields)
    return st


# ---- references, computed once --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(oracle):
    """oracle step + model pass, 40 steps, no re-sort"""
    return M.pool_reference(oracle, POOL_STEPS)


@pytest.fixture(scope="module")
def pool_resorted(oracle):
    return M.pool_reference(oracle, POOL_STEPS, resort_every=16, resort_first=True)


@pytest.fixture(scope="module")
def pool_plain(oracle):
    """the same scene without fields: the oracle alone"""
    return M.pool_reference(oracle, 20, fields=None)


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
def _one_field():
    return M.field(M.CIRCLE, M.RADIAL, M.LINEAR, (60, 70, 25, 0), pole=(60, 70), strength=500.0, reach=25.0)


def _mixed_fields(everywhere):
    """40 fields: every shape x kind x falloff, special regions behind them; with `everywhere`, an EVERYWHERE drag
    in the middle (41)"""
    rng = np.random.default_rng(7)
    fs = []
    for i in range(36):
        kind = i % 4
        circle = (i // 4) % 2 == 0
        falloff = M.LINEAR if kind in (M.RADIAL, M.VORTEX) and (i // 8) % 2 == 0 else M.NONE
        x, y = rng.uniform(10, 190, 2)
        size = rng.uniform(5, 40, 2)
        region = (x, y, size[0] * 0.6, 0) if circle else (x, y, x + size[0], y + size[1])
        pole = (x + rng.uniform(-5, 5), y + rng.uniform(-5, 5)) if i % 3 else (x, y)
        strength = rng.uniform(0.3, 1.0) if kind == M.DRAG else rng.uniform(-600, 900)
        fs.append(M.field(M.CIRCLE if circle else M.BOX, kind, falloff, region, pole=pole, f=rng.uniform(-80, 80, 2),
                          strength=strength, reach=rng.uniform(4, 30) if falloff else 0.0))
    fs += [M.field(M.BOX, M.UNIFORM, M.NONE, (-20, 90, 15, 110), f=(50.0, -20.0)),      # straddles the left wall
           M.field(M.CIRCLE, M.DRAG, M.NONE, (100, 100, 0, 0), strength=0.5),           # radius 0: its centre alone
           M.field(M.BOX, M.VORTEX, M.NONE, (120, 60, 110, 90), pole=(115, 75), strength=300.0),   # x0 > x1: empty
           M.field(M.CIRCLE, M.RADIAL, M.LINEAR, (50, 150, 20, 0), pole=(50, 150), strength=700.0, reach=20.0)]
    if everywhere:
        fs.insert(20, M.field(M.EVERYWHERE, M.DRAG, strength=0.875))
    fs = M.rows(*fs)
    combos = {(int(f["shape"]), int(f["kind"]), int(f["falloff"])) for f in fs}
    assert {(s, k, 0) for s in (1, 2) for k in range(4)} <= combos and {(s, k, 1) for s in (1, 2) for k in (1, 2)} <= combos
    return fs


def _special_points(fs, world):
    """where the pass can go wrong: region borders and one ulp outside, poles, at reach, lookup-cell borders and one ulp
    below them, NaN coordinates"""
    f0 = fs[0]
    pts = []
    if f0["shape"] == M.CIRCLE:
        pts += [(f0["x0"] + f0["x1"], f0["y0"]), (NAN, 50.0), (up(f0["x0"] + f0["x1"]), f0["y0"])]
    else:
        pts += [(f0["x0"], f0["y0"]), (NAN, 50.0), (down(f0["x0"]), f0["y0"])]
    for f in list(fs[:14]) + list(fs[-5:]):
        x0, y0, x1, y1 = f["x0"], f["y0"], f["x1"], f["y1"]
        if f["shape"] == M.CIRCLE:
            pts += [(x0 + x1, y0), (up(x0 + x1), y0), (x0, y0 - x1), (x0, down(y0 - x1)), (x0, y0),
                    (x0 + x1 * F32(0.6), y0 + x1 * F32(0.8)), (x0 - x1 * F32(0.8), y0 + x1 * F32(0.6))]
        elif f["shape"] == M.BOX:
            pts += [(x0, y0), (x1, y1), (down(x0), y0), (x1, up(y1)), (x0, up(y1)), ((x0 + x1) / 2, y0), ((x0 + x1) / 2, (y0 + y1) / 2)]
        if f["kind"] in (M.RADIAL, M.VORTEX):
            pts += [(f["px"], f["py"])]
            if f["falloff"] == M.LINEAR:
                pts += [(f["px"] + f["reach"], f["py"]), (f["px"], f["py"] - f["reach"]), (up(f["px"] + f["reach"]), f["py"])]
    cell = grid_dims(world)[0]
    for b in (1, 7, 100, 300, 511):
        x = F32(b * cell)
        pts += [(x, 33.3), (down(x), 33.3), (up(x), 33.3), (44.4, x), (44.4, down(x)), (x, x), (down(x), down(x))]
    pts += [(50.0, NAN), (NAN, NAN), (-0.0, 100.0), (0.0, 0.0)]
    return np.array(pts, F32)


OUTSIDE = np.array([[250.0, 100.0], [-5.0, 95.0], [100.0, -3.0], [-1e30, 100.0]], F32)   # (-5, 95): in the straddling box


def _place(n, fs, seed, world=WORLD):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.5, world[0] - 0.5, (n, 2)).astype(F32)
    sp = _special_points(fs, world)
    m = min(n, len(sp))
    pos[:m] = sp[:m]
    vel = rng.uniform(-0.4, 0.4, (n, 2)).astype(F32)
    vel[::5] = 0                                                       # some at rest
    prev = (pos - vel).astype(F32)
    return pos, prev, np.full(n, 0.5, F32)


@pytest.mark.parametrize("fields", ["one", "mixed40", "mixed41"])
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 4097])
def test_one_pass_equals_the_model(gpe, n, fields):
    """apply_fields() alone: prev bit for bit as the model, pos and radius untouched, touched the model's count.  n = 1:
    the tail lane alone; 2: one pair; 3: a pair and the tail; 127 / 128 / 129: partial and full waves; 4097: several
    workgroups.  From n = 127 on, the last particles are moved outside the world with edit_particles."""
    fs = M.rows(_one_field()) if fields == "one" else _mixed_fields(fields == "mixed41")
    assert len(fs) == {"one": 1, "mixed40": 40, "mixed41": 41}[fields]
    pos, prev, rad = _place(n, fs, seed=n)
    st = _state(gpe, pos, rad, prev=prev)
    if n >= 127:
        who = np.arange(n - len(OUTSIDE), n, dtype=U32)
        st.edit_particles(indices=who, positions=OUTSIDE, previous=OUTSIDE - F32(0.25))
        pos[who], prev[who] = OUTSIDE, OUTSIDE - F32(0.25)
    st.set_fields(fs)
    assert st.fields().tobytes() == fs.tobytes()
    want, touched = M.apply(pos, prev, fs, DT)
    st.apply_fields(DT)
    got_pos, got_prev, got_rad = _arrays(st)
    info = st.fields_info()
    print("n %d %s: touched %d, grid %d x %d, %d list entries" % (n, fields, touched.sum(), info["grid_x"], info["grid_y"],
                                                                  info["list_entries"]))
    bad = np.nonzero(~((bits(got_prev) == bits(want)) | (np.isnan(got_prev) & np.isnan(want))).all(axis=1))[0]
    assert bad.size == 0, (bad[:5], pos[bad[:5]], prev[bad[:5]], got_prev[bad[:5]], want[bad[:5]])
    assert same_bits(got_pos, pos) and same_bits(got_rad, rad)
    # an untouched particle keeps every bit
    assert same_bits(got_prev[~touched], prev[~touched])
    assert info["k"] == len(fs) and info["passes"] == 1 and info["touched"] == int(touched.sum())
    _, gx, gy = grid_dims(WORLD)
    assert (info["grid_x"], info["grid_y"]) == (gx, gy)
    assert info["list_entries"] < gx * gy * len(fs) // (2 if fields == "mixed41" else 8)
    if n >= 127:
        assert touched.any() and (fields == "mixed41" or not touched.all())
        assert not same_prev(got_prev, prev)
    # a second pass starts from the first one's result
    want2, touched2 = M.apply(pos, want, fs, DT)
    st.apply_fields(DT)
    assert same_prev(st.previous_positions(), want2)
    assert st.fields_info()["touched"] == int(touched.sum() + touched2.sum()) and st.fields_info()["passes"] == 2
    tags = _end(st)
    assert TAGS <= tags


def test_the_sum_runs_in_ascending_index_on_the_device(gpe):
    """1e8, 1 and -1e8 in three overlapping fields of three shapes: 0 with the 1 in the middle or in front, -1 * dt2 with it
    last.  dt = 1."""
    region = {M.EVERYWHERE: (0, 0, 0, 0), M.CIRCLE: (50, 50, 30, 0), M.BOX: (40, 40, 60, 60)}
    pos = np.array([[50, 50], [55, 45], [41, 59]], F32)
    rad = np.full(3, 0.5, F32)
    st = _state(gpe, pos, rad)
    seen = set()
    for values in itertools.permutations((1e8, 1.0, -1e8)):
        for shapes in ((M.EVERYWHERE, M.CIRCLE, M.BOX), (M.BOX, M.EVERYWHERE, M.CIRCLE)):
            fs = M.rows(*[M.field(s, M.UNIFORM, region=region[s], f=(v, 0.0)) for s, v in zip(shapes, values)])
            _set(st, pos, pos, rad)
            st.set_fields(fs)
            st.apply_fields(1.0)
            want, _ = M.apply(pos, pos, fs, 1.0)
            got = st.previous_positions()
            assert same_bits(got, want), values
            expect = F32(pos[:, 0] - F32(1.0)) if values[2] == 1.0 else pos[:, 0]
            assert same_bits(got[:, 0], expect), values
            seen.add(float(got[0, 0]))
    assert seen == {50.0, 49.0}
    _end(st)


# ---- 2. no result rests on the grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [(200.0, 200.0), (1000.0, 500.0), (90.0, 140.0), (1e-3, 1e-3), (200.0, INF)])
def test_the_same_set_under_other_worlds(gpe, world):
    """The model knows no world: the same particles and fields under grids of other cell sizes, a grid that covers a part
    of them, a grid that covers none, and a world that leaves one cell.  (COMPAT: particles outside the world are outside any box the native step
    takes.)"""
    fs = _mixed_fields(True)
    pos, prev, rad = _place(2001, fs, seed=5)
    st = _state(gpe, pos, rad, prev=prev, world=world, mode=gpe.MODE_COMPAT)
    st.set_fields(fs)
    want, touched = M.apply(pos, prev, fs, DT)
    st.apply_fields(DT)
    assert same_prev(st.previous_positions(), want)
    info = st.fields_info()
    assert info["touched"] == int(touched.sum())
    if not math.isfinite(world[1]):
        assert (info["grid_x"], info["grid_y"], info["list_entries"]) == (1, 1, 41)
    elif world[0] < 1:
        # every coordinate of the set lies more than 2^17 cells out: 40 fields in every list (the empty box in none), and
        # the entry cap has coarsened the grid
        assert info["grid_x"] == info["grid_y"] < 1024 and info["list_entries"] == 40 * info["grid_x"] * info["grid_y"]
    else:
        assert (info["grid_x"], info["grid_y"]) == grid_dims(world)[1:]
    _end(st)


def test_4095_boxes_and_one_everywhere_field(gpe):
    n = 6000
    gx, gy = np.meshgrid(np.arange(64), np.arange(64))
    lo = (np.stack([gx.ravel(), gy.ravel()], axis=1) * 3.125).astype(F32)
    rng = np.random.default_rng(40)
    fs = np.zeros(4096, M.DTYPE)
    fs["shape"], fs["kind"] = M.BOX, rng.integers(0, 4, 4096)
    fs["x0"], fs["y0"], fs["x1"], fs["y1"] = lo[:, 0], lo[:, 1], lo[:, 0] + F32(3.125), lo[:, 1] + F32(3.125)   # closed: neighbours share borders
    fs["px"], fs["py"] = lo[:, 0] + F32(1.5), lo[:, 1] + F32(1.5)
    fs["fx"], fs["fy"] = rng.uniform(-50, 50, 4096), rng.uniform(-50, 50, 4096)
    fs["strength"] = np.where(fs["kind"] == M.DRAG, rng.uniform(0, 1, 4096), rng.uniform(-300, 300, 4096))
    fs[2000] = M.field(M.EVERYWHERE, M.UNIFORM, f=(0.0, 25.0))[0]
    pos = rng.uniform(0.5, 199.5, (n, 2)).astype(F32)
    pos[:500] = (rng.integers(0, 65, (500, 2)) * 3.125).astype(F32)    # on the shared corners: up to four boxes each
    pos[500:1000, 0] = (rng.integers(0, 65, 500) * 3.125).astype(F32)  # on shared edges
    prev = (pos - rng.uniform(-0.3, 0.3, (n, 2))).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, prev=prev)
    st.set_fields(fs)
    want, touched = M.apply(pos, prev, fs, DT)
    st.apply_fields(DT)
    assert same_prev(st.previous_positions(), want) and same_bits(st.positions(), pos)
    info = st.fields_info()
    assert info["k"] == 4096 and info["touched"] == int(touched.sum()) == n
    cells = info["grid_x"] * info["grid_y"]
    assert cells < info["list_entries"] <= 4 << 20
    print("grid %d x %d, %d entries" % (info["grid_x"], info["grid_y"], info["list_entries"]))
    with pytest.raises(gpe.GpeError) as e:                             # 4097 is one too many; the set stays
        st.set_fields(np.concatenate([fs, fs[:1]]))
    assert e.value.status == gpe._lib.GPE_ERR_INVALID_ARG and len(st.fields()) == 4096
    _end(st)


def test_far_and_huge_fields(gpe):
    fs = M.rows(M.field(M.BOX, M.UNIFORM, region=(-1e30, -1e30, 1e30, 1e30), f=(3.0, 4.0)),          # accepts everything finite
                M.field(M.CIRCLE, M.RADIAL, region=(3e9, 30, 3e9, 0), pole=(3e9, 30), strength=50.0),  # its rim crosses the world
                M.field(M.BOX, M.DRAG, region=(3e9, 3e9, 3.1e9, 3.1e9), strength=0.5),                # far and outside
                M.field(M.CIRCLE, M.VORTEX, region=(1e30, 0, 1, 0), pole=(1e30, 0), strength=5.0),     # dx * dx overflows
                M.field(M.CIRCLE, M.RADIAL, M.LINEAR, region=(100, 100, 1e6, 0), pole=(-1e6, 100), strength=80.0, reach=2e6),
                M.field(M.BOX, M.VORTEX, region=(50, 50, 150, 150), pole=(1e20, 1e20), strength=9.0),  # a pole whose distance overflows
                M.field(M.CIRCLE, M.DRAG, region=(100, 100, 40, 0), strength=0.25))
    pos, prev, rad = _place(3001, fs, seed=8)
    pos[-3:] = [[3.05e9, 3.05e9], [1e30, 0.5], [-1e29, 7.0]]
    prev[-3:] = pos[-3:]
    st = _state(gpe, pos, rad, prev=prev, mode=gpe.MODE_COMPAT)
    st.set_fields(fs)
    want, touched = M.apply(pos, prev, fs, DT)
    st.apply_fields(DT)
    assert same_prev(st.previous_positions(), want)
    info = st.fields_info()
    assert info["touched"] == int(touched.sum()) and touched[-3:].all()
    assert info["list_entries"] >= 4 * info["grid_x"] * info["grid_y"]    # the far ones are in every list
    _end(st)


# ---- 3. the kicks ---------------------------------------------------------------------------------------------------
def test_a_drag_box_and_a_uniform_box_are_the_two_kicks(gpe):
    L = gpe._lib
    lo, hi, s, f = (40.0, 30.0), (150.0, 120.0), 0.8125, (70.0, -35.0)
    pos, prev, rad = _place(4001, M.rows(M.field(M.BOX, region=lo + hi)), seed=21)
    st = _state(gpe, pos, rad, prev=prev)
    twin = _state(gpe, pos, rad, prev=prev)
    # the acceleration in front of the drag: drags act first all the same
    st.set_fields(M.rows(M.field(M.BOX, M.UNIFORM, region=lo + hi, f=f), M.field(M.BOX, M.DRAG, region=lo + hi, strength=s)))
    st.apply_fields(DT)
    dt2 = F32(F32(DT) * F32(DT))
    k1 = twin.kick_box(lo, hi, L.VEL_SCALE, (s, s))
    k2 = twin.kick_box(lo, hi, L.VEL_ADD, (float(F32(f[0]) * dt2), float(F32(f[1]) * dt2)))
    assert same_bits(st.previous_positions(), twin.previous_positions()) and same_bits(st.positions(), twin.positions())
    assert st.fields_info()["touched"] == k1 == k2 and 500 < k1 < 4001
    assert not same_bits(st.previous_positions(), prev)
    _end(twin)
    _end(st)


# ---- 4. the hook ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_oracle_plus_the_model(gpe, pool, mode):
    frames, total = pool
    L = gpe._lib
    st = _pool_state(gpe, mode=L.MODE_COMPAT if mode == "compat" else None)
    for s in range(POOL_STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_prev(prev, frames[s][1]), s
    info, pipe = st.fields_info(), st.ctx.pipeline_info()
    assert info["passes"] == POOL_STEPS and info["touched"] == total and info["k"] == 4 and total > POOL_STEPS * 500
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == POOL_STEPS
    else:
        assert pipe["compat_steps"] == POOL_STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_loop_with_and_without_resorts(gpe, pool, pool_resorted, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else None
    for (frames, total), every, first in ((pool, 0, False), (pool_resorted, 16, True)):
        st = _pool_state(gpe, mode=m)
        st.run(DT, POOL_STEPS, resort_every=every, resort_first=first)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[-1][0]) and same_prev(prev, frames[-1][1]), every
        info = st.fields_info()
        assert info["passes"] == POOL_STEPS and info["touched"] == total
        _end(st)
    # the loop of gpe_step with the same re-sorts
    frames, total = pool_resorted
    st = _pool_state(gpe, mode=m)
    for s in range(POOL_STEPS):
        st.update(DT, resort=(s % 16 == 0))
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_prev(prev, frames[-1][1])
    assert st.fields_info()["touched"] == total
    _end(st)


def test_the_fields_do_something(pool, pool_plain):
    """the scene with fields leaves the plain one at once: the references differ, so the equalities above mean something"""
    assert not same_bits(pool[0][0][1], pool_plain[0][0][1])          # prev after step 1
    assert not same_bits(pool[0][19][0], pool_plain[0][19][0])


def test_fields_run_behind_the_colliders(gpe, oracle):
    """A particle the collider pass pushes across a region's border is kicked in that very step."""
    rng = np.random.default_rng(3)
    n = 300
    pos = rng.uniform(5, 195, (n, 2)).astype(F32)
    pos[:, 1] = pos[:, 1] * F32(0.4)                                   # the others stay clear of y > 80
    pos[0] = (100.0, 103.0)                                            # inside the disc: pushed to (100, 104.5)
    rad = np.full(n, 0.5, F32)
    cs = np.array([[100, 100, 100, 100, 4]], F32)
    fs = M.rows(M.field(M.BOX, M.UNIFORM, region=(90, 104.25, 110, 120), f=(0.0, 3600.0)))
    assert not M.matches(pos[:1], fs[0])[0]
    tw = MC.Twin(oracle, pos, rad, world=WORLD)
    tw.set_colliders(cs)
    tw.step(DT)                                                        # the step, then the colliders
    p, q, _ = tw.arrays()
    assert tuple(p[0]) == (100.0, 104.5) and tuple(q[0]) == (100.0, 103.0)
    want, touched = M.apply(p, q, fs, DT)
    assert touched[0] and touched.sum() == 1 and want[0, 1] == F32(103.0) - F32(3600.0) * F32(F32(DT) * F32(DT))
    for mode in (None, gpe.MODE_COMPAT):
        st = _state(gpe, pos, rad, mode=mode)
        st.set_colliders(cs)
        st.set_fields(fs)
        st.update(DT)
        got = _arrays(st)
        assert same_bits(got[0], p) and same_bits(got[1], want)
        assert st.fields_info()["touched"] == 1 and st.colliders_info()["pushed"] == 1
        _end(st)
    tw.close()


# ---- 5. observers ---------------------------------------------------------------------------------------------------
def test_tracer_and_monitor_frames_show_the_kicked_prev(gpe, pool):
    frames, _ = pool
    pos0, _ = M.pool_scene()
    in_vortex = np.nonzero(M.matches(pos0, M.POOL_FIELDS[0]))[0]
    uids = np.concatenate([in_vortex[:4], [0, 2999]]).astype(U32)
    st = _pool_state(gpe)
    st.enable_uids()
    st.tracers_begin(uids, every=1, frames=32, prev=True)
    st.monitor_begin(every=1, frames=32)
    st.run(DT, 12, resort_every=0, resort_first=False)
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == 12 and recorded == 12
    for s in range(12):
        pos, prev = frames[s]
        assert same_bits(tr.pos[s], pos[uids]) and same_bits(tr.prev[s], prev[uids]), s
        vx, vy = pos[:, 0] - prev[:, 0], pos[:, 1] - prev[:, 1]
        assert rec["max_v2"][s] == (vx * vx + vy * vy).max() and rec["n"][s] == 3000, s
    # the frame of step 1 already holds the vortex's kick: a particle at rest would have prev == its start
    assert not same_bits(tr.prev[0][:4], pos0[uids[:4]])
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 6. what a pass leaves alone, and a context without fields ------------------------------------------------------
def test_a_pass_touches_prev_alone(gpe):
    L = gpe._lib
    st = _pool_state(gpe)
    st.run(DT, 8, resort_every=0, resort_first=True)
    pos, prev, rad = _arrays(st)
    before = st.ctx.pipeline_info()
    st.apply_fields(DT)
    st.apply_fields(DT)
    after = st.ctx.pipeline_info()
    assert before["pipeline"] == L.PIPELINE_NATIVE
    for name in ("native_sorts", "roster_stamp", "native_steps"):
        assert before[name] == after[name], name
    got = _arrays(st)
    assert same_bits(got[0], pos) and same_bits(got[2], rad) and not same_bits(got[1], prev)
    want, _ = M.apply(pos, prev, M.POOL_FIELDS, DT)
    want, _ = M.apply(pos, want, M.POOL_FIELDS, DT)
    assert same_prev(got[1], want)
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_fields_nothing_changes_and_nothing_is_allocated(gpe, pool, pool_plain, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else None
    plain, _ = pool_plain
    never = _pool_state(gpe, mode=m, fields=None, profiling=True)
    cleared = _pool_state(gpe, mode=m, profiling=True)
    assert TAGS - {"grid.field_cell_start", "grid.field_items"} <= _live_tags(cleared)
    cleared.clear_fields()
    empty = dict(k=0, passes=0, touched=0, grid_x=0, grid_y=0, list_entries=0)
    assert len(cleared.fields()) == 0 and cleared.fields_info() == empty and never.fields_info() == empty
    for st in (never, cleared):
        st.apply_fields(DT)                                            # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, plain[19][0]) and same_bits(prev, plain[19][1])
        assert "Fields" not in st.ctx.timings()
        assert not any(t.startswith("grid.field_") for t in _live_tags(st))
    assert not any(t.startswith("grid.field_") for t, _, _, _ in never.ctx.guard_registry())   # not even a released one
    _end(never)
    _end(cleared)
    armed = _pool_state(gpe, mode=m, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), pool[0][19][0])
    assert armed.ctx.timings()["Fields"][1] == 20
    _end(armed)


# ---- 7. lifecycle ---------------------------------------------------------------------------------------------------
def _same_as_twin(st, tw, what):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    assert same_bits(got[0], pos) and same_prev(got[1], prev) and same_bits(got[2], rad), what
    assert st.fields().tobytes() == tw.fields.tobytes(), what


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_survives_everything_but_set_fields(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    m = L.MODE_COMPAT if mode == "compat" else L.MODE_NATIVE
    world, gravity = (100.0, 100.0), (0.0, 40.0)
    fs = M.rows(M.field(M.CIRCLE, M.VORTEX, region=(35, 35, 25, 0), pole=(35, 35), strength=300.0),
                M.field(M.CIRCLE, M.RADIAL, M.LINEAR, region=(70, 40, 22, 0), pole=(70, 40), strength=600.0, reach=22.0),
                M.field(M.BOX, M.DRAG, region=(5, 60, 95, 99), strength=0.9),
                M.field(M.CIRCLE, M.UNIFORM, region=(150, 150, 12, 0), f=(0.0, -500.0)))   # outside the first world
    rng = np.random.default_rng(12)
    n = 3999
    pos = rng.uniform(1, 99, (n, 2)).astype(F32)
    pos[:, 1] = pos[:, 1] * F32(0.7)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, mode=m)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    st.set_fields(fs); tw.set_fields(fs)

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what)
        info = st.fields_info()
        assert (info["passes"], info["touched"]) == (tw.passes, tw.touched), what
        return info

    steps("start")
    pos2 = rng.uniform(1, 99, (n - 500, 2)).astype(F32)
    _set(st, pos2, pos2, rad[:n - 500]); tw.set_particles(pos2, pos2, rad[:n - 500])
    steps("set_particles")
    add = rng.uniform(5, 95, (300, 2)).astype(F32)
    st.add_particles(add, np.full(300, 0.5, F32)); tw.add(add, np.full(300, 0.5, F32))
    steps("add")
    assert st.remove_particles_in_circle((50, 40), 12.0) == tw.remove_circle(50, 40, 12.0) > 0
    steps("remove")
    who = np.arange(0, 400, 2, dtype=U32)
    where = rng.uniform(25, 45, (200, 2)).astype(F32)                  # into the vortex
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
    before = steps("uids off")
    # gpe_set_world: the grid follows, the field at (150, 150) in the newly uncovered part acts
    st.ctx.call("gpe_set_world", 200.0, 200.0); tw.set_world(200.0, 200.0)
    who = np.array([3, 4], U32)
    where = np.array([[153.0, 150.0], [150.0, 144.0]], F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    touched = tw.touched
    st.apply_fields(DT); tw.apply_fields(DT)
    _same_as_twin(st, tw, "set_world")
    after = st.fields_info()
    assert tw.touched >= touched + 2 and after["touched"] == tw.touched
    assert (before["grid_x"], after["grid_x"]) == (grid_dims(world)[1], grid_dims((200.0, 200.0))[1])
    assert st.previous_positions()[3, 1] == F32(150.0) + F32(500.0) * F32(F32(DT) * F32(DT))
    steps("after set_world")
    # save -> load: the set and a bit-identical continuation
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["fields"].tobytes() == M.stored(fs).tobytes()
    back = gpe.State.load(path, mode=m, flags=L.FLAG_GUARD_ALLOCS)
    assert back.fields().tobytes() == st.fields().tobytes()
    for _ in range(3):
        back.update(DT)
    steps("beside the loaded one")
    assert same_bits(back.positions(), st.positions()) and same_prev(back.previous_positions(), st.previous_positions())
    assert back.fields_info()["passes"] == 3
    _end(back)
    # a new set replaces the old one and zeroes the counters
    st.set_fields(fs[:2]); tw.set_fields(fs[:2])
    assert st.fields_info()["passes"] == 0 and st.fields_info()["touched"] == 0
    steps("new set")
    # k = 0 frees the buffers; a context without fields writes none and loads none
    assert TAGS <= _live_tags(st)
    st.set_fields(np.zeros(0, M.DTYPE))
    assert not any(t.startswith("grid.field_") for t in _live_tags(st)) and len(st.fields()) == 0
    st.save(path)
    with np.load(path) as d:
        assert "fields" not in d.files
    tw.close()
    _end(st)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    pos, rad = M.pool_scene(600)
    st = _state(gpe, pos, rad, world=M.POOL_WORLD, gravity=M.POOL_GRAVITY)
    tw = M.Twin(oracle, pos, rad, world=M.POOL_WORLD, gravity=M.POOL_GRAVITY)
    st.set_fields(M.POOL_FIELDS); tw.set_fields(M.POOL_FIELDS)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.fields_info()

    def untouched(what):
        assert st.fields().tobytes() == M.POOL_FIELDS.tobytes(), what
        assert st.fields_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    def ptr(rows):
        rows = np.ascontiguousarray(rows, M.DTYPE)
        return rows.ctypes.data_as(C.POINTER(L.GpeField)), rows             # (the array is kept alive by the caller)

    def set_one(**changes):
        """POOL_FIELDS[1] (a circle, RADIAL, LINEAR) with some members changed, behind a good row"""
        rows = M.POOL_FIELDS[:2].copy()
        for name, v in changes.items():
            rows[1][name] = v
        p, keep = ptr(rows)
        return lib.gpe_set_fields(h, p, 2)

    h = st.ctx.h
    k = C.c_uint64()
    good, keep_good = ptr(M.POOL_FIELDS)
    finfo = L.GpeFieldsInfo(struct_size=C.sizeof(L.GpeFieldsInfo))
    assert lib.gpe_set_fields(None, good, 4) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_fields(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_fields(None, DT) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_fields_info(None, C.byref(finfo)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    many, keep_many = ptr(np.repeat(M.POOL_FIELDS[:1], L.FIELDS_MAX + 1))
    bad = {
        "NULL fields with k > 0": lambda: lib.gpe_set_fields(h, None, 2),
        "k > GPE_FIELDS_MAX": lambda: lib.gpe_set_fields(h, many, L.FIELDS_MAX + 1),
        "unknown shape": lambda: set_one(shape=3),
        "unknown kind": lambda: set_one(kind=4),
        "unknown falloff": lambda: set_one(falloff=2),
        "flags": lambda: set_one(flags=1),
        "negative radius": lambda: set_one(x1=-0.25),
        "falloff on UNIFORM": lambda: set_one(kind=M.UNIFORM),
        "falloff on DRAG": lambda: set_one(kind=M.DRAG, strength=0.5),
        "LINEAR with reach 0": lambda: set_one(reach=0.0),
        "LINEAR with a negative reach": lambda: set_one(reach=-3.0),
        "DRAG strength above 1": lambda: set_one(kind=M.DRAG, falloff=M.NONE, strength=1.5),
        "DRAG strength below 0": lambda: set_one(kind=M.DRAG, falloff=M.NONE, strength=-0.5),
        "dt NaN": lambda: lib.gpe_apply_fields(h, NAN),
        "dt inf": lambda: lib.gpe_apply_fields(h, INF),
        "info struct_size": lambda: lib.gpe_get_fields_info(h, C.byref(L.GpeFieldsInfo(struct_size=C.sizeof(L.GpeFieldsInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_fields_info(h, None),
        "get NULL k": lambda: lib.gpe_get_fields(h, None, 0, None),
        "get NULL out": lambda: lib.gpe_get_fields(h, None, 3, C.byref(k)),
    }
    for name in ("x0", "y0", "x1", "y1", "px", "py", "fx", "fy", "strength", "reach"):
        for v in (NAN, INF, -INF):
            bad["%s = %r" % (name, v)] = lambda name=name, v=v: set_one(**{name: v})
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        untouched(what)
    # the other way round: sharding a context that holds fields
    keys = np.arange(600, dtype=U32)
    sharding = {
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, 600, 500),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), 600, 0),
    }
    for what, call in sharding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"force fields" in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK                    # switching them off is no sharding
    # accepted: -0.0 as a radius (stored as +0), an empty box, DRAG strengths 0 and 1, a DRAG that carries a reach
    rows = M.rows(M.field(M.CIRCLE, M.UNIFORM, region=(1, 2, -0.0, 0), f=(1.0, 1.0)),
                  M.field(M.BOX, M.UNIFORM, region=(30, 20, 10, 40), f=(1.0, 1.0)),
                  M.field(M.EVERYWHERE, M.DRAG, strength=1.0, reach=5.0), M.field(M.EVERYWHERE, M.DRAG, strength=0.0))
    p, keep = ptr(rows)
    assert lib.gpe_set_fields(h, p, 4) == L.GPE_OK
    out = np.zeros(3, M.DTYPE)
    out["strength"] = 7.0
    assert lib.gpe_get_fields(h, out.ctypes.data_as(C.POINTER(L.GpeField)), 1, C.byref(k)) == L.GPE_OK and k.value == 4
    assert bits(out["x1"][:1]).tolist() == [0] and out["y0"][0] == 2.0
    assert out["strength"].tolist() == [0.0, 7.0, 7.0]                 # past the capacity: left as they were
    # the context goes on as the twin does
    st.set_fields(M.POOL_FIELDS)
    tw.passes = tw.touched = 0
    for _ in range(5):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_fields(gpe, how):
    L = gpe._lib
    pos, rad = M.pool_scene(600)
    st = _state(gpe, pos, rad, world=M.POOL_WORLD)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_fields(M.POOL_FIELDS)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.fields()) == 0 and st.fields_info()["k"] == 0
    st.apply_fields(DT)
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    assert not any(t.startswith("grid.field_") for t in _live_tags(st))
    _end(st)


def test_fields_before_there_are_particles(gpe):
    L = gpe._lib
    ctx = gpe.Context(world=M.POOL_WORLD, gravity=M.POOL_GRAVITY, flags=L.FLAG_GUARD_ALLOCS)
    ps = gpe.ParticleSystem(ctx)
    ps.set_fields(M.POOL_FIELDS)
    ps.apply_fields(DT)                                                # no particles: GPE_OK, nothing done
    assert ps.fields_info() == dict(k=4, passes=0, touched=0, grid_x=0, grid_y=0, list_entries=0)
    pos, rad = M.pool_scene(101)
    f = C.POINTER(C.c_float)
    ctx.call("gpe_set_particles", pos.ctypes.data_as(f), None, rad.ctypes.data_as(f), 101)
    ps.apply_fields(DT)
    want, touched = M.apply(pos, pos, M.POOL_FIELDS, DT)
    assert same_prev(ctx.download(L.PREV, F32, (-1, 2)), want) and touched.any()
    assert ps.fields_info()["touched"] == int(touched.sum())
    ctx.guard_check()
    assert ctx.guard_damaged == 0
    ctx.close()
