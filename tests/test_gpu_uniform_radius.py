"""GPU (-m gpu): the native step's uniform-radius kernels and its key-less kept-table steps.

While every radius of a context is one ordinary number (1e-30 .. 1e30) the hash and the direct-slot tiles take it as a
kernel constant (gpe_pipeline_info.uniform_radius == 1); GPE_FLAG_GENERAL_RADII keeps the kernels that read a radius per
particle.  Independently, a step that keeps its block table stores no sort keys: the gated histogram launch forms them
from the positions on the steps that sort.  Everything here is compared bit for bit -- uniform against general, against
the oracle, against sorting every step and against the fused histograms (which store the keys every step, as before).

A scene must sort in two radix passes to keep its table at all, which a 40 x 40 world never does; the kept-table cases
use a 200 x 200 world at the benchmark density, about 12.5 k particles.
"""
import ctypes

import numpy as np
import pytest

from tests import _oracle_model as om

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0
WORLD = (200.0, 200.0)
LEFT_THE_BOX = "native collide: a particle left the world box between steps"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    ba, bb = _bits(a), _bits(b)
    if not np.array_equal(ba, bb):
        bad = np.flatnonzero((ba != bb).reshape(len(ba), -1).any(1))
        pytest.fail("%s: %d particles differ, first %s: %s / %s" % (what, len(bad), bad[:4], a[bad[:2]], b[bad[:2]]))


def _scene(gpe, radius, seed=61, walls=True):
    """The bench density in a 200 x 200 world; with `walls`, particles on the four walls, in and near the four corners
    (the Verlet clamp puts them at r and W - r: cells along the walls fill up) and a few coincident ones."""
    n = int(gpe.scenes.REF_DENSITY * WORLD[0] * WORLD[1])
    pos, rad = gpe.scenes.uniform_cloud(n, WORLD, seed=seed, radius=radius)
    if walls:
        rng = np.random.default_rng(seed + 1)
        w, h = np.float32(WORLD[0]), np.float32(WORLD[1])
        k = 160
        t = (rng.random(k, dtype=np.float32) * w).astype(np.float32)
        pos[0:k] = np.stack([np.zeros(k, np.float32), t], 1)                       # x = 0
        pos[k:2 * k] = np.stack([np.full(k, w), t], 1)                             # x = W
        pos[2 * k:3 * k] = np.stack([t, np.zeros(k, np.float32)], 1)               # y = 0
        pos[3 * k:4 * k] = np.stack([t, np.full(k, h)], 1)                         # y = H
        corners = np.array([[0, 0], [w, 0], [0, h], [w, h]], np.float32)
        for j, c in enumerate(corners):
            lo = 4 * k + 12 * j
            pos[lo:lo + 4] = c                                                     # four in the corner itself
            inward = np.where(c == 0, np.float32(1), np.float32(-1))
            pos[lo + 4:lo + 12] = c + inward * rng.random((8, 2), dtype=np.float32) * np.float32(1.5)
    return pos.astype(np.float32), rad


def _info(st):
    st.ctx.sync()
    return st.ctx.pipeline_info()


# ---------------------------------------------------------------------------------------------------------------------
# 2. uniform against general and the oracle


@pytest.mark.parametrize("radius,gravity,guard", [(0.5, (0.0, 0.0), False), (0.5, (2.0, -9.81), True),
                                                   (0.37, (0.0, 0.0), False), (0.37, (-3.0, -9.81), False)])
def test_uniform_equals_general_and_the_oracle(gpe, oracle, radius, gravity, guard):
    L = gpe._lib
    pos, rad = _scene(gpe, radius)
    extra = L.FLAG_GUARD_ALLOCS if guard else 0
    uni = gpe.State(pos, rad, world=WORLD, gravity=gravity, flags=extra)
    gen = gpe.State(pos, rad, world=WORLD, gravity=gravity, flags=extra | L.FLAG_GENERAL_RADII)
    sim = oracle.Sim(pos, rad, oracle.default_params(WORLD[0], WORLD[1], radius, gravity=gravity))
    assert uni.ctx.pipeline_info()["uniform_radius"] == 1 and gen.ctx.pipeline_info()["uniform_radius"] == 0
    steps = 40
    for s in range(steps):
        rs = s == 0
        uni.update(DT, resort=rs); gen.update(DT, resort=rs); sim.step(DT, resort=rs)
        pu, qu = uni.positions(), uni.previous_positions()
        _same_bits(pu, gen.positions(), "uniform vs general, pos, step %d" % s)
        _same_bits(qu, gen.previous_positions(), "uniform vs general, prev, step %d" % s)
        _same_bits(pu, sim.pos, "uniform vs oracle, pos, step %d" % s)
        _same_bits(qu, sim.prev, "uniform vs oracle, prev, step %d" % s)
    iu, ig = _info(uni), _info(gen)
    print("uniform", iu, "general", ig)
    assert iu["uniform_radius"] == 1 and ig["uniform_radius"] == 0
    assert iu["pipeline"] == L.PIPELINE_NATIVE and iu["native_steps"] == steps and iu["compat_steps"] == 0, iu
    assert iu["sort_passes"] == 2 and iu["native_sorts"] < steps, iu              # the table was kept
    assert ig["native_sorts"] == iu["native_sorts"], (iu, ig)
    if guard:
        assert uni.ctx.guard_check() == [] and gen.ctx.guard_check() == []
    uni.close(); gen.close(); sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the other tile forms: tiles beyond the direct-slot form, in whichever variant they have


def _crushed_blobs(sizes):
    """The scene of test_gpu_native.test_native_crushed_cells_are_exact."""
    rng = np.random.default_rng(21)
    world = (40.0, 40.0)
    bg = (rng.random((1500, 2), dtype=np.float32) * np.float32(40.0)).astype(np.float32)
    blobs = [np.array(c, np.float32) + rng.random((k, 2), dtype=np.float32) * np.float32(0.9)
             for c, k in zip(((11.1, 11.1), (22.1, 16.6), (30.9, 30.9)), sizes)]
    pos = np.concatenate([bg] + blobs).astype(np.float32)
    return pos, np.full(len(pos), 0.5, np.float32), world, (0.0, 0.0), 3


def _half_tiles(gpe, n, tiles, seed):
    """The scenes of test_gpu_native's half-tile and hinted-tile tests at the smallest size that still has them: a patch
    of tiles x tiles tiles at 1.9 x the benchmark density (they keep more than the direct-slot form's 928: the half-tile
    launch, and from the second step on the dense launch's front workgroups, redo them as 32 x 16 halves) and a blob
    crowded beyond the halves, in an ordinary cloud under gravity."""
    world = gpe.scenes.world_for(n)
    pos, _ = gpe.scenes.uniform_cloud(n, world, seed=seed)
    rng = np.random.default_rng(seed + 1)
    side = np.float32(tiles * 32 * 1.1)
    extra = int(0.9 * gpe.scenes.REF_DENSITY * float(side) ** 2)
    patch = (np.array([150.0, 60.0], np.float32) + rng.random((extra, 2), dtype=np.float32) * side).astype(np.float32)
    blob = (np.array([40.0, 30.0], np.float32) + rng.random((1500, 2), dtype=np.float32) * np.float32(20.0)).astype(np.float32)
    pos = np.concatenate([pos, patch, blob]).astype(np.float32)
    return pos, np.full(len(pos), 0.5, np.float32), world, (2.0, -9.81), 12


@pytest.mark.parametrize("scene", ["blobs-90-150-240", "blobs-300-640-1000", "half-tiles", "hinted-tiles"])
def test_tile_forms_beyond_direct_uniform_equals_general(gpe, scene):
    L = gpe._lib
    if scene.startswith("blobs"):
        pos, rad, world, g, steps = _crushed_blobs(tuple(int(v) for v in scene.split("-")[1:]))
        flags = L.FLAG_NATIVE_FORCE
    elif scene == "half-tiles":
        pos, rad, world, g, steps = _half_tiles(gpe, 60_000, 2, 23)
        flags = 0
    else:
        pos, rad, world, g, steps = _half_tiles(gpe, 120_000, 3, 31)
        flags = 0
    uni = gpe.State(pos, rad, world=world, gravity=g, flags=flags)
    gen = gpe.State(pos, rad, world=world, gravity=g, flags=flags | L.FLAG_GENERAL_RADII)
    over = []
    for s in range(steps):
        uni.update(DT, resort=(s == 0)); gen.update(DT, resort=(s == 0))
        _same_bits(uni.positions(), gen.positions(), "%s: pos, step %d" % (scene, s))
        _same_bits(uni.previous_positions(), gen.previous_positions(), "%s: prev, step %d" % (scene, s))
        over.append(_info(uni)["overflow_tiles"])
    iu, ig = _info(uni), _info(gen)
    print(scene, "overflow tiles per step", over, iu)
    assert iu["uniform_radius"] == 1 and ig["uniform_radius"] == 0
    assert iu["compat_steps"] == 0 and max(over) > 0, (over, iu)                   # the forms beyond Direct ran
    uni.close(); gen.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. switching off


def _switch_off_case(gpe, how):
    L = gpe._lib
    pos, rad = _scene(gpe, 0.5, seed=71)
    uni = gpe.State(pos, rad, world=WORLD, gravity=(1.0, -9.81))
    gen = gpe.State(pos, rad, world=WORLD, gravity=(1.0, -9.81), flags=L.FLAG_GENERAL_RADII)
    both = (uni, gen)
    for st in both:
        st.run(DT, 3, resort_every=0, resort_first=True)
    assert _info(uni)["uniform_radius"] == 1 and _info(gen)["uniform_radius"] == 0
    for st in both:
        if how == "edit":
            assert st.edit_particles(indices=[777], radii=[0.3]) == 1
        elif how == "add":
            st.add_particles(np.array([[100.25, 100.5]], np.float32), np.array([0.4], np.float32))
        else:
            ptr, nbytes = st.ctx.device_ptr(L.RADIUS)
            assert nbytes == 4 * len(rad)
            r = rad.copy()
            r[777] = 0.3
            st.ctx.call("gpe_buffer_upload", ptr, r.ctypes.data_as(ctypes.c_void_p), r.nbytes)
    assert _info(uni)["uniform_radius"] == 0, how                                  # from the next step on
    for s in range(10):
        for st in both:
            st.update(DT)
        assert uni.ctx.pipeline_info()["uniform_radius"] == 0
        _same_bits(uni.positions(), gen.positions(), "%s: pos, step %d after" % (how, s))
        _same_bits(uni.previous_positions(), gen.previous_positions(), "%s: prev, step %d after" % (how, s))
    assert np.array_equal(_bits(uni.radii()), _bits(gen.radii()))
    assert _info(uni)["compat_steps"] == 0
    uni.close(); gen.close()


@pytest.mark.parametrize("how", ["edit", "add", "device_ptr"])
def test_a_changed_radius_switches_the_uniform_kernels_off(gpe, how):
    _switch_off_case(gpe, how)


def test_equal_radii_again_switch_the_uniform_kernels_back_on(gpe):
    """The decision is native_configure's: an edit that makes the radii equal again (to another value) brings the uniform
    kernels back, with that value."""
    pos, rad = _scene(gpe, 0.5, seed=72, walls=False)
    st = gpe.State(pos, rad, world=WORLD)
    st.run(DT, 2, resort_every=0, resort_first=True)
    assert st.edit_particles(indices=[5], radii=[0.25]) == 1
    assert _info(st)["uniform_radius"] == 0
    assert st.edit_particles(indices=[5], radii=[0.5]) == 1
    assert _info(st)["uniform_radius"] == 1
    st.close()


@pytest.mark.parametrize("radius", [-0.5, 0.0, 1e31])
def test_radii_outside_the_plain_range_never_report_uniform(gpe, radius):
    """One radius for all, but not an ordinary one: negative, zero, above 1e30 (the world sized for the cell size it gives).
    Whatever pipeline such a context is configured for, it does not report the uniform kernels -- at creation, and after
    being configured again.  (Not stepped: what the step does with such radii is the business of other tests.)"""
    rng = np.random.default_rng(9)
    world = (4e32, 4e32) if radius > 1 else (60.0, 60.0)
    pos = (rng.random((800, 2), dtype=np.float32) * np.float32(0.5 * world[0]) + np.float32(0.25 * world[0])).astype(np.float32)
    rad = np.full(len(pos), radius, np.float32)
    st = gpe.State(pos, rad, world=world)
    assert st.ctx.pipeline_info()["uniform_radius"] == 0
    st.ctx.call("gpe_refresh")
    assert st.ctx.pipeline_info()["uniform_radius"] == 0
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. keys: a kept-table step stores none; the gated histogram launch forms them when a sort is due


def test_a_sort_raised_on_a_kept_step_finds_its_keys(gpe, oracle):
    """After step 5 about 1 % of the particles (those in a disc) are kicked to 12 cells per step.  The kick goes through no
    configuration, so the next step keeps its table and its hash stores no keys; the step after it -- the first whose hash
    sees the kicked particles where the Verlet step put them, far out of reach of their blocks and more of them than the
    straggler lists take -- raises need_sort on a kept step: the gated launch forms the keys the hash did not store.
    Bits equal sorting every step, the fused histograms (keys stored every step) and the oracle; native_sorts rises
    there and not on the steps before."""
    L = gpe._lib
    pos, rad = _scene(gpe, 0.5, seed=81)
    kinds = {"default": 0, "sort every step": L.FLAG_SORT_EVERY_STEP, "fused histograms": L.FLAG_FUSED_HISTOGRAMS,
             "general radii": L.FLAG_GENERAL_RADII}
    sts = {k: gpe.State(pos, rad, world=WORLD, flags=f) for k, f in kinds.items()}
    sim = oracle.Sim(pos, rad, oracle.default_params(WORLD[0], WORLD[1], 0.5))
    cell = np.float32(0.5 * 2.2)
    kick = (float(np.float32(12) * cell), 0.0)
    centre, reach = (40.0, 100.0), float(np.sqrt(0.01 * WORLD[0] * WORLD[1] / np.pi))
    sorts = []
    for s in range(12):
        if s == 5:
            counts = {k: st.kick_circle(centre, reach, L.VEL_SET, kick) for k, st in sts.items()}
            # the oracle's side of the kick (tests/_oracle_model.py: the float32 formulas of include/gpe.h), carried into
            # a Sim that starts from the oracle's own state -- after the re-sort of step 0 both hold the same order
            mask = om.circle_mask(sim.pos, centre[0], centre[1], reach)
            print("kicked", counts, "of", len(pos), "oracle", int(mask.sum()))
            assert set(counts.values()) == {int(mask.sum())} and 0.005 * len(pos) < mask.sum() < 0.02 * len(pos), counts
            p_now, q_now = sim.pos, om.kicked_prev(L.VEL_SET, sim.pos, sim.prev, mask, kick)
            sim.close()
            sim = oracle.Sim(p_now, rad, oracle.default_params(WORLD[0], WORLD[1], 0.5), prev=q_now)
        for st in sts.values():
            st.update(DT, resort=(s == 0))
        sim.step(DT, resort=(s == 0))
        want_p, want_q = sim.pos, sim.prev
        for k, st in sts.items():
            _same_bits(st.positions(), want_p, "%s vs oracle, pos, step %d" % (k, s))
            _same_bits(st.previous_positions(), want_q, "%s vs oracle, prev, step %d" % (k, s))
        sorts.append(_info(sts["default"])["native_sorts"])
    print("native_sorts after each step", sorts)
    assert sorts[5] == sorts[4] == sorts[3] == sorts[2], sorts                     # kept steps up to and with the kick's own
    assert sorts[6] == sorts[5] + 1, sorts                                         # the first hash that sees the kicked cloud
    info = _info(sts["default"])
    assert info["uniform_radius"] == 1 and info["compat_steps"] == 0 and info["sort_passes"] == 2, info
    assert _info(sts["sort every step"])["native_sorts"] >= 12
    for st in sts.values():
        st.close()
    sim.close()


def _raw(st, what, n):
    """The array as the device holds it, through its pointer: works behind a sticky error, which every download reports."""
    ptr, nbytes = st.ctx.device_ptr(what)
    out = np.empty(nbytes // 4, np.uint32)
    st.ctx.call("gpe_buffer_download", ptr, out.ctypes.data_as(ctypes.c_void_p), nbytes)
    return out


def test_a_particle_outside_the_box_gives_the_same_error_and_bits_without_stored_keys(gpe):
    """A position written through gpe_device_ptr(GPE_POS) to outside the world, on a run that keeps its table: the hash
    flags it (key 0, as ever) whether or not it stores keys.  The default context (no keys on kept steps), the fused
    histograms (keys stored every step, as before this file's change) and sorting every step report the same sticky
    error and hold the same bits."""
    L = gpe._lib
    pos, rad = _scene(gpe, 0.5, seed=91, walls=False)
    kinds = {"default": 0, "fused histograms": L.FLAG_FUSED_HISTOGRAMS, "sort every step": L.FLAG_SORT_EVERY_STEP}
    got = {}
    for k, f in kinds.items():
        st = gpe.State(pos, rad, world=WORLD, flags=f)
        st.run(DT, 3, resort_every=0, resort_first=True)
        p = st.positions()
        p[4321] = (-30.0, 77.0)
        ptr, nbytes = st.ctx.device_ptr(L.POS)
        st.ctx.call("gpe_buffer_upload", ptr, p.ctypes.data_as(ctypes.c_void_p), p.nbytes)
        st.update(DT)
        with pytest.raises(L.GpeError) as err:
            st.ctx.sync()
        assert err.value.status == L.GPE_ERR_STATE and LEFT_THE_BOX in str(err.value), (k, str(err.value))
        got[k] = (_raw(st, L.POS, len(pos)), _raw(st, L.PREV, len(pos)))
        st.close()
    for k in ("fused histograms", "sort every step"):
        assert np.array_equal(got["default"][0], got[k][0]), "pos: default vs %s" % k
        assert np.array_equal(got["default"][1], got[k][1]), "prev: default vs %s" % k
