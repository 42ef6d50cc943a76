"""CPU: the swept form of the static colliders' pass as the numpy model states it (tests/_sweep_model.py, include/gpe.h
"static colliders", csrc/k_sweep.h): resting particles get the plain passes' bits, nothing leaves a closed box of thin
walls (float64, no tolerance) where the plain rule loses particles, a particle slides over a polyline's joints without
stopping, the stepped scene of the GPU tests keeps its particles, the table the C++ definition replays
(tests/golden/sweep_cases.txt), the stand-alone test program (tests/cpp/sweep_tests.cpp over csrc/k_sweep.h), plain and
under the host sanitizers, and what needs no device of the binding and of save / load."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _surfaces_model as SM
from tests import _sweep_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TABLE = os.path.join(ROOT, "tests", "golden", "sweep_cases.txt")


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def one(p, prev, colliders, r=0.5, world=S.BOX_WORLD, surfaces=None):
    out, out_prev, info = S.apply([p], [prev], [r], colliders, world, surfaces=surfaces)
    return tuple(out[0]), tuple(out_prev[0]), {k: bool(v[0]) for k, v in info.items()}


# ---- the rule on one particle ----------------------------------------------------------------------------------------
def test_a_thin_wall_holds_a_fast_particle():
    wall = [[0, 100, 200, 100, 0]]
    assert not CM.apply([(50, 120)], [0.5], wall, S.BOX_WORLD)[1][0]   # the plain rule: 20.5 beyond it, untouched
    p, q, info = one((50, 120), (50, 90), wall)
    assert p == (50.0, 99.5) and q == (50.0, 90.0) and info == dict(moved=True, swept=True, stopped=False, plain=False)
    # moving away from it, or along it at a distance: every bit kept
    for pos, prev in (((50, 80), (50, 95)), ((150, 99.5), (50, 99.5)), ((150, 90), (50, 90))):
        p, q, info = one(pos, prev, wall)
        assert p == tuple(map(float, pos)) and q == tuple(map(float, prev)) and not info["moved"], pos
    # a particle that starts beyond the wall stays beyond it
    p, _, info = one((50, 130), (50, 110), wall)
    assert p == (50.0, 130.0) and not info["moved"]
    # with e = 1 the particle leaves with its normal velocity reflected, from the wall's face
    p, q, info = one((50, 120), (50, 90), wall, surfaces=SM.rows((1.0, 0.0)))
    assert p == (50.0, 99.5) and q == (50.0, 129.5) and info["swept"] and not info["stopped"]


def test_the_first_contact_wins_and_a_corner_stops_the_particle():
    near, far = [0, 100, 200, 100, 0], [0, 110, 200, 110, 3]
    for cs in ([near, far], [far, near]):                              # the thick wall behind is deeper at pos: t decides
        p, _, info = one((50, 109), (50, 90), cs)
        assert p == (50.0, 99.5) and info["swept"]
    # into a corner of two thin walls: the push out of the first leads through the second, the particle stops where it
    # first touched
    corner = [[100, 0, 100, 200, 0], [0, 100, 200, 100, 0]]
    p, q, info = one((110, 130), (90, 95), corner)
    assert info["stopped"] and info["swept"] and q == (90.0, 95.0)
    assert p[0] < 100 and p[1] < 100 and abs(p[1] - 99.5) < 1e-4


def test_resting_and_not_finite_particles_get_the_plain_bits():
    """m == 0 for every particle: the colliders' model, and with surfaces the surfaces' model, bit for bit; a prev that
    is NaN or infinite likewise"""
    cs, surf, pos, prev, rad = SM.collider_scene(4000)
    want, moved = CM.apply(pos, rad, cs, SM.ONE_PASS_WORLD)
    got, got_prev, info = S.apply(pos, pos, rad, cs, SM.ONE_PASS_WORLD)
    assert same_bits(got, want) and same_bits(got_prev, pos) and np.array_equal(info["moved"], moved)
    assert info["plain"].all() and not info["swept"].any() and not info["stopped"].any() and moved.sum() > 1000
    want, want_prev, moved, _ = SM.apply(pos, pos, rad, cs, surf, SM.ONE_PASS_WORLD)
    got, got_prev, info = S.apply(pos, pos, rad, cs, SM.ONE_PASS_WORLD, surfaces=surf)
    assert same_bits(got, want) and same_bits(got_prev, want_prev) and np.array_equal(info["moved"], moved)
    odd = ~np.isfinite(prev).all(axis=1)
    assert odd.sum() > 100
    want, want_prev, moved, _ = SM.apply(pos[odd], prev[odd], rad[odd], cs, surf, SM.ONE_PASS_WORLD)
    got, got_prev, info = S.apply(pos[odd], prev[odd], rad[odd], cs, SM.ONE_PASS_WORLD, surfaces=surf)
    assert same_bits(got, want) and same_bits(got_prev, want_prev) and info["plain"].all() and moved.any()


# ---- the box ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surfaces", [False, True], ids=["plain", "surfaces"])
@pytest.mark.parametrize("R", [0.0, 0.05])
def test_nothing_leaves_the_box(R, surfaces):
    """Four walls of radius R closed to a box, a V of two thin walls, a straight polyline, a peg; 4000 particles of
    radius 0.5 displaced by 0.1 to 150 in one pass.  float64, no tolerance: every finite particle ends inside the box
    polygon and none has crossed an arm of the V.  The plain rule lets particles out of the same scene."""
    cs, start, end, rad = S.box_scene(R)
    prev = S.box_prev(start)
    finite = np.isfinite(prev).all(axis=1)
    assert len(rad) == 4000 and (~finite).sum() == 16
    length = np.linalg.norm(end[finite].astype(np.float64) - start[finite], axis=1)
    assert length.min() < 0.2 and length.max() > 140
    surf = SM.scene_surfaces(len(cs), seed=41) if surfaces else None
    out, out_prev, info = S.apply(end, prev, rad, cs, S.BOX_WORLD, surfaces=surf)
    outside, crossed = S.check_box(start, out, finite)
    print("R %g: moved %d swept %d stopped %d" % (R, info["moved"].sum(), info["swept"].sum(), info["stopped"].sum()))
    assert not outside.any(), (np.nonzero(outside)[0][:5], start[outside][:5], end[outside][:5], out[outside][:5])
    assert not crossed.any(), (np.nonzero(crossed)[0][:5], start[crossed][:5], end[crossed][:5], out[crossed][:5])
    assert info["swept"].sum() > 1000 and info["stopped"].sum() > 100 and info["plain"].sum() == 16
    assert same_bits(out_prev[info["stopped"]], prev[info["stopped"]])
    assert same_bits(out[~info["moved"]], end[~info["moved"]])         # who met nothing keeps every bit
    plain, _ = CM.apply(end, rad, cs, S.BOX_WORLD)
    lost, through = S.check_box(start, plain, finite)
    assert lost.sum() > 500 and through.sum() > 50


def test_a_particle_slides_over_the_joints_of_a_polyline():
    """Along the top of the straight polyline, pressed into it every step: never stopped, the tangential displacement
    survives every pass (the normal of a horizontal capsule has no x beyond the rounding of u * dx)"""
    cs = S.box_colliders(0.0)
    s = S.LINE_R + S.BOX_RADIUS
    prev = np.array([[S.LINE_X[0] + 2.0, S.LINE_Y - s]], F32)
    rad = np.array([S.BOX_RADIUS], F32)
    steps, swept = 0, 0
    while prev[0, 0] < S.LINE_X[3] - 2.0:
        pos = (prev + np.array([0.43, 0.05], F32)).astype(F32)
        out, out_prev, info = S.apply(pos, prev, rad, cs, S.BOX_WORLD)
        assert info["moved"][0] and not info["stopped"][0], (steps, prev, pos)
        assert abs(float(out[0, 0]) - float(pos[0, 0])) <= 1e-5 and abs(float(out[0, 1]) - (S.LINE_Y - s)) <= 1e-4, (steps, out)
        assert same_bits(out_prev, prev)
        prev = out
        steps += 1
    assert steps > 190                                                 # both joints (x = 90, 120) lie behind it


# ---- the stepped scene of the GPU tests ------------------------------------------------------------------------------
def test_the_stepped_scene_keeps_every_particle_inside_where_the_plain_pass_does_not(oracle):
    for kw in (dict(), dict(resort_every=16, resort_first=True, kick_every=4)):
        frames, counts = S.step_reference(oracle, **kw)
        for s, (pos, _) in enumerate(frames):
            assert S.inside_step_box(pos).all(), (kw, s)
        assert counts["swept"] > 100 and counts["stopped"] > 0 and counts["movers"] > 0 and counts["passes"] == S.STEP_STEPS
    frames, _ = S.step_reference(oracle, sweep=False)
    assert not S.inside_step_box(frames[-1][0]).all()


# ---- the table and the stand-alone program ---------------------------------------------------------------------------
def test_the_table_the_cpp_definition_replays_is_the_models():
    assert open(TABLE).read() == S.table_text()
    assert os.path.getsize(TABLE) < 128 * 1024


SRC = os.path.join(ROOT, "tests", "cpp", "sweep_tests.cpp")
TESTS = ["table", "properties"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_sweep_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "sweep_tests")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_holds_no_hip_and_states_its_limits():
    text = open(os.path.join(ROOT, "gpu-physics-engine_amd", "csrc", "k_sweep.h")).read()
    assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text)
    for word in ("movers", "collision response", "wrong side", "THE SLACK", "2^-10", "2^-19"):
        assert word in text, word
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    assert "gpe_set_collider_sweep" in header and "the movers have no sweep" in header
    assert re.search(r"#define GPE_ABI_VERSION 1u\b", header)


# ---- the binding, save and load --------------------------------------------------------------------------------------
def test_the_struct_and_the_constants_mirror_the_header(gpe):
    L = gpe._lib
    assert C.sizeof(L.GpeSweepInfo) == 32 and C.sizeof(L.GpeCollidersInfo) == 40
    assert [n for n, _ in L.GpeSweepInfo._fields_] == ["struct_size", "mode", "passes", "swept", "stopped"]
    assert (L.SWEEP_OFF, L.SWEEP_ON) == (0, 1)
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    assert re.search(r"#define GPE_SWEEP_OFF 0u", header) and re.search(r"#define GPE_SWEEP_ON 1u", header)
    for name in ("set_collider_sweep", "collider_sweep", "sweep_info"):
        assert hasattr(gpe.State, name), name


def test_save_writes_the_key_only_when_on_and_load_accepts_files_without_it(gpe, tmp_path, monkeypatch):
    calls = []

    class Fake(gpe.State):
        def __init__(self, pos, radius, **kw):
            self._on = False
            self._pos, self._rad = np.array(pos, F32), np.array(radius, F32)
            calls.append("init")

        def set_collider_sweep(self, on):
            self._on = bool(on)
            calls.append(("sweep", bool(on)))

        def collider_sweep(self):
            return self._on

    empty = lambda self, *a: np.zeros(0, F32)
    for name in ("movers", "fields", "colliders"):
        monkeypatch.setattr(Fake, name, empty)
    monkeypatch.setattr(Fake, "mover_sweep", lambda self: False)       # (save() asks the context for this mode too)
    monkeypatch.setattr(Fake, "surfaces", lambda self, target: np.zeros(0, gpe.SURFACE_DTYPE))
    monkeypatch.setattr(Fake, "bodies", lambda self: (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)))
    monkeypatch.setattr(Fake, "bonds", lambda self: (np.zeros(0), np.zeros(0)))
    monkeypatch.setattr(Fake, "_uids_on", lambda self: False)
    monkeypatch.setattr(Fake, "positions", lambda self: self._pos)
    monkeypatch.setattr(Fake, "previous_positions", lambda self: self._pos)
    monkeypatch.setattr(Fake, "radii", lambda self: self._rad)

    class Ctx:
        def mouse(self):
            return False, (0.0, 0.0)

        def world(self):
            return (10.0, 10.0)

        def gravity(self):
            return (0.0, 0.0)

    class Grid:
        def max_radius(self):
            return 0.5

    st = Fake([(1, 1), (2, 2)], [0.5, 0.5])
    st.ctx, st.grid = Ctx(), Grid()
    off, on = str(tmp_path / "off.npz"), str(tmp_path / "on.npz")
    st.save(off)
    st.set_collider_sweep(True)
    st.save(on)
    with np.load(off) as d:
        assert "collider_sweep" not in d.files
    with np.load(on) as d:
        assert d["collider_sweep"].tolist() == [1] and d["collider_sweep"].dtype == np.uint32
    del calls[:]
    assert not Fake.load(off).collider_sweep() and calls == ["init"]
    del calls[:]
    assert Fake.load(on).collider_sweep() and calls == ["init", ("sweep", True)]
