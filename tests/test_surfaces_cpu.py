"""CPU: the surface materials as the numpy model states them (tests/_surfaces_model.py, include/gpe.h "surface
materials"): what the rule does to one particle (bounce, sliding, a slope), its exact properties, the coverage of the
one-pass scenes the GPU tests share, the table the C++ definition replays (tests/golden/surface_cases.txt), the
stand-alone test program (tests/cpp/surface_tests.cpp over csrc/k_surface.h, csrc/k_collider.h and csrc/k_mover.h),
plain and under the host sanitizers, and what needs no device of the binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _movers_model as M
from tests import _surfaces_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TABLE = os.path.join(ROOT, "tests", "golden", "surface_cases.txt")
FLOOR = (-5, 50, 65, 50, 9.5)                                          # centres of r = 0.5 rest at y = 40
GRAVITY = (0.0, 100.0)
DT = 1.0 / 60.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same(a, b):
    """the same bits, a NaN where there is a NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def apexes(trail):
    """the heights above the resting level y = 40 a dropped particle reaches between two contacts"""
    y = trail[:, 1]
    hits = np.nonzero(y >= 40.0 - 1e-6)[0]
    return [float(40.0 - y[s].min()) for s in np.split(np.arange(len(y)), hits) if len(s) > 2], hits


# ---- what the rule does to one particle -----------------------------------------------------------------------------
def test_a_dropped_particle_bounces_by_its_restitution():
    """Dropped from rest at y = 20 on the floor.  The drop height the contact sees is the apex of the elastic rebound
    (e = 1 returns the impact speed whole); with e = 0.5 the first apex is e^2 of it within 5 %."""
    elastic, _ = apexes(S.drop(FLOOR, (1.0, 0.0), (30, 20), GRAVITY, DT, 600))
    half, _ = apexes(S.drop(FLOOR, (0.5, 0.0), (30, 20), GRAVITY, DT, 600))
    dead, hits = apexes(S.drop(FLOOR, (0.0, 0.0), (30, 20), GRAVITY, DT, 200))
    ratio = half[1] / elastic[1]
    print("drop %.3f, elastic apexes %s, e = 0.5: first apex %.3f (ratio %.4f)" % (elastic[0], elastic[1:7], half[1], ratio))
    assert abs(ratio - 0.25) <= 0.05 * 0.25
    assert len(elastic) >= 7 and max(elastic[1:7]) - min(elastic[1:7]) <= 1e-3
    assert len(dead) == 1 and len(hits) == 200 - hits[0]               # e = 0: from the first contact on it lies there


def test_a_sliding_particle_stops_after_the_coulomb_time():
    """0.2 per step along the floor, mu = 0.3: every step the contact takes mu * g * dt^2 off: 0.2 / that = 24 steps."""
    trail = S.drop(FLOOR, (0.0, 0.3), (30, 40), GRAVITY, DT, 60, prev=(29.8, 40))
    x = trail[:, 0]
    stopped = int(np.nonzero(np.diff(x) == 0)[0][0]) + 1
    want = 0.2 / (0.3 * 100.0 * DT * DT)
    print("stopped after %d steps (%.1f expected), at x = %.4f" % (stopped, want, x[-1]))
    assert abs(stopped - want) <= 1.0 and (np.diff(x) >= 0).all() and x[-1] == x[stopped]
    ice = S.drop(FLOOR, (0.0, 0.0), (30, 40), GRAVITY, DT, 60, prev=(29.8, 40))
    assert abs(float(ice[-1, 0] - ice[0, 0]) - 59 * 0.2) < 1e-3       # without friction it slides for ever


def test_a_particle_on_a_slope_stays_above_the_friction_angle_and_runs_off_below_it():
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    slope = (20.0, 30.0, 20.0 + 60.0 * c, 30.0 + 60.0 * s, 2.0)
    start = np.array([20.0 + 10.0 * c, 30.0 + 10.0 * s]) + 2.5 * np.array([s, -c])   # on the face, above it (y grows downwards)
    moved = {}
    for mu in (0.8, 0.3):
        trail = S.drop(slope, (0.0, mu), start, GRAVITY, DT, 120, world=(100.0, 100.0))
        moved[mu] = float(np.hypot(*(trail[-1] - trail[0])))
    print("on a 30 degree slope after 120 steps: mu 0.8 moved %.3g, mu 0.3 moved %.3g" % (moved[0.8], moved[0.3]))
    assert moved[0.8] < 1e-4 and moved[0.3] > 10.0


def test_a_moving_wall_drags_what_lies_on_it_and_a_plain_one_does_not():
    """A plate sliding sideways under a particle that gravity presses on it: with friction the particle reaches the
    plate's speed, on a frictionless surface it stays where it is."""
    speed = 0.1 * 60
    gain = {}
    for mu in (0.5, 0.0):
        mv = S.Movers(M.rows(M.linear((-50, 50), (150, 50), 9.5, v=(speed, 0.0))))
        mv.set_surfaces(S.rows((0.0, mu)))
        p = np.array([[30.0, 40.0]], F32)
        q, r = p.copy(), np.array([0.5], F32)
        g = (np.array(GRAVITY, F32) * F32(DT) * F32(DT)).astype(F32)
        for _ in range(60):
            q, p = p, (p + (p - q) + g).astype(F32)
            p, q, moved, br = mv.apply_surface(p, q, r, (100.0, 100.0), DT)
            assert moved[0] and br["wall_moved"][0]
        gain[mu] = float(p[0, 0] - q[0, 0])
    print("velocity along a plate moving 0.1 per step: mu 0.5 -> %.4f, mu 0 -> %.4f" % (gain[0.5], gain[0.0]))
    assert abs(gain[0.5] - 0.1) < 1e-4 and gain[0.0] == 0.0


# ---- exact properties and the coverage of the shared scenes ---------------------------------------------------------
@pytest.fixture(scope="module", params=[4000, 3999])
def collider_pass(request):
    n = request.param
    cs, surf, pos, prev, rad = S.collider_scene(n)
    return n, cs, surf, pos, prev, rad, S.apply(pos, prev, rad, cs, surf, S.ONE_PASS_WORLD)


def test_the_collider_scene_takes_every_branch(collider_pass):
    n, cs, surf, pos, prev, rad, (out, out_prev, moved, br) = collider_pass
    counts = S.coverage(moved, br, n)
    print("n %d: %s" % (n, counts))
    assert len(cs) == 40 and (surf["flags"] & S.PLAIN).sum() == 10
    assert counts["touched"] < n - 300                                 # both outcomes


def test_the_mover_scene_takes_every_branch():
    movers, surf = S.mover_scene_set()
    mv = S.Movers(movers)
    mv.set_surfaces(surf)
    for n in (4000, 3999):
        pos, prev, rad = S.mover_scene_particles(n, mv, M.RUN_DT, seed=n)
        out, out_prev, moved, br = mv.apply_surface(pos, prev, rad, S.ONE_PASS_WORLD, M.RUN_DT)
        counts = S.coverage(moved, br, n, movers=True)
        print("n %d: %s" % (n, counts))


def test_exact_properties(collider_pass):
    n, cs, surf, pos, prev, rad, (out, out_prev, moved, br) = collider_pass
    plain, plain_moved = CM.apply(pos, rad, cs, S.ONE_PASS_WORLD)
    assert np.array_equal(moved, plain_moved)
    # a particle nothing touches keeps every bit
    assert np.array_equal(bits(out[~moved]), bits(pos[~moved])) and np.array_equal(bits(out_prev[~moved]), bits(prev[~moved]))
    # PLAIN rows and velocities that are not finite take the plain rule: pos pushed, prev untouched
    escaped = br["plain"] | br["not_finite"]
    assert escaped.sum() >= 32
    assert np.array_equal(bits(out[escaped]), bits(plain[escaped])) and same(out_prev[escaped], prev[escaped])
    # prev is written for every other touched particle
    acts = moved & ~escaped
    assert not np.array_equal(bits(out_prev[acts]), bits(prev[acts]))
    # mu = 0: the plain pass's pos bits
    ice = surf.copy()
    ice["friction"] = 0
    o2, q2, m2, _ = S.apply(pos, prev, rad, cs, ice, S.ONE_PASS_WORLD)
    assert same(o2, plain) and np.array_equal(m2, moved)
    # an all-PLAIN table: the plain pass's pos and prev bits
    o3, q3, m3, b3 = S.apply(pos, prev, rad, cs, S.uniform(len(cs), 0.5, 0.5, S.PLAIN), S.ONE_PASS_WORLD)
    assert same(o3, plain) and same(q3, prev) and b3["plain"].sum() == moved.sum()
    # restitution and friction act: the full table differs from the frictionless one in pos, and from PLAIN in prev
    assert not same(out, plain) and not same(out_prev, prev)


def test_minus_zero_becomes_zero():
    s = S.stored(S.rows((-0.0, -0.0)))
    assert s.view(U32).tolist() == [0, 0, 0, 0]


def test_the_table_the_cpp_definition_replays_is_the_models():
    assert open(TABLE).read() == S.table_text()
    assert os.path.getsize(TABLE) < 128 * 1024


# ---- the stand-alone program ----------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "surface_tests.cpp")
TESTS = ["table", "properties", "refusals"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_surface_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "surface_tests")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_holds_no_hip_and_the_old_sentences_stay():
    csrc = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
    text = open(os.path.join(csrc, "k_surface.h")).read()
    assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text)
    assert "restitution" in text and "friction" in text and "Coulomb" in text
    assert "deepest" in open(os.path.join(csrc, "k_collider.h")).read()
    mover = open(os.path.join(csrc, "k_mover.h")).read()
    assert "swept" in mover and "thick" in mover and "0.5" in mover


# ---- the binding and the refusals that need no device ---------------------------------------------------------------
def test_the_binding_mirrors_the_header(gpe):
    L = gpe._lib
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    assert re.search(r"GPE_SURFACES_OF_COLLIDERS = 0, GPE_SURFACES_OF_MOVERS = 1", header)
    assert (L.SURFACES_OF_COLLIDERS, L.SURFACES_OF_MOVERS) == (0, 1)
    assert re.search(r"GPE_SURFACE_PLAIN = 1u", header) and L.SURFACE_PLAIN == S.PLAIN == 1
    assert C.sizeof(L.GpeSurface) == 16
    body = re.search(r"typedef struct gpe_surface \{(.*?)\} gpe_surface;", header, flags=re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in L.GpeSurface._fields_] == list(S.SURFACE_DTYPE.names)
    assert gpe.SURFACE_DTYPE == S.SURFACE_DTYPE
    for method in ("set_surfaces", "surfaces", "clear_surfaces"):
        assert hasattr(gpe.State, method) and hasattr(gpe.ParticleSystem, method), method
    assert "gpe_set_surfaces" in open(os.path.join(ROOT, "gpu-physics-engine_amd", "host", "gpe_host.hpp")).read()
    assert lib_version(L) == 1


def lib_version(L):
    return L.load().gpe_abi_version()


def test_a_null_context_is_refused_by_both_calls(gpe):
    L = gpe._lib
    lib = L.load()
    k = C.c_uint64()
    row = L.GpeSurface(0.5, 0.5, 0, 0)
    for target in (0, 1):
        assert lib.gpe_set_surfaces(None, target, C.byref(row), 1) == L.GPE_ERR_INVALID_ARG
        assert lib.gpe_set_surfaces(None, target, None, 0) == L.GPE_ERR_INVALID_ARG
        assert lib.gpe_get_surfaces(None, target, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG


# ---- the run scene: the oracle's step with the model's passes behind it ---------------------------------------------
def test_the_run_scene_with_surfaces(oracle):
    """The movers' run scene with surfaces on the floor, the piston and the paddle, over steps whose dt is also zero and
    negative: everything stays finite and above the floor, the surfaces change pos and prev, and an all-PLAIN table is
    the run without surfaces bit for bit."""
    dts = M.TABLE_DTS
    assert all(M.dt_allowed(M.run_movers(), dt) for dt in dts) and 0.0 in dts and min(dts) < 0
    frames, pushed_movers, pushed_floor = S.run_reference(oracle, dts)
    plain, plain_movers, plain_floor = M.run_reference(oracle, dts)
    masked, _, _ = S.run_reference(oracle, dts, collider_surfaces=S.uniform(1, 0.9, 0.7, S.PLAIN),
                                   mover_surfaces=S.uniform(2, 0.9, 0.7, S.PLAIN))
    print("with surfaces: movers pushed %d, the floor %d; without: %d, %d" % (pushed_movers, pushed_floor, plain_movers, plain_floor))
    assert pushed_movers > 100 and pushed_floor > 1000
    for (pos, prev, poses), (ppos, pprev, pposes), (mpos, mprev, _) in zip(frames, plain, masked):
        assert np.isfinite(pos).all() and np.isfinite(prev).all() and not (pos[:, 1] > 40.0).any()
        assert np.array_equal(poses.view(U32), pposes.view(U32))      # the motion does not depend on the surfaces
        assert same(mpos, ppos) and same(mprev, pprev)
    assert not same(frames[-1][0], plain[-1][0]) and not same(frames[-1][1], plain[-1][1])
    # the floor bounces: particles leave it upwards, which they never do on the plain floor's first contact
    up = [(pos[:, 1] - prev[:, 1] < -0.01).sum() for pos, prev, _ in frames]
    assert max(up) > 50
