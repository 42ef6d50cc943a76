"""CPU: the swept form of the movers' pass as the numpy model states it (tests/_mover_sweep_model.py, include/gpe.h
"moving colliders", csrc/k_mover_sweep.h): the mode off is the plain models' pass bit for bit, a resting particle under
a resting mover gets the plain rule, the winner's order is total, the pass does not commute with its neighbour, a thin
gate and a thin blade carry every particle in their way along (float64, no tolerance) where the plain rule leaves all of
them behind, the table the C++ definition replays (tests/golden/mover_sweep_cases.txt), the stand-alone test program
(tests/cpp/mover_sweep_tests.cpp over csrc/k_mover_sweep.h), plain and under the host sanitizers, and what needs no
device of the binding and of save / load."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _colliders_model as CM
from tests import _mover_sweep_model as MS
from tests import _movers_model as M
from tests import _surfaces_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TABLE = os.path.join(ROOT, "tests", "golden", "mover_sweep_cases.txt")
WORLD = SM.ONE_PASS_WORLD
DT = 1.0 / 60.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def one(movers, p, prev, r=1.0, dt=DT, world=MS.SCENE_WORLD, surfaces=None):
    out, out_prev, mv = MS.one_pass(movers, [p], [prev], [r], True, world=world, dt=dt, surfaces=surfaces)
    return tuple(float(v) for v in out[0]), tuple(float(v) for v in out_prev[0]), mv


# ---- the rule on one particle ----------------------------------------------------------------------------------------
def test_a_thin_gate_takes_a_resting_particle_along():
    cap = MS.first_pose(MS.GATE)                                       # the face after its first step: x = 70
    assert abs(cap[0] - 70.0) < 1e-4
    plain, _, _ = MS.one_pass(MS.GATE, [(60, 100)], [(60, 100)], [1.0], False)
    assert tuple(plain[0]) == (60.0, 100.0)                            # the plain rule: 10 behind the new face, untouched
    p, q, mv = one(MS.GATE, (60, 100), (60, 100))
    assert abs(p[0] - (cap[0] + 1.0)) < 1e-4 and p[1] == 100.0 and q == (60.0, 100.0)
    assert (mv.pushed, mv.swept, mv.stopped, mv.sweep_passes) == (1, 1, 0, 1)
    # behind the old face, or beyond the new one by more than s: every bit kept
    for pos in ((45, 100), (72, 100), (60, 20)):
        p, q, mv = one(MS.GATE, pos, pos)
        assert p == tuple(map(float, pos)) and mv.pushed == 0, pos
    # a particle that keeps pace with the gate is not met: its relative path has no length along the gate's way
    p, _, mv = one(MS.GATE, (80, 100), (60, 100))
    assert p == (80.0, 100.0) and mv.pushed == 0
    # with e = 1 and no friction the particle leaves with the gate's velocity reflected in the gate's frame: 2 D per step
    p, q, _ = one(MS.GATE, (60, 100), (60, 100), surfaces=SM.rows((1.0, 0.0)))
    assert abs(p[0] - (cap[0] + 1.0)) < 1e-4 and abs((p[0] - q[0]) - 40.0) < 1e-3


def test_a_thin_blade_takes_a_resting_particle_along():
    cap = MS.first_pose(MS.BLADE)
    pos = (100 + 30 * np.cos(0.2), 100 + 30 * np.sin(0.2))             # half way through the swept sector
    plain, _, _ = MS.one_pass(MS.BLADE, [pos], [pos], [1.0], False)
    assert same_bits(plain[0], np.array(pos, F32))
    p, _, mv = one(MS.BLADE, pos, pos)
    behind, close = MS.check_leading(cap, [p], MS.BLADE_SIDE)
    assert not behind[0] and not close[0] and mv.swept == 1
    # the gate: a fast particle that passes the blade's disc at a distance is not judged by its chord at all
    far = (100 + 52.5, 100 - 40.0), (100 + 52.5, 100 + 40.0)
    p, _, mv = one(MS.BLADE, far[1], far[0])
    assert p == tuple(float(F32(v)) for v in far[1]) and mv.pushed == 0


# ---- off, and at rest --------------------------------------------------------------------------------------------------
def test_the_mode_off_is_the_movers_model_bit_for_bit():
    movers, surf = SM.mover_scene_set()
    for surfaces in (None, surf):
        a, b = MS.Movers(movers), SM.Movers(movers)
        if surfaces is not None:
            a.set_surfaces(surfaces)
            b.set_surfaces(surfaces)
        for s in range(3):
            pos, prev, rad = SM.mover_scene_particles(2000, b, DT, seed=90 + s)
            got = a.apply_surface(pos, prev, rad, WORLD, DT)
            want = b.apply_surface(pos, prev, rad, WORLD, DT)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert same_bits(a.q0, b.q0) and same_bits(a.q1, b.q1)
        assert (a.passes, a.pushed) == (b.passes, b.pushed) and a.pushed > 500 and a.sweep_passes == 0
    plain = M.Movers(movers)
    again = MS.Movers(movers)
    pos, prev, rad = SM.mover_scene_particles(2000, SM.Movers(movers), DT, seed=7)
    want, moved = plain.apply(pos, rad, WORLD, DT)
    got = again.apply_surface(pos, prev, rad, WORLD, DT)
    assert same_bits(got[0], want) and same_bits(got[1], prev) and np.array_equal(got[2], moved)


def _resting_set():
    """the movers' one-pass scene with every motion taken out: v = 0, omega = 0"""
    movers, surf = SM.mover_scene_set()
    still = movers.copy()
    still["vx"] = still["vy"] = still["omega"] = 0
    return still, surf


def test_a_resting_particle_under_a_resting_mover_gets_the_plain_rule():
    still, surf = _resting_set()
    pos, _, rad = SM.mover_scene_particles(3000, SM.Movers(still), DT, seed=3)
    want, moved = M.Movers(still).apply(pos, rad, WORLD, DT)
    got, got_prev, mv = MS.one_pass(still, pos, pos, rad, True, world=WORLD, dt=DT)
    # without surfaces a stop is the push (sweep_stop of a touch at t = 1 is p + n * depth): every bit, every particle
    assert same_bits(got, want) and same_bits(got_prev, pos) and np.array_equal(mv.last["moved"], moved)
    assert moved.sum() > 700 and mv.swept == 0
    want, want_prev, moved, _ = _surface_pass(still, surf, pos, rad)
    got, got_prev, mv = MS.one_pass(still, pos, pos, rad, True, world=WORLD, dt=DT, surfaces=surf)
    # the scene's 40 movers overlap: a particle pushed out of one deep into another stops where it is touched instead,
    # prev untouched (the one verification); every other one has the surface pass's bits
    keep = ~mv.last["stopped"]
    assert same_bits(got[keep], want[keep]) and same_bits(got_prev[keep], want_prev[keep])
    assert same_bits(got_prev[~keep], pos[~keep])
    assert np.array_equal(mv.last["moved"], moved) and (moved & keep).sum() > 1500 and mv.swept == 0


def _surface_pass(movers, surf, pos, rad):
    mv = SM.Movers(movers)
    mv.set_surfaces(surf)
    return mv.apply_surface(pos, pos, rad, WORLD, DT)


# ---- the order -------------------------------------------------------------------------------------------------------
def test_the_winners_order_is_total_judging_a_mover_twice_or_in_another_order_changes_nothing():
    t = MS.table_cases()
    win, over = MS.search(t["pos"], t["prev"], t["rad"], t["rec"], t["caps"])
    rng = np.random.default_rng(1)
    k = len(t["caps"])
    for trial in range(3):
        order = np.concatenate([rng.permutation(k), rng.integers(0, k, 5)])   # every mover, five of them twice
        best = None
        for j in order:
            c, _ = MS.judge(t["rec"], int(j), t["caps"][j], t["pos"], t["prev"], t["rad"])
            c["who"] = np.full(len(c["t"]), int(j))
            if best is None:
                best = c
                continue
            with np.errstate(all="ignore"):
                better = (c["t"] < best["t"]) | ((c["t"] == best["t"]) & ((c["depth"] > best["depth"]) |
                                                                            ((c["depth"] == best["depth"]) & (c["who"] < best["who"]))))
            take = c["has"] & (~best["has"] | better)
            best = {name: np.where(take, c[name], best[name]) for name in c}
            best["has"] = best["has"] | take
        has = win["has"]
        assert np.array_equal(best["has"], has) and has.sum() > 60
        assert np.array_equal(best["who"][has], win["who"][has])
        for name in MS.NAMES:
            assert same_bits(np.asarray(best[name], F32)[has], win[name][has]), name


def test_swapping_the_movers_pass_with_the_static_colliders_pass_changes_bits():
    """the gate shoves the particles of its scene against a wall that stands 0.5 beyond their new place: movers then
    colliders leaves them before the wall, colliders then movers inside it"""
    movers, pos, prev, rad = MS.gate_scene()
    wall = np.array([[72.5, 0, 72.5, 200, 1.0]], F32)
    a, a_prev, _ = MS.one_pass(movers, pos, prev, rad, True)
    a, _ = CM.apply(a, rad, wall, MS.SCENE_WORLD)
    b, _ = CM.apply(pos, rad, wall, MS.SCENE_WORLD)
    b, _, _ = MS.one_pass(movers, b, prev, rad, True)
    assert not same_bits(a, b) and (bits(a) != bits(b)).any(axis=1).sum() == len(pos)


# ---- the two tunnelling scenes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("surfaces", [False, True], ids=["plain", "surfaces"])
@pytest.mark.parametrize("name", ["gate", "blade"])
def test_a_thin_mover_carries_every_particle_in_its_way_where_the_plain_rule_leaves_them_behind(name, surfaces):
    """(a) an R = 0 LINEAR gate that advances 20 units per step over resting and slowly drifting particles of radius 1;
    (b) an R = 0 ROTATE blade at |omega dt| = 0.4 over particles resting in the sector it sweeps.  float64, no tolerance,
    no particle left out: each ends on the leading side of the new pose, no nearer than s (1 - 2^-9) to it.  The same
    checker fails on the plain model's output for every particle."""
    scene, side = (MS.gate_scene, MS.GATE_SIDE) if name == "gate" else (MS.blade_scene, MS.BLADE_SIDE)
    movers, pos, prev, rad = scene()
    cap = MS.first_pose(movers)
    start_behind, _ = MS.check_leading(MS.first_pose(movers, dt=0.0), pos, side)
    assert not start_behind.any() and len(pos) >= 36                   # ahead of the old face ...
    now_behind, _ = MS.check_leading(cap, pos, side)
    assert now_behind.all()                                            # ... and behind the new one: inside what it sweeps
    surf = SM.rows((0.5, 0.3)) if surfaces else None
    out, out_prev, mv = MS.one_pass(movers, pos, prev, rad, True, surfaces=surf)
    behind, close = MS.check_leading(cap, out, side)
    print("%s: %d particles, swept %d stopped %d" % (name, len(pos), mv.swept, mv.stopped))
    assert not behind.any(), (np.nonzero(behind)[0][:5], pos[behind][:5], out[behind][:5])
    assert not close.any(), (np.nonzero(close)[0][:5], pos[close][:5], out[close][:5])
    assert mv.swept == len(pos) and mv.pushed == len(pos)
    if name == "gate":
        assert ((pos != prev).any(axis=1)).sum() >= 60                 # the drifting ones
    plain, _, _ = MS.one_pass(movers, pos, prev, rad, False, surfaces=surf)
    lost, _ = MS.check_leading(cap, plain, side)
    assert lost.all()


# ---- the table and the stand-alone program ---------------------------------------------------------------------------
def test_the_table_the_cpp_definition_replays_is_the_models():
    assert open(TABLE).read() == MS.table_text()
    assert os.path.getsize(TABLE) < 128 * 1024
    t = MS.table_cases()
    info = t["plain"][2]
    assert info["swept"].sum() >= 50 and info["stopped"].sum() >= 20 and (~info["moved"]).sum() >= 100
    assert set(t["rec"]["kind"].tolist()) == {MS.STILL, MS.SHIFT, MS.TURN}
    assert len(np.unique(info["who"][info["moved"]])) >= 7             # nearly every mover wins somewhere


SRC = os.path.join(ROOT, "tests", "cpp", "mover_sweep_tests.cpp")
TESTS = ["table", "properties"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_mover_sweep_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "mover_sweep_tests")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_holds_no_hip_and_states_its_limits():
    text = open(os.path.join(ROOT, "gpu-physics-engine_amd", "csrc", "k_mover_sweep.h")).read()
    assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text)
    for word in ("WHAT IS GUARANTEED", "WHAT IS NOT", "chord", "collision solver", "starts inside", "Two movers", "total order",
                 "THE LOOKUP", "2^-10"):
        assert word in text, word
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    for name in ("gpe_set_mover_sweep", "gpe_get_mover_sweep", "gpe_get_mover_sweep_info"):
        assert re.search(r"gpe_status %s\(" % name, header), name
    assert re.search(r"#define GPE_ABI_VERSION 1u\b", header)
    mover = open(os.path.join(ROOT, "gpu-physics-engine_amd", "csrc", "k_mover.h")).read()
    assert re.search(r"float pad0, pad1;", mover)                      # MoverDef stays three float4: the arm lives in a pad


# ---- the binding, save and load --------------------------------------------------------------------------------------
def test_the_binding_declares_the_entry_points(gpe):
    L = gpe._lib
    assert C.sizeof(L.GpeSweepInfo) == 32
    for name in ("set_mover_sweep", "mover_sweep", "mover_sweep_info"):
        assert hasattr(gpe.State, name), name
        assert hasattr(gpe.ParticleSystem, name), name
    text = open(os.path.join(ROOT, "gpu-physics-engine_amd", "_lib.py")).read()
    for name in ("gpe_set_mover_sweep", "gpe_get_mover_sweep", "gpe_get_mover_sweep_info"):
        assert '"%s"' % name in text, name
    hpp = open(os.path.join(ROOT, "gpu-physics-engine_amd", "host", "gpe_host.hpp")).read()
    for name in ("set_mover_sweep", "mover_sweep()", "mover_sweep_info"):
        assert name in hpp, name


def test_save_writes_the_key_only_when_on_and_load_accepts_files_without_it(gpe, tmp_path, monkeypatch):
    calls = []

    class Particles:
        """answers mover_sweep() from what set_mover_sweep was last told, as the context does"""
        on = False

        def set_mover_sweep(self, on):
            calls.append(("mover_sweep", bool(on)))
            self.on = bool(on)

        def mover_sweep(self):
            return self.on

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

    class Fake(gpe.State):
        def __init__(self, pos, radius, **kw):
            self._pos, self._rad = np.array(pos, F32), np.array(radius, F32)
            self.ctx, self.grid, self.particles = Ctx(), Grid(), Particles()
            calls.append("init")

    empty = lambda self, *a: np.zeros(0, F32)
    for name in ("movers", "fields", "colliders"):
        monkeypatch.setattr(Fake, name, empty)
    monkeypatch.setattr(Fake, "collider_sweep", lambda self: False)
    monkeypatch.setattr(Fake, "surfaces", lambda self, target: np.zeros(0, gpe.SURFACE_DTYPE))
    monkeypatch.setattr(Fake, "bodies", lambda self: (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)))
    monkeypatch.setattr(Fake, "bonds", lambda self: (np.zeros(0), np.zeros(0)))
    monkeypatch.setattr(Fake, "_uids_on", lambda self: False)
    monkeypatch.setattr(Fake, "positions", lambda self: self._pos)
    monkeypatch.setattr(Fake, "previous_positions", lambda self: self._pos)
    monkeypatch.setattr(Fake, "radii", lambda self: self._rad)
    st = Fake([(1, 1), (2, 2)], [0.5, 0.5])
    off, on = str(tmp_path / "off.npz"), str(tmp_path / "on.npz")
    st.save(off)
    st.set_mover_sweep(True)
    st.save(on)
    st.set_mover_sweep(False)
    st.save(off + ".again.npz")
    with np.load(off) as d:
        assert "mover_sweep" not in d.files
    with np.load(off + ".again.npz") as d:
        assert "mover_sweep" not in d.files
    with np.load(on) as d:
        assert d["mover_sweep"].tolist() == [1] and d["mover_sweep"].dtype == np.uint32 and "collider_sweep" not in d.files
    del calls[:]
    Fake.load(off)
    assert calls == ["init"]
    del calls[:]
    Fake.load(on)
    assert calls == ["init", ("mover_sweep", True)]
    # save() asks the context, not a mirror in State: a mode set below State (ParticleSystem.set_mover_sweep, ctx.call)
    # is written, and one set through State and unset below it is not
    below, unset = str(tmp_path / "below.npz"), str(tmp_path / "unset.npz")
    st = Fake([(1, 1), (2, 2)], [0.5, 0.5])
    st.particles.set_mover_sweep(True)
    st.save(below)
    with np.load(below) as d:
        assert "mover_sweep" in d.files and d["mover_sweep"].tolist() == [1]
    st = Fake([(1, 1), (2, 2)], [0.5, 0.5])
    st.set_mover_sweep(True)
    st.particles.set_mover_sweep(False)
    st.save(unset)
    with np.load(unset) as d:
        assert "mover_sweep" not in d.files
    del calls[:]
    Fake.load(below)
    assert calls == ["init", ("mover_sweep", True)]
    del calls[:]
    Fake.load(unset)
    assert calls == ["init"]
