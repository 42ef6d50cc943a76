"""CPU: the bonds' coloured solver (include/gpe.h "the bonds' solver") as the numpy model states it
(tests/_bond_solver_model.py): the colouring, the vectorised sweep against a one-bond-at-a-time loop, the stand-alone
program over csrc/bond_colours.h and csrc/k_bond.h (tests/cpp/bond_colours_tests.cpp, plain and under the host
sanitizers) replaying the model's table, what a hanging rope gains, and the binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _bond_solver_model as S
from tests import _bonds_model as BM
from tests import _fields_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
SRC = os.path.join(ROOT, "tests", "cpp", "bond_colours_tests.cpp")
TESTS = ["small_sets", "duplicates_and_anchors", "stars_and_the_cap", "random_sets", "table"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


# ---- the colouring ----------------------------------------------------------------------------------------------------
def test_the_colouring_is_proper_least_and_a_function_of_the_bond_order():
    chain = BM.pairs([1, 2, 3, 4], [2, 3, 4, 5], 1.0)
    assert S.colours(chain).tolist() == [0, 1, 0, 1]
    assert S.colours(chain[[1, 0, 3, 2]]).tolist() == [0, 1, 0, 1]     # (2, 3) first: it has colour 0 now
    twice = np.concatenate([BM.pairs([1, 1, 2], [2, 2, 1], 1.0), BM.anchors([1, 2, 1, 9], np.zeros((4, 2))),
                            BM.pairs([9], [10], 1.0)])
    assert S.colours(twice).tolist() == [0, 1, 2, 3, 3, 4, 0, 1]       # twins differ; an anchor occupies uid_a only
    assert S.colour_info(twice) == (5, 2) and S.colour_info(twice[:0]) == (0, 0)
    pos, rad, uids, bonds, _ = S.hostile_scene(4000)
    col = S.colours(bonds)
    anchor = (bonds["flags"] & BM.BOND_ANCHOR) != 0
    ends = np.concatenate([np.stack([bonds["uid_a"], col], 1), np.stack([bonds["uid_b"], col], 1)[~anchor]])
    assert len(np.unique(ends, axis=0)) == len(ends)                   # proper: no (uid, colour) twice
    assert S.HUB_DEGREE <= col.max() + 1 <= S.COLOURS_MAX
    # 64 spokes fit, 65 do not: the twin refuses from either call and keeps what it had
    star = lambda d: BM.pairs(np.full(d, 1000), np.arange(d), 1.0)
    assert S.colour_info(star(64)) == (64, 1) and S.colour_info(star(65)) == (65, 1)


# ---- the vectorised sweep against one bond at a time ------------------------------------------------------------------
def _clamp(x, lo, hi):
    m = x if x > lo else lo                                            # K12's clamp: a NaN x gives lo
    return m if m < hi else hi


def loop_pass(pos, rad, uids, bonds, iterations, world):
    """A coloured pass written as the sentence of the header reads: a sequential sweep in (colour, index) order, one
    bond at a time, binary32 scalars, one rounding per operation."""
    p = [[F32(x), F32(y)] for x, y in np.asarray(pos, F32)]
    r = [F32(v) for v in rad]
    slot = {int(u): i for i, u in enumerate(uids)}
    col = S.colours(bonds)
    order = np.lexsort((np.arange(len(bonds)), col))
    broken = np.zeros(len(bonds), bool)
    W, H = F32(world[0]), F32(world[1])
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            for j in order:
                q = bonds[j]
                if broken[j]:
                    continue
                anchor = bool(q["flags"] & BM.BOND_ANCHOR)
                sa = slot.get(int(q["uid_a"]))
                sb = None if anchor else slot.get(int(q["uid_b"]))
                if sa is None or (not anchor and sb is None):
                    continue
                ax, ay = p[sa]
                bx, by = (F32(q["anchor_x"]), F32(q["anchor_y"])) if anchor else p[sb]
                w = F32(q["stiffness"]) if anchor else F32(F32(0.5) * F32(q["stiffness"]))
                dx = F32(bx - ax)
                dy = F32(by - ay)
                d = F32(np.sqrt(F32(F32(dx * dx) + F32(dy * dy))))
                if not (d > 0 and d < np.inf):
                    continue
                if q["max_length"] > 0 and d > q["max_length"]:
                    broken[j] = True
                    continue
                g = F32(F32(F32(d - F32(q["rest_length"])) / d) * w)
                cx, cy = F32(g * dx), F32(g * dy)
                p[sa] = [_clamp(F32(ax + cx), r[sa], F32(W - r[sa])), _clamp(F32(ay + cy), r[sa], F32(H - r[sa]))]
                if not anchor:
                    p[sb] = [_clamp(F32(bx + F32(-cx)), r[sb], F32(W - r[sb])), _clamp(F32(by + F32(-cy)), r[sb], F32(H - r[sb]))]
    return np.array(p, F32), broken


@pytest.mark.parametrize("n", [4000, 3999])
def test_the_vectorised_sweep_equals_one_bond_at_a_time(n):
    pos, rad, uids, bonds, third = S.hostile_scene(n)
    assert 2700 < len(bonds) < 3000
    none = np.zeros(len(bonds), bool)
    for iterations in (1, 3):
        want, want_broken = loop_pass(pos, rad, uids, bonds, iterations, S.WORLD)
        got, got_broken = S.apply(pos, rad, uids, bonds, none, iterations, S.WORLD)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_broken, want_broken)
        assert got_broken[third - 2] and got_broken[third] == (iterations == 3)       # the early break, the late one
        assert 50 < got_broken.sum() < 1500
    moved = (bits(got) != bits(pos)).any(axis=1)
    assert 1000 < moved.sum() < n - 20
    assert tuple(got[3956]) == (0.5, 150.0) and tuple(got[3957]) == (199.5, 199.5)    # across the edge: clamped
    # it is no Jacobi pass: the bits differ
    jac, _ = BM.apply(pos, rad, uids, bonds, none, 3, S.WORLD)
    assert not np.array_equal(bits(jac), bits(got))
    # three passes of one relaxation are one pass of three
    p, b = pos, none
    for _ in range(3):
        p, b = S.apply(p, rad, uids, bonds, b, 1, S.WORLD)
    assert np.array_equal(bits(p), bits(got)) and np.array_equal(b, got_broken)


def test_a_bond_sees_the_colours_before_it():
    # three in a row, 10 apart, rest 6, stiffness 1.  Bond 0 (colour 0) pulls 0 and 1 together: 12, 18.  Bond 1 (colour
    # 1) sees 1 at 18: d = 12, each end moves 3: 21, 27.  Jacobi would judge both from the start: 12, 20, 28
    pos = np.array([[10, 10], [20, 10], [30, 10]], F32)
    bonds = BM.pairs([0, 1], [1, 2], 6.0)
    out, _ = S.apply(pos, np.full(3, 0.5, F32), np.arange(3, dtype=U32), bonds, np.zeros(2, bool), 1, S.WORLD)
    assert out.tolist() == [[12, 10], [21, 10], [27, 10]]
    # the other order of the same bonds is another result
    out, _ = S.apply(pos, np.full(3, 0.5, F32), np.arange(3, dtype=U32), bonds[::-1], np.zeros(2, bool), 1, S.WORLD)
    assert out.tolist() == [[13, 10], [19, 10], [28, 10]]
    # stiffness 1 at a hub of 16 settles where Jacobi throws the hub across (a hub displaced by e gets 16 half errors
    # back, 4 e along e: it lands at -3 e, and further out every relaxation): the spokes sit at rest + 1 around it
    ang = np.arange(16) * np.pi / 8
    pos = np.concatenate([[[100.0, 100.0]], 100.0 + 6.0 * np.stack([np.cos(ang), np.sin(ang)], 1)]).astype(F32)
    pos[0, 0] += 1.0
    star = BM.pairs(np.zeros(16), np.arange(1, 17), 5.0)
    args = (np.full(17, 0.5, F32), np.arange(17, dtype=U32), star, np.zeros(16, bool))
    col, _ = S.apply(pos, *args, 8, S.WORLD)
    jac, _ = BM.apply(pos, *args, 8, S.WORLD)
    err = lambda p: np.abs(np.linalg.norm(p[1:] - p[0], axis=1) - 5.0).max()
    assert err(col) < 0.05 and err(jac) > 1.0


# ---- the stand-alone program ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bond_colours_program_replays_the_models_table(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once plain
    and once under AddressSanitizer and UndefinedBehaviorSanitizer; the table is the model's, written here."""
    exe, table = str(tmp_path / "bond_colours_tests"), str(tmp_path / "table.txt")
    with open(table, "w") as f:
        f.write(S.table_text())
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe, table], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the gain ---------------------------------------------------------------------------------------------------------
ROPE, ROPE_REST = 64, 2.0
ROPE_WORLD, ROPE_GRAVITY, ROPE_DT = (40.0, 600.0), (0.0, 100.0), 1.0 / 60.0
ROPE_DRAG = 0.9


def hang(oracle, solver, stiffness, max_steps=8000):
    """-> (the excess stretch of the rope at rest, steps taken): end to end over rest length, minus 1, once no particle
    moves more than 1e-3 in a step"""
    y = 10.0 + ROPE_REST * np.arange(1, ROPE + 1)
    pos = np.stack([np.full(ROPE, 20.0), y], axis=1).astype(F32)
    uid = np.arange(ROPE, dtype=U32)
    bonds = np.concatenate([BM.anchors([0], [(20.0, 10.0)], ROPE_REST, stiffness),
                            BM.pairs(uid[:-1], uid[1:], ROPE_REST, stiffness)])
    tw = S.everything_class()(oracle, pos, np.full(ROPE, 0.5, F32), world=ROPE_WORLD, gravity=ROPE_GRAVITY)
    tw.enable_uids()
    tw.set_bond_solver(solver)
    tw.set_bonds(bonds, 1)
    tw.set_fields(FM.rows(FM.field(shape=FM.EVERYWHERE, kind=FM.DRAG, strength=ROPE_DRAG)))
    for step in range(max_steps):
        tw.step(ROPE_DT)
        p, q, _ = tw.arrays()
        speed = float(np.abs(p.astype(np.float64) - q).max())
        assert np.isfinite(speed)
        if step > 100 and speed < 1e-3:
            break
    else:
        raise AssertionError("the rope never came to rest: %g per step" % speed)
    length = float(p[-1, 1]) - 10.0
    assert tw.bonds_info()["broken"] == 0 and abs(float(p[-1, 0]) - 20.0) < 1e-3
    tw.close()
    return length / (ROPE * ROPE_REST) - 1.0, step + 1


def test_a_hanging_rope_stretches_half_as_much_at_most(oracle):
    """64 particles hang from an anchor, one relaxation per step, an EVERYWHERE drag brings them to rest.  The coloured
    solver at stiffness 1 must leave at most half the excess stretch Jacobi leaves at 0.5, its stable maximum along a
    chain (the float64 experiment of the design gives a quarter: 1.452 against 2.806; the factor of two is the margin
    for binary32 and the engine's integrator).  Measured here: Jacobi 1.7711 after 3751 steps, coloured 0.4429 after 931 (the ratio is 0.25)."""
    jacobi, steps_j = hang(oracle, "jacobi", 0.5)
    coloured, steps_c = hang(oracle, "coloured", 1.0)
    print("excess stretch at rest: jacobi %.4f after %d steps, coloured %.4f after %d steps" % (jacobi, steps_j, coloured, steps_c))
    assert jacobi > 0.5                                                # the limit the README states is there
    assert 0 < coloured <= 0.5 * jacobi


# ---- the headers, the binding, save and load --------------------------------------------------------------------------
def test_the_header_holds_no_hip_and_the_layers_agree(gpe):
    csrc = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
    text = open(os.path.join(csrc, "bond_colours.h")).read()
    assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text)
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    L = gpe._lib
    for name, value in (("GPE_BOND_COLOURS_MAX", L.BOND_COLOURS_MAX), ("GPE_BOND_SOLVER_JACOBI", L.BOND_SOLVER_JACOBI),
                        ("GPE_BOND_SOLVER_COLOURED", L.BOND_SOLVER_COLOURED)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, header).group(1)) == value, name
    assert (L.BOND_COLOURS_MAX, S.COLOURS_MAX, S.JACOBI, S.COLOURED) == (64, 64, L.BOND_SOLVER_JACOBI, L.BOND_SOLVER_COLOURED)
    assert C.sizeof(L.GpeBondSolverInfo) == 32
    body = re.search(r"typedef struct gpe_bond_solver_info \{(.*?)\} gpe_bond_solver_info;",
                     re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [n for n, _ in L.GpeBondSolverInfo._fields_]
    bound = {name for name, _, _ in L.SYMBOLS}
    assert {"gpe_set_bond_solver", "gpe_get_bond_solver", "gpe_get_bond_solver_info"} <= bound
    for name in ("set_bond_solver", "bond_solver", "bond_solver_info"):
        assert hasattr(gpe.State, name) and hasattr(gpe.ParticleSystem, name), name
    for what in ("the bends and the areas stay Jacobi", "GPE_BOND_COLOURS_MAX colours", "sharded", "order of the colours"):
        assert what in header, what
    readme = open(os.path.join(ROOT, "README.md")).read()
    for what in ("gpe_set_bond_solver", "64 colours", "stays a Jacobi customer"):
        assert what in readme, what
    # the policy constant of the launcher is the one the info reports, and within the LDS the kernel declares
    internal = open(os.path.join(csrc, "gpe_internal.h")).read()
    policy = int(re.search(r"#define GPE_BOND_LDS_NODES_MAX (\d+)", internal).group(1))
    assert "kBondLdsNodesCap = kBondLdsNodesMax > 0 ? kBondLdsNodesMax : 1;" in internal and policy * 12 <= 160 * 1024
