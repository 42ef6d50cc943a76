"""CPU: the bend constraints' function as the numpy model states it (tests/_bends_model.py, include/gpe.h "bend
constraints"), a cantilever stepped by the CPU oracle with the model's passes behind every step, and the bend graph's
stand-alone test program (tests/cpp/bend_graph_tests.cpp over csrc/bend_graph.h and csrc/k_bend.h), plain and under the
host sanitizers, replaying a table the model wrote."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _bends_model as M
from tests import _bonds_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
WORLD = (200.0, 200.0)
NAN, INF = float("nan"), float("inf")
PI = math.pi
GRAPH_SRC = os.path.join(ROOT, "tests", "cpp", "bend_graph_tests.cpp")
GRAPH_TESTS = ["node_list", "csr_order_and_roles", "degree_cap", "k0_and_k1", "duplicate_bends", "validation", "replay"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def once(pos, bends, rad=0.5, world=WORLD, uids=None, iterations=1):
    pos = np.array(pos, F32).reshape(-1, 2)
    n = len(pos)
    uids = np.arange(n, dtype=U32) if uids is None else np.array(uids, U32)
    return M.apply(pos, np.full(n, rad, F32), uids, bends, iterations, world)


def s_of(pos, bends):
    pos = np.array(pos, F32).reshape(-1, 2)
    acts, s = M.corrections(pos, np.arange(len(pos), dtype=U32), bends)[:2]
    assert acts.all()
    return s


# ---- the function ---------------------------------------------------------------------------------------------------
# a = (102, 100), the hinge (100, 100), c (100, 102) or (100, 98): a right angle, turning either way
RIGHT = {"left": [[102, 100], [100, 100], [100, 102]], "right": [[102, 100], [100, 100], [100, 98]]}
STRAIGHT = [[102, 100], [100, 100], [98, 100]]


@pytest.mark.parametrize("stiffness, relaxations", [(0.5, 12), (1.0, 3)])
@pytest.mark.parametrize("sense", ["left", "right"])
def test_a_right_angle_relaxes_monotonically_to_a_straight_rest(sense, stiffness, relaxations):
    bends = M.bends([0], [1], [2], PI, stiffness)
    pos = np.array(RIGHT[sense], F32)
    centroid = pos.astype(np.float64).mean(axis=0)
    trail = [abs(float(s_of(pos, bends)[0]))]
    dev0 = float(M.deviation(pos, np.arange(3), bends)[0])
    assert abs(abs(dev0) - PI / 2) < 1e-6 and (dev0 > 0) == (sense == "right")       # the two senses differ in sign
    for _ in range(relaxations):
        pos = once(pos, bends)
        trail.append(abs(float(s_of(pos, bends)[0])))
    print("|s| after each relaxation (%s, stiffness %g): %s" % (sense, stiffness, " ".join("%.2e" % v for v in trail)))
    assert all(b < a for a, b in zip(trail, trail[1:]) if a >= 1e-3), trail      # monotonic down to the bound
    assert trail[-1] < 1e-3
    assert abs(float(M.deviation(pos, np.arange(3), bends)[0])) < 2e-3             # straight, not folded back
    assert np.abs(pos.astype(np.float64).mean(axis=0) - centroid).max() < 1e-5


@pytest.mark.parametrize("rest", [PI / 2, -PI / 2])
@pytest.mark.parametrize("start", ["straight", "left", "right"])
def test_a_triple_relaxes_monotonically_to_a_right_angle_rest(rest, start):
    bends = M.bends([0], [1], [2], rest, 0.5)
    pos = np.array(STRAIGHT if start == "straight" else RIGHT[start], F32)
    trail = [abs(float(M.deviation(pos, np.arange(3), bends)[0]))]
    for _ in range(16):
        pos = once(pos, bends)
        trail.append(abs(float(M.deviation(pos, np.arange(3), bends)[0])))
    print("|deviation| (rest %+.2f from %s): %s" % (rest, start, " ".join("%.2e" % v for v in trail)))
    assert all(b < a for a, b in zip(trail, trail[1:]) if a >= 1e-3), trail
    assert trail[-1] < 1e-3
    p = pos.astype(np.float64)
    u, v = p[0] - p[1], p[2] - p[1]
    angle = math.atan2(u[0] * v[1] - u[1] * v[0], u[0] * v[0] + u[1] * v[1])
    assert abs(angle - rest) < 2e-3                                    # the sign of the rest angle is kept


def test_mirror_images_stay_mirror_images():
    """x <-> y is a reflection that is exact in binary32, and the rule is symmetric under it bit for bit when the rest
    angle's sine changes sign"""
    rng = np.random.default_rng(11)
    pos = rng.uniform(90, 110, (12, 2)).astype(F32)
    t = np.array([rng.permutation(12)[:3] for _ in range(30)], U32)
    bends = M.bends(t[:, 0], t[:, 1], t[:, 2], rng.uniform(-PI, PI, 30), 0.5)
    mirrored = bends.copy()
    mirrored["rest_sin"] = -mirrored["rest_sin"]
    a, b = pos.copy(), pos[:, ::-1].copy()
    for _ in range(6):
        a, b = once(a, bends), once(b, mirrored)
        assert bits(a[:, ::-1]).tolist() == bits(b).tolist()
    assert not np.array_equal(a, pos)


def test_the_three_corrections_sum_to_zero_bit_for_bit_as_formed():
    rng = np.random.default_rng(5)
    n = 400
    p = rng.uniform(50, 150, (3, n, 2)).astype(F32)
    theta = rng.uniform(-PI, PI, n)
    acts, s, dax, day, dcx, dcy = M.rule(p[0, :, 0], p[0, :, 1], p[1, :, 0], p[1, :, 1], p[2, :, 0], p[2, :, 1],
                                         np.cos(theta).astype(F32), np.sin(theta).astype(F32), F32(0.7))
    assert acts.all() and (np.abs(s) <= 1).all() and (np.abs(s) == 1).any() and (np.abs(s) < 1).any()
    hx, hy = -(dax + dcx), -(day + dcy)
    assert bits((dax + dcx) + hx).tolist() == [0] * n and bits((day + dcy) + hy).tolist() == [0] * n
    # ... and one relaxation of a lone triple moves the hinge by exactly that share
    for j in range(5):
        pos = p[:, j, :]
        row = np.zeros(1, M.BEND_DTYPE)
        row["uid_a"], row["uid_b"], row["uid_c"] = 0, 1, 2
        row["rest_cos"], row["rest_sin"], row["stiffness"] = np.cos(theta[j]), np.sin(theta[j]), 0.7
        out = once(pos, row)
        want = np.array([[pos[0, 0] + dax[j], pos[0, 1] + day[j]], [pos[1, 0] + hx[j], pos[1, 1] + hy[j]],
                         [pos[2, 0] + dcx[j], pos[2, 1] + dcy[j]]], F32)
        assert bits(out).tolist() == bits(want).tolist()


def test_a_node_in_three_bends_sums_in_ascending_bend_index():
    """values for which another order of addition rounds differently: found by a seeded search, asserted to differ;
    particle 0 is a in bend 0, the hinge of bend 1 and c in bend 2"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        pos = rng.uniform(50, 150, (5, 2)).astype(F32)
        bends = M.bends([0, 1, 3], [1, 0, 4], [2, 3, 0], rng.uniform(-PI, PI, 3), 0.45)
        part, bend, vx, vy = M.shares(pos, np.arange(5, dtype=U32), bends)
        mine = part == 0
        assert bend[mine].tolist() == [0, 1, 2]
        c = [np.array([vx[mine][j], vy[mine][j]], F32) for j in range(3)]
        sums = {p: bits((F32(0) + c[p[0]]) + c[p[1]] + c[p[2]]).tolist() for p in itertools.permutations(range(3))}
        if len({tuple(v) for v in sums.values()}) > 1:
            break
    else:
        raise AssertionError("no values found whose sum depends on the order")
    acc = (np.zeros(2, F32) + c[0]) + c[1] + c[2]
    assert any(v != bits(acc).tolist() for v in sums.values())
    out = once(pos, bends)
    assert bits(out[0]).tolist() == bits(pos[0] + acc).tolist()
    # the same bends listed in another order are another set: the sum follows the new indices
    out2 = once(pos, bends[[2, 1, 0]])
    acc2 = (np.zeros(2, F32) + c[2]) + c[1] + c[0]
    assert bits(out2[0]).tolist() == bits(pos[0] + acc2).tolist()
    # where the particles are stored does not matter: permuted storage, the same positions by uid
    perm = np.array([3, 1, 4, 0, 2])
    out3 = once(pos[perm], bends, uids=perm)
    assert bits(out3).tolist() == bits(out[perm]).tolist()


def test_beyond_90_degrees_the_largest_correction_in_either_sense_and_the_fold_back():
    # rest pi.  c folded back to within 45 degrees of a, on either side: dt < 0, s = -1 / +1, never the small sine
    left, right = [[102, 100], [100, 100], [102, 101]], [[102, 100], [100, 100], [102, 99]]
    bends = M.bends([0], [1], [2], PI, 1.0)
    s_left, s_right = float(s_of(left, bends)[0]), float(s_of(right, bends)[0])
    assert {s_left, s_right} == {-1.0, 1.0}
    for pos, s in ((left, s_left), (right, s_right)):
        dev = float(M.deviation(np.array(pos, F32), np.arange(3), bends)[0])
        assert abs(dev) > PI / 2 and (dev > 0) == (s > 0)
        after = abs(float(M.deviation(once(pos, bends), np.arange(3), bends)[0]))
        assert after < abs(dev)                                        # it opens, it does not fold further
    # at exactly 90 degrees dt == 0 is not < 0: the sine itself, which is 1 there
    assert abs(float(s_of(RIGHT["left"], M.bends([0], [1], [2], -PI, 1.0))[0])) == 1.0
    # the exact fold-back: c on a.  cr == 0 and dt < 0 give s = +1 (with the exact rest (-1, 0))
    row = np.zeros(1, M.BEND_DTYPE)
    row["uid_a"], row["uid_b"], row["uid_c"], row["rest_cos"], row["stiffness"] = 0, 1, 2, -1.0, 1.0
    fold = [[102, 100], [100, 100], [104, 100]]
    acts, s, dax, day, dcx, dcy, _ = M.corrections(np.array(fold, F32), np.arange(3, dtype=U32), row)
    assert acts.all() and bits(s).tolist() == bits([1.0]).tolist()
    out = once(fold, row)
    assert not np.array_equal(out, np.array(fold, F32))
    assert abs(float(M.deviation(out, np.arange(3), row)[0])) < PI     # no longer folded flat


@pytest.mark.parametrize("other", [(100.0, 100.0), (NAN, 100.0), (100.0, NAN), (INF, 100.0), (-INF, INF),
                                   (1e20, 100.0), (3e38, -3e38), (100.0 + 1e-30, 100.0)])
@pytest.mark.parametrize("role", [0, 1, 2])
def test_every_inert_case_leaves_all_three_particles_alone(other, role):
    """coincident with the hinge (or the hinge with a), NaN, inf, an overflowing arm: inert, while a healthy bend on
    other particles acts.  All lie outside the world: an inert bend's particles are not even clamped."""
    pos = np.array([[-5.0, 100.0], [100.0, 100.0], [100.0, -7.0], [50, 50], [52, 50], [52, 52]], F32)
    if role == 1 and other == (100.0, 100.0):
        other = (-5.0, 100.0)                                          # the hinge on a
    pos[role] = other
    if role != 1 and other[0] == F32(100.0) and other[1] == 100.0:
        assert pos[role].tolist() == pos[1].tolist()                   # (100 + 1e-30 rounds to coincident)
    bends = np.concatenate([M.bends([0], [1], [2], 0.5, 1.0), M.bends([3], [4], [5], PI, 1.0)])
    acts = M.corrections(pos, np.arange(6, dtype=U32), bends)[0]
    assert acts.tolist() == [False, True]
    out = once(pos, bends)
    assert bits(out[:3]).tolist() == bits(pos[:3]).tolist()
    assert not np.array_equal(out[3:], pos[3:])


def test_an_underflowing_arm_and_an_absent_uid_are_inert():
    pos = np.array([[1e-30, 0.0], [0.0, 0.0], [0.0, 5.0]], F32)        # |u|^2 underflows to 0
    bends = M.bends([0], [1], [2], PI, 1.0)
    assert not M.corrections(pos, np.arange(3, dtype=U32), bends)[0].any()
    assert bits(once(pos, bends)).tolist() == bits(pos).tolist()
    pos = np.array([[1e-18, 5.0], [0.0, 5.0], [0.0, 9.0]], F32)        # lu = 1e-36 is positive: it acts, the lever is huge
    assert M.corrections(pos, np.arange(3, dtype=U32), bends)[0].all()
    # an absent uid: inert until the uid reappears
    bends = M.bends([0], [1], [7], PI, 1.0)
    assert bits(once(RIGHT["left"], bends)).tolist() == bits(RIGHT["left"]).tolist()
    assert not np.array_equal(once(RIGHT["left"], bends, uids=[0, 1, 7]), np.array(RIGHT["left"], F32))


def test_only_particles_with_an_acting_bend_are_clamped():
    world = (100.0, 100.0)
    # 0, 1, 2 form a bend at rest (stiffness 0 too): a zero correction still counts, all three are clamped.  3, 4, 5 lie
    # outside as well, sit in an inert bend (5 on 4) and keep every bit
    pos = [[-3.0, 50.0], [-3.0, 60.0], [-3.0, 70.0], [120.0, -7.0], [130.0, -7.0], [130.0, -7.0]]
    bends = np.concatenate([M.bends([0], [1], [2], PI, 0.0), M.bends([3], [4], [5], PI, 1.0)])
    out = once(pos, bends, world=world)
    assert out.tolist() == [[0.5, 50.0], [0.5, 60.0], [0.5, 70.0], [120.0, -7.0], [130.0, -7.0], [130.0, -7.0]]
    # pushed across the edge: the clamp keeps the particle inside, by its radius
    # (a right angle opening to a straight rest: the hinge moves in by (0.5, 0.5), a and c out by 0.5 each)
    corner = [[2.75, 0.75], [0.75, 0.75], [0.75, 2.75]]
    flat = M.bends([0], [1], [2], PI, 1.0)
    flat["rest_sin"] = 0.0                                             # (the exact (-1, 0): round numbers below)
    free = once(np.array(corner, F32) + F32(10), flat, world=world) - F32(10)
    assert free.tolist() == [[2.75, 0.25], [1.25, 1.25], [0.25, 2.75]]
    out = once(corner, flat, world=world)
    assert out.tolist() == [[2.75, 0.5], [1.25, 1.25], [0.5, 2.75]]


def test_duplicate_bends_both_act_and_a_relaxation_is_jacobi():
    one = once(RIGHT["left"], M.bends([0], [1], [2], PI, 0.25))
    two = once(RIGHT["left"], M.bends([0, 0], [1, 1], [2, 2], PI, 0.25))
    start = np.array(RIGHT["left"], F32)
    d1, d2 = one - start, two - start
    assert bits(d2).tolist() == bits(d1 + d1).tolist() and np.abs(d1).max() == 0.125   # (exact in these numbers)
    # Jacobi: two bends that share particles are both judged from the start
    chain = [[100, 100], [102, 100], [104, 101], [106, 100]]
    both = M.bends([0, 1], [1, 2], [2, 3], PI, 0.5)
    out = once(chain, both)
    start, uid = np.array(chain, F32), np.arange(4, dtype=U32)
    part, bend, vx, vy = M.shares(start, uid, both)
    for j in (0, 1):                                                   # each bend's shares are those it has alone
        alone = M.shares(start, uid, both[j:j + 1])
        assert bits(vx[bend == j]).tolist() == bits(alone[2]).tolist() and bits(vy[bend == j]).tolist() == bits(alone[3]).tolist()
    for p in (1, 2):                                                   # the two shared particles receive both, in order
        sx, sy = vx[part == p], vy[part == p]
        assert len(sx) == 2 and bend[part == p].tolist() == [0, 1]
        want = [start[p, 0] + ((F32(0) + sx[0]) + sx[1]), start[p, 1] + ((F32(0) + sy[0]) + sy[1])]
        assert bits(out[p]).tolist() == bits(want).tolist()
    assert not np.array_equal(out, once(once(chain, both[:1]), both[1:]))          # (one after the other differs)


# ---- one scene on the oracle ----------------------------------------------------------------------------------------
def cantilever(oracle, bend_iterations, steps=600):
    """8 particles in a horizontal row, spacing 2, the first two pinned by anchors: -> the tip's worst droop"""
    n = 8
    pos = np.stack([10.0 + 2.0 * np.arange(n), np.full(n, 10.0)], axis=1).astype(F32)
    uid = np.arange(n, dtype=U32)
    bonds = np.concatenate([BM.anchors([0, 1], pos[:2], stiffness=0.5), BM.pairs(uid[:-1], uid[1:], 2.0, stiffness=0.5)])
    tw = M.Twin(oracle, pos, np.full(n, 0.5, F32), world=(60.0, 60.0), gravity=(0.0, 10.0))
    tw.enable_uids()
    tw.set_bonds(bonds, 4)
    if bend_iterations:
        tw.set_bends(M.bends(uid[:-2], uid[1:-1], uid[2:], PI, 0.5), bend_iterations)
    droop = 0.0
    for _ in range(steps):
        tw.step(1.0 / 60.0)
        p = tw.arrays()[0]
        assert np.isfinite(p).all()
        droop = max(droop, float(p[-1, 1]) - 10.0)
    info = tw.bends_info()
    tw.close()
    assert info["passes"] == (steps if bend_iterations else 0)
    return droop


def test_a_cantilever_droops_less_with_bends_and_less_again_with_iterations(oracle):
    free, one, eight = cantilever(oracle, 0), cantilever(oracle, 1), cantilever(oracle, 8)
    print("the tip's worst droop in 600 steps: %.3f without bends, %.3f with 1 bend iteration, %.3f with 8" % (free, one, eight))
    assert eight < 0.5 * free
    assert eight < one


# ---- the stand-alone program and the headers ------------------------------------------------------------------------
def write_table(path):
    """a random set over 60 particles (uid = index; uids from 60 up name nobody), one relaxation by the model"""
    rng = np.random.default_rng(17)
    n, k = 60, 200
    world = (120.0, 90.0)
    pos = rng.uniform(2, 80, (n, 2)).astype(F32)
    pos[:12] = rng.uniform(-3, 3, (12, 2)).astype(F32) + F32(1.0)      # near and across the edge: the clamp works
    pos[20] = (NAN, 30.0)
    pos[22] = pos[21]                                                  # a coincident pair
    pos[24] = (1e20, 5.0)
    rad = rng.uniform(0.25, 1.0, n).astype(F32)
    t = np.array([rng.permutation(n + 6)[:3] for _ in range(k)], U32)
    t[:4] = [[20, 1, 2], [21, 22, 3], [4, 21, 22], [5, 24, 6]]
    theta = rng.choice([PI, PI / 2, -PI / 2, 0.3, -2.5], k)
    bends = M.bends(t[:, 0], t[:, 1], t[:, 2], theta, rng.choice([0.0, 0.25, 0.5, 1.0], k))
    bends["rest_cos"][7], bends["rest_sin"][7] = -1.0, -0.0
    uids = np.arange(n, dtype=U32)
    acts, _, dax, day, dcx, dcy, _ = M.corrections(pos, uids, bends)
    out, _ = M.relax(pos, rad, uids, bends, world)
    assert 100 < acts.sum() < k and not acts[:4].any()
    h = lambda a: " ".join("%08x" % v for v in bits(a).reshape(-1))
    with open(path, "w") as f:
        f.write("%d %d %s\n" % (n, k, h(world)))
        for i in range(n):
            f.write("%s %s\n" % (h(pos[i]), h(rad[i])))
        for b in bends:
            f.write("%d %d %d %s\n" % (b["uid_a"], b["uid_b"], b["uid_c"], h([b["rest_cos"], b["rest_sin"], b["stiffness"]])))
        for j in range(k):
            f.write("%d %s\n" % (acts[j], h([dax[j], day[j], dcx[j], dcy[j]])))
        for i in range(n):
            f.write("%s\n" % h(out[i]))
    return int(acts.sum())


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bend_graph_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer, replaying the model's table bit for bit."""
    exe = str(tmp_path / "bend_graph_tests")
    table = str(tmp_path / "table.txt")
    acting = write_table(table)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [GRAPH_SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == GRAPH_TESTS
    r = subprocess.run([exe, "--table", table], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in GRAPH_TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "replayed 200 bends, %d acting, 60 particles" % acting in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_headers_hold_no_hip_and_the_layers_agree_on_the_constants():
    csrc = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
    for name in ("k_bend.h", "bend_graph.h"):
        text = open(os.path.join(csrc, name)).read()
        assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text), name
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    lib = open(os.path.join(ROOT, "gpu-physics-engine_amd", "_lib.py")).read()
    for name, value in (("BENDS_MAX", M.BENDS_MAX), ("BEND_MAX_DEGREE", M.BEND_MAX_DEGREE), ("BEND_ITER_MAX", M.BEND_ITER_MAX)):
        assert int(re.search(r"#define GPE_%s\s+(\d+)u" % name, header).group(1)) == value, name
    m = re.search(r"^BENDS_MAX, BEND_MAX_DEGREE, BEND_ITER_MAX = (\d+), (\d+), (\d+)$", lib, flags=re.M)
    assert [int(v) for v in m.groups()] == [M.BENDS_MAX, M.BEND_MAX_DEGREE, M.BEND_ITER_MAX]
    body = re.search(r"typedef struct gpe_bend \{(.*?)\} gpe_bend;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == list(M.BEND_DTYPE.names)
    fields = re.search(r"class GpeBend\(C\.Structure\):.*?_fields_ = \[(.*?)\]\n", lib, flags=re.S).group(1)
    assert re.findall(r"\(\"([a-z_]+)\"", fields) == list(M.BEND_DTYPE.names)
    for what in ("no angular constraint", "gpe_set_bends", "step -> bends -> bonds -> bodies", "Jacobi relaxation is weak"):
        assert what in header, what
