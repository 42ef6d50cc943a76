"""CPU: the rigid and soft bodies' pass as the numpy model states it (tests/_bodies_model.py, include/gpe.h "rigid and
soft bodies"): exact poses for rest shapes on small-integer coordinates, stiffness, breaks, every inert case; and the
body table's stand-alone test program (tests/cpp/body_table_tests.cpp over csrc/body_table.h and csrc/k_body.h), plain
and under the host sanitizers, which also runs k_body.h's host restatement of the pass against vectors the model
writes."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import _bodies_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
WORLD = (4000.0, 4000.0)
NAN, INF = float("nan"), float("inf")
TABLE_SRC = os.path.join(ROOT, "tests", "cpp", "body_table_tests.cpp")
TABLE_TESTS = ["validation", "widths_and_classes", "class_lists", "records_and_broken", "sum_order", "vectors"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def once(pos, rest, counts=None, stiffness=1.0, bd=0.0, rad=0.5, broken=None, world=WORLD, uids=None, member_uid=None):
    """one pass over bodies that own the particles in storage order (or member_uid's)"""
    pos = np.array(pos, F32).reshape(-1, 2)
    rest = np.array(rest, F32).reshape(-1, 2)
    n = len(pos)
    counts = [len(rest)] if counts is None else counts
    bodies = M.rows(counts, stiffness, bd)
    uids = np.arange(n, dtype=U32) if uids is None else np.array(uids, U32)
    member_uid = np.arange(len(rest), dtype=U32) if member_uid is None else np.array(member_uid, U32)
    broken = np.zeros(len(bodies), bool) if broken is None else np.array(broken, bool)
    return M.apply(pos, np.full(n, rad, F32), uids, bodies, member_uid, rest, broken, world)


def lattice(count):
    """count members at small-integer coordinates: a block 16 wide"""
    j = np.arange(count)
    return np.stack([j % 16, j // 16], axis=1).astype(F32)


# ---- exactness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 4, 8, 16, 32, 64, 128, 256])
def test_a_rest_pose_translated_or_turned_by_right_angles_is_exact(count):
    """Small integers and a power-of-two count: every sum, mean and product is exact, so a body in its rest shape is
    left unchanged to the bit, with the pose of the turn."""
    rest = lattice(count)
    shift = np.array([100.0, 200.0], F32)
    turns = {(1.0, 0.0): rest, (0.0, 1.0): np.stack([-rest[:, 1], rest[:, 0]], axis=1),
             (-1.0, 0.0): -rest}
    for (co, si), shape in turns.items():
        pos = (shape + shift).astype(F32)
        out, broken, pose, verdict = once(pos, rest, bd=1e-3)
        assert verdict.tolist() == [M.ACTS] and not broken.any()
        assert bits(out).tolist() == bits(pos).tolist(), (count, co, si)
        centre = pos.astype(np.float64).mean(axis=0)
        assert pose[0].tolist() == [centre[0], centre[1], co, si], (count, co, si)


def test_the_rest_frame_does_not_matter_and_stiffness_scales_the_way():
    rest = lattice(8)
    pos = (rest + F32(50)).astype(F32)
    pos[3] += F32(2)                                                   # one member pushed out of shape
    full, _, pose1, _ = once(pos, rest)
    moved, _, pose2, _ = once(pos, rest + F32(1024))                    # the rest shape given in another frame
    assert bits(full).tolist() == bits(moved).tolist() and bits(pose1).tolist() == bits(pose2).tolist()
    assert not np.array_equal(full, pos)
    # full stiffness lands every member on the matched pose: a second pass is (nearly) still
    again, _, _, _ = once(full, rest)
    assert np.abs(again - full).max() < 1e-4
    # stiffness 0 moves nothing, to the bit; the pose is reported all the same
    none, _, pose0, verdict = once(pos, rest, stiffness=0.0)
    assert bits(none).tolist() == bits(pos).tolist() and verdict.tolist() == [M.ACTS]
    assert bits(pose0).tolist() == bits(pose1).tolist()
    # stiffness 0.5 goes half of the way (exactly half: a power of two)
    half, _, _, _ = once(pos, rest, stiffness=0.5)
    e = full.astype(np.float64) - pos
    assert np.abs(half - (pos + 0.5 * e)).max() < 1e-5
    # the members' order is part of the body, not of the storage: permuted storage, the same positions by uid
    perm = np.array([3, 1, 0, 2, 7, 6, 5, 4])
    stored, _, _, _ = once(pos[perm], rest, uids=perm)
    assert bits(stored).tolist() == bits(full[perm]).tolist()


def test_a_break_is_strict_sticky_and_moves_nothing():
    # two members 4 apart at rest, 8 apart now: every number is exact, each member is 2 from its place, e2 = 4
    rest = np.array([[0, 0], [4, 0]], F32)
    pos = np.array([[10, 10], [18, 10]], F32)
    worst = F32(2)
    out, broken, pose, verdict = once(pos, rest, bd=worst)
    assert verdict.tolist() == [M.ACTS] and not broken.any()          # d == break_distance holds
    assert out.tolist() == [[12.0, 10.0], [16.0, 10.0]] and pose.tolist() == [[14.0, 10.0, 1.0, 0.0]]
    below = np.nextafter(worst, F32(0))
    out, broken, pose, verdict = once(pos, rest, bd=below)
    assert verdict.tolist() == [M.BROKEN] and broken.tolist() == [True]
    assert bits(out).tolist() == bits(pos).tolist() and np.isnan(pose).all()    # nothing moves in the breaking pass
    # sticky: back in its rest shape, still broken and still silent
    out, broken, pose, verdict = once(rest + F32(10), rest, bd=below, broken=[True])
    assert broken.tolist() == [True] and bits(out).tolist() == bits(rest + F32(10)).tolist() and np.isnan(pose).all()
    # a break distance of 0 never breaks, however far
    far = pos.copy()
    far[0] = (3000.0, 3000.0)
    _, broken, _, verdict = once(far, rest, bd=0.0)
    assert verdict.tolist() == [M.ACTS] and not broken.any()
    # one body breaks, its neighbour in the set acts
    two = np.concatenate([pos, rest + F32(100)])
    out, broken, pose, verdict = once(two, np.concatenate([rest, rest]), counts=[2, 2], bd=below)
    assert verdict.tolist() == [M.BROKEN, M.ACTS] and broken.tolist() == [True, False]
    assert np.isnan(pose[0]).all() and pose[1].tolist() == [102.0, 100.0, 1.0, 0.0]


@pytest.mark.parametrize("what", ["nan", "inf", "overflow", "coincident", "underflow", "one_live", "none_live"])
def test_every_inert_case_leaves_pos_untouched_and_is_not_broken(what):
    rest = lattice(8)
    pos = (rest + F32(50)).astype(F32)
    pos[2] += F32(1)
    uids = np.arange(8, dtype=U32)
    if what == "nan":
        pos[5] = (NAN, 50.0)
    elif what == "inf":
        pos[5] = (INF, 50.0)
    elif what == "overflow":
        pos[5] = (1e30, -1e30)
    elif what == "coincident":
        pos[:] = (70.0, 70.0)
    elif what == "underflow":
        rest = rest * F32(1e-25)                                        # A, B are about 1e-23: A*A + B*B underflows to 0
    elif what == "one_live":
        uids = np.array([0, 90, 91, 92, 93, 94, 95, 96], U32)
    else:
        uids = np.arange(90, 98, dtype=U32)
    out, broken, pose, verdict = once(pos, rest, bd=0.001, uids=uids)
    assert verdict.tolist() == [M.INERT] and not broken.any()
    assert bits(out).tolist() == bits(pos).tolist() and np.isnan(pose).all()
    # and it acts again when the trouble is gone
    out, broken, pose, verdict = once(lattice(8) + F32(50), lattice(8), bd=0.001)
    assert verdict.tolist() == [M.ACTS]


def test_absent_members_are_left_out_of_every_sum():
    """the live members of a body with absent ones move as the body of the live members alone would (the same lanes
    add the same values: an absent member adds +0.0f where it stands)"""
    rest = lattice(8)
    pos = (rest + F32(50)).astype(F32)
    pos[1] += F32(1.5)
    uids = np.array([0, 1, 2, 3, 90, 5, 6, 7], U32)                     # member 4 names no particle
    out, _, pose, verdict = once(pos, rest, uids=uids)
    assert verdict.tolist() == [M.ACTS] and bits(out[4]).tolist() == bits(pos[4]).tolist()
    live = [0, 1, 2, 3, 5, 6, 7]
    want = pos.astype(np.float64)[live].mean(axis=0)
    assert np.abs(pose[0, :2] - want).max() < 1e-5
    assert (bits(out[live]) != bits(pos[live])).any()


def test_members_are_clamped_into_the_world_with_their_radius():
    rest = np.array([[0, 0], [10, 0]], F32)
    pos = np.array([[1.0, 50.0], [7.0, 50.0]], F32)                     # squeezed to 6 apart: the match pushes both out by 2
    out, _, _, _ = once(pos, rest, world=(100.0, 100.0))
    assert out.tolist() == [[0.5, 50.0], [9.0, 50.0]]                   # -1 is outside: clamped to the radius
    out, _, _, _ = once(pos, rest, world=(100.0, 100.0), rad=2.0)
    assert out.tolist() == [[2.0, 50.0], [9.0, 50.0]]


def test_the_canonical_sum_is_the_lanes_then_the_halving_tree():
    v = np.array([[1e8, 1.0, -1e8, 1.0, 3.0]], F32)
    assert M.canon_sum(v).tolist() == [2.0] and float(np.cumsum(v[0])[-1]) == 4.0
    assert [M.width(c) for c in (2, 3, 4, 5, 8, 9, 33, 64, 65, 4096)] == [2, 4, 4, 8, 8, 16, 64, 64, 64, 64]
    rng = np.random.default_rng(1)
    w = rng.uniform(-1000, 1000, (3, 130)).astype(F32)
    partial = np.zeros((3, 64), F32)
    for j in range(130):
        partial[:, j % 64] = partial[:, j % 64] + w[:, j]
    off = 32
    while off:
        partial[:, :off] = partial[:, :off] + partial[:, off:2 * off]
        off //= 2
    assert bits(M.canon_sum(w)).tolist() == bits(partial[:, 0]).tolist()
    assert not np.signbit(M.canon_sum(np.array([[-0.0, -0.0]], F32)))[0]


# ---- the stand-alone program and the headers ------------------------------------------------------------------------
def _vector_cases():
    """(count, stiffness, bd, rest, pos, radius, live) over every width, counts beyond 64, absent members, breaks and
    the inert kinds"""
    rng = np.random.default_rng(11)
    cases = []
    for count in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 1000, 4096):
        rest = rng.uniform(-20, 20, (count, 2)).astype(F32)
        angle = rng.uniform(0, 2 * np.pi)
        turn = np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
        pos = (rest.astype(np.float64) @ turn + (300, 300) + rng.uniform(-0.3, 0.3, (count, 2))).astype(F32)
        rad = rng.uniform(0.2, 1.0, count).astype(F32)
        live = np.ones(count, bool)
        cases.append((count, 1.0, 0.0, rest, pos, rad, live))
        cases.append((count, float(rng.uniform(0, 1)), 5.0, rest, pos, rad, live))
        cases.append((count, 0.5, 0.05, rest, pos, rad, live))                      # the jitter breaks it
        some = rng.random(count) < 0.7
        cases.append((count, 0.75, 0.0, rest, pos, rad, some))
        one = np.zeros(count, bool)
        one[count // 2] = True
        cases.append((count, 1.0, 0.0, rest, pos, rad, one))                         # inert: L = 1
        odd = pos.copy()
        odd[count - 1] = (NAN, 1.0) if count % 2 else (1e30, 1e30)
        cases.append((count, 1.0, 1.0, rest, odd, rad, live))                        # inert: NaN / overflow
        edge = (pos - F32(295)).astype(F32)
        cases.append((count, 1.0, 0.0, rest, edge, rad, live))                       # across the world's edge: clamped
    return cases


def _write_vectors(path):
    acts = breaks = inert = 0
    with open(path, "wb") as f:
        cases = _vector_cases()
        f.write(struct.pack("<I", len(cases)))
        for count, stiffness, bd, rest, pos, rad, live in cases:
            verdict, target, pose = M.match(rest[None], np.where(live[:, None], pos, F32(0)).astype(F32)[None], live[None],
                                            np.array([stiffness], F32), np.array([bd], F32))
            out = pos.copy()
            if verdict[0] == M.ACTS:
                from tests import _colliders_model as CM
                with np.errstate(all="ignore"):
                    x = CM.clamp_f(target[0, :, 0], rad, F32(WORLD[0]) - rad)
                    y = CM.clamp_f(target[0, :, 1], rad, F32(WORLD[1]) - rad)
                out[live, 0], out[live, 1] = x[live], y[live]
            acts, breaks, inert = acts + (verdict[0] == M.ACTS), breaks + (verdict[0] == M.BROKEN), inert + (verdict[0] == M.INERT)
            f.write(struct.pack("<Iffff", count, stiffness, bd, *WORLD))
            for a in (rest[:, 0], rest[:, 1], pos[:, 0], pos[:, 1], rad):
                f.write(np.ascontiguousarray(a, "<f4").tobytes())
            f.write(live.astype("<u4").tobytes())
            f.write(struct.pack("<I", int(verdict[0])))
            f.write(np.ascontiguousarray(pose[0], "<f4").tobytes())
            f.write(np.ascontiguousarray(out[:, 0], "<f4").tobytes())
            f.write(np.ascontiguousarray(out[:, 1], "<f4").tobytes())
    assert acts >= 40 and breaks >= 10 and inert >= 30, (acts, breaks, inert)
    return len(cases)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_body_table_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  It checks every refusal and the class lists
    and runs k_body.h's pass on the host against the model's vectors."""
    exe = str(tmp_path / "body_table_tests")
    vectors = str(tmp_path / "vectors.bin")
    cases = _write_vectors(vectors)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [TABLE_SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TABLE_TESTS
    r = subprocess.run([exe, "--vectors", vectors], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TABLE_TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "%d cases:" % cases in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_headers_hold_no_hip_and_the_layers_agree_on_the_constants():
    csrc = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
    for name in ("k_body.h", "body_table.h"):
        text = open(os.path.join(csrc, name)).read()
        assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text), name
    header = open(os.path.join(ROOT, "include", "gpe.h")).read()
    for name, value in (("GPE_BODIES_MAX", M.BODIES_MAX), ("GPE_BODY_MAX_MEMBERS", M.BODY_MAX_MEMBERS),
                        ("GPE_BODY_MEMBERS_MAX", M.BODY_MEMBERS_MAX), ("GPE_BODY_BROKEN", M.BODY_BROKEN)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, header).group(1)) == value, name
    body = re.search(r"typedef struct gpe_body \{(.*?)\} gpe_body;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == list(M.BODY_DTYPE.names)
    for what in ("deforms a body until the next pass", "overlap at rest", "breaks at the first touch"):
        assert what in " ".join(header.split()).replace(" * ", " "), what
    lib = open(os.path.join(ROOT, "gpu-physics-engine_amd", "_lib.py")).read()
    for name in ("gpe_set_bodies", "gpe_get_bodies", "gpe_apply_bodies", "gpe_get_body_poses", "gpe_get_bodies_info"):
        assert '"%s"' % name in lib and re.search(r"\b%s\(" % name, header), name
