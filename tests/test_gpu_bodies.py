"""GPU (-m gpu): rigid and soft bodies (gpe_set_bodies / _get_bodies / _apply_bodies / _get_body_poses /
_get_bodies_info, csrc/k_bodies.hip, csrc/gpe_bodies.hip, csrc/body_table.h).

A pass is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy model
(tests/_bodies_model.py: no tables, no width classes, the uids looked up afresh), and the steps against the CPU oracle
with the model's bonds, bodies and colliders passes behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS
and ends with no damaged red zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _bodies_model as M
from tests import _bonds_model as BM
from tests._oracle_model import circle_mask

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
NAN, INF = float("nan"), float("inf")
ABSENT = M.UID_ABSENT
BODY_TAGS = {"uid.body_rec", "uid.body_order", "uid.body_member_uid", "uid.body_member_slot", "uid.body_member_rest",
             "uid.body_pose", "uid.body_state", "uid.body_broken"}
COUNTS = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 4095, 4096]


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def same_poses(a, b):
    """bit for bit, any NaN equal to any NaN (the buffer starts as all-ones NaNs, the pass writes the default NaN)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE


def _state(gpe, pos, rad, world, mode="native", prev=None, gravity=(0.0, 0.0), flags=0, uids=True, **kw):
    st = gpe.State(pos, rad, world=world, gravity=gravity, prev=prev, mode=_mode(gpe, mode),
                   flags=gpe._lib.FLAG_GUARD_ALLOCS | flags, **kw)
    if uids:
        st.enable_uids()
    return st


def _end(st):
    """every context ends here: no red zone of a live or a released buffer is damaged"""
    zones = st.ctx.guard_check()
    assert st.ctx.guard_damaged == 0, zones
    tags = {t for t, _, _, _ in st.ctx.guard_registry()}
    st.close()
    return tags


def _arrays(st):
    return st.positions(), st.previous_positions(), st.radii()


def _rows(gpe, bodies):
    assert gpe.BODY_DTYPE == M.BODY_DTYPE
    return np.ascontiguousarray(bodies, gpe.BODY_DTYPE)


def _info(st):
    info = st.bodies_info()
    info.pop("resolves")
    return info


def _same_set(st, tw, what):
    rec, broken, uid, rest = st.bodies()
    assert rec.tobytes() == tw.bodies.tobytes() and np.array_equal(broken, tw.bodies_broken), what
    assert np.array_equal(uid, tw.member_uid) and same_bits(rest, tw.member_rest), what
    assert _info(st) == tw.bodies_info(), what


def _same_as_twin(st, tw, what, by_uid=False, poses=True):
    pos, prev, rad = tw.arrays()
    got = _arrays(st)
    if by_uid:
        a, b = np.argsort(st.uids()), np.argsort(tw.uids)
        assert np.array_equal(st.uids()[a], tw.uids[b]), what
        got, (pos, prev, rad) = [x[a] for x in got], [x[b] for x in (pos, prev, rad)]
    elif tw.uids is not None:
        assert np.array_equal(st.uids(), tw.uids), what
    bad = np.nonzero((bits(got[0]) != bits(pos)).any(axis=1))[0] if got[0].shape == pos.shape else "shape"
    assert same_bits(got[0], pos), (what, bad[:5], got[0][bad[:5]], pos[bad[:5]])
    assert same_bits(got[1], prev) and same_bits(got[2], rad), what
    _same_set(st, tw, what)
    if poses and tw.body_passes > 0:
        assert same_poses(st.body_poses(), tw.poses), what
    rec, broken = st.bonds()
    assert rec.tobytes() == tw.bonds.tobytes() and np.array_equal(broken, tw.broken), what


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
PASS_WORLD = (400.0, 400.0)
SPECIAL = ["one_absent", "all_but_one_absent", "all_absent", "coincident", "nan", "inf", "1e30", "breaks_first",
           "breaks_third", "edge"]


def _pass_scene():
    """12 000 particles on a jittered 128-wide lattice of spacing 3, stored in a random order under uids that are no
    storage indices.  Bodies of every count of COUNTS over runs of lattice neighbours (the big two first), their rest
    shapes the lattice turned by a random angle in a frame of their own; then the special bodies of SPECIAL.  ->
    (pos, rad, uids, bodies, member_uid, member_rest, body index of every special, body index per count)."""
    rng = np.random.default_rng(12)
    n = 12000
    i = np.arange(n)
    grid = np.stack([5.0 + 3.0 * (i % 128), 5.0 + 3.0 * (i // 128)], axis=1)
    where = (grid + rng.uniform(-0.3, 0.3, (n, 2))).astype(F32)          # by lattice index
    uid_of = (rng.permutation(n).astype(np.uint64) * 7919 + 11).astype(U32)          # by lattice index
    counts, groups, stiff, bd = [], [], [], []
    at = 0
    plain = {}
    for count in sorted(COUNTS, reverse=True) + [4] * 40 + [2] * 35 + [7] * 10 + [12] * 6 + [20] * 3 + [40, 50, 70]:
        plain.setdefault(count, len(counts))
        counts.append(count)
        groups.append(np.arange(at, at + count))
        free = float(rng.choice([1.0, 0.5, 0.25, 0.0, rng.uniform(0, 1)]))
        stiff.append((1.0, 0.625, 0.25)[len(counts) % 3] if len(counts) <= len(COUNTS) else free)   # the first of each count moves
        bd.append(float(rng.choice([0.0, 0.0, 50.0])))
        at += count
    special = {}
    for name in SPECIAL:
        count = {"one_absent": 9, "all_but_one_absent": 5, "all_absent": 3, "edge": 2, "breaks_first": 6}.get(name, 4)
        special[name] = len(counts)
        counts.append(count)
        groups.append(np.arange(at, at + count))
        stiff.append(1.0)
        bd.append({"breaks_first": 2.0, "breaks_third": 2.0}.get(name, 0.5 if name in ("coincident", "nan", "inf", "1e30") else 0.0))
        at += count
    assert at < n - 200
    member = np.concatenate(groups)
    member_uid = uid_of[member].copy()
    rest = []
    for g in groups:
        a = rng.uniform(0, 2 * np.pi)
        turn = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        rest.append(grid[g] @ turn + rng.uniform(-500, 500, 2))
    member_rest = np.concatenate(rest).astype(F32)
    bodies = M.rows(counts, np.array(stiff, F32), np.array(bd, F32))

    def members(name):
        b = bodies[special[name]]
        return np.arange(b["first"], b["first"] + b["count"])

    ghosts = 0xF0000000 + np.arange(16, dtype=U32)                       # uids no particle has
    member_uid[members("one_absent")[4]] = ghosts[0]
    member_uid[members("all_but_one_absent")[1:]] = ghosts[1:5]
    member_uid[members("all_absent")] = ghosts[5:8]
    where[member[members("coincident")]] = where[member[members("coincident")[0]]]
    where[member[members("nan")[1]]] = (NAN, 100.0)
    where[member[members("inf")[2]]] = (100.0, -INF)
    where[member[members("1e30")[0]]] = (1e30, 100.0)
    where[member[members("breaks_first")[3]]] += F32(9.0)                # far out of shape: e2 > 4
    # the edge: two members 3 apart now, 30 at rest, next to the left wall: the match pushes one of them out
    e = member[members("edge")]
    where[e] = [(2.0, 390.0), (5.0, 390.0)]
    member_rest[members("edge")] = [(0.0, 0.0), (30.0, 0.0)]
    order = rng.permutation(n)                                           # storage order
    return (where[order], np.full(n, 0.5, F32), uid_of[order], bodies, member_uid, member_rest, special, plain)


def _pass_reference():
    """three passes of the model over _pass_scene; before the third, one member of `breaks_third` is put 9 away"""
    pos, rad, uids, bodies, member_uid, member_rest, special, plain = _pass_scene()
    b = bodies[special["breaks_third"]]
    pushed_uid = member_uid[b["first"] + 2]
    frames = []
    p, broken = pos, np.zeros(len(bodies), bool)
    for k in range(3):
        if k == 2:
            p = p.copy()
            p[BM.slots_of(uids, [pushed_uid])[0]] += F32(9.0)
        p, broken, pose, verdict = M.apply(p, rad, uids, bodies, member_uid, member_rest, broken, PASS_WORLD)
        frames.append((p, broken.copy(), pose, verdict))
    # no case may hide: every class acts, every inert kind and both breaks occur, in the model's own outcome
    v0 = frames[0][3]
    for count in COUNTS:
        assert v0[plain[count]] == M.ACTS, count
    for G in (2, 4, 8, 16, 32, 64):
        of_class = np.array([M.width(c) == G for c in bodies["count"]])
        assert (v0[of_class] == M.ACTS).sum() >= 2, G
    for name in ("all_but_one_absent", "all_absent", "coincident", "nan", "inf", "1e30"):
        assert all(f[3][special[name]] == M.INERT for f in frames), name
    assert v0[special["one_absent"]] == M.ACTS and v0[special["edge"]] == M.ACTS
    assert [bool(f[1][special["breaks_first"]]) for f in frames] == [True, True, True]
    assert [bool(f[1][special["breaks_third"]]) for f in frames] == [False, False, True]
    assert frames[0][3][special["breaks_third"]] == M.ACTS
    edge = BM.slots_of(uids, member_uid[bodies[special["edge"]]["first"]:][:2])
    assert frames[0][0][edge[0]].tolist() == [0.5, 390.0]                # pushed across the wall: clamped by its radius
    moved = (bits(frames[0][0]) != bits(pos)).any(axis=1)
    assert 8000 < moved.sum() < 11800                                    # both outcomes
    assert (bodies["stiffness"] == 0).sum() >= 3
    return (pos, rad, uids, bodies, member_uid, member_rest), pushed_uid, frames


@pytest.fixture(scope="module")
def pass_reference():
    return _pass_reference()


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_pass_equals_the_model(gpe, pass_reference, mode):
    """apply_bodies() alone, three passes: pos bit for bit as the model, prev and radius untouched, the poses, the
    broken flags and the counters the model's."""
    (pos, rad, uids, bodies, member_uid, member_rest), pushed_uid, frames = pass_reference
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, PASS_WORLD, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bodies(_rows(gpe, bodies), member_uid, member_rest)
    rec, broken, uid, rest = st.bodies()
    assert rec.tobytes() == bodies.tobytes() and not broken.any()
    assert np.array_equal(uid, member_uid) and same_bits(rest, member_rest)
    assert np.isnan(st.body_poses()).all() and st.body_poses().shape == (len(bodies), 4)
    for k, (want, want_broken, want_pose, _) in enumerate(frames):
        if k == 2:
            where = st.find_uids([pushed_uid])[1] + F32(9.0)
            assert st.edit_particles(uids=[pushed_uid], positions=where) == 1
            prev = st.previous_positions()                               # (an edit of pos carries prev along: the velocity stays)
        st.apply_bodies()
        got, got_prev, got_rad = _arrays(st)
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (k, bad[:5], got[bad[:5]], want[bad[:5]])
        off = np.nonzero((bits(got_prev) != bits(prev)).any(axis=1))[0]
        assert off.size == 0 and same_bits(got_rad, rad), (k, off[:5], got_prev[off[:5]], prev[off[:5]])
        assert np.array_equal(st.bodies()[1], want_broken), (k, np.nonzero(st.bodies()[1] != want_broken)[0][:10])
        poses = st.body_poses()
        off = np.nonzero(~((bits(poses) == bits(want_pose)) | (np.isnan(poses) & np.isnan(want_pose))).all(axis=1))[0]
        assert off.size == 0, (k, off[:5], poses[off[:5]], want_pose[off[:5]])
        nb = int(want_broken.sum())
        assert st.bodies_info() == dict(k=len(bodies), members=len(member_uid), passes=k + 1, live=len(bodies) - nb,
                                        broken=nb, resolves=1)
    tags = _end(st)
    assert BODY_TAGS <= tags


@pytest.mark.parametrize("G", [2, 4, 8, 16, 32, 64])
def test_the_wave_boundary_of_every_class(gpe, G):
    """1 body, and one fewer than, exactly and one more than the bodies a wave serves, of one class alone; the sets
    replace each other on one context"""
    per = 64 // G
    rng = np.random.default_rng(G)
    n = 3000
    pos = np.stack([rng.uniform(5, 195, n), rng.uniform(5, 195, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    uids = (rng.permutation(n).astype(np.uint64) * 13 + 5).astype(U32)
    st = _state(gpe, pos, rad, (200.0, 200.0), prev=pos)
    st.set_uids(uids)
    for nb in sorted({1, max(per - 1, 1), per, per + 1, 4 * per + 1}):
        st.edit_particles(indices=np.arange(n, dtype=U32), positions=pos)
        lo = G // 2 + 1
        counts = rng.integers(lo, G + 1, nb)
        counts[0] = G
        if G == 64 and nb > 1:
            counts[-1] = 200                                            # a looping body among the one-round ones
        bodies = M.rows(counts, rng.uniform(0.2, 1.0, nb).astype(F32), 0.0)
        m = int(counts.sum())
        member = rng.choice(n, m, replace=False)
        # members scattered anywhere; the rest shape: where they are, turned, with noise: every body acts
        a = rng.uniform(0, 2 * np.pi)
        turn = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        rest = (pos[member].astype(np.float64) @ turn + rng.uniform(-1, 1, (m, 2))).astype(F32)
        st.set_bodies(_rows(gpe, bodies), uids[member], rest)
        want, broken, pose, verdict = M.apply(pos, rad, uids, bodies, uids[member], rest, np.zeros(nb, bool), (200.0, 200.0))
        assert (verdict == M.ACTS).all() and not broken.any()
        st.apply_bodies()
        got = st.positions()
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (nb, bad[:5], got[bad[:5]], want[bad[:5]])
        assert same_poses(st.body_poses(), pose), nb
        assert (bits(want) != bits(pos)).any(axis=1).sum() == m
        assert st.bodies_info() == dict(k=nb, members=m, passes=1, live=nb, broken=0, resolves=1)
    _end(st)


# ---- 2. the hook: a pendulum and bricks above a floor ---------------------------------------------------------------
YARD_WORLD, YARD_GRAVITY = (60.0, 60.0), (0.0, 100.0)
YARD_COLLIDERS = np.array([[-5, 45, 65, 45, 5], [40, 30, 40, 30, 3]], F32)      # a floor and a peg
STEPS = 60


def yard_scene():
    """uid = storage index at the start.  A 3 x 3 pendulum hung by an anchor bond from its top centre member, six
    bricks of 4 x 2 (one of them brittle) over the floor, a soft blob of 17, and 120 loose particles falling on them."""
    rng = np.random.default_rng(4)
    block = lambda x, y, w, h, d=1.05: np.stack([x + d * (np.arange(w * h) % w), y + d * (np.arange(w * h) // w)], axis=1)
    parts = [block(10.0, 12.0, 3, 3)]
    parts += [block(18.0 + 6.0 * b, 30.0 - 3.0 * (b % 2), 4, 2) for b in range(6)]
    a = 2 * np.pi * np.arange(16) / 16
    parts.append(np.concatenate([[[30.0, 15.0]], 30.0 + 0 * a[:, None] + np.stack([2.7 * np.cos(a), 2.7 * np.sin(a) - 15.0], axis=1)]))
    counts = [len(p) for p in parts]
    loose = np.stack([rng.uniform(8, 52, 120), rng.uniform(2, 9, 120)], axis=1)
    pos = np.concatenate(parts + [loose]).astype(F32)
    m = int(np.sum(counts))
    bodies = M.rows(counts, 1.0, 0.0)
    bodies["stiffness"][7] = 0.3                                         # the blob is soft
    bodies["break_distance"][3] = 0.08                                   # one brick is brittle
    member_uid = np.arange(m, dtype=U32)
    member_rest = pos[:m].copy()
    bonds = np.concatenate([BM.anchors([1], [(11.05, 6.0)], 6.0, 1.0), BM.pairs([9], [17], 6.0, 0.2, 0.0)])
    return pos, np.full(len(pos), 0.5, F32), bodies, member_uid, member_rest, bonds


def yard_twin(oracle, bodies=True, bonds=True, colliders=True):
    pos, rad, b, mu, mr, bo = yard_scene()
    tw = M.Twin(oracle, pos, rad, world=YARD_WORLD, gravity=YARD_GRAVITY)
    tw.enable_uids()
    if bonds:
        tw.set_bonds(bo, 2)
    if bodies:
        tw.set_bodies(b, mu, mr)
    if colliders:
        tw.set_colliders(YARD_COLLIDERS)
    return tw


def yard_state(gpe, mode="native", bodies=True, bonds=True, colliders=True, **kw):
    pos, rad, b, mu, mr, bo = yard_scene()
    st = _state(gpe, pos, rad, YARD_WORLD, gravity=YARD_GRAVITY, mode=mode, **kw)
    if bonds:
        st.set_bonds(np.ascontiguousarray(bo, gpe.BOND_DTYPE), 2)
    if bodies:
        st.set_bodies(_rows(gpe, b), mu, mr)
    if colliders:
        st.set_colliders(YARD_COLLIDERS)
    return st


def _frames(tw, steps, resort_every=0, resort_first=False):
    frames = []
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(DT, resort=bool(resort))
        pos, prev, _ = tw.arrays()
        frames.append((pos.copy(), prev.copy(), tw.uids.copy(), tw.bodies_broken.copy(), tw.poses.copy()))
    return frames


@pytest.fixture(scope="module")
def yard(oracle):
    """the reference of the hook tests: oracle step -> model bonds -> model bodies -> model colliders, 60 steps"""
    tw = yard_twin(oracle)
    frames = _frames(tw, STEPS)
    info, pushed, bonds_info = tw.bodies_info(), tw.pushed, tw.bonds_info()
    tw.close()
    pos = frames[-1][0]
    assert pushed > 0 and np.isfinite(pos).all()
    assert frames[-1][3].tolist() == [False, False, False, True, False, False, False, False]   # the brittle brick broke
    assert not frames[5][3].any()                                        # ... on landing, not at once
    assert pos[:9, 1].max() < 20.0 and pos[9:57, 1].mean() > 33.0 and pos[9:57, 1].max() < 39.6   # the pendulum hangs, the bricks fell from 29 on to the floor at 40
    brick = pos[9:17].astype(np.float64)                                 # a whole brick is still a 4 x 2 block
    d = np.sqrt(((brick[:, None] - brick[None]) ** 2).sum(axis=2))
    d0 = np.sqrt(((yard_scene()[0][9:17, None].astype(np.float64) - yard_scene()[0][None, 9:17]) ** 2).sum(axis=2))
    assert np.abs(d - d0).max() < 0.25
    return frames, info, pushed, bonds_info


@pytest.fixture(scope="module")
def yard_resorted(oracle):
    tw = yard_twin(oracle)
    frames = _frames(tw, STEPS, resort_every=16, resort_first=True)
    info = tw.bodies_info()
    tw.close()
    return frames, info


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_twin(gpe, yard, mode):
    frames, info, pushed, bonds_info = yard
    L = gpe._lib
    st = yard_state(gpe, mode)
    for s in range(STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
        if s % 10 == 9:
            assert same_poses(st.body_poses(), frames[s][4]) and np.array_equal(st.bodies()[1], frames[s][3]), s
    assert _info(st) == info and st.bodies_info()["resolves"] == 1 and st.colliders_info()["pushed"] == pushed
    got = st.bonds_info()
    got.pop("resolves")
    assert got == bonds_info
    pipe = st.ctx.pipeline_info()
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == STEPS
    else:
        assert pipe["compat_steps"] == STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_twin_and_the_observers_see_the_result(gpe, yard, mode):
    frames, info, pushed, _ = yard
    st = yard_state(gpe, mode)
    uids = np.array([0, 4, 9, 30, 60, 100], U32)
    st.tracers_begin(uids, every=1, frames=64, prev=True)
    st.monitor_begin(every=1, frames=64)
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
    assert _info(st) == info and st.colliders_info()["pushed"] == pushed
    assert same_poses(st.body_poses(), frames[-1][4]) and np.array_equal(st.bodies()[1], frames[-1][3])
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == STEPS and recorded == STEPS
    n = len(pos)
    for s in range(STEPS):                                               # frames taken behind the bodies and the colliders
        p, q = frames[s][0], frames[s][1]
        assert same_bits(tr.pos[s], p[uids]) and same_bits(tr.prev[s], q[uids]), s
        assert rec["max_y"][s] == p[:, 1].max() and rec["min_y"][s] == p[:, 1].min() and rec["n"][s] == n
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 3. re-sorts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_resorts_keep_the_bodies_on_their_particles(gpe, yard_resorted, mode):
    frames, info = yard_resorted

    def by_uid(st, s):
        a, b = np.argsort(st.uids()), np.argsort(frames[s][2])
        pos, prev, _ = _arrays(st)
        assert same_bits(pos[a], frames[s][0][b]) and same_bits(prev[a], frames[s][1][b]), s

    st = yard_state(gpe, mode)
    st.run(DT, STEPS, resort_every=16, resort_first=True)
    by_uid(st, STEPS - 1)
    assert not np.array_equal(st.uids(), np.arange(len(frames[0][0])))   # the re-sorts did move the particles
    assert _info(st) == info and st.bodies_info()["resolves"] == 4       # before steps 0, 16, 32, 48
    assert np.array_equal(st.bodies()[1], frames[-1][3]) and same_poses(st.body_poses(), frames[-1][4])
    _end(st)
    # step by step: the uids are looked up again only on the steps after a re-sort
    st = yard_state(gpe, mode)
    for s in range(40):
        st.update(DT, resort=(s % 16 == 0))
        assert st.bodies_info()["resolves"] == 1 + s // 16, s
        if s in (0, 15, 16, 17, 39):
            by_uid(st, s)
    _end(st)


# ---- 4. the kept block table ----------------------------------------------------------------------------------------
def test_the_kept_block_table_survives_positions_moved_behind_its_back(gpe, oracle):
    """220 x 220 (625 blocks: two radix passes): most native steps reuse the kept table, with the bonds, the bodies and
    the colliders moving particles behind it.  Every step as the twin, by gpe_step and by gpe_run."""
    L = gpe._lib
    world, gravity, n, steps = (220.0, 220.0), (0.0, 40.0), 4000, 40
    rng = np.random.default_rng(8)
    pos = np.stack([rng.uniform(1, 219, n), rng.uniform(1, 150, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    # 20 bodies of 20 particles (the first 400), 4 x 5 blocks, every other one hung from an anchor by its first member
    j = np.arange(400)
    b, i = j // 20, j % 20
    pos[:400] = np.stack([8.0 + 10.5 * b + 1.1 * (i % 4), 5.0 + 12.0 * (b % 3) + 1.1 * (i // 4)], axis=1)
    bodies = M.rows([20] * 20, np.where(np.arange(20) % 4 == 3, 0.5, 1.0).astype(F32), 0.0)
    heads = np.arange(0, 400, 40)
    bonds = BM.anchors(heads, pos[heads], 0.0, 0.5)
    pegs = [[20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 3.0]
            for i in range(11) for j in range(4)]
    cs = np.array([[-5, 185, 225, 185, 10], [30, 40, 110, 70, 1], [200, 30, 120, 75, 0]] + pegs, F32)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids(); tw.set_bonds(bonds, 1); tw.set_bodies(bodies, np.arange(400), pos[:400]); tw.set_colliders(cs)
    ctxs = []
    for _ in range(2):
        st = _state(gpe, pos, rad, world, gravity=gravity)
        st.set_bonds(np.ascontiguousarray(bonds, gpe.BOND_DTYPE), 1)
        st.set_bodies(_rows(gpe, bodies), np.arange(400), pos[:400]); st.set_colliders(cs)
        ctxs.append(st)
    st, runner = ctxs
    for s in range(steps):
        st.update(DT, resort=(s == 0)); tw.step(DT, resort=(s == 0))
        _same_as_twin(st, tw, s)
    runner.run(DT, steps, resort_every=0, resort_first=True)
    _same_as_twin(runner, tw, "gpe_run")
    assert not np.isnan(tw.poses).any() and tw.pushed > 0
    for ctx in (st, runner):
        pipe = ctx.ctx.pipeline_info()
        print("native sorts in %d steps: %d" % (steps, pipe["native_sorts"]))
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == steps and pipe["sort_passes"] >= 2
        assert pipe["native_sorts"] < steps, "every step sorted: the kept table was never used"
        assert ctx.bodies_info()["resolves"] == 1
        _end(ctx)
    tw.close()


# ---- 5. no bodies, no trace -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_bodies_nothing_changes_and_nothing_is_launched(gpe, oracle, yard, mode):
    tw = yard_twin(oracle, bodies=False)
    plain = _frames(tw, 20)
    tw.close()
    never = yard_state(gpe, mode, bodies=False, profiling=True)
    cleared = yard_state(gpe, mode, profiling=True)
    cleared.clear_bodies()
    empty = dict(k=0, members=0, passes=0, live=0, broken=0, resolves=0)
    seen = []
    for st in (never, cleared):
        rec, broken, uid, rest = st.bodies()
        assert len(rec) == len(broken) == len(uid) == len(rest) == 0 and st.bodies_info() == empty
        assert st.body_poses().shape == (0, 4)
        st.ctx.reset_timings()
        st.apply_bodies()                                                # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, plain[19][0]) and same_bits(prev, plain[19][1])
        scopes = {name: v[1] for name, v in st.ctx.timings().items()}
        live = sorted(t for t, _, _, state in st.ctx.guard_registry() if state == "live")
        assert not any(name == "Bodies" or name.startswith("bodies/") for name in scopes)
        assert not any(t.startswith("uid.body_") for t in live)
        seen.append((scopes, live))
        _end(st)
    assert seen[0] == seen[1]                                            # the scopes, their counts and the live buffers
    armed = yard_state(gpe, mode, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), yard[0][19][0])
    t = armed.ctx.timings()
    classes = len({M.width(c) for c in yard_scene()[2]["count"]})
    assert classes == 3 and t["Bodies"][1] == 20 and t["bodies/match"][1] == 20 * classes and t["bodies/resolve"][1] == 1
    _end(armed)


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_and_the_broken_flags_survive_everything_but_set_bodies(gpe, oracle, mode):
    L = gpe._lib
    st = yard_state(gpe, mode)
    tw = yard_twin(oracle)
    rng = np.random.default_rng(21)

    def steps(what, k=3):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what)

    steps("start", 45)
    assert tw.bodies_broken.tolist() == [False, False, False, True, False, False, False, False]
    band = circle_mask(tw.arrays()[0], 30.0, 38.0, 4.0)
    assert st.kick_circle((30.0, 38.0), 4.0, L.VEL_ADD, (1.0, -3.0)) == tw.kick(band, L.VEL_ADD, 1.0, -3.0) > 0
    steps("kick", 4)
    add = rng.uniform(2, 12, (100, 2)).astype(F32)
    st.add_particles(add, np.full(100, 0.5, F32)); tw.add(add, np.full(100, 0.5, F32))
    steps("add")
    cand = rng.uniform(1, 59, (60, 2)).astype(F32)
    added, _ = st.add_particles_free(cand, np.full(60, 0.5, F32))
    assert added == tw.add_free(cand, np.full(60, 0.5, F32))[1] > 0
    steps("add_particles_free")
    # an eraser through the first brick: some of its members go, the rest stays rigid
    p = tw.arrays()[0]
    slots = BM.slots_of(tw.uids, np.arange(9, 17))
    centre = p[slots[:2]].mean(axis=0)
    gone = st.remove_particles_in_circle(centre, 0.8)
    assert gone == tw.remove_circle(centre[0], centre[1], 0.8) > 0
    steps("eraser")
    left = BM.slots_of(tw.uids, np.arange(9, 17))
    assert 2 <= (left >= 0).sum() < 8 and not tw.bodies_broken[1] and not np.isnan(tw.poses[1]).any()
    q = tw.arrays()[0][left[left >= 0]].astype(np.float64)
    r0 = yard_scene()[4][9:17][left >= 0].astype(np.float64)
    dist = lambda x: np.sqrt(((x[:, None] - x[None]) ** 2).sum(axis=2))
    assert np.abs(dist(q) - dist(r0)).max() < 0.3                        # the survivors keep their distances
    mask = np.zeros(len(tw), np.uint8); mask[BM.slots_of(tw.uids, [20, 40])] = 1
    assert st.remove_particles(mask) == tw.remove_mask(mask) == 2
    steps("remove mask")
    assert st.remove_particles_by_uid([0, 58, 4000000]) == tw.remove_uids([0, 58, 4000000]) == 2
    steps("remove uid")
    who = np.arange(0, 60, 2, dtype=U32)
    where = (tw.arrays()[0][who] + F32(0.25)).astype(F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit by index")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    resolves = st.bodies_info()["resolves"]
    steps("quiet steps")
    assert st.bodies_info()["resolves"] == resolves                      # nothing moved the particles: no new lookup
    grow = np.stack([rng.uniform(2, 58, 1500), rng.uniform(1, 9, 1500)], axis=1).astype(F32)     # past the capacity
    st.add_particles(grow, np.full(1500, 0.2, F32)); tw.add(grow, np.full(1500, 0.2, F32))
    steps("growth", 2)
    st.ctx.call("gpe_reserve", 20000)
    steps("reserve", 1)
    other = L.MODE_NATIVE if mode == "compat" else L.MODE_COMPAT
    st.ctx.call("gpe_set_mode", other); tw.set_mode(other)
    steps("set_mode", 2)
    # a removed uid comes back on another particle: it is a member again
    u = tw.uids.copy()
    assert 58 not in u
    u[len(u) - 1] = 58
    st.set_uids(u); tw.set_uids(u)
    st.apply_bodies(); tw.apply_bodies()
    _same_as_twin(st, tw, "set_uids")
    assert tw.bodies_broken[7] or not np.isnan(tw.poses[7]).any()
    # gpe_set_particles renumbers the uids from 0: the bodies name the new particles
    pos, rad = yard_scene()[:2]
    pos = (pos + F32(1.0)).astype(F32)
    f = C.POINTER(C.c_float)
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), pos.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))
    tw.set_particles(pos, pos, rad)
    steps("set_particles")
    assert tw.bodies_broken[3]                                           # the flags are the set's, not the particles'
    # a new set clears the flags and the counters
    st.set_bodies(_rows(gpe, tw.bodies), tw.member_uid, tw.member_rest); tw.set_bodies(tw.bodies, tw.member_uid, tw.member_rest)
    assert st.bodies_info() == dict(k=8, members=len(tw.member_uid), passes=0, live=8, broken=0, resolves=0)
    assert np.isnan(st.body_poses()).all()
    steps("new set")
    tw.close()
    _end(st)


# ---- 7. save / load -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_continue_on_the_same_bits(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    st = yard_state(gpe, mode)
    tw = yard_twin(oracle)
    st.run(DT, 45, resort_every=8, resort_first=True); tw.run(DT, 45, resort_every=8, resort_first=True)
    _same_as_twin(st, tw, "before save", by_uid=False)
    assert tw.bodies_broken.any() and not tw.bodies_broken.all()
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["bodies"].tobytes() == tw.bodies.tobytes() and np.array_equal(d["bodies_broken"], tw.bodies_broken)
        assert np.array_equal(d["body_member_uid"], tw.member_uid) and same_bits(d["body_member_rest"], tw.member_rest)
        assert "bonds" in d.files
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    rec, broken, uid, rest = back.bodies()
    assert rec.tobytes() == tw.bodies.tobytes() and np.array_equal(broken, tw.bodies_broken)
    nb = int(broken.sum())
    assert back.bodies_info() == dict(k=8, members=len(uid), passes=0, live=8 - nb, broken=nb, resolves=0)
    passes, bond_passes = tw.body_passes, tw.bond_passes
    tw.run(DT, 12, resort_every=5, resort_first=False)
    for s in (st, back):
        s.run(DT, 12, resort_every=5, resort_first=False)
        tw.body_passes = passes + 12 if s is st else 12
        tw.bond_passes = bond_passes + 12 if s is st else 12
        _same_as_twin(s, tw, "after load")
        info = s.bonds_info(); info.pop("resolves")
        assert info == tw.bonds_info()
    _end(back)
    # a context without bodies writes none and loads none
    st.clear_bodies()
    st.save(path)
    with np.load(path) as d:
        assert not any(name.startswith("bod") for name in d.files)
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    assert len(back.bodies()[0]) == 0
    _end(back)
    _end(st)
    tw.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    st = yard_state(gpe)
    tw = yard_twin(oracle)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.bodies_info()
    held = st.bodies()
    poses = st.body_poses()

    def untouched(what):
        rec, broken, uid, rest = st.bodies()
        assert rec.tobytes() == held[0].tobytes() and np.array_equal(broken, held[1]), what
        assert np.array_equal(uid, held[2]) and same_bits(rest, held[3]), what
        assert st.bodies_info() == info and same_poses(st.body_poses(), poses), what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    h = st.ctx.h
    k, m = C.c_uint64(), C.c_uint64()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def attempt(bodies, uid, rest, k=None, members=None, null=()):
        """bodies: (first, count, stiffness, break_distance, flags, reserved) each"""
        rows = (L.GpeBody * max(len(bodies), 1))()
        for o, b in zip(rows, bodies):
            o.first, o.count, o.stiffness, o.break_distance, o.flags, o.reserved = b
        uid = np.array(uid, U32)
        rest = np.array(rest, F32).reshape(-1)
        return lib.gpe_set_bodies(h, None if "bodies" in null else rows, len(bodies) if k is None else k,
                                  None if "uid" in null else uid.ctypes.data_as(u32p),
                                  None if "rest" in null else rest.ctypes.data_as(f32p),
                                  len(uid) if members is None else members)

    ok = [(0, 3, 1.0, 0.0, 0, 0), (3, 2, 0.5, 1.0, 0, 0)]
    uid5, rest5 = [1, 2, 3, 4, 5], [[0, 0], [1, 0], [0, 1], [5, 5], [6, 5]]

    def one(body=1, uid=uid5, rest=rest5, **change):
        names = ["first", "count", "stiffness", "break_distance", "flags", "reserved"]
        rows = [list(b) for b in ok]
        for name, v in change.items():
            rows[body][names.index(name)] = v
        return lambda: attempt([tuple(r) for r in rows], uid, rest)

    binfo = L.GpeBodiesInfo(struct_size=C.sizeof(L.GpeBodiesInfo))
    assert lib.gpe_set_bodies(None, None, 0, None, None, 0) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bodies(None, None, None, 0, C.byref(k), None, None, 0, C.byref(m)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_bodies(None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_body_poses(None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bodies_info(None, C.byref(binfo)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")
    bad = {
        "NULL bodies": lambda: attempt(ok, uid5, rest5, null=("bodies",)),
        "NULL member_uid": lambda: attempt(ok, uid5, rest5, null=("uid",)),
        "NULL member_rest": lambda: attempt(ok, uid5, rest5, null=("rest",)),
        "k > GPE_BODIES_MAX": lambda: attempt(ok, uid5, rest5, k=L.BODIES_MAX + 1),
        "members > GPE_BODY_MEMBERS_MAX": lambda: attempt(ok, uid5, rest5, members=L.BODY_MEMBERS_MAX + 1),
        "count 1": one(count=1, first=4), "count 0": one(count=0),
        "count 4097": lambda: attempt([(0, L.BODY_MAX_MEMBERS + 1, 1.0, 0.0, 0, 0)], np.arange(L.BODY_MAX_MEMBERS + 1),
                                      np.zeros((L.BODY_MAX_MEMBERS + 1, 2))),
        "ranges overlap": one(first=2, count=3), "past members": one(count=3),
        "members unused at the end": one(uid=uid5 + [6], rest=rest5 + [[7, 7]]),
        "members unused in between": lambda: attempt([(0, 2, 1.0, 0.0, 0, 0), (3, 2, 1.0, 0.0, 0, 0)], uid5, rest5),
        "uid absent": one(uid=[1, 2, ABSENT, 4, 5]), "uid twice": one(uid=[1, 2, 3, 4, 1]),
        "NaN rest": one(rest=[[0, 0], [NAN, 0], [0, 1], [5, 5], [6, 5]]),
        "inf rest": one(rest=[[0, 0], [1, 0], [0, 1], [5, -INF], [6, 5]]),
        "NaN stiffness": one(stiffness=NAN), "stiffness > 1": one(stiffness=1.5), "stiffness < 0": one(stiffness=-0.25),
        "NaN break": one(break_distance=NAN), "inf break": one(break_distance=INF), "negative break": one(break_distance=-0.5),
        "unknown flag": one(flags=2), "reserved": one(reserved=1),
        "info struct_size": lambda: lib.gpe_get_bodies_info(h, C.byref(L.GpeBodiesInfo(struct_size=C.sizeof(L.GpeBodiesInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_bodies_info(h, None),
        "get NULL k": lambda: lib.gpe_get_bodies(h, None, None, 0, None, None, None, 0, C.byref(m)),
        "get NULL members": lambda: lib.gpe_get_bodies(h, None, None, 0, C.byref(k), None, None, 0, None),
        "poses NULL k": lambda: lib.gpe_get_body_poses(h, None, 0, None),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        assert b"gpe_" in lib.gpe_last_error(h), what                    # the message names the call
        untouched(what)
    assert (L.BODIES_MAX, L.BODY_MAX_MEMBERS, L.BODY_MEMBERS_MAX, L.BODY_BROKEN) == (1048576, 4096, 16777216, 1)
    # while the set is held: the uids stay on, and the context cannot be sharded
    pos, rad = yard_scene()[:2]
    keys = np.arange(len(rad), dtype=U32)
    st.clear_bonds()                                                     # (the bonds refuse the same calls, and first)
    holding = {
        "gpe_enable_uids": lambda: lib.gpe_enable_uids(h, 0),
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, len(rad), len(rad) - 10),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), len(rad), 0),
    }
    for what, call in holding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"bodies" in lib.gpe_last_error(h) and what.encode() in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK and lib.gpe_enable_uids(h, 1) == L.GPE_OK     # no change: allowed
    untouched("allowed calls")
    st.set_bonds(np.ascontiguousarray(yard_scene()[5], gpe.BOND_DTYPE), 2)
    # a partial read delivers the first rows; each output may be NULL
    out, flags = (L.GpeBody * 3)(), (C.c_uint8 * 3)(9, 9, 9)
    some_uid, some_rest = np.full(4, 77, U32), np.full(8, 77.0, F32)
    assert lib.gpe_get_bodies(h, out, flags, 2, C.byref(k), some_uid.ctypes.data_as(u32p), some_rest.ctypes.data_as(f32p), 3,
                              C.byref(m)) == L.GPE_OK
    assert (k.value, m.value) == (8, len(held[2]))
    assert (out[0].count, out[1].first, out[1].count, out[2].count) == (9, 9, 8, 0) and list(flags) == [0, 0, 9]
    assert some_uid.tolist() == [0, 1, 2, 77] and same_bits(some_rest[:6], held[3][:3].ravel()) and some_rest[6] == 77.0
    assert lib.gpe_get_bodies(h, None, flags, 3, C.byref(k), None, None, 0, C.byref(m)) == L.GPE_OK and list(flags) == [0, 0, 0]
    two = np.full(12, 5.0, F32)
    assert lib.gpe_get_body_poses(h, two.ctypes.data_as(f32p), 2, C.byref(k)) == L.GPE_OK and k.value == 8
    assert same_poses(two[:8].reshape(2, 4), poses[:2]) and (two[8:] == 5.0).all()
    # the context goes on as the twin does
    for _ in range(5):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 in break_distance is accepted and stored as +0; a body given broken starts broken; the largest count is taken
    assert attempt([(0, 3, 1.0, -0.0, 0, 0), (3, 2, 0.5, 1.0, L.BODY_BROKEN, 0)], uid5, rest5) == L.GPE_OK
    rec, broken, _, _ = st.bodies()
    assert bits(rec["break_distance"][:1]).tolist() == [0] and rec["flags"].tolist() == [0, 0] and broken.tolist() == [False, True]
    assert st.bodies_info() == dict(k=2, members=5, passes=0, live=1, broken=1, resolves=0)
    st.update(DT)
    assert st.bodies()[1].tolist() == [False, True] and np.isnan(st.body_poses()[1]).all()
    big = np.arange(L.BODY_MAX_MEMBERS)
    assert attempt([(0, L.BODY_MAX_MEMBERS, 1.0, 0.0, 0, 0)], big, np.stack([big % 64, big // 64], axis=1)) == L.GPE_OK
    st.update(DT)
    # without uids: GPE_ERR_STATE, and nothing is held
    st.clear_bodies(); st.clear_bonds()
    st.enable_uids(False)
    assert attempt(ok, uid5, rest5) == L.GPE_ERR_STATE and b"gpe_set_bodies" in lib.gpe_last_error(h)
    assert st.bodies_info()["k"] == 0
    assert lib.gpe_set_bodies(h, None, 0, None, None, 0) == L.GPE_OK     # clearing nothing needs no uids
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_bodies(gpe, how):
    L = gpe._lib
    pos, rad, b, mu, mr, _ = yard_scene()
    st = _state(gpe, pos, rad, YARD_WORLD, uids=False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_bodies(_rows(gpe, b), mu, mr)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.bodies()[0]) == 0 and st.bodies_info()["k"] == 0
    st.apply_bodies()
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)


def test_bodies_from_groups_captures_the_current_positions(gpe):
    pos, rad, _, _, _, _ = yard_scene()
    st = _state(gpe, pos, rad, YARD_WORLD, gravity=YARD_GRAVITY)
    st.run(DT, 3, resort_every=0, resort_first=True)                     # (the storage order is no longer the uids')
    groups = [[5, 3, 8], np.arange(20, 30), [100, 57]]
    rows, uid, rest = st.bodies_from_groups(groups, stiffness=[1.0, 0.5, 0.25], break_distance=2.0)
    assert rows["first"].tolist() == [0, 3, 13] and rows["count"].tolist() == [3, 10, 2]
    assert rows["stiffness"].tolist() == [1.0, 0.5, 0.25] and rows["break_distance"].tolist() == [2.0] * 3
    assert uid.tolist() == [5, 3, 8] + list(range(20, 30)) + [100, 57]
    assert same_bits(rest, st.positions()[BM.slots_of(st.uids(), uid)])
    st.set_bodies(rows, uid, rest)
    before = st.positions()
    st.apply_bodies()                                                    # in its rest shape: nothing moves further than rounding
    assert np.abs(st.positions() - before).max() < 1e-4 and not np.isnan(st.body_poses()).any()
    with pytest.raises(ValueError):
        st.bodies_from_groups([[1, 2, 4000000]])
    _end(st)


# ---- 9. a seeded random interleaving --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_random_interleaving_against_the_twin(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    rng = np.random.default_rng(87 if mode == "native" else 88)
    world, gravity = (60.0, 60.0), (0.0, 80.0)
    n = 600
    pos = np.stack([rng.uniform(2, 58, n), rng.uniform(2, 40, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world, gravity=gravity, mode=mode)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids()

    def random_set():
        """bodies over particles that are close now (their current shape, a little off), and a few uids nobody has"""
        p, uids = tw.arrays()[0], tw.uids
        free = np.ones(len(uids), bool)
        groups = []
        for _ in range(int(rng.integers(3, 25))):
            count = int(rng.choice([2, 3, 4, 5, 8, 9, 17, 33, 70]))
            seed = int(rng.integers(0, len(uids)))
            near = np.argsort(((p - p[seed]) ** 2).sum(axis=1))
            near = near[free[near]][:count]
            if len(near) < 2:
                continue
            free[near] = False
            groups.append(near)
        counts = [len(g) for g in groups]
        slot = np.concatenate(groups)
        member_uid = uids[slot].copy()
        ghosts = rng.choice(len(member_uid), 3, replace=False)
        member_uid[ghosts] = 3000000000 + np.arange(3)
        rest = (p[slot] + rng.uniform(-0.2, 0.2, (len(slot), 2))).astype(F32)
        bodies = M.rows(counts, rng.uniform(0.1, 1.0, len(counts)).astype(F32),
                        np.where(rng.random(len(counts)) < 0.4, 0.6, 0.0).astype(F32))
        return bodies, member_uid, rest

    def random_bonds():
        uids, p = tw.uids, tw.arrays()[0]
        pins = rng.choice(len(uids), 5, replace=False)
        return BM.anchors(uids[pins], p[pins], 0.0, 0.5)

    def random_colliders():
        return np.array([[-5, 52, 65, 52, 8], [rng.uniform(10, 50), 35, rng.uniform(10, 50), 38, rng.uniform(0, 3)]], F32)

    ops = ["set_bodies", "clear", "step", "run", "add", "remove", "edit", "kick", "resort", "apply", "colliders", "bonds",
           "saveload"]
    weights = np.array([4, 1, 6, 5, 2, 3, 2, 2, 2, 2, 2, 2, 2], float)
    log, most_passes, all_passes, ever_broken, ever_acting = [], 0, 0, 0, 0
    b = random_set()
    st.set_bodies(_rows(gpe, b[0]), b[1], b[2]); tw.set_bodies(*b)
    for i in range(40):
        op = str(rng.choice(ops, p=weights / weights.sum()))
        passes_before = tw.body_passes
        log.append(op)
        if op == "set_bodies":
            b = random_set()
            st.set_bodies(_rows(gpe, b[0]), b[1], b[2]); tw.set_bodies(*b)
        elif op == "clear":                                              # a step without bodies, then another set
            st.clear_bodies(); tw.set_bodies(np.zeros(0, M.BODY_DTYPE), np.zeros(0, U32), np.zeros((0, 2), F32))
            st.update(DT); tw.step(DT)
            _same_as_twin(st, tw, (i, log, "cleared"))
            b = random_set()
            st.set_bodies(_rows(gpe, b[0]), b[1], b[2]); tw.set_bodies(*b)
        elif op == "step":
            for _ in range(int(rng.integers(1, 4))):
                resort = bool(rng.integers(0, 4) == 0)
                st.update(DT, resort=resort); tw.step(DT, resort=resort)
        elif op == "run":
            k, every, first = int(rng.integers(2, 9)), int(rng.integers(0, 4)), bool(rng.integers(0, 2))
            st.run(DT, k, resort_every=every, resort_first=first); tw.run(DT, k, resort_every=every, resort_first=first)
        elif op == "add":
            k = int(rng.integers(1, 40))
            p = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 30, k)], axis=1).astype(F32)
            st.add_particles(p, np.full(k, 0.5, F32)); tw.add(p, np.full(k, 0.5, F32))
        elif op == "remove":
            if rng.integers(0, 2):
                c, r = rng.uniform(10, 50, 2), float(rng.uniform(1, 5))
                if 0 < int(circle_mask(tw.arrays()[0], c[0], c[1], r).sum()) < len(tw):
                    assert st.remove_particles_in_circle(c, r) == tw.remove_circle(c[0], c[1], r)
            else:
                gone = rng.choice(tw.uids, 6, replace=False)
                assert st.remove_particles_by_uid(gone) == tw.remove_uids(gone) == 6
        elif op == "edit":
            k = int(rng.integers(1, 30))
            who = rng.choice(len(tw), k, replace=False).astype(U32)
            where = np.stack([rng.uniform(1, 59, k), rng.uniform(1, 45, k)], axis=1).astype(F32)
            st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
        elif op == "kick":
            c, r = rng.uniform(10, 50, 2), float(rng.uniform(3, 10))
            a = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
            mask = circle_mask(tw.arrays()[0], c[0], c[1], r)
            assert st.kick_circle(c, r, L.VEL_ADD, a) == tw.kick(mask, 0, a[0], a[1])
        elif op == "resort":
            st.particles.sort_by_cell_id(); tw.morton_resort()
        elif op == "apply":
            st.apply_bodies(); tw.apply_bodies()
        elif op == "colliders":
            cs = random_colliders() if rng.integers(0, 3) else np.zeros((0, 5), F32)
            st.set_colliders(cs); tw.set_colliders(cs)
        elif op == "bonds":
            bo = random_bonds() if rng.integers(0, 3) else np.zeros(0, BM.BOND_DTYPE)
            st.set_bonds(np.ascontiguousarray(bo, gpe.BOND_DTYPE), 1); tw.set_bonds(bo, 1)
        else:
            path = str(tmp_path / ("s%d.npz" % i))
            st.save(path)
            _end(st)
            st = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
            tw.body_passes = tw.bond_passes = 0                          # (load sets both anew, the flags with them)
            tw.passes = tw.pushed = 0
            tw.poses = np.full((len(tw.bodies), 4), np.nan, F32)
        _same_as_twin(st, tw, (i, log))
        assert same_bits(st.colliders(), tw.colliders), (i, log)
        all_passes += tw.body_passes - (0 if op in ("set_bodies", "clear", "saveload") else passes_before)
        most_passes = max(most_passes, tw.body_passes)
        ever_broken = max(ever_broken, int(tw.bodies_broken.sum()))
        ever_acting = max(ever_acting, int((~np.isnan(tw.poses).any(axis=1)).sum()) if tw.body_passes else 0)
    print(" ".join(log), "| passes:", all_passes, "| most under one set:", most_passes, "| most broken:", ever_broken,
          "| most acting:", ever_acting)
    assert {"set_bodies", "step", "run"} <= set(log) and all_passes >= 20 and most_passes >= 3 and ever_acting > 2
    tw.close()
    _end(st)
