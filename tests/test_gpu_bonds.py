"""GPU (-m gpu): distance bonds (gpe_set_bonds / _get_bonds / _apply_bonds / _get_bonds_info, csrc/k_bonds.hip,
csrc/gpe_bonds.hip, csrc/bond_graph.h).

A relaxation is a binary32 function of the set and the particles: every comparison is bit for bit against the numpy
model (tests/_bonds_model.py: no graph, the uids looked up afresh), and the steps against the CPU oracle with the
model's bonds pass and the colliders' pass behind every step.  Every context runs under GPE_FLAG_GUARD_ALLOCS and ends
with no damaged red zone."""
import ctypes as C

import numpy as np
import pytest

from tests import _bonds_model as M
from tests._oracle_model import circle_mask

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
DT = 1.0 / 60.0
NAN, INF = float("nan"), float("inf")
WORLD = (200.0, 200.0)
ABSENT = M.UID_ABSENT
# (the registry's naming scheme has no prefix of its own for them: they are keyed by uid and carry "uid.bond_")
BOND_TAGS = {"uid.bond_rec", "uid.bond_node_uid", "uid.bond_node_slot", "uid.bond_row_start", "uid.bond_inc",
             "uid.bond_corr", "uid.bond_state", "uid.bond_broken"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _mode(gpe, mode):
    return gpe.MODE_COMPAT if mode == "compat" else gpe.MODE_NATIVE


def _state(gpe, pos, rad, world=WORLD, mode="native", prev=None, gravity=(0.0, 0.0), flags=0, uids=True, **kw):
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


def _rows(gpe, bonds):
    """the model's rows as the engine's (the same layout)"""
    assert gpe.BOND_DTYPE == M.BOND_DTYPE
    return np.ascontiguousarray(bonds, gpe.BOND_DTYPE)


def _info(st):
    info = st.bonds_info()
    info.pop("resolves")
    return info


def _same_as_twin(st, tw, what, by_uid=False):
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
    rec, broken = st.bonds()
    assert rec.tobytes() == tw.bonds.tobytes() and np.array_equal(broken, tw.broken), what
    assert _info(st) == tw.bonds_info(), what


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------
def _pass_scene(n):
    """n particles on a jittered 64-wide lattice of spacing 3 with uids that are no storage indices, and about 3000
    bonds: near pairs, a chain, a hub of degree 200, a leaf, a duplicate, absent uids, anchors, coincident ends, NaN /
    inf / 1e30 positions, breaks in the first and in the third relaxation, a pull across the world's edge.  The last
    60 storage slots hold the particles with a special role; the near pairs stay out of them."""
    rng = np.random.default_rng(n)
    full = 4000
    i = np.arange(full)
    pos = np.stack([4.0 + 3.0 * (i % 64), 4.0 + 3.0 * (i // 64)], axis=1) + rng.uniform(-0.4, 0.4, (full, 2))
    pos = pos.astype(F32)
    rad = np.full(full, 0.5, F32)
    uids = (rng.permutation(full).astype(np.uint64) * 7919 + 11).astype(U32)     # distinct, far above n, unordered
    s = full - 60                                                                  # the first special slot
    u = lambda slot: uids[slot]
    parts = []
    # near pairs: right and lower neighbours on the lattice, some breakable (about one in ten breaks at once)
    a = rng.integers(0, s - 65, 2700)
    a = a[(a % 64) != 63]
    b = np.where(rng.random(len(a)) < 0.5, a + 1, a + 64)
    near = M.pairs(u(a), u(b), rng.uniform(2.0, 4.0, len(a)).astype(F32), rng.uniform(0.0, 1.0, len(a)).astype(F32))
    near["max_length"] = np.where(rng.random(len(a)) < 0.3, rng.uniform(2.6, 4.5, len(a)), 0.0).astype(F32)
    near["stiffness"][:20] = (0.0, 1.0) * 10
    parts.append(near)
    parts.append(M.pairs(u(np.arange(100, 160)), u(np.arange(101, 161)), 2.5, 0.5))           # a chain along a row
    hub, spokes = s + 0, rng.choice(s, 200, replace=False)
    hub_bonds = M.pairs(u(np.full(200, hub)), u(spokes), 30.0, 0.01)
    hub_bonds["uid_a"][::2], hub_bonds["uid_b"][::2] = hub_bonds["uid_b"][::2].copy(), hub_bonds["uid_a"][::2].copy()
    parts.append(hub_bonds)                                                        # degree 200: the hub on either side
    parts.append(M.pairs([u(s + 1)], [u(5)], 1.0, 1.0))                             # a leaf: s + 1 has this bond only
    parts.append(np.repeat(M.pairs([u(s + 2)], [u(s + 3)], 1.0, 0.75), 2))          # the same bond twice
    parts.append(M.pairs([u(7), 0xFFFFFFF0, 3], [0xFFFFFFF0, u(8), 5], 1.0, 1.0, 0.001))   # uids no particle has
    anchored = rng.choice(s, 50, replace=False)
    parts.append(M.anchors(u(anchored), pos[anchored] + rng.uniform(-2, 2, (50, 2)).astype(F32), rng.uniform(0, 1, 50),
                           rng.uniform(0, 1, 50)))
    pos[s + 5] = pos[s + 4]                                                        # coincident centres
    parts.append(M.pairs([u(s + 4)], [u(s + 5)], 1.0, 1.0, 0.5))
    parts.append(M.anchors([u(s + 4)], [pos[s + 4]], 1.0, 1.0, 0.5))                # and an anchor on its particle
    odd = [(NAN, 100.0), (100.0, NAN), (INF, 100.0), (-INF, -INF), (1e30, 100.0), (-3e38, 3e38)]
    for j, p in enumerate(odd):
        pos[s + 6 + j] = p
    parts.append(M.pairs(u(np.arange(s + 6, s + 12)), u(np.arange(20, 26)), 1.0, 1.0, 2.0))  # left alone, not broken
    parts.append(M.anchors(u(np.arange(s + 6, s + 12)), np.full((6, 2), 50.0, F32), 1.0, 1.0, 2.0))
    # breaks in the first relaxation: 10 apart, max_length 4
    pos[s + 12], pos[s + 13] = (150.0, 190.0), (160.0, 190.0)
    parts.append(M.pairs([u(s + 12)], [u(s + 13)], 1.0, 1.0, 4.0))
    # breaks in the third: P is drawn towards an anchor 16 away by a quarter of the rest per relaxation (0, 4, 7, 9.25),
    # Q, 2 behind it, holds it by a bond of stiffness 0 and max_length 8: 2, 6, 9 > 8
    pos[s + 14], pos[s + 15] = (100.0, 195.0), (98.0, 195.0)
    parts.append(M.anchors([u(s + 14)], [(116.0, 195.0)], 0.0, 0.25))
    parts.append(M.pairs([u(s + 15)], [u(s + 14)], 2.0, 0.0, 8.0))
    # pulled across the world's edge: the clamp is seen
    pos[s + 16], pos[s + 17] = (2.0, 150.0), (198.0, 198.5)
    parts.append(M.anchors([u(s + 16), u(s + 17)], [(-20.0, 150.0), (230.0, 260.0)], 0.0, 1.0))
    parts.append(M.pairs([u(full - 1)], [u(9)], 3.0, 0.5))                          # (absent when n = 3999)
    bonds = np.concatenate(parts)
    third = len(bonds) - 4                                                         # the bond that breaks in the third
    return pos[:n], rad[:n], uids[:n], bonds, third


def _check_passes(gpe, st, pos, prev, rad, uids, bonds, iterations, passes, k_resolves=1):
    broken = np.zeros(len(bonds), bool)
    want = pos
    for p in range(passes):
        want, broken = M.apply(want, rad, uids, bonds, broken, iterations, WORLD)
        st.apply_bonds()
        got, got_prev, got_rad = _arrays(st)
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (p, bad[:5], pos[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert same_bits(got_prev, prev) and same_bits(got_rad, rad)
        rec, got_broken = st.bonds()
        assert np.array_equal(got_broken, broken), (p, np.nonzero(got_broken != broken)[0][:10])
        assert st.bonds_info() == dict(iterations=iterations, k=len(bonds), nodes=M.node_count(bonds), passes=p + 1,
                                       live=len(bonds) - int(broken.sum()), broken=int(broken.sum()), resolves=k_resolves)
    return want, broken


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("n", [4000, 3999])
def test_one_pass_equals_the_model(gpe, n, iterations, mode):
    """apply_bonds() alone, three passes: pos bit for bit as the model, prev and radius untouched, the broken flags and
    the counters the model's."""
    pos, rad, uids, bonds, third = _pass_scene(n)
    assert 2800 < len(bonds) < 3200
    prev = (pos + F32(0.125)).astype(F32)
    st = _state(gpe, pos, rad, prev=prev, mode=mode)
    st.set_uids(uids)
    st.set_bonds(_rows(gpe, bonds), iterations)
    rec, broken = st.bonds()
    assert rec.tobytes() == bonds.tobytes() and not broken.any()
    want, broken = _check_passes(gpe, st, pos, prev, rad, uids, bonds, iterations, 1)
    first = broken.copy()
    assert 50 < first.sum() < 1500 and first[third - 2] and first[third] == (iterations == 4)
    moved = (bits(want) != bits(pos)).any(axis=1)
    assert 1000 < moved.sum() < n - 20                                 # both outcomes
    assert tuple(want[3956]) == (0.5, 150.0) and tuple(want[3957]) == (199.5, 199.5)      # across the edge: clamped
    # two more passes start from the first one's result; with one relaxation per pass the third bond breaks in pass 3
    broken2 = first
    for p in (1, 2):
        want, broken2 = M.apply(want, rad, uids, bonds, broken2, iterations, WORLD)
        st.apply_bonds()
        assert same_bits(st.positions(), want), p
        assert np.array_equal(st.bonds()[1], broken2), p
        assert broken2[third] == (iterations == 4 or p == 2)
    info = st.bonds_info()
    assert (info["passes"], info["broken"], info["resolves"]) == (3, int(broken2.sum()), 1)
    assert same_bits(st.previous_positions(), prev) and same_bits(st.radii(), rad)
    tags = _end(st)
    assert BOND_TAGS | {"uid.bond_max_length", "uid.bond_anchors"} <= tags


@pytest.mark.parametrize("mode", ["native", "compat"])
@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("n", [2, 1])
def test_one_pass_on_one_and_two_particles(gpe, n, iterations, mode):
    pos = np.array([[10.0, 10.0], [13.0, 14.0]], F32)[:n]
    rad = np.array([0.5, 0.75], F32)[:n]
    uids = np.array([40, 7], U32)[:n]
    bonds = np.concatenate([M.pairs([40], [7], 3.0, 0.5), M.anchors([40], [(2.0, 10.0)], 1.0, 0.25),
                            M.pairs([7, 40], [99, 98], 1.0, 1.0, 0.01), M.anchors([7], [(500.0, 14.0)], 0.0, 1.0)])
    st = _state(gpe, pos, rad, prev=pos + F32(1), mode=mode)
    st.set_uids(uids)
    st.set_bonds(_rows(gpe, bonds), iterations)
    want, broken = _check_passes(gpe, st, pos, (pos + F32(1)).astype(F32), rad, uids, bonds, iterations, 2)
    assert not broken.any() and not same_bits(want, pos)
    if n == 2:
        assert want[1, 0] == 200.0 - 0.75                              # drawn to the anchor outside, clamped by its radius
    _end(st)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_the_tails_of_both_phases(gpe, k):
    """k bonds on 4000 particles: fewer than a wave, one wave exactly, one more, a block and one more"""
    pos, rad, uids, bonds, _ = _pass_scene(4000)
    bonds = bonds[np.random.default_rng(k).permutation(len(bonds))[:k]]
    st = _state(gpe, pos, rad, prev=pos)
    st.set_uids(uids)
    st.set_bonds(_rows(gpe, bonds), 2)
    want, _ = _check_passes(gpe, st, pos, pos, rad, uids, bonds, 2, 1)
    assert not same_bits(want, pos)
    _end(st)


# ---- 2. the hook: a cloth above a floor -----------------------------------------------------------------------------
CLOTH, CLOTH_REST = 24, 1.25
CLOTH_WORLD, CLOTH_GRAVITY = (60.0, 60.0), (0.0, 100.0)
CLOTH_COLLIDERS = np.array([[-5, 45, 65, 45, 5], [30, 28, 30, 28, 4]], F32)    # a floor and a disc in the cloth's way
CLOTH_ITERATIONS = 4
STEPS = 60


def cloth_scene():
    """a 24 x 24 sheet hanging from its two upper corners; uid = row * 24 + column"""
    j, i = np.meshgrid(np.arange(CLOTH), np.arange(CLOTH))
    pos = np.stack([15.0 + CLOTH_REST * j.ravel(), 5.0 + CLOTH_REST * i.ravel()], axis=1).astype(F32)
    uid = (i * CLOTH + j)
    right = M.pairs(uid[:, :-1].ravel(), uid[:, 1:].ravel(), CLOTH_REST, 0.25, 6.0)
    down = M.pairs(uid[:-1, :].ravel(), uid[1:, :].ravel(), CLOTH_REST, 0.25, 6.0)
    pins = M.anchors([0, CLOTH - 1], pos[[0, CLOTH - 1]], 0.0, 1.0)
    return pos, np.full(CLOTH * CLOTH, 0.5, F32), np.concatenate([pins, right, down])


def cloth_twin(oracle, bonds=True, colliders=True):
    pos, rad, b = cloth_scene()
    tw = M.Twin(oracle, pos, rad, world=CLOTH_WORLD, gravity=CLOTH_GRAVITY)
    tw.enable_uids()
    if bonds:
        tw.set_bonds(b, CLOTH_ITERATIONS)
    if colliders:
        tw.set_colliders(CLOTH_COLLIDERS)
    return tw


def cloth_state(gpe, mode="native", bonds=True, colliders=True, **kw):
    pos, rad, b = cloth_scene()
    st = _state(gpe, pos, rad, world=CLOTH_WORLD, gravity=CLOTH_GRAVITY, mode=mode, **kw)
    if bonds:
        st.set_bonds(_rows(gpe, b), CLOTH_ITERATIONS)
    if colliders:
        st.set_colliders(CLOTH_COLLIDERS)
    return st


def _frames(tw, steps, resort_every=0, resort_first=False):
    frames = []
    for s in range(steps):
        resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
        tw.step(DT, resort=bool(resort))
        pos, prev, _ = tw.arrays()
        frames.append((pos.copy(), prev.copy(), tw.uids.copy(), tw.broken.copy()))
    return frames


@pytest.fixture(scope="module")
def cloth(oracle):
    """the reference of the hook tests: oracle step -> model bonds -> model colliders, 60 steps, no re-sort"""
    tw = cloth_twin(oracle)
    frames = _frames(tw, STEPS)
    info, pushed = tw.bonds_info(), tw.pushed
    tw.close()
    assert pushed > 0 and np.isfinite(frames[-1][0]).all()
    return frames, info, pushed


@pytest.fixture(scope="module")
def cloth_resorted(oracle):
    tw = cloth_twin(oracle)
    frames = _frames(tw, STEPS, resort_every=16, resort_first=True)
    info = tw.bonds_info()
    tw.close()
    return frames, info


@pytest.fixture(scope="module")
def cloth_plain(oracle):
    """the same particles with neither bonds nor colliders: the oracle alone"""
    tw = cloth_twin(oracle, bonds=False, colliders=False)
    frames = _frames(tw, 20)
    tw.close()
    return frames


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_every_step_equals_the_twin(gpe, cloth, mode):
    frames, info, pushed = cloth
    L = gpe._lib
    st = cloth_state(gpe, mode)
    for s in range(STEPS):
        st.update(DT)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, frames[s][0]) and same_bits(prev, frames[s][1]), s
    assert np.array_equal(st.bonds()[1], frames[-1][3])
    assert _info(st) == info and st.bonds_info()["resolves"] == 1 and st.colliders_info()["pushed"] == pushed
    assert pos[:, 1].max() > 30.0 and abs(pos[0] - np.array([15.0, 5.0])).max() < 1.0     # it hangs from its pins
    pipe = st.ctx.pipeline_info()
    if mode == "native":
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == STEPS
    else:
        assert pipe["compat_steps"] == STEPS
    _end(st)


@pytest.mark.parametrize("mode", ["native", "compat"])
def test_one_run_equals_the_twin_and_the_observers_see_the_result(gpe, cloth, mode):
    frames, info, pushed = cloth
    st = cloth_state(gpe, mode)
    uids = np.array([0, 23, 300, 575, 12], U32)
    st.tracers_begin(uids, every=1, frames=64, prev=True)
    st.monitor_begin(every=1, frames=64)
    st.run(DT, STEPS, resort_every=0, resort_first=False)
    pos, prev, _ = _arrays(st)
    assert same_bits(pos, frames[-1][0]) and same_bits(prev, frames[-1][1])
    assert _info(st) == info and st.colliders_info()["pushed"] == pushed
    tr = st.tracers_read()
    rec, recorded = st.monitor_read()
    assert len(tr.step) == STEPS and recorded == STEPS
    for s in range(STEPS):                                             # frames taken behind the bonds and the colliders
        p, q = frames[s][0], frames[s][1]
        assert same_bits(tr.pos[s], p[uids]) and same_bits(tr.prev[s], q[uids]), s
        assert rec["max_y"][s] == p[:, 1].max() and rec["min_y"][s] == p[:, 1].min() and rec["n"][s] == CLOTH * CLOTH
    st.tracers_end(); st.monitor_end()
    _end(st)


# ---- 3. re-sorts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_resorts_keep_the_bonds_on_their_particles(gpe, cloth_resorted, mode):
    frames, info = cloth_resorted

    def by_uid(st, s):
        a, b = np.argsort(st.uids()), np.argsort(frames[s][2])
        pos, prev, _ = _arrays(st)
        assert same_bits(pos[a], frames[s][0][b]) and same_bits(prev[a], frames[s][1][b]), s

    st = cloth_state(gpe, mode)
    st.run(DT, STEPS, resort_every=16, resort_first=True)
    by_uid(st, STEPS - 1)
    assert not np.array_equal(st.uids(), np.arange(CLOTH * CLOTH))     # the re-sorts did move the particles
    assert _info(st) == info and st.bonds_info()["resolves"] == 4      # before steps 0, 16, 32, 48
    assert np.array_equal(st.bonds()[1], frames[-1][3])
    _end(st)
    # step by step: the uids are looked up again only on the steps after a re-sort
    st = cloth_state(gpe, mode)
    for s in range(40):
        st.update(DT, resort=(s % 16 == 0))
        assert st.bonds_info()["resolves"] == 1 + s // 16, s
        if s in (0, 15, 16, 17, 39):
            by_uid(st, s)
    _end(st)


# ---- 4. the kept block table ----------------------------------------------------------------------------------------
def test_the_kept_block_table_survives_positions_moved_behind_its_back(gpe, oracle):
    """220 x 220 (625 blocks: two radix passes): most native steps reuse the kept table, with the bonds and the colliders
    moving particles behind it.  Every step as the twin, by gpe_step and by gpe_run."""
    L = gpe._lib
    world, gravity, n, steps = (220.0, 220.0), (0.0, 40.0), 4000, 40
    rng = np.random.default_rng(8)
    pos = np.stack([rng.uniform(1, 219, n), rng.uniform(1, 150, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    # 20 ropes of 20 particles (the first 400), each hung from an anchor at its head
    rope = np.arange(400).reshape(20, 20)
    pos[:400] = np.stack([10.0 + 10.0 * (rope // 20), 5.0 + 1.25 * (rope % 20)], axis=-1).reshape(-1, 2)
    bonds = np.concatenate([M.anchors(rope[:, 0], pos[rope[:, 0]], 0.0, 1.0),
                            M.pairs(rope[:, :-1].ravel(), rope[:, 1:].ravel(), 1.25, 0.5, 10.0)])
    pegs = [[20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 20.0 * i + 10.0 * (j % 2), 60.0 + 25.0 * j, 3.0]
            for i in range(11) for j in range(4)]
    cs = np.array([[-5, 185, 225, 185, 10], [30, 40, 110, 70, 1], [200, 30, 120, 75, 0]] + pegs, F32)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids(); tw.set_bonds(bonds, 2); tw.set_colliders(cs)
    ctxs = []
    for _ in range(2):
        st = _state(gpe, pos, rad, world=world, gravity=gravity)
        st.set_bonds(_rows(gpe, bonds), 2); st.set_colliders(cs)
        ctxs.append(st)
    st, runner = ctxs
    for s in range(steps):
        st.update(DT, resort=(s == 0)); tw.step(DT, resort=(s == 0))
        _same_as_twin(st, tw, s)
    runner.run(DT, steps, resort_every=0, resort_first=True)
    _same_as_twin(runner, tw, "gpe_run")
    for ctx in (st, runner):
        pipe = ctx.ctx.pipeline_info()
        print("native sorts in %d steps: %d" % (steps, pipe["native_sorts"]))
        assert pipe["pipeline"] == L.PIPELINE_NATIVE and pipe["native_steps"] == steps and pipe["sort_passes"] >= 2
        assert pipe["native_sorts"] < steps, "every step sorted: the kept table was never used"
        assert ctx.bonds_info()["resolves"] == 1
        _end(ctx)
    tw.close()


# ---- 5. no bonds, no trace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_without_bonds_nothing_changes_and_nothing_is_launched(gpe, cloth, cloth_plain, mode):
    never = cloth_state(gpe, mode, bonds=False, colliders=False, uids=False, profiling=True)
    cleared = cloth_state(gpe, mode, colliders=False, profiling=True)
    cleared.clear_bonds()
    empty = dict(iterations=0, k=0, nodes=0, passes=0, live=0, broken=0, resolves=0)
    for st in (never, cleared):
        rec, broken = st.bonds()
        assert len(rec) == 0 and len(broken) == 0 and st.bonds_info() == empty
        st.ctx.reset_timings()
        st.apply_bonds()                                               # GPE_OK, nothing done
        for s in range(10):
            st.update(DT)
        st.run(DT, 10, resort_every=0, resort_first=False)
        pos, prev, _ = _arrays(st)
        assert same_bits(pos, cloth_plain[19][0]) and same_bits(prev, cloth_plain[19][1])
        assert not any(name == "Bonds" or name.startswith("bonds/") for name in st.ctx.timings())
        assert not any(t.startswith("uid.bond_") for t, _, _, state in st.ctx.guard_registry() if state == "live")
        _end(st)
    armed = cloth_state(gpe, mode, profiling=True)
    armed.run(DT, 20, resort_every=0, resort_first=False)
    assert same_bits(armed.positions(), cloth[0][19][0])
    t = armed.ctx.timings()
    assert t["Bonds"][1] == 20 and t["bonds/bond"][1] == t["bonds/node"][1] == 20 * CLOTH_ITERATIONS
    assert t["bonds/resolve"][1] == 1
    _end(armed)


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_the_set_and_the_broken_flags_survive_everything_but_set_bonds(gpe, oracle, mode):
    L = gpe._lib
    st = cloth_state(gpe, mode)
    tw = cloth_twin(oracle)
    rng = np.random.default_rng(21)

    def steps(what, k=3, by_uid=False):
        for _ in range(k):
            st.update(DT); tw.step(DT)
        _same_as_twin(st, tw, what, by_uid=by_uid)

    steps("start", 6)
    # tear it: a kick of 20 per step, which no bond of max_length 6 between a kicked particle and its neighbour survives
    band = circle_mask(tw.arrays()[0], 22.0, 18.0, 3.0)
    assert st.kick_circle((22.0, 18.0), 3.0, L.VEL_ADD, (0.0, 20.0)) == tw.kick(band, L.VEL_ADD, 0.0, 20.0) > 0
    steps("kick", 4)
    assert tw.broken.any()
    torn = int(tw.broken.sum())
    add = rng.uniform(2, 12, (100, 2)).astype(F32)
    st.add_particles(add, np.full(100, 0.5, F32)); tw.add(add, np.full(100, 0.5, F32))
    steps("add")
    cand = rng.uniform(1, 59, (60, 2)).astype(F32)
    added, _ = st.add_particles_free(cand, np.full(60, 0.5, F32))
    assert added == tw.add_free(cand, np.full(60, 0.5, F32))[1] > 0
    steps("add_particles_free")
    # removals: a corner by circle (its bonds go inert), two particles by mask, three by uid
    assert st.remove_particles_in_circle((15.0 + 23 * 1.25, 5.0), 1.0) == tw.remove_circle(15.0 + 23 * 1.25, 5.0, 1.0) > 0
    steps("remove circle")
    mask = np.zeros(len(tw), np.uint8); mask[[3, 200]] = 1
    gone = tw.uids[[3, 200]].copy()
    assert st.remove_particles(mask) == tw.remove_mask(mask) == 2
    steps("remove mask")
    assert st.remove_particles_by_uid([100, 101, 4000000]) == tw.remove_uids([100, 101, 4000000]) == 2
    steps("remove uid")
    assert int(tw.broken.sum()) >= torn                                # a removed end breaks nothing, it only silences
    who = np.arange(0, 60, 2, dtype=U32)
    where = (tw.arrays()[0][who] + F32(0.25)).astype(F32)
    st.edit_particles(indices=who, positions=where); tw.edit(who, "index", pos=where)
    steps("edit by index")
    keys = np.array([300, 301, 100, 350], U32)                         # (100 is gone: skipped)
    where = (tw.arrays()[0][M.slots_of(tw.uids, keys[[0, 1, 3]])] + F32(0.5)).astype(F32)
    where = np.stack([where[0], where[1], where[1], where[2]])
    assert st.edit_particles(uids=keys, positions=where) == tw.edit(keys, "uid", pos=where) == 3
    steps("edit by uid")
    st.particles.sort_by_cell_id(); tw.morton_resort()
    steps("morton_resort")
    resolves = st.bonds_info()["resolves"]
    steps("quiet steps")
    assert st.bonds_info()["resolves"] == resolves                     # nothing moved the particles: no new lookup
    grow = np.stack([rng.uniform(2, 58, 1500), rng.uniform(51, 59, 1500)], axis=1).astype(F32)   # past the capacity again
    st.add_particles(grow, np.full(1500, 0.2, F32)); tw.add(grow, np.full(1500, 0.2, F32))
    steps("growth", 2)
    st.ctx.call("gpe_reserve", 20000)
    steps("reserve", 1)
    other = L.MODE_NATIVE if mode == "compat" else L.MODE_COMPAT
    st.ctx.call("gpe_set_mode", other); tw.set_mode(other)
    steps("set_mode", 2)
    # the removed uids come back on two other particles, put next to the old ones' right neighbours: their bonds act again
    u = tw.uids.copy()
    assert not np.isin(gone, u).any() and np.isin(gone + 1, u).all()
    last = np.array([len(u) - 1, len(u) - 2], U32)
    where = (tw.arrays()[0][M.slots_of(u, gone + 1)] + np.array([-1.0, 0.3], F32)).astype(F32)
    st.edit_particles(indices=last, positions=where); tw.edit(last, "index", pos=where)
    u[last] = gone
    before = tw.arrays()[0].copy()
    st.set_uids(u); tw.set_uids(u)
    st.apply_bonds(); tw.apply_bonds()
    _same_as_twin(st, tw, "set_uids")
    moved = (bits(tw.arrays()[0]) != bits(before)).any(axis=1)
    assert moved[len(u) - 1] or moved[len(u) - 2]
    # gpe_set_particles renumbers the uids from 0: the bonds name the new particles
    pos, rad, _ = cloth_scene()
    pos = (pos + F32(3.0)).astype(F32)
    f = C.POINTER(C.c_float)
    st.ctx.call("gpe_set_particles", pos.ctypes.data_as(f), pos.ctypes.data_as(f), rad.ctypes.data_as(f), len(rad))
    tw.set_particles(pos, pos, rad)
    steps("set_particles")
    assert int(tw.broken.sum()) >= torn                                # the flags are the set's, not the particles'
    # a new set clears the flags and the counters
    st.set_bonds(_rows(gpe, tw.bonds), 2); tw.set_bonds(tw.bonds, 2)
    assert st.bonds_info() == dict(iterations=2, k=len(tw.bonds), nodes=CLOTH * CLOTH, passes=0, live=len(tw.bonds),
                                   broken=0, resolves=0)
    steps("new set")
    tw.close()
    _end(st)


# ---- 7. save / load -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_save_and_load_continue_on_the_same_bits(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    st = cloth_state(gpe, mode)
    tw = cloth_twin(oracle)
    for s in range(8):
        st.update(DT); tw.step(DT)
    band = circle_mask(tw.arrays()[0], 22.0, 18.0, 3.0)
    assert st.kick_circle((22.0, 18.0), 3.0, L.VEL_ADD, (0.0, 20.0)) == tw.kick(band, L.VEL_ADD, 0.0, 20.0) > 0
    st.run(DT, 10, resort_every=4, resort_first=True); tw.run(DT, 10, resort_every=4, resort_first=True)
    _same_as_twin(st, tw, "before save")
    assert tw.broken.any() and not tw.broken.all()
    path = str(tmp_path / "snap.npz")
    st.save(path)
    with np.load(path) as d:
        assert d["bonds"].tobytes() == tw.bonds.tobytes() and int(d["bond_iterations"][0]) == CLOTH_ITERATIONS
        assert np.array_equal(d["bonds_broken"], tw.broken)
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    rec, broken = back.bonds()
    assert rec.tobytes() == tw.bonds.tobytes() and np.array_equal(broken, tw.broken)
    assert back.bonds_info() == dict(iterations=CLOTH_ITERATIONS, k=len(rec), nodes=CLOTH * CLOTH, passes=0,
                                     live=len(rec) - int(broken.sum()), broken=int(broken.sum()), resolves=0)
    passes = tw.bond_passes
    tw.run(DT, 12, resort_every=5, resort_first=False)
    for s in (st, back):
        s.run(DT, 12, resort_every=5, resort_first=False)
        tw.bond_passes = passes + 12 if s is st else 12
        _same_as_twin(s, tw, "after load")
    _end(back)
    # a context without bonds writes none and loads none
    st.clear_bonds()
    st.save(path)
    with np.load(path) as d:
        assert "bonds" not in d.files and "bonds_broken" not in d.files
    back = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
    assert len(back.bonds()[0]) == 0
    _end(back)
    _end(st)
    tw.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_and_the_context_untouched(gpe, oracle):
    L = gpe._lib
    lib = L.load()
    st = cloth_state(gpe)
    tw = cloth_twin(oracle)
    for _ in range(5):
        st.update(DT); tw.step(DT)
    before = _arrays(st)
    info = st.bonds_info()
    held = st.bonds()

    def untouched(what):
        rec, broken = st.bonds()
        assert rec.tobytes() == held[0].tobytes() and np.array_equal(broken, held[1]), what
        assert st.bonds_info() == info, what
        assert all(same_bits(a, b) for a, b in zip(_arrays(st), before)), what

    def rows(*bs):
        out = (L.GpeBond * len(bs))()
        for o, b in zip(out, bs):
            o.uid_a, o.uid_b, o.rest_length, o.stiffness, o.max_length, o.flags, o.anchor_x, o.anchor_y = b
        return out

    ok = (1, 2, 1.0, 0.5, 3.0, 0, 0.0, 0.0)
    pin = (1, ABSENT, 1.0, 0.5, 3.0, L.BOND_ANCHOR, 4.0, 5.0)
    h = st.ctx.h
    k = C.c_uint64()
    binfo = L.GpeBondsInfo(struct_size=C.sizeof(L.GpeBondsInfo))
    assert lib.gpe_set_bonds(None, rows(ok), 1, 1) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bonds(None, None, None, 0, C.byref(k)) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_apply_bonds(None) == L.GPE_ERR_INVALID_ARG
    assert lib.gpe_get_bonds_info(None, C.byref(binfo)) == L.GPE_ERR_INVALID_ARG
    untouched("NULL ctx")

    def one(**change):
        names = ["uid_a", "uid_b", "rest_length", "stiffness", "max_length", "flags", "anchor_x", "anchor_y"]
        base = list(pin if change.pop("anchor", False) else ok)
        for name, v in change.items():
            base[names.index(name)] = v
        return lambda: lib.gpe_set_bonds(h, rows(ok, tuple(base)), 2, 1)

    hub = rows(*[(0, j + 1, 1.0, 0.5, 0.0, 0, 0.0, 0.0) for j in range(L.BOND_MAX_DEGREE + 1)])
    bad = {
        "NULL bonds with k > 0": lambda: lib.gpe_set_bonds(h, None, 2, 1),
        "k > GPE_BONDS_MAX": lambda: lib.gpe_set_bonds(h, rows(ok), L.BONDS_MAX + 1, 1),
        "iterations 0": lambda: lib.gpe_set_bonds(h, rows(ok), 1, 0),
        "iterations 33": lambda: lib.gpe_set_bonds(h, rows(ok), 1, L.BOND_ITER_MAX + 1),
        "NaN rest": one(rest_length=NAN), "inf rest": one(rest_length=INF), "negative rest": one(rest_length=-1.0),
        "NaN max": one(max_length=NAN), "inf max": one(max_length=INF), "negative max": one(max_length=-0.5),
        "NaN stiffness": one(stiffness=NAN), "stiffness > 1": one(stiffness=1.5), "stiffness < 0": one(stiffness=-0.25),
        "unknown flag": one(flags=4), "unknown flag on an anchor": one(anchor=True, flags=L.BOND_ANCHOR | 8),
        "uid_a absent": one(uid_a=ABSENT), "uid_a == uid_b": one(uid_b=1),
        "anchor with a uid_b": one(anchor=True, uid_b=2), "pair without a uid_b": one(uid_b=ABSENT),
        "NaN anchor x": one(anchor=True, anchor_x=NAN), "inf anchor y": one(anchor=True, anchor_y=-INF),
        "degree 1025": lambda: lib.gpe_set_bonds(h, hub, L.BOND_MAX_DEGREE + 1, 1),
        "info struct_size": lambda: lib.gpe_get_bonds_info(h, C.byref(L.GpeBondsInfo(struct_size=C.sizeof(L.GpeBondsInfo) - 8))),
        "info NULL": lambda: lib.gpe_get_bonds_info(h, None),
        "get NULL k": lambda: lib.gpe_get_bonds(h, None, None, 0, None),
    }
    for what, call in bad.items():
        assert call() == L.GPE_ERR_INVALID_ARG, what
        assert b"gpe_" in lib.gpe_last_error(h), what                  # the message names the call
        untouched(what)
    assert (L.BONDS_MAX, L.BOND_MAX_DEGREE, L.BOND_ITER_MAX) == (4194304, 1024, 32)
    # while the set is held: the uids stay on, and the context cannot be sharded
    pos, rad, _ = cloth_scene()
    keys = np.arange(len(rad), dtype=U32)
    holding = {
        "gpe_enable_uids": lambda: lib.gpe_enable_uids(h, 0),
        "gpe_use_order_keys": lambda: lib.gpe_use_order_keys(h, 1),
        "gpe_set_counts": lambda: lib.gpe_set_counts(h, len(rad), len(rad) - 10),
        "gpe_shard_set_particles": lambda: lib.gpe_shard_set_particles(
            h, pos.ctypes.data_as(C.c_void_p), None, rad.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), len(rad), 0),
    }
    for what, call in holding.items():
        assert call() == L.GPE_ERR_UNSUPPORTED, what
        assert b"bonds" in lib.gpe_last_error(h) and what.encode() in lib.gpe_last_error(h), what
        untouched(what)
    assert lib.gpe_use_order_keys(h, 0) == L.GPE_OK and lib.gpe_enable_uids(h, 1) == L.GPE_OK     # no change: allowed
    untouched("allowed calls")
    # a partial read delivers the first rows; each output may be NULL
    out, flags = rows(ok, ok, ok), (C.c_uint8 * 3)(9, 9, 9)
    assert lib.gpe_get_bonds(h, out, flags, 2, C.byref(k)) == L.GPE_OK and k.value == len(held[0])
    assert (out[0].uid_a, out[0].flags, out[1].uid_a, out[2].uid_a) == (0, L.BOND_ANCHOR, CLOTH - 1, 1)
    assert list(flags) == [0, 0, 9]
    assert lib.gpe_get_bonds(h, None, flags, 3, C.byref(k)) == L.GPE_OK and list(flags) == [0, 0, 0]
    assert lib.gpe_get_bonds(h, out, None, 3, C.byref(k)) == L.GPE_OK and out[2].uid_a == 0 and out[2].uid_b == 1
    # the context goes on as the twin does
    for _ in range(5):
        st.update(DT); tw.step(DT)
    _same_as_twin(st, tw, "after the refusals")
    # -0.0 is accepted and stored as +0; the degree cap itself is accepted; duplicates are
    z = rows((1, 2, -0.0, 0.5, -0.0, 0, 0.0, 0.0), ok, ok)
    assert lib.gpe_set_bonds(h, z, 3, L.BOND_ITER_MAX) == L.GPE_OK
    rec, _ = st.bonds()
    assert bits(rec["rest_length"][:1]).tolist() == [0] and bits(rec["max_length"][:1]).tolist() == [0]
    assert lib.gpe_set_bonds(h, hub, L.BOND_MAX_DEGREE, 1) == L.GPE_OK
    assert st.bonds_info()["nodes"] == L.BOND_MAX_DEGREE + 1
    st.update(DT)
    # without uids: GPE_ERR_STATE, and nothing is held
    st.clear_bonds()
    st.enable_uids(False)
    assert lib.gpe_set_bonds(h, rows(ok), 1, 1) == L.GPE_ERR_STATE and b"gpe_set_bonds" in lib.gpe_last_error(h)
    assert st.bonds_info()["k"] == 0
    assert lib.gpe_set_bonds(h, None, 0, 1) == L.GPE_OK                # clearing nothing needs no uids
    tw.close()
    _end(st)


@pytest.mark.parametrize("how", ["order_keys", "active_cells"])
def test_a_sharded_context_takes_no_bonds(gpe, how):
    L = gpe._lib
    pos, rad, b = cloth_scene()
    st = _state(gpe, pos, rad, world=CLOTH_WORLD, uids=False)
    if how == "order_keys":
        st.ctx.call("gpe_use_order_keys", 1)
    else:
        st.ctx.call("gpe_set_active_cells", 0, 0, 20, 20)
    before = _arrays(st)
    with pytest.raises(gpe.GpeError) as e:
        st.set_bonds(_rows(gpe, b), 1)
    assert e.value.status == L.GPE_ERR_UNSUPPORTED
    assert len(st.bonds()[0]) == 0 and st.bonds_info()["k"] == 0
    st.apply_bonds()
    assert all(same_bits(a, b) for a, b in zip(_arrays(st), before))
    _end(st)


# ---- 9. a seeded random interleaving --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["native", "compat"])
def test_a_random_interleaving_against_the_twin(gpe, oracle, tmp_path, mode):
    L = gpe._lib
    rng = np.random.default_rng(77 if mode == "native" else 78)
    world, gravity = (60.0, 60.0), (0.0, 80.0)
    n = 600
    pos = np.stack([rng.uniform(2, 58, n), rng.uniform(2, 40, n)], axis=1).astype(F32)
    rad = np.full(n, 0.5, F32)
    st = _state(gpe, pos, rad, world=world, gravity=gravity, mode=mode)
    tw = M.Twin(oracle, pos, rad, world=world, gravity=gravity)
    tw.enable_uids()

    def random_set():
        """bonds between particles that are close now, a few anchors, a few uids nobody has"""
        p, uids = tw.arrays()[0], tw.uids
        k = int(rng.integers(20, 300))
        a = rng.integers(0, len(uids), k)
        d2 = ((p[a, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(k), a] = np.inf
        b = np.argmin(d2, axis=1)
        pairs = M.pairs(uids[a], uids[b], rng.uniform(1.0, 2.0, k).astype(F32), rng.uniform(0.1, 0.5, k).astype(F32),
                        np.where(rng.random(k) < 0.5, 4.0, 0.0).astype(F32))
        pins = rng.integers(0, len(uids), 5)
        ghosts = M.pairs(uids[pins], np.arange(5) + 3000000000, 1.0, 0.5)
        return np.concatenate([pairs, M.anchors(uids[pins], p[pins], 0.0, 0.5), ghosts]), int(rng.integers(1, 5))

    def random_colliders():
        return np.array([[-5, 52, 65, 52, 8], [rng.uniform(10, 50), 35, rng.uniform(10, 50), 38, rng.uniform(0, 3)]], F32)

    ops = ["set_bonds", "clear", "step", "run", "add", "remove", "edit", "kick", "resort", "apply", "colliders", "saveload"]
    weights = np.array([4, 1, 6, 5, 2, 3, 2, 2, 2, 2, 2, 2], float)
    log, most_passes, ever_broken = [], 0, 0
    b, it = random_set()
    st.set_bonds(_rows(gpe, b), it); tw.set_bonds(b, it)
    for i in range(40):
        op = str(rng.choice(ops, p=weights / weights.sum()))
        log.append(op)
        if op == "set_bonds":
            b, it = random_set()
            st.set_bonds(_rows(gpe, b), it); tw.set_bonds(b, it)
        elif op == "clear":
            st.clear_bonds(); tw.set_bonds(np.zeros(0, M.BOND_DTYPE), 1)
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
            st.apply_bonds(); tw.apply_bonds()
        elif op == "colliders":
            cs = random_colliders() if rng.integers(0, 3) else np.zeros((0, 5), F32)
            st.set_colliders(cs); tw.set_colliders(cs)
        else:
            path = str(tmp_path / ("s%d.npz" % i))
            st.save(path)
            _end(st)
            st = gpe.State.load(path, mode=_mode(gpe, mode), flags=L.FLAG_GUARD_ALLOCS)
            tw.bond_passes = 0                                         # (load sets the bonds anew, the flags with them)
            tw.passes = tw.pushed = 0
        _same_as_twin(st, tw, (i, log))
        assert same_bits(st.colliders(), tw.colliders), (i, log)
        most_passes = max(most_passes, tw.bond_passes)
        ever_broken = max(ever_broken, int(tw.broken.sum()))
    print(" ".join(log), "| most passes under one set:", most_passes, "| most broken:", ever_broken)
    assert {"set_bonds", "step", "run"} <= set(log) and most_passes > 5
    tw.close()
    _end(st)
