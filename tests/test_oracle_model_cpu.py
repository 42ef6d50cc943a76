"""CPU: the oracle model of a context (tests/_oracle_model.py) that tests/test_gpu_api_sequences.py checks call
sequences against.  Rebuilding its Sim mid-run loses nothing, and its add / removal / max-radius / uid rules are the
ones include/gpe.h states; so are its keyed edits, kicks, checked adds and read-only queries."""
import os
import re

import numpy as np

from _oracle_model import OracleModel, VEL_ADD, VEL_SCALE, VEL_SET, circle_mask, max_abs_radius

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpe.h")).read()
DT = 1.0 / 60.0


def _scene(n, seed, world=(120.0, 80.0)):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2), dtype=np.float32) * (np.array(world, np.float32) - 4.0) + 2.0).astype(np.float32)
    rad = rng.choice(np.array([0.5, 0.75, 1.0], np.float32), n)
    return pos, rad, world


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_rebuilt_sims_equal_one_long_lived_sim(oracle):
    """200 steps with re-sorts, gravity and the mouse on: the model, whose Sim is rebuilt from its arrays every few
    steps (the same constants set again), holds the bits of one Sim that runs throughout."""
    pos, rad, world = _scene(3000, seed=1)
    g, mouse = (1.5, -9.81), (60.0, 40.0)
    params = oracle.default_params(world[0], world[1], float(np.abs(rad).max()), gravity=g)
    params.mouse_pressed, params.mouse_x, params.mouse_y = 1, mouse[0], mouse[1]
    ref = oracle.Sim(pos, rad, params)
    model = OracleModel(oracle, pos, rad, world=world, gravity=g)
    model.set_mouse(True, *mouse)
    rebuilt = 0
    for s in range(200):
        resort = s % 16 == 0
        ref.step(DT, resort=resort)
        if s % 7 == 3:
            model.set_gravity(*g)                      # drops the Sim: the next step builds a new one
            rebuilt += 1
        if s % 11 == 5:
            model.run(DT, 1, resort_every=0, resort_first=resort)
        else:
            model.step(DT, resort=resort)
    p, q, r = model.arrays()
    assert rebuilt > 20
    assert np.array_equal(_bits(p), _bits(ref.pos)) and np.array_equal(_bits(q), _bits(ref.prev))
    assert np.array_equal(_bits(r), _bits(ref.radius))
    ref.close(); model.close()


def test_module_calls_equal_a_step(oracle):
    pos, rad, world = _scene(2000, seed=2)
    a = OracleModel(oracle, pos, rad, world=world)
    b = OracleModel(oracle, pos, rad, world=world)
    for _ in range(5):
        a.step(DT)
        b.module_calls(DT)
    assert np.array_equal(_bits(a.arrays()[0]), _bits(b.arrays()[0]))


def test_max_radius_rules_are_the_headers():
    """gpe.h: removal leaves gpe_max_radius as set_particles does -- "largest magnitude, last on ties, sign kept"."""
    text = " ".join(HEADER.split())
    assert "largest magnitude, last on ties, sign kept" in re.sub(r"\s*\*\s*", " ", text)
    assert max_abs_radius([2.0, -2.0]) == np.float32(-2.0)
    assert max_abs_radius([-2.0, 2.0]) == np.float32(2.0)
    assert max_abs_radius([0.5, -3.0, 1.0]) == np.float32(-3.0)
    assert max_abs_radius([0.5]) == np.float32(0.5)


def test_add_and_remove_reset_the_grid_radius(oracle):
    pos, rad, world = _scene(100, seed=3)
    m = OracleModel(oracle, pos, rad, world=world)
    assert m.max_radius == m.grid_max_radius == np.float32(1.0)
    assert _bits(m.cell_size) == _bits(np.float32(1.0) * np.float32(2.2))
    m.grid_set_max_radius(0.4)
    assert m.grid_max_radius == np.float32(0.4) and m.max_radius == np.float32(1.0)
    # add: fmaxf over the new radii, and the grid radius follows the max radius again
    m.add(np.full((3, 2), 10.0, np.float32), np.array([0.5, 2.5, 1.5], np.float32))
    assert len(m) == 103 and m.max_radius == m.grid_max_radius == np.float32(2.5)
    assert np.array_equal(m.prev[-3:], m.pos[-3:])
    m.grid_set_max_radius(3.0)
    # removing nothing leaves everything as it was, the override included
    assert m.remove_mask(np.zeros(103, np.uint8)) == 0 and m.grid_max_radius == np.float32(3.0)
    # removing the largest one: the survivors' largest magnitude
    gone = np.zeros(103, np.uint8); gone[101] = 1
    assert m.remove_mask(gone) == 1
    assert len(m) == 102 and m.max_radius == m.grid_max_radius == np.float32(1.5)
    try:
        m.remove_mask(np.ones(102, np.uint8))
        raise AssertionError("removing every particle must be refused")
    except ValueError:
        pass


def test_circle_is_the_closed_disc_in_binary32():
    # (3, 1e-4): 9 + 1e-8 rounds to 9 in binary32, on the rim; (3, 1e-2) is outside
    pos = np.array([[3.0, 0.0], [0.0, 3.0], [3.0, 1e-4], [3.0, 1e-2], [2.1, 2.1], [0.1, 0.2]], np.float32)
    got = circle_mask(pos, 0.0, 0.0, 3.0)
    assert got.tolist() == [True, True, True, False, True, True]
    # 0.1 is not exact in binary32: the float32 sum decides, not the real-number one
    p = np.array([[np.float32(0.1) + np.float32(0.2), 0.0]], np.float32)
    r = np.float32(0.1) + np.float32(0.2)
    assert circle_mask(p, 0.0, 0.0, r).tolist() == [True]


def test_uid_rules(oracle):
    pos, rad, world = _scene(50, seed=4)
    m = OracleModel(oracle, pos, rad, world=world)
    m.enable_uids()
    assert np.array_equal(m.uids, np.arange(50)) and m.next_uid == 50
    m.enable_uids()                                    # on -> on keeps them
    m.add(np.full((2, 2), 5.0, np.float32), np.full(2, 0.5, np.float32))
    assert m.uids[-2:].tolist() == [50, 51] and m.next_uid == 52
    assert m.remove_uids([0, 51, 51, 9999]) == 2
    assert 0 not in m.uids and 51 not in m.uids and m.next_uid == 52     # never reused
    m.add(np.full((1, 2), 6.0, np.float32), np.full(1, 0.5, np.float32))
    assert m.uids[-1] == 52
    m.set_uids(np.arange(len(m), dtype=np.uint32)[::-1] * 3)
    assert m.next_uid == 3 * (len(m) - 1) + 1
    m.set_next_uid(1000)
    assert m.next_uid == 1000
    m.enable_uids(False)
    assert m.uids is None and m.next_uid is None


def test_uids_follow_the_resort_permutation(oracle):
    pos, rad, world = _scene(2000, seed=5)
    m = OracleModel(oracle, pos, rad, world=world)
    m.enable_uids()
    m.step(DT, resort=True)
    m.morton_resort()
    m.run(DT, 5, resort_every=2, resort_first=True)
    # a twin with uids off runs the same bits; the uids are a permutation that maps each particle back to its origin
    t = OracleModel(oracle, pos, rad, world=world)
    t.step(DT, resort=True); t.morton_resort(); t.run(DT, 5, resort_every=2, resort_first=True)
    assert np.array_equal(_bits(m.arrays()[0]), _bits(t.arrays()[0]))
    assert sorted(m.uids.tolist()) == list(range(2000))
    assert np.array_equal(m.radius, rad[m.uids])


# ---- the interactive calls: gpe_edit_particles, gpe_kick_*, gpe_add_particles_free, the queries ------------------------
def test_an_edited_model_steps_like_a_fresh_sim_of_the_edited_arrays(oracle):
    """gpe.h: an edit leaves "what gpe_set_particles(edited pos, edited prev, edited radius) would leave, as far as a
    step can see".  After steps (a live Sim behind the model), edits of every field subset by index and by uid, the model
    steps bit for bit like an oracle.Sim built from its arrays."""
    pos, rad, world = _scene(2500, seed=6)
    m = OracleModel(oracle, pos, rad, world=world, gravity=(0.0, -9.81))
    m.enable_uids()
    m.run(DT, 6, resort_every=4, resort_first=True)
    rng = np.random.default_rng(7)
    uids_before = m.uids.copy()
    who = rng.choice(2500, 300, replace=False).astype(np.uint32)
    p_new = (rng.random((300, 2), dtype=np.float32) * np.float32(60.0) + np.float32(5.0)).astype(np.float32)
    assert m.edit(who[:100], "index", pos=p_new[:100]) == 100
    p, q, r = m.arrays()
    assert np.array_equal(_bits(p[who[:100]]), _bits(p_new[:100])) and np.array_equal(_bits(q[who[:100]]), _bits(p_new[:100]))
    q_new = (p_new + np.float32(0.03)).astype(np.float32)
    keys = np.concatenate([uids_before[who[100:200]], [99999, 0xFFFFFFFE]]).astype(np.uint32)
    rows_p = np.concatenate([p_new[100:200], np.zeros((2, 2), np.float32)])
    rows_q = np.concatenate([q_new[100:200], np.zeros((2, 2), np.float32)])
    assert m.edit(keys, "uid", pos=rows_p, prev=rows_q) == 100         # the two absent uids are skipped
    r_new = rng.choice(np.array([0.5, 1.25], np.float32), 100)
    assert m.edit(who[200:], "index", radius=r_new, prev=q_new[200:], pos=p_new[200:]) == 100
    p, q, r = m.arrays()
    assert np.array_equal(_bits(p[who[100:200]]), _bits(p_new[100:200])) and np.array_equal(_bits(q[who[100:]]), _bits(q_new[100:]))
    assert np.array_equal(_bits(r[who[200:]]), _bits(r_new))
    assert np.array_equal(m.uids, uids_before)                         # uids and order are kept
    assert m.max_radius == m.grid_max_radius == np.float32(1.25)
    params = oracle.default_params(world[0], world[1], 1.25, gravity=(0.0, -9.81))
    ref = oracle.Sim(p.copy(), r.copy(), params, prev=q.copy())
    for s in range(12):
        m.step(DT, resort=(s == 5)); ref.step(DT, resort=(s == 5))
    p, q, r = m.arrays()
    assert np.array_equal(_bits(p), _bits(ref.pos)) and np.array_equal(_bits(q), _bits(ref.prev))
    assert np.array_equal(_bits(r), _bits(ref.radius))
    ref.close(); m.close()


def test_edit_radius_and_override_bookkeeping(oracle):
    """gpe.h: "radius non-NULL: gpe_max_radius is recomputed ... gpe_grid_max_radius is set to it"; "radius NULL: max
    radius, the grid max radius (a gpe_grid_set_max_radius override included) and the cell size are untouched"; only
    prev: nothing else changes."""
    text = re.sub(r"\s*\*\s*", " ", " ".join(HEADER.split()))
    assert "radius NULL: max radius, the grid max radius (a gpe_grid_set_max_radius override included)" in text
    pos, rad, world = _scene(100, seed=8)
    m = OracleModel(oracle, pos, rad, world=world)
    m.grid_set_max_radius(2.5)
    before = [a.copy() for a in m.arrays()]
    # NULL radius: pos, and prev only, under a pending override
    assert m.edit([3, 4], "index", pos=np.full((2, 2), 9.0, np.float32)) == 2
    assert m.grid_max_radius == np.float32(2.5) and m.max_radius == np.float32(1.0)
    assert m.edit([5], "index", prev=np.full((1, 2), 8.0, np.float32)) == 1
    assert m.grid_max_radius == np.float32(2.5) and m.max_radius == np.float32(1.0)
    p, q, r = m.arrays()
    assert np.array_equal(p[5], before[0][5]) and np.array_equal(r, before[2]) and q[5].tolist() == [8.0, 8.0]
    untouched = np.ones(100, bool); untouched[[3, 4, 5]] = False
    assert np.array_equal(_bits(p[untouched]), _bits(before[0][untouched]))
    assert np.array_equal(_bits(q[untouched]), _bits(before[1][untouched]))
    # non-NULL radius: a new largest radius, the override is gone
    assert m.edit([7], "index", radius=[3.0]) == 1
    assert m.max_radius == m.grid_max_radius == np.float32(3.0) and _bits(m.cell_size) == _bits(np.float32(3.0) * np.float32(2.2))
    # ... the largest shrunk, under an override again: the largest of the rest, and the grid radius follows it
    m.grid_set_max_radius(5.0)
    assert m.edit([7], "index", radius=[0.25]) == 1
    assert m.max_radius == m.grid_max_radius == np.float32(1.0)
    # ... a radius edit that changes no maximum still drops the override
    m.grid_set_max_radius(5.0)
    assert m.edit([7], "index", radius=[0.5]) == 1 and m.grid_max_radius == np.float32(1.0)
    # sign kept, last on ties, as after a removal
    assert m.edit([0, 99], "index", radius=[-4.0, 4.0]) == 2 and m.max_radius == np.float32(4.0)
    assert m.edit([99], "index", radius=[1.0]) == 1 and m.max_radius == np.float32(-4.0)
    # by uid while every key is absent: nothing is written
    m.enable_uids()
    m.grid_set_max_radius(2.0)
    assert m.edit([1000, 1001], "uid", radius=[9.0, 9.0]) == 0
    assert np.array_equal(m.arrays()[2][:3], np.array([-4.0, rad[1], rad[2]], np.float32))
    m.close()


def test_kick_edge_cases(oracle):
    """gpe.h: ADD with a = 0 changes no bit; SET with a = 0 freezes, prev = pos exactly; SCALE with a = 0 gives
    prev = pos - 0 = pos, with a = 1 prev = pos - (pos - prev) (rounded twice), only the masked particles move."""
    pos, rad, world = _scene(500, seed=9)
    rng = np.random.default_rng(10)
    prev = (pos + rng.uniform(-0.1, 0.1, pos.shape).astype(np.float32)).astype(np.float32)
    mask = circle_mask(pos, 60.0, 40.0, 25.0)
    assert 0 < mask.sum() < 500
    for op in (VEL_ADD, VEL_SET, VEL_SCALE):
        m = OracleModel(oracle, pos, rad, world=world, prev=prev)
        assert m.kick(mask, op, 0.0, 0.0) == int(mask.sum())
        p, q, _ = m.arrays()
        assert np.array_equal(_bits(p), _bits(pos))
        assert np.array_equal(_bits(q[~mask]), _bits(prev[~mask]))
        if op == VEL_ADD:
            assert np.array_equal(_bits(q), _bits(prev))
        else:
            assert np.array_equal(_bits(q[mask]), _bits(pos[mask]))    # frozen exactly
        m.close()
    m = OracleModel(oracle, pos, rad, world=world, prev=prev)
    m.kick(mask, VEL_SET, 0.0, 0.0)
    m.step(DT)                                           # no gravity: a frozen particle nobody can reach stays put
    from tests._contacts_model import contacts
    lonely = mask & (contacts(pos, rad + np.float32(1.0))[1] == 0)
    assert lonely.any() and np.array_equal(_bits(m.arrays()[0][lonely]), _bits(pos[lonely]))
    m.close()
    # the float32 formulas, one rounding per operation
    m = OracleModel(oracle, pos, rad, world=world, prev=prev)
    m.kick(mask, VEL_ADD, 0.25, -0.5)
    want = prev.copy(); want[mask, 0] = prev[mask, 0] - np.float32(0.25); want[mask, 1] = prev[mask, 1] - np.float32(-0.5)
    assert np.array_equal(_bits(m.arrays()[1]), _bits(want))
    m.kick(mask, VEL_SCALE, -1.5, 0.3)
    v = (pos - want).astype(np.float32) * np.array([-1.5, 0.3], np.float32)
    want2 = want.copy(); want2[mask] = (pos - v.astype(np.float32))[mask]
    assert np.array_equal(_bits(m.arrays()[1]), _bits(want2))
    m.kick(mask, VEL_SET, 0.125, 2.0)
    want3 = want2.copy(); want3[mask] = (pos - np.array([0.125, 2.0], np.float32))[mask]
    assert np.array_equal(_bits(m.arrays()[1]), _bits(want3))
    m.close()


def test_add_free_equals_add_of_the_accepted_rows(oracle):
    from tests import _spawn_model
    pos, rad, world = _scene(1500, seed=11)
    rng = np.random.default_rng(12)
    cpos, crad = _spawn_model.reference_spray(rng, (60.0, 40.0), 300)
    for separate in (False, True):
        for inside_world in (False, True):
            a = OracleModel(oracle, pos, rad, world=world); a.enable_uids(); a.grid_set_max_radius(2.0)
            b = OracleModel(oracle, pos, rad, world=world); b.enable_uids(); b.grid_set_max_radius(2.0)
            dry, n_dry = a.add_free(cpos, crad, separate=separate, inside_world=inside_world, dry_run=True)
            assert len(a) == 1500 and a.grid_max_radius == np.float32(2.0) and a.next_uid == 1500   # a dry run changes nothing
            verdict, added = a.add_free(cpos, crad, separate=separate, inside_world=inside_world)
            assert np.array_equal(verdict, dry) and added == n_dry == int((verdict == _spawn_model.ADDED).sum()) > 0
            assert (verdict == _spawn_model.BLOCKED_BY_PARTICLE).any()
            assert (verdict == _spawn_model.OUTSIDE_WORLD).any() == inside_world
            keep = verdict == _spawn_model.ADDED
            b.add(cpos[keep], crad[keep])
            assert len(a) == len(b) == 1500 + added and a.next_uid == b.next_uid == 1500 + added
            assert np.array_equal(a.uids, b.uids) and a.max_radius == b.max_radius == a.grid_max_radius
            assert a.max_radius == _spawn_model.max_radius_after(1.0, crad[keep]) and a.max_radius > np.float32(1.0)
            for s in range(4):
                a.step(DT, resort=(s == 0)); b.step(DT, resort=(s == 0))
            for x, y in zip(a.arrays(), b.arrays()):
                assert np.array_equal(_bits(x), _bits(y))
            a.close(); b.close()
    # nothing accepted: untouched, the grid override included
    m = OracleModel(oracle, pos, rad, world=world); m.grid_set_max_radius(2.0)
    verdict, added = m.add_free(pos[:50], rad[:50])
    assert added == 0 and (verdict == _spawn_model.BLOCKED_BY_PARTICLE).all() and len(m) == 1500
    assert m.grid_max_radius == np.float32(2.0)
    m.close()


def test_query_rows_are_the_predicates_rows(oracle):
    from tests._oracle_model import box_mask, pick_oracle
    pos, rad, world = _scene(800, seed=13)
    m = OracleModel(oracle, pos, rad, world=world)
    m.enable_uids()
    m.step(DT, resort=True)
    p, q, r = [a.copy() for a in m.arrays()]
    got = m.query_circle(50.0, 40.0, 15.0)
    want = np.nonzero(circle_mask(p, 50.0, 40.0, 15.0))[0]
    assert len(want) > 3 and np.array_equal(got.index, want) and np.array_equal(got.uid, m.uids[want])
    assert np.array_equal(_bits(got.pos), _bits(p[want])) and np.array_equal(_bits(got.prev), _bits(q[want]))
    assert np.array_equal(_bits(got.radius), _bits(r[want]))
    assert np.array_equal(m.query_box(10.0, 10.0, 30.0, 50.0).index, np.nonzero(box_mask(p, 10.0, 10.0, 30.0, 50.0))[0])
    hit = m.pick(float(p[17, 0]), float(p[17, 1]))
    assert hit.index.tolist() == [pick_oracle(p, r, p[17, 0], p[17, 1])] and m.pick(-50.0, -50.0) is None
    c = m.contacts()
    assert c.count == len(c.a) > 0 and (c.a < c.b).all() and int(c.degree.sum()) == 2 * c.count
    assert np.array_equal(c.uid_a, m.uids[c.a]) and np.array_equal(c.uid_b, m.uids[c.b])
    k = m.clusters()
    assert k.count == int((k.label == np.arange(800)).sum()) and np.array_equal(k.label_uid, m.uids[k.label])
    assert (k.label[c.a] == k.label[c.b]).all() and k.largest_size == int(k.size.max())
    i = int(k.largest_label)
    members = m.cluster_of(index=i)
    assert np.array_equal(members.index, np.nonzero(k.label == k.label[i])[0]) and len(members.index) == k.largest_size
    assert np.array_equal(m.cluster_of(uid=int(m.uids[i])).index, members.index)
    assert len(m.cluster_of(uid=4000).index) == 0
    m.close()
