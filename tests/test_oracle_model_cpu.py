"""CPU: the oracle model of a context (tests/_oracle_model.py) that tests/test_gpu_api_sequences.py checks call
sequences against.  Rebuilding its Sim mid-run loses nothing, and its add / removal / max-radius / uid rules are the
ones include/gpe.h states."""
import os
import re

import numpy as np

from _oracle_model import OracleModel, circle_mask, max_abs_radius

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
