"""GPU (-m gpu), one process: the sharded run fuzzed against one context, and its refusals.

The scenes are tests/_shard_scenes.py's; tests/test_shard_scenes_cpu.py proves on the oracle that each of them stays
inside the conditions of an exact sharded run (less than a block of motion a step, rectangles two blocks wide, at most 8
neighbours, no empty rank behind a re-cut).  Here every seed runs as a local group of `ws` contexts, as one NATIVE
context and on the oracle, and after every chunk of the schedule the three hold the same bits.

The refusals: each sticky error word of the device-resident exchange and each refusal of the set-up and the re-cut that
the public ABI can reach, on the smallest scene that reaches it.  Every rank's call must come back with an error."""
import importlib

import numpy as np
import pytest

import _shard_scenes as S

pytestmark = pytest.mark.gpu


def _lg():
    return importlib.import_module("gpu-physics-engine_amd.local_group")


@pytest.mark.parametrize("seed", S.SEEDS)
def test_sharded_fuzz_scenes_equal_single_context_and_oracle(gpe, oracle, seed):
    """After every chunk: the ranks' order keys partition 0 .. n-1, pos and prev at those keys are the single context's
    bits, and the single context's are the oracle's (so a failure says which side moved).  At the end every rank counted
    the schedule's steps and re-sorts, ran native steps only, and the pile-up seeds were re-cut."""
    L = gpe._lib
    sc = S.shard_scene(seed)
    n, ws, dt = len(sc["rad"]), sc["ws"], sc["dt"]
    run = _lg().LocalShardedRun(sc["pos"], sc["rad"], sc["world"], ws, gravity=sc["gravity"], prev=sc["prev"], grid=sc["grid"],
                                xcuts=sc["xcuts"], ycuts=sc["ycuts"], mouse=sc["mouse"],
                                flags=L.FLAG_SHARD_OVERLAP if sc["overlap"] else 0)
    ref = gpe.State(sc["pos"], sc["rad"], world=sc["world"], gravity=sc["gravity"], mode=gpe.MODE_NATIVE, prev=sc["prev"])
    if sc["mouse"] is not None:
        ref.particles.mouse_click_callback(True, sc["mouse"])
    sim = S.oracle_sim(sc, oracle)
    steps_done = resorts = 0
    for ci, (steps, every, first) in enumerate(sc["chunks"]):
        what = "seed %d (ws %d, grid %s, n %d), chunk %d" % (seed, ws, sc["grid"], n, ci)
        run.run(dt, steps, resort_every=every, resort_first=first)
        ref.run(dt, steps, resort_every=every, resort_first=first)
        for s in range(steps):
            resort = bool((s == 0 and first) or (every and s > 0 and s % every == 0))
            resorts += resort
            sim.step(dt, resort=resort)
        steps_done += steps
        want_pos, want_prev = ref.positions(), ref.previous_positions()
        assert np.array_equal(want_pos, sim.pos), "single context against the oracle, positions: " + what
        assert np.array_equal(want_prev, sim.prev), "single context against the oracle, previous positions: " + what
        owned = run.owned()                                # ownership read back between the chunks
        keys = np.concatenate([gid for gid, _, _ in owned])
        assert np.array_equal(np.sort(keys), np.arange(n)), "the ranks' order keys do not partition 0 .. n-1: " + what
        for r, (gid, p, q) in enumerate(owned):
            assert np.array_equal(p, want_pos[gid]), "rank %d positions: %s" % (r, what)
            assert np.array_equal(q, want_prev[gid]), "rank %d previous positions: %s" % (r, what)
    stats = run.stats()
    infos = [c.pipeline_info() for c in run.ctx]
    run.close()
    ref.close(); sim.close()
    print("seed %d: re-cuts per rank %s" % (seed, [s["recuts"] for s in stats]))
    for r in range(ws):
        assert stats[r]["transport"] == 2 and stats[r]["steps"] == steps_done and stats[r]["resorts"] == resorts, (r, stats[r])
        assert infos[r]["pipeline"] == L.PIPELINE_NATIVE and infos[r]["compat_steps"] == 0, (r, infos[r])
    if sc["claims"]["pile_up"]:
        assert all(s["recuts"] >= 1 for s in stats), stats


# ---- refusals -------------------------------------------------------------------------------------------------------
def _each_rank(run, fn):
    """fn(rank) on the group's threads (LocalShardedRun._each: the first failure aborts the group, so no rank waits);
    returns what every rank raised (None: it came back without an error)."""
    return _each_rank_of(type(run)._each, run, fn)


def _each_rank_of(each, run, fn):
    raised = [None] * run.ws

    def body(r):
        try:
            return fn(r)
        except BaseException as e:                          # noqa: BLE001 -- recorded, then reported by _each as ever
            raised[r] = e
            raise
    try:
        each(run, body)
    except Exception:                                       # noqa: BLE001 -- the per-rank record is what is asserted
        pass
    return raised


def _run_then_read(run, dt, steps, every, first=True):
    """gpe_shard_run_scheduled, then the read-back that reports a sticky error of the last steps."""
    import ctypes as C

    def go(r):
        c = run.ctx[r]
        c.call("gpe_shard_run_scheduled", float(dt), int(steps), int(every), 1 if first else 0)
        no, nt = C.c_uint64(), C.c_uint64()
        c.call("gpe_shard_counts", C.byref(no), C.byref(nt), 0)
    return _each_rank(run, go)


def _assert_all_failed(gpe, raised, text, status, where=None):
    """Every rank raised a GpeError; the ranks in `where` (default: at least one) carry `text` and `status`, the others
    left their collective because the group was aborted, or report what their own end of the exchange saw."""
    assert all(isinstance(e, gpe.GpeError) for e in raised), raised
    hit = [r for r, e in enumerate(raised) if text in str(e)]
    assert hit and (where is None or set(where) <= set(hit)), (text, [str(e) for e in raised])
    for r, e in enumerate(raised):
        if r in hit:
            assert e.status == status, (r, str(e))
        else:
            assert "aborted" in str(e) or "another rank failed" in str(e) or "sharded exchange failed" in str(e), (r, str(e))


def _flags(e):
    import re
    m = re.search(r"flags 0x([0-9a-f]+)", str(e))
    return int(m.group(1), 16) if m else 0


CELL = float(np.float32(0.5) * np.float32(2.2))             # r = 0.5 everywhere below
EDGE = 8 * CELL                                             # one block in world units
ERR_SEND, ERR_NO_SLOT, ERR_CAPACITY, ERR_HOLES, ERR_RECV = 1, 2, 4, 8, 16      # csrc/gpe_internal.h kShardErr*


def _strips(bx_per_rank, ranks, by, per_block, seed, axis=0):
    """`ranks` strips of `bx_per_rank` blocks each along `axis`, `by` blocks the other way, a uniform r = 0.5 cloud."""
    size = [0.0, 0.0]
    size[axis], size[1 - axis] = (ranks * bx_per_rank * 8 - 0.5) * CELL, (by * 8 - 0.5) * CELL
    n = int(per_block * ranks * bx_per_rank * by)
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2), dtype=np.float32) * np.array(size, np.float32)).astype(np.float32)
    return pos, np.full(n, 0.5, np.float32), tuple(size)


def no_slot_scene():
    """Three strips two blocks wide; five particles of rank 0 carry a `prev` that takes them 2.5 blocks to the right in
    one step: into rank 2's rectangle, which is no neighbour of rank 0."""
    pos, rad, world = _strips(2, 3, 2, 20, seed=3)
    prev = pos.copy()
    pos[:5] = np.array([1.7 * EDGE, 0.5 * EDGE], np.float32) + np.arange(5, dtype=np.float32)[:, None] * np.array([0.0, 1.3], np.float32)
    prev[:5] = pos[:5] - np.array([2.5 * EDGE, 0.0], np.float32)
    return dict(pos=pos, rad=rad, world=world, prev=prev, ws=3, grid=(3, 1))


def holes_scene():
    """Two strips; rank 0's whole border block column (1500 particles on a lattice, beside a sparse cloud) moves one
    block to the right in one step.  At capacity_scale 0.5 the ghost rows of the segment (about 1800) still take the
    column, and the hole list has 1024 entries (the migrant rows of all neighbour segments, about 700 here, and 1024 at
    least: gpe_shard_configure)."""
    pos, rad, world = _strips(3, 2, 3, 4, seed=4)
    gx, gy = np.meshgrid(np.arange(30, dtype=np.float32), np.arange(50, dtype=np.float32))
    col = np.stack([2.05 * EDGE + gx.ravel() * np.float32(0.27), 0.2 * EDGE + gy.ravel() * np.float32(0.4)], 1).astype(np.float32)
    pos = np.concatenate([col, pos]).astype(np.float32)
    prev = pos.copy()
    prev[:len(col), 0] -= np.float32(EDGE)
    return dict(pos=pos, rad=np.full(len(pos), 0.5, np.float32), world=world, prev=prev, ws=2, grid=(2, 1), capacity_scale=0.5)


def capacity_scene():
    """Two strips at 30 per block; capacity= 1 asks for no room beyond the rank's own particles (the library takes the
    larger of the two), so the first ghost band does not fit."""
    pos, rad, world = _strips(3, 2, 3, 30, seed=5)
    return dict(pos=pos, rad=rad, world=world, prev=None, ws=2, grid=(2, 1), capacity=1)


def recv_overflow_scene():
    """Two strips at 40 per block with segments of a handful of rows (capacity_scale 0.002): the sender's header counts
    every row it wanted to send, which is more than the receiver's segment holds."""
    pos, rad, world = _strips(3, 2, 3, 40, seed=6)
    return dict(pos=pos, rad=rad, world=world, prev=None, ws=2, grid=(2, 1), capacity_scale=0.002)


def empty_after_recut_scene():
    """Four horizontal strips of three block rows; a cloud in the bottom block row and one particle in the lowest block
    row of each other strip (rows 3, 6, 9).  The re-sort step re-cuts at the quantiles: [0, 2, 4, 6, 12] with the
    minimum width of two, and rank 2 (rows 4 and 5) owns nothing."""
    rng = np.random.default_rng(7)
    world = ((4 * 8 - 0.5) * CELL, (12 * 8 - 0.5) * CELL)
    cloud = (rng.random((1200, 2), dtype=np.float32) * np.array([world[0], 0.9 * EDGE], np.float32)).astype(np.float32)
    lone = np.array([[0.5 * world[0], (row + 0.5) * EDGE] for row in (3, 6, 9)], np.float32)
    pos = np.concatenate([lone, cloud]).astype(np.float32)
    return dict(pos=pos, rad=np.full(len(pos), 0.5, np.float32), world=world, prev=None, ws=4, grid=(1, 4))


def _local_run(gpe, scene, **kw):
    return _lg().LocalShardedRun(scene["pos"], scene["rad"], scene["world"], scene["ws"], prev=scene["prev"], grid=scene["grid"],
                                 capacity_scale=scene.get("capacity_scale", 1.0), capacity=scene.get("capacity"), **kw)


def refuse_no_slot(gpe):
    run = _local_run(gpe, no_slot_scene())
    try:
        raised = _run_then_read(run, 1 / 60, 3, 2)          # the jump is step 0; the re-sort of step 2 brings everybody home
    finally:
        run.close()
    _assert_all_failed(gpe, raised, "a particle moved more than one block in a step", gpe._lib.GPE_ERR_UNSUPPORTED, where=[0])
    assert _flags(raised[0]) & ERR_NO_SLOT


def refuse_holes(gpe):
    run = _local_run(gpe, holes_scene())
    try:
        raised = _run_then_read(run, 1 / 60, 3, 2)
    finally:
        run.close()
    _assert_all_failed(gpe, raised, "too many migrants in one step", gpe._lib.GPE_ERR_UNSUPPORTED, where=[0])
    assert _flags(raised[0]) & ERR_HOLES


def refuse_capacity(gpe):
    run = _local_run(gpe, capacity_scene())
    try:
        raised = _run_then_read(run, 1 / 60, 3, 2)
    finally:
        run.close()
    _assert_all_failed(gpe, raised, "particle capacity exceeded", gpe._lib.GPE_ERR_UNSUPPORTED)
    assert any(_flags(e) & ERR_CAPACITY for e in raised)


def refuse_recv_overflow(gpe):
    run = _local_run(gpe, recv_overflow_scene())
    try:
        raised = _run_then_read(run, 1 / 60, 3, 2)
    finally:
        run.close()
    _assert_all_failed(gpe, raised, "a neighbour segment overflowed", gpe._lib.GPE_ERR_UNSUPPORTED)
    assert any(_flags(e) & ERR_RECV for e in raised), [str(e) for e in raised]


def refuse_empty_after_recut(gpe):
    run = _local_run(gpe, empty_after_recut_scene(), gravity=(0.0, -9.81))
    try:
        raised = _run_then_read(run, 1 / 60, 3, 2, first=False)          # two steps, then the re-sort step that re-cuts
        recuts = [s["recuts"] for s in run.stats()]
    finally:
        run.close()
    _assert_all_failed(gpe, raised, "this rank owns no particle after the re-cut", gpe._lib.GPE_ERR_UNSUPPORTED, where=[2])
    assert "another rank failed in the re-cut" in str(raised[0]), str(raised[0])
    assert recuts == [0, 0, 0, 0]                           # nobody moved on to the new cuts


REFUSALS = {"no-slot": refuse_no_slot, "holes": refuse_holes, "capacity": refuse_capacity, "recv-overflow": refuse_recv_overflow,
            "empty-after-re-cut": refuse_empty_after_recut}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_is_loud_on_every_rank(gpe, case):
    """A handled error path each (no scene faults the device): rows that have no place are dropped and the sticky error
    word says why at the next call that synchronises; a re-cut that would leave a rank empty fails on all ranks together."""
    REFUSALS[case](gpe)


def test_setup_refuses_a_rectangle_one_block_wide(gpe):
    """gpe_shard_setup with an explicit layout whose middle column is one block wide: every rank refuses for itself (the
    same layout, the same verdict) and the ranks leave the set-up together, before anything is planned."""
    lg = _lg()
    pos, rad, world = _strips(2, 3, 2, 10, seed=8)

    class Recording(lg.LocalShardedRun):
        raised = None

        def _each(self, fn):
            self.raised = _each_rank_of(lg.LocalShardedRun._each, self, fn)
            bad = [e for e in self.raised if e is not None]
            if bad:
                raise bad[0]

    run = Recording.__new__(Recording)
    try:
        with pytest.raises(gpe.GpeError):
            run.__init__(pos, rad, world, 3, grid=(3, 1), xcuts=[0, 3, 4, 6])
        raised = run.raised
    finally:
        run.close()
    assert len(raised) == 3 and all(isinstance(e, gpe.GpeError) for e in raised), raised
    for e in raised:
        assert "every rectangle must be at least two blocks wide" in str(e) and e.status == gpe._lib.GPE_ERR_UNSUPPORTED, str(e)
