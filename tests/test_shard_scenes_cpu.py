"""CPU: the scenes of tests/_shard_scenes.py claim what they exercise, and stay inside the conditions under which the
library promises a sharded run that is bit-identical to the single context (testing).  The oracle runs every
seed's whole schedule; tests/test_gpu_sharded_fuzz.py runs the same scenes on the device, where a failure is then a
bug of the library and never a badly chosen scene.  If a seed breaks a condition the generator changes, not this file."""
import collections

import numpy as np
import pytest

import _shard_scenes as S


@pytest.fixture(scope="module")
def threaded(oracle):
    before = oracle.get_threads()
    oracle.set_threads(8)
    yield oracle
    oracle.set_threads(before)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_scene_stays_inside_the_documented_limits(threaded, seed):
    scene = S.shard_scene(seed)
    c = scene["claims"]
    n, ws = len(scene["rad"]), scene["ws"]
    assert n == c["n"] <= 40_000 and sum(steps for steps, _, _ in scene["chunks"]) <= 40 and 2 <= len(scene["chunks"]) <= 4
    assert scene["pos"].dtype == np.float32 and scene["pos"].shape == (n, 2) and np.isfinite(scene["pos"]).all()
    assert (scene["pos"] >= 0).all() and (scene["pos"] <= np.array(scene["world"], np.float32)).all()
    assert np.float32(np.abs(scene["rad"]).max()) * np.float32(2.2) == scene["cell"]
    got = S.replay(scene, threaded)
    print("seed %d: n %d, ws %d grid %s, owned at re-sorts min %d, largest step %.2f cells, owner changes %d, re-cuts %d, "
          "largest max/mean %.2f" % (seed, n, ws, scene["grid"], min(int(o.min()) for o in got["owned_at_resort"]),
                                     got["max_step_cells"], got["owner_changes"], got["recuts"], got["worst_ratio"]))
    for counts in got["owned_at_resort"]:                  # the start, every re-sort step, and behind every re-cut
        assert counts.sum() == n and counts.min() >= 1, counts
    for dec in got["decs"]:
        assert dec.min_region_blocks() >= 2, (dec.xcuts, dec.ycuts)
        assert max(len(dec.neighbours(r)) for r in range(ws)) <= 8
    # the documented limit is one block (8 cells) a step; half of it, because the sharded run re-sorts at other steps
    assert got["max_step_cells"] < 4.0, got["max_step_cells"]
    assert got["owner_changes"] > 0
    if c["pile_up"]:
        assert got["worst_ratio"] > S.RECUT_ABOVE and got["recuts"] >= 1, (got["worst_ratio"], got["recuts"])
    # what the scene says about itself
    dec = got["decs"][0]
    assert (c["cuts"] == "default") == (scene["xcuts"] is None and scene["ycuts"] is None)
    if c["cuts"] == "two_wide":
        assert dec.min_region_blocks() == 2
    if c["cuts"] == "uneven":
        widths = [np.diff(dec.xcuts), np.diff(dec.ycuts)]
        assert any(len(set(w.tolist())) > 1 for w in widths), widths
    assert c["ragged"] == (dec.gx % 8 != 0 and dec.gy % 8 != 0)
    own = dec.owner_of(scene["pos"])
    big = scene["rad"] >= 2.0
    if c["radii"] == "one":
        assert len(np.unique(scene["rad"])) == 1
    elif c["radii"] == "mixed":
        assert big.any() and set(own[big]) == {ws - 1} and scene["rad"].max() == 3.0      # one corner holds every big one
    else:
        assert len(np.unique(scene["rad"])) > n // 2
    cs, edge = scene["cell"], np.float32(8) * scene["cell"]
    if "on_cuts" in c["placed"]:
        on = [(np.isin(scene["pos"][:, ax], (np.array(cuts[1:-1], np.float32) * np.float32(8)) * cs)).sum()
              for ax, cuts in ((0, dec.xcuts), (1, dec.ycuts))]
        assert sum(on) >= 1, on
    if "walls" in c["placed"]:
        assert (scene["pos"][:, 0] == scene["rad"]).any() or (scene["pos"][:, 1] == scene["rad"]).any()
    for name, centres in (("cut_clump", [(x * float(edge), None) for x in dec.xcuts[1:-1]] + [(None, y * float(edge)) for y in dec.ycuts[1:-1]]),
                          ("corner_clump", [(x * float(edge), y * float(edge)) for x in dec.xcuts[1:-1] for y in dec.ycuts[1:-1]])):
        if name in c["placed"]:
            near = 0
            for cx, cy in centres:
                dx = np.abs(scene["pos"][:, 0] - cx) if cx is not None else np.zeros(n)
                dy = np.abs(scene["pos"][:, 1] - cy) if cy is not None else np.zeros(n)
                inside = (dx <= 2 * float(cs)) & (dy <= 2 * float(cs))
                if cx is not None and cy is not None:      # the clump has members in all four rectangles
                    near = max(near, int(inside.sum()) if len(set(own[inside])) == 4 else 0)
                else:
                    near = max(near, int(inside.sum()) if len(set(own[inside])) >= 2 else 0)
            assert near >= 2, name
    assert c["prev"] == (scene["prev"] is not None) and c["mouse"] == (scene["mouse"] is not None)
    assert c["overlap"] == scene["overlap"] == (seed % 2 == 1)


def test_the_seeds_cover_what_the_fuzz_is_for():
    claims = [S.shard_scene(seed)["claims"] for seed in S.SEEDS]
    count = collections.Counter()
    for c in claims:
        px, py = c["grid"]
        keys = [("ws", c["ws"]), ("cuts", c["cuts"]), ("ragged", c["ragged"]), ("radii", c["radii"]), ("density", c["density"]),
                ("dt", c["dt"]), ("prev", c["prev"]), ("mouse", c["mouse"]), ("chunks", c["chunks"]), ("overlap", c["overlap"]),
                ("pile_up", c["pile_up"]), ("gx", int(np.sign(c["gravity"][0]))), ("gy", int(np.sign(c["gravity"][1])))]
        keys += [("placed", p) for p in c["placed"]]
        if py == 1 and px > 1:
            keys.append(("grid", "strip-x"))
        elif px == 1 and py > 1:
            keys.append(("grid", "strip-y"))
        else:
            keys.append(("grid", "2d"))
        if c["ws"] & (c["ws"] - 1):
            keys.append(("ws", "not a power of two"))
        count.update(keys)
    need = ([("ws", w) for w in (2, 3, 4, 5, 6, 7, 8, 9, 12, 16)] + [("grid", g) for g in ("strip-x", "strip-y", "2d")]
            + [("cuts", k) for k in ("default", "uneven", "two_wide")] + [("ragged", True), ("ragged", False)]
            + [("radii", k) for k in ("one", "mixed", "cont")] + [("density", d) for d in S.DENSITIES]
            + [("placed", p) for p in ("cut_clump", "corner_clump", "on_cuts", "walls")]
            + [("gx", s) for s in (-1, 0, 1)] + [("gy", s) for s in (-1, 0, 1)] + [("dt", float(t)) for t in S.TIME_STEPS]
            + [("prev", True), ("prev", False), ("chunks", 2), ("chunks", 3), ("chunks", 4), ("ws", "not a power of two")])
    short = {k: count[k] for k in need if count[k] < 2}
    assert not short, short
    assert count[("mouse", True)] == 6 and count[("overlap", True)] == 12 and count[("pile_up", True)] >= 3, count
    assert len({c["grid"] for c in claims}) >= 12                      # many factorisations, not one per rank count
