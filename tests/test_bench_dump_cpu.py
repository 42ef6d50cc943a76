"""CPU: `bench.py --dump-outputs DIR` -- the writer (float32 .npy files, at most 64 MB in all, the same seeded sample
of rows from every array above that) and its refusal for more than one GPU.  The dump of a real run is checked
against the oracle in tests/test_gpu_bench_dump.py."""
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
bench = importlib.import_module("bench")


def _arrays(n, seed=1):
    rng = np.random.default_rng(seed)
    return {"positions": rng.random((n, 2), dtype=np.float32), "previous_positions": rng.random((n, 2), dtype=np.float32),
            "radii": rng.random(n, dtype=np.float32)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_array_as_float32(tmp_path):
    a = _arrays(1000)
    a["radii"] = a["radii"].astype(np.float16)                  # anything not float64 is written as float32
    assert bench.dump_outputs(str(tmp_path), a) == ["positions", "previous_positions", "radii"]
    got = _load(str(tmp_path))
    assert sorted(got) == ["positions", "previous_positions", "radii"]
    for k, v in a.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v.astype(np.float32)), k


def test_dump_over_the_cap_keeps_the_same_seeded_rows_of_every_array(tmp_path):
    a = _arrays(100_000)                                        # 2 MB
    cap = 256 << 10
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, a, max_bytes=cap)
    bench.dump_outputs(d2, a, max_bytes=cap)
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= cap
    g1, g2 = _load(d1), _load(d2)
    assert sorted(g1) == ["positions", "previous_positions", "radii", "sample_rows"]
    rows = g1["sample_rows"]
    assert rows.dtype == np.float64 and len(rows) > 1000 and np.all(np.diff(rows) > 0)
    keep = rows.astype(np.int64)
    for k, v in a.items():
        assert np.array_equal(g1[k], v[keep]), k                # the same rows in every array
        assert np.array_equal(g1[k], g2[k]), k                  # and the same sample on every run
    bench.dump_outputs(d1, _arrays(10))                         # a later dump under the cap: no stale row indices
    assert sorted(_load(d1)) == ["positions", "previous_positions", "radii"]


def test_dump_outputs_needs_one_gpu(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs needs --gpus 1" in r.stderr
    assert not out.exists()
