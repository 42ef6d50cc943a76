"""GPU (-m gpu): `bench.py --steps K --warmup W --dump-outputs DIR` times exactly K steps and dumps what the last of
them left: the positions, previous positions and radii of the seeded bench scene after W + K steps of its schedule
(re-sort on step 0 and every 240th step), bit-exact against the CPU oracle run through the same steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_times_steps_and_dumps_the_last_step(gpe, oracle, tmp_path):
    n, warmup, steps = 20_000, 3, 240                          # the re-sort at step 240 falls inside the timed window
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--particles", str(n), "--no-extra", "--no-cpu-baseline",
                        "--dump-outputs", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["timed_steps_total"] == steps and d["timing"]["windows"] == 1
    assert d["ms_per_step"] == pytest.approx(d["timing"]["timed_seconds_total"] * 1e3 / steps, rel=1e-2)

    world = gpe.scenes.world_for(n)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=0x5EED)    # bench.py's scene (rank 0)
    sim = oracle.Sim(pos, rad, oracle.default_params(world[0], world[1], 0.5))
    for s in range(warmup + steps):
        sim.step(1 / 60, resort=(s % 240) == 0)
    want = {"positions": sim.pos, "previous_positions": sim.prev, "radii": sim.radius}
    sim.close()
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got = np.load(os.path.join(out, k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v), k
