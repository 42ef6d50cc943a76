"""The start of a freshly configured context in the native step's launch heuristics (native_policy.h) on the CPU:
tests/cpp/native_startup_tests.cpp drives it step by step -- no half-tile launch and the 128-workgroup over-capacity
grid until a tile has been reported, today's start for a scene that is dense at configuration time.  The transitions
that were there before stay pinned by tests/cpp/native_policy_tests.cpp (test_native_policy_cpu.py)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "native_startup_tests.cpp")

TESTS = [
    "quiet_context_from_step_one", "first_reported_tile_brings_both_back", "halves_over_alone_brings_the_grid_back",
    "with_front_workgroups_hinted_tiles_do_not_count", "dense_configuration_starts_as_before",
    "configure_resets_the_member",
]


def test_native_startup_policy(tmp_path):
    exe = str(tmp_path / "native_startup_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
