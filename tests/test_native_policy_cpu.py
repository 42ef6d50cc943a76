"""The native step's launch heuristics (gpu-physics-engine_amd/csrc/native_policy.h) on the CPU: the header compiles on
its own with g++ (no HIP header) and tests/cpp/native_policy_tests.cpp drives every decision step by step."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "native_policy_tests.cpp")

TESTS = [
    "admission_at_configuration", "handover_above_the_window_population", "probe_every_256_held_steps",
    "return_when_the_probe_finds_thin_windows", "must_stay_readmits_inside_the_box",
    "arena_doubles_when_more_than_half_used", "failed_arena_growth", "sort_hold_after_48_of_64_steps_sorted",
    "probe_skips_the_sort_hold_window", "fused_histograms_when_a_quarter_sorted",
    "crowded_tiles_take_the_counting_sort_form", "front_workgroups", "half_tile_launch_without_front_workgroups",
    "half_tile_launch_with_front_workgroups", "over_capacity_grid", "configuration_resets",
]


def test_native_policy_transitions(tmp_path):
    exe = str(tmp_path / "native_policy_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
