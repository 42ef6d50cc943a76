"""The bookkeeping behind the profiling scopes (gpu-physics-engine_amd/csrc/scope_events.h) on the CPU: the header
compiles on its own with g++ (no HIP header), and tests/cpp/scope_events_tests.cpp drives open / close / nested / reset
sequences against a stub of the event calls -- which scopes share an event, seven records for a kept-table native step,
every event back in the pool and destroyed exactly once.  Built with the address and undefined-behaviour sanitizers: a
stand-alone program, nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scope_events_tests.cpp")

TESTS = [
    "own_events_outside_a_region", "native_step_records_seven_events", "events_are_reused_step_after_step",
    "enqueue_between_two_nested_scopes", "enqueue_behind_the_last_nested_scope",
    "a_scope_nobody_vouches_for_keeps_its_pair", "boundaries_are_not_shared_across_a_region_s_ends",
    "an_empty_scope_takes_one_event", "resolving_in_the_middle_keeps_the_boundary", "reset_and_profiling_off_and_on",
    "destroy_with_scopes_pending", "event_creation_fails",
]


def test_scope_event_bookkeeping_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scope_events_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
