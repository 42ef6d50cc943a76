"""The transaction behind every gpe_set_* call that replaces device tables (gpu-physics-engine_amd/csrc/set_upload.h) on
the CPU: the header compiles on its own with g++ (no HIP header), and tests/cpp/set_upload_tests.cpp drives it against a
fake of the device calls that counts live blocks and fails its n-th call -- five tables, three copies, two fills and the
wait, each of the eleven failing in turn: nothing reserved is left, nothing is released twice, the caller's pointers are
null, no call follows the failing one, and its status and text are what the caller gets.  Built with the address and
undefined-behaviour sanitizers: a stand-alone program, nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "set_upload_tests.cpp")

TESTS = ["failing_reserve_%d" % i for i in range(1, 6)] + ["failing_copy_%d" % i for i in range(1, 4)] + [
    "failing_fill_1", "failing_fill_2", "failing_wait", "no_failure", "an_optional_table_of_count_zero_is_skipped",
    "destroyed_without_finish", "a_second_failure_does_not_replace_the_first",
]


def test_set_upload_unwinding_under_sanitizers(tmp_path):
    exe = str(tmp_path / "set_upload_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == TESTS
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in TESTS:
        assert "test %s ... ok" % name in r.stdout
