"""The run monitor through the C++ host mirror (gpu-physics-engine_amd/host/gpe_host.hpp): tests/cpp/monitor.cpp.
CPU: it compiles, links against libgpe.so and lists its tests.  GPU: it runs and every test passes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "monitor.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "monitor")
LIBDIR = os.path.join(ROOT, "gpu-physics-engine_amd")
MONITOR_TESTS = ["frames_equal_a_twin_that_measures_after_every_step"]


def _build(gpe):
    gpe.build()
    deps = [SRC, os.path.join(LIBDIR, "host", "gpe_host.hpp"), os.path.join(ROOT, "include", "gpe.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", SRC, "-L" + LIBDIR, "-lgpe",
                               "-Wl,-rpath," + LIBDIR, "-o", EXE])
    return EXE


def test_cpp_monitor_host_compiles_and_lists_its_tests(gpe):
    exe = _build(gpe)
    assert subprocess.check_output([exe, "--list"], text=True).split() == MONITOR_TESTS


@pytest.mark.gpu
def test_cpp_monitor_passes_on_gpu(gpe):
    exe = _build(gpe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for n in MONITOR_TESTS:
        assert "test %s ... ok" % n in r.stdout
