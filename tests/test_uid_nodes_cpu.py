"""CPU: the node list and rows shared by the step sets that name their particles by uid (csrc/uid_nodes.h), through
its stand-alone test program (tests/cpp/uid_nodes_tests.cpp), plain and under the host sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")
NODES_SRC = os.path.join(ROOT, "tests", "cpp", "uid_nodes_tests.cpp")
NODES_TESTS = ["no_incidences", "one_uid", "descending_uids", "random_incidences"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_uid_nodes_program(tmp_path, sanitize):
    """The stand-alone program (its own main; nothing of it is loaded into python): g++ without a HIP header, once
    plain and once under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "uid_nodes_tests")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [NODES_SRC, "-o", exe])
    assert subprocess.check_output([exe, "--list"], text=True).split() == NODES_TESTS
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in NODES_TESTS:
        assert "test %s ... ok" % name in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_holds_no_hip_and_the_node_search_has_one_home():
    text = open(os.path.join(CSRC, "uid_nodes.h")).read()
    assert not re.search(r"#include\s*[<\"](hip/|gpe_internal)", text)
    sources = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip"))]
    homes = [name for name in sources if "lower_bound(nodes" in open(os.path.join(CSRC, name)).read()]
    assert homes == ["uid_nodes.h"], homes
