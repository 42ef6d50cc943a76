"""CPU: the cluster query entry points (gpe_query_clusters, gpe_query_cluster_of) are declared by include/gpe.h with
the documented argument lists, the result struct agrees between the header, _lib.GpeClusterResult and the Rust struct
in INTEGRATION.md, libgpe.so exports both, _lib.SYMBOLS binds them, a NULL context and a NULL result are refused,
engine.py, gpe_host.hpp and INTEGRATION.md mirror them, and the numpy model (tests/_clusters_model.py) is right on
hand-made graphs.  What the device computes is checked against that model by tests/test_gpu_clusters.py."""
import ctypes
import os
import re

import numpy as np

from tests._clusters_model import clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpe.h")).read()
DOC = open(os.path.join(ROOT, "INTEGRATION.md")).read()

VP = ctypes.c_void_p
F32 = np.float32
DECLARATIONS = {"gpe_query_clusters": ["gpe_ctx *ctx", "gpe_cluster_result *out"],
                "gpe_query_cluster_of": ["gpe_ctx *ctx", "uint32_t key_kind", "uint32_t key", "gpe_query_result *out"]}
# (name, C type, pointer) in the header's order
FIELDS = [("struct_size", "uint32_t", False), ("reserved", "uint32_t", False), ("count", "uint64_t", False),
          ("largest_size", "uint32_t", False), ("largest_label", "uint32_t", False), ("label", "uint32_t", True),
          ("size", "uint32_t", True), ("label_uid", "uint32_t", True)]
RUST = {"uint32_t": "u32", "uint64_t": "u64"}
PY_METHODS = ("clusters(self)", "count_clusters(self)", "cluster_of(self, index=None, uid=None, capacity=None)")


def _strip(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _header_fields():
    body = re.search(r"typedef struct gpe_cluster_result \{(.*?)\} gpe_cluster_result;", _strip(HEADER), flags=re.S)
    assert body, "gpe_cluster_result is not defined in include/gpe.h"
    out = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            m = re.match(r"([a-z0-9_]+)\s*(\*?)\s*([a-z0-9_]+)$", decl)
            assert m, decl
            out.append((m.group(3), m.group(1), bool(m.group(2))))
    return out


def test_header_declares_the_cluster_queries_argument_for_argument():
    for name, want in DECLARATIONS.items():
        m = re.search(r"gpe_status\s+%s\s*\(([^;]*?)\)\s*;" % name, _strip(HEADER), flags=re.S)
        assert m, "%s is not declared in include/gpe.h" % name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert re.search(r"enum\s*\{\s*GPE_CLUSTER_BY_INDEX\s*=\s*0\s*,\s*GPE_CLUSTER_BY_UID\s*=\s*1\s*\}", _strip(HEADER))
    assert re.search(r"#define\s+GPE_ABI_VERSION\s+1u", _strip(HEADER))
    # the section follows the contact queries
    assert HEADER.index("gpe_query_contacts(gpe_ctx") < HEADER.index("typedef struct gpe_cluster_result")


def test_result_struct_agrees_in_header_ctypes_and_rust(gpe):
    assert _header_fields() == FIELDS
    R = gpe._lib.GpeClusterResult
    assert [f[0] for f in R._fields_] == [f[0] for f in FIELDS]
    assert ctypes.sizeof(R) == 48
    offset = 0
    for name, ctype, ptr in FIELDS:
        width = 8 if ptr else {"uint32_t": 4, "uint64_t": 8}[ctype]
        offset = (offset + width - 1) // width * width
        assert getattr(R, name).offset == offset, name
        assert getattr(R, name).size == width, name
        offset += width
    assert offset == 48
    body = re.search(r"pub struct gpe_cluster_result \{(.*?)\}", DOC, flags=re.S)
    assert body, "INTEGRATION.md lacks #[repr(C)] pub struct gpe_cluster_result"
    assert re.search(r"#\[repr\(C\)\]\s*pub struct gpe_cluster_result", DOC)
    decls = [" ".join(d.split()) for d in re.sub(r"//[^\n]*", " ", body.group(1)).split(",") if d.strip()]
    want = ["pub %s: %s%s" % (name, "*mut " if ptr else "", RUST[ctype]) for name, ctype, ptr in FIELDS]
    assert decls == want
    assert (gpe._lib.CLUSTER_BY_INDEX, gpe._lib.CLUSTER_BY_UID) == (0, 1)


def test_library_exports_and_binds_the_cluster_queries(gpe):
    gpe.build()
    lib = ctypes.CDLL(gpe._lib.LIB_PATH)
    assert hasattr(lib, "gpe_query_clusters") and hasattr(lib, "gpe_query_cluster_of")
    bound = {name: (res, args) for name, res, args in gpe._lib.SYMBOLS}
    assert bound["gpe_query_clusters"] == (ctypes.c_int32, [VP, ctypes.POINTER(gpe._lib.GpeClusterResult)])
    assert bound["gpe_query_cluster_of"] == (ctypes.c_int32, [VP, ctypes.c_uint32, ctypes.c_uint32,
                                                              ctypes.POINTER(gpe._lib.GpeQueryResult)])


def test_null_context_and_null_result_are_refused(gpe):
    gpe.build()
    L = gpe._lib
    lib = L.load()
    res = L.GpeClusterResult(struct_size=ctypes.sizeof(L.GpeClusterResult), count=99, largest_size=7, largest_label=5)
    assert lib.gpe_query_clusters(None, ctypes.byref(res)) == L.GPE_ERR_INVALID_ARG
    assert (res.count, res.largest_size, res.largest_label) == (99, 7, 5)       # nothing written without a context
    assert lib.gpe_query_clusters(None, None) == L.GPE_ERR_INVALID_ARG
    rows = L.GpeQueryResult(struct_size=ctypes.sizeof(L.GpeQueryResult), capacity=0, count=99)
    assert lib.gpe_query_cluster_of(None, L.CLUSTER_BY_INDEX, 0, ctypes.byref(rows)) == L.GPE_ERR_INVALID_ARG
    assert rows.count == 99
    assert lib.gpe_query_cluster_of(None, L.CLUSTER_BY_UID, 0, None) == L.GPE_ERR_INVALID_ARG


def test_host_layers_mirror_the_cluster_queries(gpe):
    py = open(os.path.join(ROOT, "gpu-physics-engine_amd", "engine.py")).read()
    hpp = open(os.path.join(ROOT, "gpu-physics-engine_amd", "host", "gpe_host.hpp")).read()
    for cls in ("ParticleSystem", "State"):
        body = re.search(r"\nclass %s\b.*?(?=\nclass |\Z)" % cls, py, flags=re.S).group(0)
        for m in PY_METHODS:
            assert "def " + m in body, (cls, m)
    assert re.search(r'ClusterResult\s*=\s*collections\.namedtuple\("ClusterResult",\s*'
                     r'"label size label_uid count largest_size largest_label"\)', py)
    assert gpe.ClusterResult._fields == ("label", "size", "label_uid", "count", "largest_size", "largest_label")
    for m in ("clusters", "count_clusters", "cluster_of"):
        assert re.search(r"\b%s\s*\(" % m, hpp), "gpe_host.hpp lacks %s" % m
        assert re.search(r"pub fn %s\b" % m, DOC), "INTEGRATION.md shim lacks %s" % m
    assert "gpe_query_clusters(ctx_->raw()" in hpp and "gpe_query_cluster_of(ctx_->raw()" in hpp
    block = re.search(r'extern "C" \{(.*?)\n\}', DOC, flags=re.S).group(1)
    assert "pub fn gpe_query_clusters(" in block and "pub fn gpe_query_cluster_of(" in block


# ---- the model on hand-made graphs ---------------------------------------------------------------------------------
def _model(pos, rad):
    label, size, count, largest_size, largest_label = clusters(np.array(pos, F32).reshape(-1, 2), np.array(rad, F32))
    assert label.dtype == np.uint32 and size.dtype == np.uint32
    assert count == int((label == np.arange(len(label))).sum())
    return label.tolist(), size.tolist(), count, largest_size, largest_label


def test_model_chain_whose_ends_do_not_touch_is_one_cluster():
    # 0-1 and 1-2 touch (distance 1.5 < 2), 0-2 do not (3 > 2)
    assert _model([[0, 0], [1.5, 0], [3, 0]], [1, 1, 1]) == ([0, 0, 0], [3, 3, 3], 1, 3, 0)
    assert _model([[0, 0], [1.5, 0], [30, 0]], [1, 1, 1]) == ([0, 0, 2], [2, 2, 1], 2, 2, 0)
    assert _model([[0, 0]], [1]) == ([0], [1], 1, 1, 0)
    assert _model(np.zeros((0, 2)), []) == ([], [], 0, 0, 0)


def test_model_boundary_is_two_clusters_and_one_ulp_inside_is_one():
    # 3-4-5: q = 9 + 16 = 25 = (2.5 + 2.5)^2, every step exact in binary32
    assert _model([[0, 0], [3, 4]], [2.5, 2.5]) == ([0, 1], [1, 1], 2, 1, 0)
    r = F32(2.5) + F32(2.0 ** -21)                                  # the radius sum grows by one ulp of 5
    assert F32(r) + F32(2.5) == np.nextafter(F32(5), F32(6))
    assert _model([[0, 0], [3, 4]], [r, 2.5]) == ([0, 0], [2, 2], 1, 2, 0)


def test_model_zero_radius_sum_and_nan_are_singletons():
    assert _model([[1, 1], [1, 1]], [0.0, 0.0]) == ([0, 1], [1, 1], 2, 1, 0)      # coincident, radius sum 0: separate
    assert _model([[1, 1], [1, 1]], [0.5, -0.5])[0] == [0, 1]
    assert _model([[1, 1], [1, 1]], [0.5, 0.25])[0] == [0, 0]
    nan = float("nan")
    # the NaN particle sits between two that touch each other, on top of both
    assert _model([[1, 1], [nan, 1], [1, 1.5]], [1, 1, 1]) == ([0, 1, 0], [2, 1, 2], 2, 2, 0)
    assert _model([[1, 1], [1, 1], [1, 1.5]], [1, nan, 1])[0] == [0, 1, 0]


def test_model_label_is_the_minimum_index_even_in_the_middle_of_the_chain():
    # along x: particles 3, 4, 0, 2, 1 -- the minimum sits in the middle, the ends carry high indices
    order = [3, 4, 0, 2, 1]
    pos = np.zeros((6, 2), F32)
    for k, i in enumerate(order):
        pos[i] = (1.5 * k, 0.0)
    pos[5] = (100.0, 100.0)
    assert _model(pos, np.ones(6, F32)) == ([0] * 5 + [5], [5] * 5 + [1], 2, 5, 0)
    # two clusters of equal size: the largest is the one with the lower label
    assert _model([[50, 0], [0, 0], [51, 0], [1, 0]], [1, 1, 1, 1]) == ([0, 1, 0, 1], [2, 2, 2, 2], 2, 2, 0)
    assert _model([[50, 0], [0, 0], [1, 0], [2.5, 0]], [1, 1, 1, 1]) == ([0, 1, 1, 1], [1, 3, 3, 3], 2, 3, 1)


def test_model_permuting_storage_permutes_the_partition_and_re_minimises_the_labels():
    rng = np.random.default_rng(5)
    pos = rng.uniform(0, 40, (300, 2)).astype(F32)
    rad = rng.choice(np.array([0.1, 0.5, 1.0, 2.0], F32), 300)
    label, size, count, largest_size, largest_label = clusters(pos, rad)
    assert 10 < count < 290 and largest_size > 3
    perm = rng.permutation(300)                                     # new slot k holds old particle perm[k]
    inv = np.argsort(perm)                                          # old particle i sits in new slot inv[i]
    label2, size2, count2, largest_size2, largest_label2 = clusters(pos[perm], rad[perm])
    assert (count2, largest_size2) == (count, largest_size)
    assert np.array_equal(size2, size[perm])
    want = np.full(300, 300, np.int64)                              # per old cluster: the lowest new slot of its members
    np.minimum.at(want, label, inv)
    assert np.array_equal(label2, want[label][perm].astype(np.uint32))
    sizes_of_roots = np.bincount(label2, minlength=300)
    assert largest_label2 == int(np.flatnonzero(sizes_of_roots == largest_size)[0])
