"""CPU: the particle-uid entry points (gpe_enable_uids, gpe_set_uids, gpe_next_uid, gpe_set_next_uid, gpe_find_uids,
gpe_remove_particles_by_uid) are declared by include/gpe.h with the documented argument shapes, exported by libgpe.so,
bound by _lib.SYMBOLS, refuse a NULL context, and are mirrored by engine.py, gpe_host.hpp and INTEGRATION.md.  What
they compute is checked on the device by tests/test_gpu_uids.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpe.h")).read()

U64P = ctypes.POINTER(ctypes.c_uint64)
VP, U64, I32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32

DECLARATIONS = {
    "gpe_enable_uids": ["gpe_ctx *ctx", "int32_t enable"],
    "gpe_set_uids": ["gpe_ctx *ctx", "const uint32_t *uids", "uint64_t n"],
    "gpe_next_uid": ["const gpe_ctx *ctx", "uint64_t *next"],
    "gpe_set_next_uid": ["gpe_ctx *ctx", "uint64_t next"],
    "gpe_find_uids": ["gpe_ctx *ctx", "const uint32_t *uids", "uint64_t k", "uint32_t *index_out", "float *pos_xy_out",
                      "float *prev_xy_out", "float *radius_out"],
    "gpe_remove_particles_by_uid": ["gpe_ctx *ctx", "const uint32_t *uids", "uint64_t k", "uint64_t *n_removed"],
}
BINDINGS = {
    "gpe_enable_uids": [VP, I32],
    "gpe_set_uids": [VP, VP, U64],
    "gpe_next_uid": [VP, U64P],
    "gpe_set_next_uid": [VP, U64],
    "gpe_find_uids": [VP, VP, U64, VP, VP, VP, VP],
    "gpe_remove_particles_by_uid": [VP, VP, U64, U64P],
}
PY_METHODS = ("enable_uids(self, on=True)", "uids(self)", "set_uids(self, uids)", "next_uid(self)",
              "set_next_uid(self, next_uid)", "find_uids(self, uids)", "remove_particles_by_uid(self, uids)")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"gpe_status\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared in include/gpe.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_uid_api_argument_for_argument():
    for name, args in DECLARATIONS.items():
        assert _declaration(name) == args, name


def test_header_defines_the_uid_array_and_absent_marker():
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    assert re.search(r"\bGPE_UIDS\s*=\s*12\b", text)
    assert re.search(r"#define\s+GPE_UID_ABSENT\s+0xffffffffu", text)
    assert re.search(r"#define\s+GPE_ABI_VERSION\s+1u", text)


def test_library_exports_and_binds_the_uid_api(gpe):
    gpe.build()
    lib = ctypes.CDLL(gpe._lib.LIB_PATH)
    bound = {name: args for name, _, args in gpe._lib.SYMBOLS}
    for name, args in BINDINGS.items():
        assert hasattr(lib, name), name
        assert bound[name] == args, name
    assert gpe._lib.UIDS == 12 and gpe._lib.UID_ABSENT == 0xFFFFFFFF


def test_null_context_is_refused(gpe):
    gpe.build()
    lib = gpe._lib.load()
    bad = gpe._lib.GPE_ERR_INVALID_ARG
    q = (ctypes.c_uint32 * 2)(0, 1)
    nxt = ctypes.c_uint64(5)
    removed = ctypes.c_uint64(7)
    assert lib.gpe_enable_uids(None, 1) == bad
    assert lib.gpe_enable_uids(None, 0) == bad
    assert lib.gpe_set_uids(None, q, 2) == bad
    assert lib.gpe_next_uid(None, ctypes.byref(nxt)) == bad
    assert lib.gpe_set_next_uid(None, 3) == bad
    assert lib.gpe_find_uids(None, q, 2, None, None, None, None) == bad
    assert lib.gpe_remove_particles_by_uid(None, q, 2, ctypes.byref(removed)) == bad
    assert removed.value == 0


def test_host_layers_mirror_the_uid_api():
    py = open(os.path.join(ROOT, "gpu-physics-engine_amd", "engine.py")).read()
    hpp = open(os.path.join(ROOT, "gpu-physics-engine_amd", "host", "gpe_host.hpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls in ("ParticleSystem", "State"):
        body = re.search(r"\nclass %s\b.*?(?=\nclass |\Z)" % cls, py, flags=re.S).group(0)
        for m in PY_METHODS:
            assert "def " + m in body, (cls, m)
    for m in ("enable_uids", "uids", "set_uids", "next_uid", "set_next_uid", "find_uids", "remove_particles_by_uid"):
        assert re.search(r"\b%s\s*\(" % m, hpp), "gpe_host.hpp lacks %s" % m
        assert re.search(r"pub fn %s\b" % m, doc), "INTEGRATION.md shim lacks %s" % m
    block = re.search(r'extern "C" \{(.*?)\n\}', doc, flags=re.S).group(1)
    for name in DECLARATIONS:
        assert "pub fn %s(" % name in block, name
    enum = re.search(r"pub enum gpe_array \{(.*?)\}", doc, flags=re.S).group(1)
    assert re.search(r"\bUIDS = 12\b", enum)


def test_snapshot_keeps_format_1_and_loads_old_snapshots():
    py = open(os.path.join(ROOT, "gpu-physics-engine_amd", "engine.py")).read()
    save = re.search(r"def save\(self, path\):.*?(?=\n    @classmethod|\n    def )", py, flags=re.S).group(0)
    load = re.search(r"def load\(cls, path.*?(?=\n    def )", py, flags=re.S).group(0)
    assert "format=np.array([1], np.int32)" in save and "uids=" in save and "next_uid=" in save
    assert '"uids" in d.files' in load            # a snapshot without them loads as before
