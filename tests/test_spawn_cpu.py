"""CPU: the overlap-checked add (gpe_add_particles_free).  The numpy model (tests/_spawn_model.py) is right on hand-worked
cases -- the exact edge, coincident candidates, the precedence of the verdicts, who may block whom, NaN -- and the struct
of _lib.py has the size and the field offsets a C compiler gives gpe_particle_spawn of include/gpe.h; libgpe.so exports
the symbol and refuses a NULL context.  What the device computes is checked against the model by
tests/test_gpu_spawn.py."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _spawn_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
WORLD = (100.0, 100.0)
FIELDS = ("struct_size", "flags", "k", "pos_xy", "radius", "verdict", "added")


def _verdicts(pos, rad, cpos, crad, **flags):
    v, app_pos, app_rad = M.spawn(np.array(pos, F32), np.array(rad, F32), np.array(cpos, F32), np.array(crad, F32), WORLD,
                                  **flags)
    keep = v == M.ADDED
    assert np.array_equal(app_pos.view(np.uint32), np.array(cpos, F32).reshape(-1, 2)[keep].view(np.uint32))
    assert np.array_equal(app_rad.view(np.uint32), np.array(crad, F32)[keep].view(np.uint32))
    return v.tolist()


def test_exact_edge_is_added_and_one_ulp_nearer_is_blocked():
    # q = 2 * 2 = 4 = (1 + 1)^2 exactly: not a contact
    assert _verdicts([[10, 10]], [1], [[12, 10]], [1]) == [M.ADDED]
    near = np.nextafter(F32(12), F32(0))
    assert _verdicts([[10, 10]], [1], [[near, 10]], [1]) == [M.BLOCKED_BY_PARTICLE]
    assert _verdicts([[10, 10]], [1], [[np.nextafter(F32(12), F32(13)), 10]], [1]) == [M.ADDED]


def test_coincident_candidates_under_separate():
    cpos, crad = [[50, 50]] * 4, [1, 1, 1, 1]
    assert _verdicts([[10, 10]], [1], cpos, crad, separate=True) == [M.ADDED] + [M.BLOCKED_BY_CANDIDATE] * 3
    assert _verdicts([[10, 10]], [1], cpos, crad) == [M.ADDED] * 4             # without the flag nobody is separated


def test_precedence_outside_world_then_particle_then_candidate():
    # candidate 0: free.  1: outside the world, on a particle and on candidate 0 -> 3.  2: on a particle and on
    # candidate 0 -> 1.  3: on candidate 0 only -> 2.
    pos, rad = [[0.5, 50], [52, 50]], [1, 1]
    cpos, crad = [[50, 50], [0.5, 50], [51, 50], [49, 50]], [1, 60, 1, 1]
    assert _verdicts(pos, rad, cpos, crad, separate=True, inside_world=True) == [0, 3, 1, 2]
    assert _verdicts(pos, rad, cpos, crad, separate=True) == [0, 1, 1, 2]      # no world test: rule 2 takes candidate 1
    assert _verdicts(pos, rad, cpos, crad, inside_world=True) == [0, 3, 1, 0]


def test_a_blocked_candidate_blocks_nobody():
    # candidate 0 sits on the particle; candidate 1 touches candidate 0 only; candidate 2 touches candidate 1
    pos, rad = [[10, 10]], [1]
    cpos, crad = [[11, 10], [12.5, 10], [14, 10]], [1, 1, 1]
    assert _verdicts(pos, rad, cpos, crad, separate=True) == [M.BLOCKED_BY_PARTICLE, M.ADDED, M.BLOCKED_BY_CANDIDATE]
    # ... nor does one blocked by a candidate: 0 added, 1 blocked by 0, 2 touches 1 only
    assert _verdicts([[90, 90]], [1], cpos, crad, separate=True) == [M.ADDED, M.BLOCKED_BY_CANDIDATE, M.ADDED]
    # ... nor one outside the world
    cpos2 = [[0.5, 50], [2, 50]]
    assert _verdicts([[90, 90]], [1], cpos2, [1, 1], separate=True, inside_world=True) == [M.OUTSIDE_WORLD, M.ADDED]
    assert _verdicts([[90, 90]], [1], cpos2, [1, 1], separate=True) == [M.ADDED, M.BLOCKED_BY_CANDIDATE]


def test_nan_candidate_is_added_unless_the_world_is_tested():
    nan = float("nan")
    pos, rad = [[10, 10]], [1]
    assert _verdicts(pos, rad, [[nan, 10], [10, nan], [10, 10]], [1, 1, nan], separate=True) == [0, 0, 0]
    assert _verdicts(pos, rad, [[nan, 10], [10, nan], [10, 10]], [1, 1, nan], inside_world=True) == [3, 3, 3]
    # the world test takes |r|: a negative radius of magnitude 2 at x = 1.5 is outside, at x = 2 inside
    assert _verdicts(pos, rad, [[1.5, 50], [2, 50]], [-2, -2], inside_world=True) == [3, 0]


def test_max_radius_is_fmaxf_over_the_appended_radii():
    assert M.max_radius_after(2.0, [1.0, 3.0, -5.0]) == F32(3.0)
    assert M.max_radius_after(-4.0, []) == F32(-4.0)
    assert M.max_radius_after(-4.0, [1.0]) == F32(1.0)


def test_struct_size_and_offsets_equal_the_compiled_header(gpe, tmp_path):
    src = tmp_path / "spawn_abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gpe.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(gpe_particle_spawn));\n'
                   + "".join('    printf("%%zu\\n", offsetof(gpe_particle_spawn, %s));\n' % f for f in FIELDS)
                   + '    printf("%d %d %d\\n", GPE_SPAWN_SEPARATE, GPE_SPAWN_INSIDE_WORLD, GPE_SPAWN_DRY_RUN);\n'
                   '    printf("%d %d %d %d\\n", GPE_SPAWN_ADDED, GPE_SPAWN_BLOCKED_BY_PARTICLE, '
                   'GPE_SPAWN_BLOCKED_BY_CANDIDATE, GPE_SPAWN_OUTSIDE_WORLD);\n    return 0;\n}\n')
    exe = str(tmp_path / "spawn_abi")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).split("\n")
    L = gpe._lib
    S = L.GpeParticleSpawn
    assert [f[0] for f in S._fields_] == list(FIELDS)
    assert int(out[0]) == ctypes.sizeof(S) == 48
    for f, line in zip(FIELDS, out[1:]):
        assert getattr(S, f).offset == int(line), f
    assert out[1 + len(FIELDS)].split() == [str(v) for v in (L.SPAWN_SEPARATE, L.SPAWN_INSIDE_WORLD, L.SPAWN_DRY_RUN)]
    assert out[2 + len(FIELDS)].split() == [str(v) for v in (L.SPAWN_ADDED, L.SPAWN_BLOCKED_BY_PARTICLE,
                                                             L.SPAWN_BLOCKED_BY_CANDIDATE, L.SPAWN_OUTSIDE_WORLD)]
    assert (M.ADDED, M.BLOCKED_BY_PARTICLE, M.BLOCKED_BY_CANDIDATE, M.OUTSIDE_WORLD) == (0, 1, 2, 3)


def test_library_exports_binds_and_refuses_null(gpe):
    gpe.build()
    L = gpe._lib
    lib = L.load()
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    assert bound["gpe_add_particles_free"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(L.GpeParticleSpawn)])
    sp = L.GpeParticleSpawn(struct_size=ctypes.sizeof(L.GpeParticleSpawn), added=99)
    assert lib.gpe_add_particles_free(None, ctypes.byref(sp)) == L.GPE_ERR_INVALID_ARG
    assert sp.added == 99                                          # nothing written without a context
    assert lib.gpe_add_particles_free(None, None) == L.GPE_ERR_INVALID_ARG
