"""Layout of the triangulation entry point's structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT


def test_triangulate_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    fields_p = [f[0] for f in api.TriangulateProblem._fields_]
    fields_r = [f[0] for f in api.TriangulateResult._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%zu %zu %d %d\\n", sizeof(slamit_triangulate_problem), sizeof(slamit_triangulate_result), SLAMIT_TRIANGULATE_MAX_N, SLAMIT_MAX_LEVELS);\n'
    for f in fields_p:
        src += '    printf("%%zu\\n", offsetof(slamit_triangulate_problem, %s));\n' % f
    for f in fields_r:
        src += '    printf("%%zu\\n", offsetof(slamit_triangulate_result, %s));\n' % f
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == C.sizeof(api.TriangulateProblem) and v[1] == C.sizeof(api.TriangulateResult)
    assert (v[2], v[3]) == (api.TRIANGULATE_MAX_N, api.MAX_LEVELS) == (8192, 16)
    want = [getattr(api.TriangulateProblem, f).offset for f in fields_p] + [getattr(api.TriangulateResult, f).offset for f in fields_r]
    assert v[4:] == want
    assert fields_p[:6] == ["Tcw1", "Tcw2", "intr1", "intr2", "n", "n_levels"] and fields_r == ["status", "x3d", "n_accepted"]


def test_triangulate_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_triangulate", "slamit_triangulate_batch"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "triangulate.hip" in build.SOURCES and "triangulate.hip" not in build.PER_FILE       # -ffp-contract=off, like the rest
    assert callable(api.triangulate) and callable(api.triangulate_batch)
