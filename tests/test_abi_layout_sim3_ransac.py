"""Layout of the Sim3Solver entry point's structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT


def test_sim3_ransac_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    fields_p = [f[0] for f in api.Sim3RansacProblem._fields_]
    fields_r = [f[0] for f in api.Sim3RansacResult._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%zu %zu %d %d\\n", sizeof(slamit_sim3_ransac_problem), sizeof(slamit_sim3_ransac_result), SLAMIT_SIM3_RANSAC_MAX_N, SLAMIT_SIM3_RANSAC_MAX_HYP);\n'
    for f in fields_p:
        src += '    printf("%%zu\\n", offsetof(slamit_sim3_ransac_problem, %s));\n' % f
    for f in fields_r:
        src += '    printf("%%zu\\n", offsetof(slamit_sim3_ransac_result, %s));\n' % f
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == C.sizeof(api.Sim3RansacProblem) and v[1] == C.sizeof(api.Sim3RansacResult)
    assert (v[2], v[3]) == (api.SIM3_RANSAC_MAX_N, api.SIM3_RANSAC_MAX_HYP)
    want = [getattr(api.Sim3RansacProblem, f).offset for f in fields_p] + [getattr(api.Sim3RansacResult, f).offset for f in fields_r]
    assert v[4:] == want


def test_sim3_ransac_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_sim3_ransac", "slamit_sim3_ransac_batch"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "sim3_ransac.hip" in build.SOURCES and "sim3_ransac.hip" not in build.PER_FILE
