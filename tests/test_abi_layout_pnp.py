"""Layout of the PnPsolver entry points' structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT

PAIRS = (("slamit_pnp_problem", "PnpProblem"), ("slamit_pnp_result", "PnpResult"),
         ("slamit_pnp_refine_problem", "PnpRefineProblem"), ("slamit_pnp_refine_result", "PnpRefineResult"))


def test_pnp_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d\\n", SLAMIT_PNP_MAX_N, SLAMIT_PNP_MAX_HYP);\n'
    want = [api.PNP_MAX_N, api.PNP_MAX_HYP]
    for cname, pyname in PAIRS:
        mirror = getattr(api, pyname)
        src += '    printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(C.sizeof(mirror))
        for f, _ in mirror._fields_:
            src += '    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f)
            want.append(getattr(mirror, f).offset)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    assert [int(x) for x in subprocess.check_output([exe]).split()] == want
    assert (api.PNP_MAX_N, api.PNP_MAX_HYP) == (8192, 1024)
    assert (C.sizeof(api.PnpProblem), C.sizeof(api.PnpResult), C.sizeof(api.PnpRefineProblem), C.sizeof(api.PnpRefineResult)) == (80, 24, 72, 112)


def test_pnp_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_pnp_ransac", "slamit_pnp_ransac_batch", "slamit_pnp_refine_batch"):
        assert "int %s(" % name in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "pnp.hip" in build.SOURCES and "pnp.hip" not in build.PER_FILE      # -ffp-contract=off like the rest
    for cname, _ in PAIRS:
        assert "typedef struct %s %s;" % (cname, cname) in hdr
