"""Layout of the Initializer entry points' structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT

PAIRS = (("slamit_init_problem", "InitProblem"), ("slamit_init_result", "InitResult"),
         ("slamit_init_reconstruct_problem", "InitReconstructProblem"), ("slamit_init_reconstruct_result", "InitReconstructResult"))
FUNCTIONS = ("slamit_init_hyp", "slamit_init_hyp_batch", "slamit_init_reconstruct", "slamit_init_reconstruct_batch",
             "slamit_init_best_hypothesis", "slamit_init_choose_h", "slamit_init_pick_f", "slamit_init_pick_h")


def test_initializer_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d %d %d\\n", SLAMIT_INIT_MAX_N, SLAMIT_INIT_MAX_HYP, SLAMIT_INIT_H, SLAMIT_INIT_F);\n'
    want = [api.INIT_MAX_N, api.INIT_MAX_HYP, api.INIT_H, api.INIT_F]
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
    assert (api.INIT_MAX_N, api.INIT_MAX_HYP, api.INIT_H, api.INIT_F) == (8192, 1024, 0, 1)
    assert (C.sizeof(api.InitProblem), C.sizeof(api.InitResult), C.sizeof(api.InitReconstructProblem), C.sizeof(api.InitReconstructResult)) == (64, 32, 136, 480)


def test_initializer_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in FUNCTIONS:
        assert "int %s(" % name in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "float slamit_init_parallax_deg(" in hdr and "slamit_init_parallax_deg" in api.EXPORTS
    assert "initializer.hip" in build.SOURCES and "initializer.hip" not in build.PER_FILE      # -ffp-contract=off like the rest
    for cname, _ in PAIRS:
        assert "typedef struct %s %s;" % (cname, cname) in hdr
