"""Layout of the projection and rotation-check entry points' structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT

STRUCTS = (("slamit_project_camera", "ProjectCamera"), ("slamit_project_problem", "ProjectProblem"), ("slamit_project_result", "ProjectResult"),
           ("slamit_project_batch_rec", "ProjectBatchRec"), ("slamit_rotation_batch", "RotationBatch"))


def test_project_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d\\n", SLAMIT_PROJECT_MAX_N, SLAMIT_MAX_LEVELS);\n'
    src += '    printf("%d %d %d %d %d %d\\n", SLAMIT_PROJECT_LAST_FRAME, SLAMIT_PROJECT_RELOC, SLAMIT_PROJECT_FUSE, SLAMIT_PROJECT_SIM3_PROJ, SLAMIT_PROJECT_SIM3_FUSE, SLAMIT_PROJECT_SIM3_PAIR);\n'
    want = []
    for cname, pname in STRUCTS:
        cls = getattr(api, pname)
        src += '    printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            src += '    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0])
            want.append(getattr(cls, f[0]).offset)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert (v[0], v[1]) == (api.PROJECT_MAX_N, api.MAX_LEVELS) == (65536, 16)
    assert v[2:8] == list(range(6)) and [api.PROJECT_FORMS.index(f) for f in ("LAST_FRAME", "RELOC", "FUSE", "SIM3_PROJ", "SIM3_FUSE", "SIM3_PAIR")] == v[2:8]
    assert v[8:] == want
    assert api.PROJECT_CAMERA_DTYPE.itemsize == C.sizeof(api.ProjectCamera) == 224
    for f in api.ProjectCamera._fields_:
        assert api.PROJECT_CAMERA_DTYPE.fields[f[0]][1] == getattr(api.ProjectCamera, f[0]).offset, f[0]
    assert [f[0] for f in api.ProjectResult._fields_] == ["status", "proj", "level", "uvr", "level_min", "level_max", "valid", "n_valid"]


def test_the_host_restatement_has_the_c_abi_camera(tmp_path):
    """csrc/project.h is built without include/slamit.h (by g++ for the tests, by hipcc for the kernel): its ProjectCamera is the C-ABI's."""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "project.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(ProjectCamera), sizeof(slamit_project_camera));\n'
    src += '    printf("%d %d\\n", (int)PRJ_FORMS, 6);\n'
    names = [f for f in ("form", "R", "t", "O", "R2", "t2", "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "th", "n_levels",
                         "scale_factors", "direction")]
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(ProjectCamera, %s), offsetof(slamit_project_camera, %s));\n' % (f, f)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_camera.cc"), str(tmp_path / "_camera")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (len(names) + 2)


def test_project_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build, synth

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_project", "slamit_project_batch", "slamit_project_batch_dev", "slamit_rotation_check_batch_dev"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    for src in ("project.hip", "rotation.hip"):
        assert src in build.SOURCES and src not in build.PER_FILE                                 # -ffp-contract=off, like the rest
    assert callable(api.project) and callable(api.project_batch) and callable(api.project_batch_dev) and callable(synth.synth_project)
    assert callable(api.ORBmatcher.rotation_check_batch_dev)
