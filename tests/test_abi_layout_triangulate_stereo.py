"""Layout of the stereo records of the mapping side (struct slamit_triangulate_stereo, slamit_bow_stereo) and their four entry
points: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT


def test_stereo_record_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    fields_t = [f[0] for f in api.TriangulateStereo._fields_]
    fields_b = [f[0] for f in api.BowStereo._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    # the record's tag is also a function's name: both spellings of the type must compile as C99
    src += '    printf("%zu %zu %zu\\n", sizeof(struct slamit_triangulate_stereo), sizeof(slamit_triangulate_stereo_rec), sizeof(slamit_bow_stereo));\n'
    for f in fields_t:
        src += '    printf("%%zu\\n", offsetof(struct slamit_triangulate_stereo, %s));\n' % f
    for f in fields_b:
        src += '    printf("%%zu\\n", offsetof(slamit_bow_stereo, %s));\n' % f
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    # the prototypes, compiled only: a mismatch of a parameter type is an error
    proto = '#include "slamit.h"\n'
    proto += "int (*one)(int, const slamit_triangulate_problem*, const struct slamit_triangulate_stereo*, slamit_triangulate_result*, uint8_t*) = slamit_triangulate_stereo;\n"
    proto += ("int (*many)(int, int, const slamit_triangulate_problem*, const struct slamit_triangulate_stereo* const*, slamit_triangulate_result*, uint8_t* const*)"
              " = slamit_triangulate_stereo_batch;\n")
    proto += ("int (*bow)(int, const uint8_t*, int32_t, const uint8_t*, const uint8_t*, int32_t, const uint8_t*, const slamit_bow_groups*, const slamit_bow_rule*,"
              " const slamit_bow_stereo*, int32_t*, int32_t*, int32_t*) = slamit_bow_search_stereo;\n")
    open(str(tmp_path / "_proto.c"), "w").write(proto)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(tmp_path / "_proto.c"), "-o", str(tmp_path / "_proto.o")])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == v[1] == C.sizeof(api.TriangulateStereo) and v[2] == C.sizeof(api.BowStereo)
    want = [getattr(api.TriangulateStereo, f).offset for f in fields_t] + [getattr(api.BowStereo, f).offset for f in fields_b]
    assert v[3:] == want
    assert fields_t == ["ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy", "mb1", "mb2", "bf"] and fields_b == ["ur1", "ur2", "only_stereo"]


def test_the_old_records_did_not_move():
    from weiner_slamit_v2_amd import api

    assert C.sizeof(api.TriangulateProblem) == 224 and C.sizeof(api.TriangulateResult) == 24
    assert C.sizeof(api.BowRule) == 216


def test_the_four_entry_points_are_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_triangulate_stereo", "slamit_triangulate_stereo_batch", "slamit_bow_search_stereo", "slamit_bow_search"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
