"""Layout of the stereo entry points' structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT

STRUCTS = (("slamit_pyramid_level", "PyramidLevel"), ("slamit_pyramid_view", "PyramidView"), ("slamit_stereo_batch", "StereoBatch"))


def test_stereo_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d %d\\n", SLAMIT_STEREO_MAX_KP, SLAMIT_SEARCH_MAX_KP, SLAMIT_MAX_LEVELS);\n'
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
    assert (v[0], v[1], v[2]) == (api.STEREO_MAX_KP, 8191, api.MAX_LEVELS) == (8191, 8191, 16)
    assert v[3:] == want
    assert C.sizeof(api.PyramidLevel) == 32 and C.sizeof(api.PyramidView) == 8 + 16 * 32
    assert [f[0] for f in api.StereoBatch._fields_][-7:] == ["d_u_right", "d_depth", "d_status", "d_best_r", "d_ham_dist", "d_sad_dist", "d_n_matched"]
    assert len(api.STEREO_STATUS) == 9


def test_the_header_builds_for_the_host_without_the_c_abi(tmp_path):
    """csrc/stereo.h is built without include/slamit.h (by g++ for the tests, by hipcc for the kernels): its constants are the C-ABI's."""
    src = '#include <stdio.h>\n#include "slamit.h"\n#include "stereo.h"\nint main() {\n'
    src += '    printf("%d %d %d %d %d\\n", STEREO_MAX_LEVELS, SLAMIT_MAX_LEVELS, STEREO_TH_HIGH, STEREO_DEPARTURE, STEREO_MEDIAN);\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_st.cc"), str(tmp_path / "_st")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [16, 16, 100, 8, 7]


def test_stereo_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build, synth

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in ("slamit_orb_pyramid_view", "slamit_stereo_match_workspace", "slamit_stereo_match_batch_dev", "slamit_stereo_match"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "stereo.hip" in build.SOURCES and "stereo.hip" not in build.PER_FILE                  # -ffp-contract=off, like the rest
    assert callable(api.stereo_match) and callable(api.stereo_match_batch_dev) and callable(synth.synth_stereo_pair)
    for word in ("DEPARTURES", "8 departure", "SLAMIT_ERR_CAPACITY"):
        assert word in hdr[hdr.index("Stereo matching: Frame::ComputeStereoMatches"):]
