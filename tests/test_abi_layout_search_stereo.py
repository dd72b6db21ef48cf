"""The C-ABI of the stereo gate: the two new structs as a C99 compiler lays them out against the ctypes mirrors, the enum, the four
symbols declared / exported / present, and every struct that existed before at the size it had."""
import ctypes as C
import os
import subprocess
import tempfile

from weiner_slamit_v2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slamit.h")
NEW_SYMBOLS = ("slamit_guided_search_stereo", "slamit_guided_search_stereo_batch_dev", "slamit_project_batch_stereo", "slamit_project_batch_dev_stereo")

# sizeof of every struct of include/slamit.h at the parent commit (x86-64, gcc -std=c99)
PARENT_SIZES = {
    "slamit_kp": 28, "slamit_orb_params": 32, "slamit_pyramid_level": 32, "slamit_pyramid_view": 520, "slamit_frame_view": 56,
    "slamit_search_queries": 56, "slamit_search_rule": 84, "slamit_bow_groups": 40, "slamit_bow_rule": 216, "slamit_voc_desc": 56,
    "slamit_camera": 36, "slamit_search_batch": 120, "slamit_ba_problem": 96, "slamit_ba_opts": 48, "slamit_ba_stats": 1304,
    "slamit_ba_result": 48, "slamit_ba_profile_out": 56, "slamit_pose_problem": 64, "slamit_pose_result": 72, "slamit_sim3_problem": 240,
    "slamit_sim3_result": 144, "slamit_sim3_ransac_problem": 88, "slamit_sim3_ransac_result": 24, "slamit_triangulate_problem": 224,
    "slamit_triangulate_result": 24, "slamit_frustum_frame": 176, "slamit_frustum_problem": 224, "slamit_frustum_result": 72,
    "slamit_frustum_batch_rec": 136, "slamit_project_camera": 224, "slamit_project_problem": 280, "slamit_project_result": 64,
    "slamit_project_batch_rec": 136, "slamit_rotation_batch": 80, "slamit_stereo_batch": 1208,
}


def _c99(body):
    d = tempfile.mkdtemp(prefix="abi_search_stereo_")
    src, exe = os.path.join(d, "a.c"), os.path.join(d, "a")
    open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include "slamit.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    return subprocess.check_output([exe]).decode().split()


def test_new_structs_match_the_ctypes_mirrors():
    lines = []
    for cname, mirror in (("slamit_search_stereo", api.SearchStereo), ("slamit_search_stereo_dev", api.SearchStereoDev)):
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        for field, _ in mirror._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
    got = [int(x) for x in _c99("\n".join(lines))]
    want = []
    for mirror in (api.SearchStereo, api.SearchStereoDev):
        want.append(C.sizeof(mirror))
        want += [getattr(mirror, f).offset for f, _ in mirror._fields_]
    assert got == want
    assert C.sizeof(api.SearchStereo) == 32 and C.sizeof(api.SearchStereoDev) == 32   # 4 + 4 + 8 + 8 + 4, padded to the pointers' 8


def test_enum_values():
    got = _c99('printf("%d %d %d\\n", SLAMIT_SEARCH_ER_NONE, SLAMIT_SEARCH_ER_RADIUS, SLAMIT_SEARCH_ER_CHI2);')
    assert [int(x) for x in got] == [0, 1, 2] == [api.SEARCH_ER_NONE, api.SEARCH_ER_RADIUS, api.SEARCH_ER_CHI2]


def test_symbols_declared_exported_present():
    text = open(HEADER).read()
    for s in NEW_SYMBOLS:
        assert "int %s(" % s in text, s
        assert s in api.EXPORTS, s
    if os.path.exists(api.LIB_PATH):   # built: the dynamic symbol table has them
        names = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
        for s in NEW_SYMBOLS:
            assert " T %s\n" % s in names, s
    # a C99 translation unit can name them with the declared types
    _c99("\n".join("(void)%s;" % s for s in NEW_SYMBOLS))


def test_existing_structs_keep_their_sizes():
    """the parent's numbers, compiled in: a _Static_assert per struct fails the build if one changed; and the header still has every
    struct the parent had, and the two new ones besides"""
    import re

    body = "\n".join('_Static_assert(sizeof(%s) == %d, "%s changed size");' % (name, size, name) for name, size in PARENT_SIZES.items())
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=('#include "slamit.h"\n' + body + "\n").encode(), check=True)
    declared = set(re.findall(r"^} (slamit_[a-z0-9_]+);", open(HEADER).read(), re.M))
    assert declared == set(PARENT_SIZES) | {"slamit_search_stereo", "slamit_search_stereo_dev"}
    assert PARENT_SIZES["slamit_project_camera"] == 224 and PARENT_SIZES["slamit_frustum_frame"] == 176
    assert C.sizeof(api.ProjectCamera) == 224 and C.sizeof(api.FrustumFrame) == 176
    assert [f for f, _ in api.ProjectResult._fields_] == ["status", "proj", "level", "uvr", "level_min", "level_max", "valid", "n_valid"]
