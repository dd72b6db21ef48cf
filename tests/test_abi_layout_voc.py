"""Layout of the vocabulary entry points' struct: a C99 compile of include/slamit.h against the ctypes mirror (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import bow_voc_ref as ref
from tests.helpers import ROOT

NAMES = ("slamit_voc_create", "slamit_voc_load_text", "slamit_voc_destroy", "slamit_voc_info", "slamit_voc_transform",
         "slamit_voc_transform_workspace", "slamit_voc_transform_batch_dev")


def test_voc_struct_layout_matches_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    fields = [f[0] for f in api.VocDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%zu %d %d %d\\n", sizeof(slamit_voc_desc), SLAMIT_VOC_MAX_K, SLAMIT_VOC_MAX_L, SLAMIT_VOC_MAX_FEATURES);\n'
    for f in fields:
        src += '    printf("%%zu\\n", offsetof(slamit_voc_desc, %s));\n' % f
    src += "    return SLAMIT_VOC_MAX_FEATURES == SLAMIT_SEARCH_MAX_KP ? 0 : 1;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == C.sizeof(api.VocDesc)
    assert tuple(v[1:4]) == (api.VOC_MAX_K, api.VOC_MAX_L, api.VOC_MAX_FEATURES) == (20, 10, 8191)
    assert v[4:] == [getattr(api.VocDesc, f).offset for f in fields]


def test_voc_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name), name
    for src in ("voc_pack.cc", "voc.hip"):
        assert src in build.SOURCES and src not in build.PER_FILE   # the default flags: -ffp-contract=off is part of the numerics
    assert api.lib().slamit_voc_transform_workspace(3, 100) >= 3 * 100 * 8


def test_a_bad_vocabulary_is_refused_before_any_device_call():
    """Validation is host work: SLAMIT_ERR_ARG with a message, with or without a GPU."""
    from weiner_slamit_v2_amd import api

    voc = ref.full_tree(3, 2, 7)
    leaf = voc["is_leaf"].copy()
    leaf[0] = 1
    keep = [np.ascontiguousarray(voc["parent"]), leaf, np.ascontiguousarray(voc["desc"]), np.ascontiguousarray(voc["weight"])]
    d = api.VocDesc(3, 2, 0, 0, len(leaf), *[a.ctypes.data for a in keep])
    h = C.c_void_p()
    assert api.lib().slamit_voc_create(C.byref(d), 0, C.byref(h)) == -1 and not h.value
    assert b"is_leaf" in api.lib().slamit_last_error()
    assert api.lib().slamit_voc_load_text(b"/nonexistent/voc.txt", 0, C.byref(h)) == -1 and b"cannot open" in api.lib().slamit_last_error()
