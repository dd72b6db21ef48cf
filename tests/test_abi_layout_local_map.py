"""Layout of the local-map records against their ctypes mirrors, the symbols, and the host forms' refusals (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.local_map_fixtures import fixture

STRUCTS = (("slamit_map_index", "MapIndexRec"), ("slamit_local_map_batch_rec", "LocalMapBatchRec"))
SYMBOLS = ("slamit_local_keyframes", "slamit_local_points", "slamit_local_map_workspace", "slamit_local_map_batch_dev")
MACROS = ("SLAMIT_LOCAL_MAP_BAD_SLOT", "SLAMIT_LOCAL_MAP_KF_OVERFLOW", "SLAMIT_LOCAL_MAP_MP_OVERFLOW", "SLAMIT_LOCAL_MAP_ROW_CUT",
          "SLAMIT_LOCAL_MAP_MAX_KF", "SLAMIT_LOCAL_MAP_MAX_ROW", "SLAMIT_LOCAL_MAP_MIN_KF_CAP", "SLAMIT_LOCAL_MAP_MAX_MAPS", "SLAMIT_LOCAL_MAP_BEST",
          "SLAMIT_FRAME_MAX_KP", "SLAMIT_FRUSTUM_MAX_N")


def test_local_map_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%s\\n", %s);\n' % (" ".join(["%d"] * len(MACROS)), ", ".join(MACROS))
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
    st = api.LOCAL_MAP_STATUS
    assert v[:len(MACROS)] == [st["BAD_SLOT"], st["KF_OVERFLOW"], st["MP_OVERFLOW"], st["ROW_CUT"], api.LOCAL_MAP_MAX_KF, api.LOCAL_MAP_MAX_ROW,
                               api.LOCAL_MAP_MIN_KF_CAP, api.LOCAL_MAP_MAX_MAPS, api.LOCAL_MAP_BEST, api.FRAME_MAX_KP, api.FRUSTUM_MAX_N]
    assert v[len(MACROS):] == want
    assert [f[0] for f in api.MapIndexRec._fields_][2:] == [name for name, _ in api.MAP_INDEX_TABLES]
    # the key of the first-occurrence search has 16 bits for each field
    assert api.LOCAL_MAP_MAX_KF == 2 ** 16 - 1 and api.LOCAL_MAP_MAX_ROW == 2 ** 16 and api.LOCAL_MAP_MIN_KF_CAP == 80 + 3


def test_the_host_restatement_has_the_c_abi_record(tmp_path):
    """csrc/local_map.h is built without include/slamit.h: its LmMap is slamit_map_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.MapIndexRec._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "local_map.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(LmMap), sizeof(slamit_map_index));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(LmMap, %s), offsetof(slamit_map_index, %s));\n' % (f, f)
    for a, b in (("LM_BAD_SLOT", "SLAMIT_LOCAL_MAP_BAD_SLOT"), ("LM_KF_OVERFLOW", "SLAMIT_LOCAL_MAP_KF_OVERFLOW"), ("LM_MP_OVERFLOW", "SLAMIT_LOCAL_MAP_MP_OVERFLOW"),
                 ("LM_ROW_CUT", "SLAMIT_LOCAL_MAP_ROW_CUT"), ("LM_MAX_KF", "SLAMIT_LOCAL_MAP_MAX_KF"), ("LM_MAX_ROW", "SLAMIT_LOCAL_MAP_MAX_ROW"),
                 ("LM_MIN_KF_CAP", "SLAMIT_LOCAL_MAP_MIN_KF_CAP"), ("LM_BEST", "SLAMIT_LOCAL_MAP_BEST")):
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (len(names) + 1 + 8)


def test_local_map_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "local_map.hip" in build.SOURCES and "local_map.hip" not in build.PER_FILE
    for f in ("local_keyframes", "local_points", "local_map_batch_dev", "local_map_workspace", "MapIndex"):
        assert callable(getattr(api, f))
    assert api.local_map_workspace(3, 1000, 96) >= 3 * 1000 * 5 + 3 * 96 * 4 and api.local_map_workspace(0, 10, 96) == 0


def _refused(call, word, code=-1):
    from weiner_slamit_v2_amd import api

    try:
        call()
        raise AssertionError("accepted: " + word)
    except api.SlamitError as e:
        assert "(%d)" % code in str(e) and word in str(e), str(e)


def test_refusals_need_no_device():
    """Every refusal of the host forms is made before a launch: the same with and without a GPU, with a message, outputs untouched."""
    from weiner_slamit_v2_amd import api

    fx = fixture("tie")
    t, fr = fx["maps"][0], fx["frames"][0]
    lk = lambda tables=t, mp=fr["frame_mp"], **kw: api.local_keyframes(tables, mp, **kw)
    lp = lambda tables=t, mp=fr["frame_mp"], kf=(0, 1), **kw: api.local_points(tables, mp, kf, **kw)
    _refused(lambda: lk(mp=[0, 6]), "frame_mp holds a slot outside")                      # n_mp = 6
    _refused(lambda: lk(mp=[-2]), "frame_mp holds a slot outside")
    _refused(lambda: lk(kf_cap=82), "SLAMIT_LOCAL_MAP_MIN_KF_CAP")
    _refused(lambda: lk(kf_cap=65536), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: lk(mp=np.zeros(30001, np.int32)), "SLAMIT_FRAME_MAX_KP")
    _refused(lambda: lk(dict(t, obs_kf=np.where(t["obs_kf"] == 3, 4, t["obs_kf"]))), "keyframe slot outside")
    _refused(lambda: lk(dict(t, kf_parent=np.array([-1, 0, 9, -1], np.int32))), "keyframe slot outside")
    _refused(lambda: lk(dict(t, kf_best=np.full((4, 10), -2, np.int32))), "keyframe slot outside")
    _refused(lambda: lk(dict(t, obs_ptr=t["obs_ptr"][::-1].copy())), "CSR pointer array")
    _refused(lambda: lk(dict(t, kf_bad=None)), "null table")
    _refused(lambda: lk(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: lp(kf=[0, 4]), "local_kf holds a slot outside")
    _refused(lambda: lp(frame_seen=[6]), "point slot outside")
    _refused(lambda: lp(dict(t, kf_mp=np.where(t["kf_mp"] == 5, 6, t["kf_mp"]))), "point slot outside")
    _refused(lambda: lp(q_cap=65537), "SLAMIT_FRUSTUM_MAX_N")
    _refused(lambda: lp(dict(t, kf_mp_ptr=None)), "null table")
    long_row = dict(t, n_kf=1, kf_mp_ptr=np.array([0, 65537], np.int32), kf_mp=np.full(65537, -1, np.int32))
    _refused(lambda: lp(long_row, kf=[0]), "SLAMIT_LOCAL_MAP_MAX_ROW")
    # a missing output through the raw entry point: the other outputs keep their bytes
    rec, keep = api._map_index_host(t)
    mp = np.ascontiguousarray(fr["frame_mp"], np.int32)
    votes, lkf, one = np.full(4, 77, np.int32), np.full(96, 77, np.int32), np.full(3, 77, np.int32)
    rc = api.lib().slamit_local_keyframes(0, C.byref(rec), len(mp), mp.ctypes.data, votes.ctypes.data, 96, lkf.ctypes.data, one[0:].ctypes.data,
                                          one[1:].ctypes.data, None)
    assert rc == -1 and b"null array" in api.lib().slamit_last_error()
    assert np.all(votes == 77) and np.all(lkf == 77) and np.all(one == 77) and np.array_equal(mp, fr["frame_mp"])
    # the resident form: what the host can see of the batch
    B = api.LocalMapBatchRec()
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == 0                  # no frames: nothing to do
    B.nframes, B.n_maps = 1, 9
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in api.lib().slamit_last_error()
    M = (api.MapIndexRec * 1)(rec)
    B.n_maps, B.maps, B.kf_cap = 1, M, 40
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == -1 and b"kf_cap" in api.lib().slamit_last_error()
    B.kf_cap, B.vote_cap, B.mp_cap = 96, 3, 6
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == -1 and b"n_kf above vote_cap" in api.lib().slamit_last_error()
    B.vote_cap = 4
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == -1 and b"null array" in api.lib().slamit_last_error()   # no frame arrays
    M[0].mp_pos = None
    assert api.lib().slamit_local_map_batch_dev(0, C.byref(B), None) == -1 and b"null table" in api.lib().slamit_last_error()   # the gather reads it
    del keep
