"""Layout of the map-point upkeep records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes
before a launch (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.upkeep_fixtures import small_map

STRUCTS = (("slamit_point_index", "PointIndexRec"), ("slamit_points_batch_rec", "PointsBatchRec"), ("slamit_point_culling_batch_rec", "PointCullingBatchRec"))
SYMBOLS = ("slamit_update_points", "slamit_update_points_batch_dev", "slamit_map_point_culling", "slamit_map_point_culling_batch_dev")
MACROS = ("SLAMIT_UPKEEP_REF_NOT_OBSERVER", "SLAMIT_UPKEEP_NO_REF", "SLAMIT_UPKEEP_REF_NO_KP", "SLAMIT_UPKEEP_OCTAVE", "SLAMIT_UPKEEP_DESC_OVERFLOW",
          "SLAMIT_UPKEEP_OBS_OVERFLOW", "SLAMIT_UPKEEP_BAD_SLOT", "SLAMIT_UPKEEP_MAX_OBS", "SLAMIT_UPKEEP_MAX_POINTS", "SLAMIT_UPKEEP_MAX_RECENT",
          "SLAMIT_DISTINCTIVE_MAX", "SLAMIT_UPKEEP_NORMAL", "SLAMIT_UPKEEP_DESC", "SLAMIT_UPKEEP_KEPT", "SLAMIT_UPKEEP_WAS_BAD", "SLAMIT_UPKEEP_LOW_RATIO",
          "SLAMIT_UPKEEP_FEW_OBS", "SLAMIT_UPKEEP_AGED", "SLAMIT_MAX_LEVELS")


def test_upkeep_struct_layouts_match_the_header(tmp_path):
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
    src += '    printf("%zu\\n", sizeof(slamit_map_index));\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.UPKEEP_STATUS
    assert v[:len(MACROS)] == [st[k] for k in ("REF_NOT_OBSERVER", "NO_REF", "REF_NO_KP", "OCTAVE", "DESC_OVERFLOW", "OBS_OVERFLOW", "BAD_SLOT")] + \
        [api.UPKEEP_MAX_OBS, api.UPKEEP_MAX_POINTS, api.UPKEEP_MAX_RECENT, api.DISTINCTIVE_MAX, api.UPKEEP_NORMAL, api.UPKEEP_DESC] + \
        [api.UPKEEP_VERDICTS.index(n) for n in ("kept", "was_bad", "low_ratio", "few_obs", "aged")] + [16]
    assert v[len(MACROS):-1] == want
    assert v[-1] == 120 == C.sizeof(api.MapIndexRec)                                       # the map record keeps its size
    assert [f[0] for f in api.PointIndexRec._fields_][3:] == [name for name, _ in api.POINT_INDEX_TABLES]
    assert set(api.POINT_PLANES) <= {name for name, _ in api.POINT_INDEX_TABLES}


def test_the_host_restatement_has_the_c_abi_record(tmp_path):
    """csrc/upkeep.h is built without include/slamit.h: its UpIndex is slamit_point_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.PointIndexRec._fields_]
    pairs = [("UP_" + n, "SLAMIT_UPKEEP_" + n) for n in ("REF_NOT_OBSERVER", "NO_REF", "REF_NO_KP", "OCTAVE", "DESC_OVERFLOW", "OBS_OVERFLOW", "BAD_SLOT", "MAX_OBS",
                                                         "MAX_POINTS", "MAX_RECENT", "NORMAL", "DESC", "KEPT", "WAS_BAD", "LOW_RATIO", "FEW_OBS", "AGED")]
    pairs += [("UP_MAX_DESC", "SLAMIT_DISTINCTIVE_MAX"), ("UNP_MAX_LEVELS", "SLAMIT_MAX_LEVELS")]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "upkeep.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(UpIndex), sizeof(slamit_point_index));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(UpIndex, %s), offsetof(slamit_point_index, %s));\n' % (f, f)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (len(names) + 1 + len(pairs))


def test_upkeep_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "upkeep.hip" in build.SOURCES and "upkeep.hip" not in build.PER_FILE                  # compiled like unproject.hip: no contraction
    for f in ("update_points", "update_points_batch_dev", "map_point_culling", "map_point_culling_batch_dev", "PointIndex"):
        assert callable(getattr(api, f))
    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    src = open(os.path.join(csrc, "upkeep.hip")).read()
    assert "getenv" not in src and '#include "wave_ops.h"' in src and "wave_inclusive_scan_i32" in src and "DISTINCTIVE_SELECT" in src
    # one selection, shared through a header, stated once
    assert "DISTINCTIVE_SELECT" in open(os.path.join(csrc, "hamming.hip")).read()
    assert sum("while (lo < hi)" in open(os.path.join(csrc, f)).read() for f in ("hamming.hip", "upkeep.hip", "distinctive.h")) == 1
    assert "struct slamit_point_index {" in hdr and "} slamit_point_index;" not in hdr


def _refused(call, word, code=-1):
    from weiner_slamit_v2_amd import api

    try:
        call()
        raise AssertionError("accepted: " + word)
    except api.SlamitError as e:
        assert "(%d)" % code in str(e) and word in str(e), str(e)


def test_refusals_need_no_device():
    """Every refusal is made before a launch: the same with and without a GPU, with a message, outputs untouched."""
    from weiner_slamit_v2_amd import api

    fx = small_map()
    t, x = fx["t"], fx["x"]                                                               # 3 keyframes, 4 points
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    up = lambda tables=t, pts=x, points=(0, 1), what=3: api.update_points(tables, pts, points, what)
    mc = lambda tables=t, pts=x, recent=(0, 1): api.map_point_culling(tables, pts, 5, True, recent)
    w = "slamit_update_points: "
    _refused(lambda: up(dict(t, obs_ptr=None)), w + "null table")
    _refused(lambda: up(dict(t, mp_pos=None)), w + "null table")
    _refused(lambda: up(dict(t, kf_bad=None)), w + "null table")
    _refused(lambda: up(pts=dict(x, kf_center=None)), w + "null table")
    _refused(lambda: up(pts=dict(x, kf_desc=None)), w + "null table")
    _refused(lambda: up(pts=dict(x, mp_desc=None)), w + "null table")
    assert up(pts=dict(x, kf_desc=None, mp_desc=None, obs_idx=None), points=(), what=1)["status"].shape == (0,)   # the other part's tables may be NULL
    _refused(lambda: up(points=(0, n_mp)), "points holds a point slot outside")
    _refused(lambda: up(points=(-1,)), "points holds a point slot outside")
    _refused(lambda: up(dict(t, obs_kf=np.where(t["obs_kf"] == 2, n_kf, t["obs_kf"]))), "obs_kf holds a keyframe slot outside")
    _refused(lambda: up(pts=dict(x, mp_ref_kf=np.array([0, 1, n_kf, 0]))), "mp_ref_kf holds a keyframe slot outside")
    _refused(lambda: up(pts=dict(x, mp_ref_kf=np.array([0, -2, 0, 0]))), "mp_ref_kf holds a keyframe slot outside")
    _refused(lambda: up(pts=dict(x, obs_idx=np.where(np.arange(len(x["obs_idx"])) == 1, 99, x["obs_idx"]))), "obs_idx holds a keypoint index outside")
    _refused(lambda: up(pts=dict(x, n_levels=0)), "n_levels outside [1, SLAMIT_MAX_LEVELS]")
    _refused(lambda: up(pts=dict(x, n_levels=17)), "n_levels outside [1, SLAMIT_MAX_LEVELS]")
    _refused(lambda: up(what=0), "`what` outside 1..3")
    _refused(lambda: up(what=4), "`what` outside 1..3")
    _refused(lambda: up(dict(t, kf_mp_ptr=t["kf_mp_ptr"][::-1].copy())), "CSR pointer array")
    _refused(lambda: up(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: up(points=np.zeros(api.UPKEEP_MAX_POINTS + 1, np.int32)), "SLAMIT_UPKEEP_MAX_POINTS", code=-3)
    w = "slamit_map_point_culling: "
    _refused(lambda: mc(dict(t, mp_bad=None)), w + "null table")
    _refused(lambda: mc(pts=dict(x, mp_visible=None)), w + "null table")
    _refused(lambda: mc(recent=(0, n_mp)), "recent holds a point slot outside")
    _refused(lambda: mc(recent=np.zeros(api.UPKEEP_MAX_RECENT + 1, np.int32)), "SLAMIT_UPKEEP_MAX_RECENT", code=-3)
    # a missing output through the raw entry points: the other outputs and the planes keep their bytes
    L = api.lib()
    err = lambda: L.slamit_last_error()
    rec, keep = api._map_index_host(t)
    xrec, xkeep = api._point_index_host(x, copy_planes=True)
    pts, st = np.array([0, 1], np.int32), np.full(2, 77, np.int32)
    assert L.slamit_update_points(0, C.byref(rec), C.byref(xrec), 2, pts.ctypes.data, 3, None) == -1 and b"slamit_update_points: null array" in err()
    assert L.slamit_update_points(0, None, C.byref(xrec), 2, pts.ctypes.data, 3, st.ctypes.data) == -1 and b"null table" in err()
    assert L.slamit_update_points(0, C.byref(rec), None, 2, pts.ctypes.data, 3, st.ctypes.data) == -1 and b"null table" in err()
    bad = np.array([0, 9], np.int32)
    assert L.slamit_update_points(0, C.byref(rec), C.byref(xrec), 2, bad.ctypes.data, 3, st.ctypes.data) == -1 and b"slot outside" in err()
    v, kp, one = np.full(2, 77, np.uint8), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
    assert L.slamit_map_point_culling(0, C.byref(rec), C.byref(xrec), 5, 1, 2, bad.ctypes.data, v.ctypes.data, kp.ctypes.data, one.ctypes.data,
                                      one[1:].ctypes.data) == -1 and b"slot outside" in err()
    assert L.slamit_map_point_culling(0, C.byref(rec), C.byref(xrec), 5, 1, 2, pts.ctypes.data, v.ctypes.data, kp.ctypes.data, None, one.ctypes.data) == -1
    assert b"slamit_map_point_culling: null array" in err()
    assert np.all(st == 77) and np.all(v == 77) and np.all(kp == 77) and np.all(one == 77)
    for key in api.POINT_PLANES:
        assert np.array_equal(xkeep[key], np.asarray(x[key]).reshape(-1)), key
    # the resident forms: what the host can see of a batch
    B = api.PointsBatchRec()
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == 0                      # no items: nothing to do
    M, X = (api.MapIndexRec * 9)(*([rec] * 9)), (api.PointIndexRec * 9)(*([xrec] * 9))
    B.nitems, B.cap, B.n_maps, B.maps, B.pts = 1, 4, 9, M, X
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()            # more than eight maps
    B.n_maps, B.cap = 1, api.UPKEEP_MAX_POINTS + 1
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -3 and b"SLAMIT_UPKEEP_MAX_POINTS" in err()
    B.cap, B.nitems = api.UPKEEP_MAX_POINTS, 513
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -3 and b"2^25" in err()
    B.cap, B.nitems = 4, 1
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -1 and b"null array" in err()                          # no item arrays
    X[0].n_levels = 17
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -1 and b"n_levels outside" in err()
    X[0].n_levels, X[0].mp_desc = 8, None
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -1 and b"null table" in err()
    X[0].mp_desc = xrec.mp_desc + 4 if xrec.mp_desc % 16 == 0 else xrec.mp_desc - xrec.mp_desc % 16 + 4
    assert L.slamit_update_points_batch_dev(0, C.byref(B), None) == -1 and b"16-byte aligned" in err()
    Q = api.PointCullingBatchRec()
    assert L.slamit_map_point_culling_batch_dev(0, C.byref(Q), None) == 0
    Q.nlists, Q.n_maps, Q.maps, Q.pts, Q.cap = 1, 9, M, X, 4
    assert L.slamit_map_point_culling_batch_dev(0, C.byref(Q), None) == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()
    Q.n_maps, Q.cap = 1, api.UPKEEP_MAX_RECENT + 1
    assert L.slamit_map_point_culling_batch_dev(0, C.byref(Q), None) == -3 and b"SLAMIT_UPKEEP_MAX_RECENT" in err()
    Q.cap = 4
    assert L.slamit_map_point_culling_batch_dev(0, C.byref(Q), None) == -1 and b"null array" in err()
    X[0].mp_found = None
    assert L.slamit_map_point_culling_batch_dev(0, C.byref(Q), None) == -1 and b"null table" in err()
    del keep
