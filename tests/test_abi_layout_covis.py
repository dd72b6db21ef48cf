"""Layout of the covisibility records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes before a
launch (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.covis_fixtures import fixture
from tests.helpers import ROOT

STRUCTS = (("slamit_covis_index", "CovisIndexRec"), ("slamit_covis_batch_rec", "CovisBatchRec"), ("slamit_culling_batch_rec", "CullingBatchRec"))
SYMBOLS = ("slamit_update_connections", "slamit_update_connections_batch_dev", "slamit_keyframe_culling", "slamit_keyframe_culling_batch_dev")
MACROS = ("SLAMIT_COVIS_NO_OBSERVER", "SLAMIT_COVIS_ROW_OVERFLOW", "SLAMIT_COVIS_BAD_SLOT", "SLAMIT_COVIS_MAX_ROW", "SLAMIT_COVIS_TH", "SLAMIT_COVIS_KEPT",
          "SLAMIT_COVIS_CULLED", "SLAMIT_COVIS_TO_BE_ERASED", "SLAMIT_COVIS_ORIGIN", "SLAMIT_LOCAL_MAP_MAX_MAPS", "SLAMIT_LOCAL_MAP_BEST")


def test_covis_struct_layouts_match_the_header(tmp_path):
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
    st = api.COVIS_STATUS
    assert v[:len(MACROS)] == [st["NO_OBSERVER"], st["ROW_OVERFLOW"], st["BAD_SLOT"], api.COVIS_MAX_ROW, api.COVIS_TH] + \
        [api.COVIS_VERDICTS.index(n) for n in ("kept", "culled", "to_be_erased", "origin")] + [api.LOCAL_MAP_MAX_MAPS, api.LOCAL_MAP_BEST]
    assert v[len(MACROS):-1] == want
    assert v[-1] == 120 == C.sizeof(api.MapIndexRec)                                       # the map record keeps its size
    assert [f[0] for f in api.CovisIndexRec._fields_][2:] == [name for name, _ in api.COVIS_INDEX_TABLES]
    assert api.COVIS_TH == 15 and api.COVIS_MAX_ROW == 1024


def test_the_host_restatement_has_the_c_abi_record(tmp_path):
    """csrc/covis.h is built without include/slamit.h: its CvIndex is slamit_covis_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.CovisIndexRec._fields_]
    pairs = (("CV_NO_OBSERVER", "SLAMIT_COVIS_NO_OBSERVER"), ("CV_ROW_OVERFLOW", "SLAMIT_COVIS_ROW_OVERFLOW"), ("CV_BAD_SLOT", "SLAMIT_COVIS_BAD_SLOT"),
             ("CV_MAX_ROW", "SLAMIT_COVIS_MAX_ROW"), ("CV_TH", "SLAMIT_COVIS_TH"), ("CV_KEPT", "SLAMIT_COVIS_KEPT"), ("CV_CULLED", "SLAMIT_COVIS_CULLED"),
             ("CV_TO_BE_ERASED", "SLAMIT_COVIS_TO_BE_ERASED"), ("CV_ORIGIN", "SLAMIT_COVIS_ORIGIN"))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "covis.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(CvIndex), sizeof(slamit_covis_index));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(CvIndex, %s), offsetof(slamit_covis_index, %s));\n' % (f, f)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (len(names) + 1 + len(pairs))


def test_covis_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "covis.hip" in build.SOURCES and "covis.hip" not in build.PER_FILE
    for f in ("update_connections", "update_connections_batch_dev", "keyframe_culling", "keyframe_culling_batch_dev", "CovisIndex"):
        assert callable(getattr(api, f))
    src = open(os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc", "covis.hip")).read()
    assert "getenv" not in src and '#include "wave_ops.h"' in src and "wave_min_u64" in src and "wave_inclusive_scan_i32" in src


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

    fx = fixture("uc", "tie_below")
    t, x = fx["t"], fx["x"]                                                               # 6 keyframes, 14 points
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    uc = lambda tables=t, covis=x, k=2: api.update_connections(tables, covis, k)
    kc = lambda tables=t, covis=x, c=2, mono=True: api.keyframe_culling(tables, covis, c, mono)
    for call, what in ((uc, "slamit_update_connections"), (kc, "slamit_keyframe_culling")):
        _refused(lambda: call(dict(t, obs_ptr=None)), what + ": null table")
        _refused(lambda: call(dict(t, kf_mp=None)), what + ": null table")
        _refused(lambda: call(covis=dict(x, ord_kf=None)), what + ": null table")
        _refused(lambda: call(t, x, n_kf), "the keyframe is a slot outside")
        _refused(lambda: call(t, x, -1), "the keyframe is a slot outside")
        _refused(lambda: call(dict(t, obs_kf=np.where(t["obs_kf"] == 3, n_kf, t["obs_kf"]))), "obs_kf holds a keyframe slot outside")
        _refused(lambda: call(dict(t, kf_mp=np.where(t["kf_mp"] == 5, n_mp, t["kf_mp"]))), "kf_mp holds a point slot outside")
        _refused(lambda: call(covis=dict(x, origin_kf=n_kf)), "origin_kf is a slot outside")
        _refused(lambda: call(covis=dict(x, row_cap=1025)), "SLAMIT_COVIS_MAX_ROW")
        _refused(lambda: call(covis=dict(x, row_cap=0)), "SLAMIT_COVIS_MAX_ROW")
        _refused(lambda: call(dict(t, kf_mp_ptr=t["kf_mp_ptr"][::-1].copy())), "CSR pointer array")
        _refused(lambda: call(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: uc(covis=dict(x, cw_n=None)), "null table")
    _refused(lambda: kc(covis=dict(x, kf_depth=None), mono=False), "kf_depth or kf_th_depth NULL with monocular == 0")
    _refused(lambda: kc(covis=dict(x, kf_th_depth=None), mono=False), "kf_depth or kf_th_depth NULL with monocular == 0")
    _refused(lambda: kc(covis=dict(x, mp_nobs=None)), "null table")
    _refused(lambda: kc(covis=dict(x, ord_kf=np.where(x["ord_kf"] == 3, n_kf, x["ord_kf"]), ord_n=np.where(np.arange(n_kf) == 2, 1, x["ord_n"]))),
             "the candidates hold a keyframe slot outside")
    # a missing output through the raw entry points: the other outputs and the graph keep their bytes
    rec, keep = api._map_index_host(t)
    xrec, xkeep = api._covis_index_host(x, copy_graph=True)
    counts, one = np.full(n_kf, 77, np.int32), np.full(4, 77, np.int32)
    rc = api.lib().slamit_update_connections(0, C.byref(rec), C.byref(xrec), 2, 0, counts.ctypes.data, one[0:].ctypes.data, one[1:].ctypes.data,
                                             one[2:].ctypes.data, None)
    assert rc == -1 and b"slamit_update_connections: null array" in api.lib().slamit_last_error()
    xbad = api.CovisIndexRec.from_buffer_copy(xrec)
    xbad.row_cap = 2000
    rc2 = api.lib().slamit_update_connections(0, C.byref(rec), C.byref(xbad), 2, 0, counts.ctypes.data, one[0:].ctypes.data, one[1:].ctypes.data,
                                              one[2:].ctypes.data, one[3:].ctypes.data)
    assert rc2 == -1 and b"SLAMIT_COVIS_MAX_ROW" in api.lib().slamit_last_error()
    v, nm = np.full(16, 77, np.uint8), np.full(16, 77, np.int32)
    tb = np.full(n_mp, 77, np.uint8)
    rc3 = api.lib().slamit_keyframe_culling(0, C.byref(rec), C.byref(xrec), 99, 1, v.ctypes.data, nm.ctypes.data, nm.ctypes.data, one.ctypes.data,
                                            tb.ctypes.data, one[1:].ctypes.data)
    assert rc3 == -1 and b"slot outside" in api.lib().slamit_last_error()
    assert np.all(counts == 77) and np.all(one == 77) and np.all(v == 77) and np.all(nm == 77) and np.all(tb == 77)
    for key in ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best"):
        assert np.array_equal(xkeep[key], np.asarray(x[key]).reshape(-1)), key
    # the resident forms: what the host can see of a batch
    L = api.lib()
    err = lambda: L.slamit_last_error()
    B = api.CovisBatchRec()
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == 0                 # no items: nothing to do
    M, X = (api.MapIndexRec * 9)(*([rec] * 9)), (api.CovisIndexRec * 9)(*([xrec] * 9))
    B.nitems, B.n_maps, B.maps, B.covis = 1, 9, M, X
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()       # more than eight maps
    B.n_maps, B.nitems, B.item_map, B.count_cap = 2, 2, (C.c_int32 * 2)(1, 1), n_kf
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"named twice" in err()                    # a repeated map
    B.item_map = (C.c_int32 * 2)(0, 2)
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"outside [0, n_maps)" in err()
    B.n_maps, B.nitems = 1, 2
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"one item per map" in err()
    B.nitems, B.item_map, B.count_cap = 1, (C.c_int32 * 1)(0), n_kf - 1
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"n_kf above count_cap" in err()
    B.count_cap = n_kf
    X[0].row_cap = 1025
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"SLAMIT_COVIS_MAX_ROW" in err()
    X[0].row_cap = 16
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"null array" in err()                     # no item arrays
    X[0].cw_w = None
    assert L.slamit_update_connections_batch_dev(0, C.byref(B), None) == -1 and b"null table" in err()
    Q = api.CullingBatchRec()
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == 0
    Q.nprob, Q.n_maps, Q.maps, Q.covis, Q.cand_cap, Q.mp_cap = 1, 9, M, X, 16, n_mp
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()
    Q.n_maps, Q.cand_cap = 1, 1025
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"SLAMIT_COVIS_MAX_ROW" in err()
    Q.cand_cap = 15
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"row_cap outside [1, cand_cap]" in err()
    Q.cand_cap, Q.mp_cap = 16, n_mp - 1
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"n_mp above mp_cap" in err()
    Q.mp_cap = n_mp
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"null array" in err()
    X[0].kf_th_depth = None                                                                # kf_depth without its thresholds
    assert L.slamit_keyframe_culling_batch_dev(0, C.byref(Q), None) == -1 and b"null table" in err()
    del keep
