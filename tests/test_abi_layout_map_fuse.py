"""Layout of the map-fuse records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes before a launch
(no GPU); slamit_map_replace_apply still refuses the third kind."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.map_fuse_fixtures import by_name
from tests.map_fuse_host import records

STRUCTS = (("slamit_map_fuse_batch_rec", "MapFuseBatchRec"), ("slamit_fuse_list_batch_rec", "FuseListBatchRec"))
SYMBOLS = ("slamit_map_fuse_apply", "slamit_map_fuse_workspace", "slamit_map_fuse_batch_dev", "slamit_fuse_list_batch_dev")
OUT = ("PLAIN", "NOMATCH", "SKIP_BAD", "SKIP_IN_KF", "ADDED", "OCCUPANT_BAD", "P_REPLACED", "Q_REPLACED")
MACROS = ("SLAMIT_FUSE_FUSE",) + tuple("SLAMIT_FUSE_OUT_" + o for o in OUT) + ("SLAMIT_FUSE_OBS_OVERFLOW", "SLAMIT_FUSE_TABLE_OVERFLOW", "SLAMIT_FUSE_BAD_SLOT",
                                                                              "SLAMIT_FUSE_MAX_OPS")
OP_FIELDS = ("kind", "a", "b", "idx", "octave", "weight", "pad")


def test_map_fuse_struct_layouts_match_the_header(tmp_path):
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
    src += '    printf("%zu %zu %zu %zu\\n", sizeof(slamit_map_index), sizeof(slamit_replace_index), sizeof(slamit_map_replace), sizeof(slamit_kp));\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.FUSE_STATUS
    assert v[:len(MACROS)] == [api.FUSE_FUSE] + [api.FUSE_OUT[o] for o in OUT] + [st["OBS_OVERFLOW"], st["TABLE_OVERFLOW"], st["BAD_SLOT"], api.FUSE_MAX_OPS]
    assert v[len(MACROS):-4] == want
    assert v[-4:] == [120, C.sizeof(api.ReplaceIndexRec), 20, 28] and C.sizeof(api.MapIndexRec) == 120   # the records are taken unchanged
    assert api.FUSE_REFUSED == st["OBS_OVERFLOW"] | st["TABLE_OVERFLOW"] and api.FUSE_MAX_OPS == 16384 and list(api.FUSE_OUT.values()) == list(range(8))
    assert {k: api.REPLACE_STATUS[k] for k in st} == st                 # one reader of a status serves both modules


def test_the_host_statement_has_the_c_abi_constants(tmp_path):
    """csrc/map_fuse.h is built without include/slamit.h: its constants are the header's."""
    pairs = [("MF_FUSE", "SLAMIT_FUSE_FUSE"), ("MF_MAX_OPS", "SLAMIT_FUSE_MAX_OPS")] + [("MF_OUT_" + o, "SLAMIT_FUSE_OUT_" + o) for o in OUT]
    pairs += [("MF_" + n, "SLAMIT_FUSE_" + n) for n in ("OBS_OVERFLOW", "TABLE_OVERFLOW", "BAD_SLOT")]
    src = '#include <stdio.h>\n#include "slamit.h"\n#include "map_fuse.h"\nint main() {\n'
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * len(pairs)


def test_map_fuse_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "map_fuse.hip" in build.SOURCES and "map_fuse.hip" not in build.PER_FILE        # no per-file flags
    for f in ("map_fuse", "map_fuse_batch_dev", "map_fuse_workspace", "fuse_list_batch_dev"):
        assert callable(getattr(api, f))
    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    src, head = open(os.path.join(csrc, "map_fuse.hip")).read(), open(os.path.join(csrc, "map_fuse.h")).read()
    assert "mf_walk_op(" in src and '#include "map_check.h"' in src and '#include "wave_ops.h"' in src and '#include "map_rows_dev.h"' in src
    for text in (src, open(os.path.join(csrc, "map_rows_dev.h")).read()):                   # the file and the shared device header, each on its own
        assert "getenv" not in text and "double" not in text
        assert "while (" not in text.replace("while (lo < hi)", "").replace("while (mask)", "")  # no kernel waits: the bisection and the ballot's bits
        assert "agent" not in text and "__threadfence" not in text and "__syncthreads" not in text  # one wavefront walks a list; no workgroup waits on another
    assert head.count("mr_walk_op(w, ") == 3 and "MrWorldSeq" in head and "push(" not in head.split("mf_apply_seq")[0]   # every outcome resolves into mr_walk_op
    assert api.map_fuse_workspace(1, 0, 0, 0) > 0 and api.map_fuse_workspace(0, 1, 1, 1) == 0 and api.map_fuse_workspace(1, api.FUSE_MAX_OPS + 1, 1, 1) == 0
    # the formula beside the declaration: four rows over the points, three words per op, the image of kf_mp, a working row per involved point
    want = 8 * (4 * 70000 + 4 * 4 * 5001 + 3 * 4 * 1000 + 2000 * (10 * 512 + 32))
    assert want <= api.map_fuse_workspace(8, 1000, 5000, 70000) <= want + 8 * 1024
    # the workspace's bytes, pinned before the rows moved into the shared layout: (n_maps, cap, mp_cap, kfmp_cap) -> bytes
    for dims, bytes_ in (((1, 0, 0, 0), 128), ((1, 1, 1, 1), 5360), ((1, 4, 7, 30), 36448), ((2, 64, 257, 1000), 1336832), ((8, 1000, 5000, 70000), 85409760),
                         ((8, 16384, 255, 3), 12116224)):
        assert api.map_fuse_workspace(*dims) == bytes_, dims


def test_one_definition_is_left():
    """The working-row world, the bisection of the row copy and the column enums stand once among the device sources: map_replace.hip and
    map_fuse.hip run the text of map_rows_dev.h, and MfWorldDev adds only what mf_walk_op asks for beyond mr_walk_op."""
    import glob

    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip"))) + [os.path.join(csrc, "map_rows_dev.h")]
    text = {f: open(f).read() for f in files}
    for once in ("sord[rank] = (uint16_t)e", "while (lo < hi)", "MR_C_LEN = 0, MR_C_BAD, MR_C_NOBS, MR_C_FOUND, MR_C_VISIBLE, MR_C_REPLACED, MR_C_RECEIVED, MR_NCOLS"):
        assert sum(t.count(once) for t in text.values()) == 1, once
        assert once in text[files[-1]], once
    world = text[os.path.join(csrc, "map_fuse.hip")].split("struct MfWorldDev")[1].split("\n};")[0]
    assert "MapWorldDev" in world and "occupant(" in world and "rank" not in world and "__popcll" not in world


def _refused(call, word, code=-1):
    from weiner_slamit_v2_amd import api

    try:
        call()
        raise AssertionError("accepted: " + word)
    except api.SlamitError as e:
        assert "(%d)" % code in str(e) and word in str(e), str(e)


def test_the_existing_entry_point_still_refuses_the_third_kind():
    from weiner_slamit_v2_amd import api

    fx = by_name("outcomes")
    _refused(lambda: api.map_replace(fx["t"], fx["x"], records(fx["ops"][3:4])), "slamit_map_replace_apply: an op's kind outside 1..2")


def test_refusals_need_no_device():
    """Every refusal is made before a launch: the same with and without a GPU, with a message, outputs untouched."""
    from weiner_slamit_v2_amd import api

    fx = by_name("mixed")
    t, x, E = fx["t"], fx["x"], fx["ops"]
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    mf = lambda tables=t, index=x, ops=E, **kw: api.map_fuse(tables, index, records(ops), **kw)
    w = "slamit_map_fuse_apply: "
    for key in ("obs_ptr", "obs_kf", "kf_mp_ptr", "kf_mp", "mp_bad"):
        _refused(lambda: mf(dict(t, **{key: None})) if key != "obs_ptr" else api.map_fuse(dict(t, obs_ptr=None), x, records(E), obs_cap_out=99), w + "null table")
    for key in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_found", "mp_visible", "mp_replaced"):
        _refused(lambda: mf(index=dict(x, **{key: None})), w + "null table")
    _refused(lambda: mf(obs_cap_out=-1), "negative obs_cap_out")
    _refused(lambda: mf(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: mf(dict(t, kf_mp_ptr=t["kf_mp_ptr"][::-1].copy())), "CSR pointer array")
    _refused(lambda: mf(dict(t, obs_ptr=t["obs_ptr"] + 1)), "CSR pointer array")
    _refused(lambda: mf(dict(t, obs_kf=np.where(t["obs_kf"] == 3, n_kf, t["obs_kf"]))), "obs_kf holds a keyframe slot outside")
    _refused(lambda: mf(index=dict(x, obs_idx=np.where(np.arange(len(x["obs_idx"])) == 1, 999, x["obs_idx"]))), "obs_idx holds a keypoint index outside")
    _refused(lambda: mf(index=dict(x, obs_weight=np.where(np.arange(len(x["obs_weight"])) == 2, 3, x["obs_weight"]))), "obs_weight holds a weight other than 1 or 2")
    for v in (n_mp, -2):
        _refused(lambda: mf(dict(t, kf_mp=np.where(np.arange(len(t["kf_mp"])) == 5, v, t["kf_mp"]))), w + "kf_mp holds a point slot outside [-1, n_mp)")
    fuse = next(e for e in E if e[0] == api.FUSE_FUSE and e[3] >= 0)
    one = lambda **kw: [tuple(kw.get(f, v) for f, v in zip(OP_FIELDS, fuse))]
    _refused(lambda: mf(ops=one(kind=0)), "an op's kind outside 1..3")
    _refused(lambda: mf(ops=one(kind=4)), "an op's kind outside 1..3")
    for kind in (api.FUSE_FUSE, api.REPLACE_ADD_OBS):
        _refused(lambda: mf(ops=one(kind=kind, a=n_mp)), "ops holds a point slot outside")
        _refused(lambda: mf(ops=one(kind=kind, a=-1)), "ops holds a point slot outside")
        _refused(lambda: mf(ops=one(kind=kind, b=n_kf)), "ops holds a keyframe slot outside")
        _refused(lambda: mf(ops=one(kind=kind, b=-1)), "ops holds a keyframe slot outside")
        _refused(lambda: mf(ops=one(kind=kind, idx=int(t["kf_mp_ptr"][fuse[2] + 1] - t["kf_mp_ptr"][fuse[2]]))), "ops holds a keypoint index outside")
        _refused(lambda: mf(ops=one(kind=kind, weight=0)), "an op's weight other than 1 or 2")
        _refused(lambda: mf(ops=one(kind=kind, weight=3)), "an op's weight other than 1 or 2")
    _refused(lambda: mf(ops=one(kind=api.REPLACE_ADD_OBS, idx=-1)), "ops holds a keypoint index outside")
    _refused(lambda: mf(ops=one(kind=api.REPLACE_REPLACE, b=n_mp)), "ops holds a point slot outside")
    _refused(lambda: api.map_fuse(t, x, np.zeros(api.FUSE_MAX_OPS + 1, api.REPLACE_DTYPE), obs_cap_out=8), "SLAMIT_FUSE_MAX_OPS", code=-3)
    # a FUSE op without a match is not read further; without a device a valid call fails loudly and says why
    for ops in (one(idx=-1, a=n_mp + 7, b=-9, weight=0), one(idx=-5), E, []):
        if api.device_count() == 0:
            _refused(lambda: mf(ops=ops), "", code=-2)
        else:
            assert mf(ops=ops)["status"] == 0
    # a missing output through the raw entry point: the other outputs and the in-place arrays keep their bytes
    L = api.lib()
    err = lambda: L.slamit_last_error()
    rec, keep = api._map_index_host(t)
    arrs = {k: np.array(v) for k, v in list(x.items()) + [("mp_bad", t["mp_bad"]), ("kf_mp", t["kf_mp"])] if k != "mp_ref_kf"}
    cap = len(t["obs_kf"]) + 8
    outs = {"obs_ptr_out": np.full(n_mp + 1, 77, np.int32), "obs_kf_out": np.full(cap, 77, np.int32), "obs_idx_out": np.full(cap, 77, np.int32),
            "obs_octave_out": np.full(cap, 77, np.uint8), "obs_weight_out": np.full(cap, 77, np.uint8)}
    xrec = api.ReplaceIndexRec(obs_cap_out=cap, **{k: v.ctypes.data for k, v in list(arrs.items()) + list(outs.items())})
    ed = records(E)
    oc, mv, er = (np.full(len(ed), 77, np.int32) for _ in range(3))
    tch, four = np.full(n_mp, 77, np.int32), np.full(4, 77, np.int32)
    p4 = [four[i:].ctypes.data for i in range(4)]
    call = lambda *a: L.slamit_map_fuse_apply(0, *a)
    R, Xr, n, e, o, m, r, tc = C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, oc.ctypes.data, mv.ctypes.data, er.ctypes.data, tch.ctypes.data
    assert call(R, Xr, n, e, o, m, r, tc, p4[0], p4[1], p4[2], None) == -1 and b"slamit_map_fuse_apply: null array" in err()
    assert call(R, Xr, n, e, o, m, r, tc, p4[0], None, p4[2], p4[3]) == -1 and b"null array" in err()
    assert call(R, Xr, n, None, o, m, r, tc, *p4) == -1 and b"null array" in err()
    assert call(R, Xr, n, e, None, m, r, tc, *p4) == -1 and b"null array" in err()
    assert call(R, Xr, n, e, o, None, r, tc, *p4) == -1 and b"null array" in err()
    assert call(R, Xr, n, e, o, m, None, tc, *p4) == -1 and b"null array" in err()
    assert call(R, Xr, -1, e, o, m, r, tc, *p4) == -1 and b"negative n" in err()
    assert call(R, Xr, n, e, o, m, r, None, *p4) == -1 and b"null array" in err()
    assert call(None, Xr, n, e, o, m, r, tc, *p4) == -1 and b"null table" in err()
    assert call(R, None, n, e, o, m, r, tc, *p4) == -1 and b"null table" in err()
    xrec.obs_idx_out = None
    assert call(R, Xr, n, e, o, m, r, tc, *p4) == -1 and b"null table" in err()
    xrec.obs_idx_out = outs["obs_idx_out"].ctypes.data
    ed["a"][1] = n_mp
    assert call(R, Xr, n, e, o, m, r, tc, *p4) == -1 and b"slot outside" in err()
    assert all(np.all(v == 77) for v in (oc, mv, er, tch, four)) and all(np.all(v == 77) for v in outs.values())
    for k, v in arrs.items():
        assert np.array_equal(v, np.asarray(x[k] if k in x else t[k]).reshape(-1)), k
    # the resident form: what the host can see of a batch
    B = api.MapFuseBatchRec()
    bd = lambda: L.slamit_map_fuse_batch_dev(0, C.byref(B), None)
    assert bd() == 0                                                                       # no maps: nothing to do
    B.cap = -1
    assert bd() == -1 and b"slamit_map_fuse_batch_dev: bad argument" in err()
    M, X = (api.MapIndexRec * 9)(*([rec] * 9)), (api.ReplaceIndexRec * 9)(*([xrec] * 9))
    B.cap, B.n_maps, B.maps, B.index, B.mp_cap, B.kfmp_cap = 4, 9, M, X, n_mp, len(t["kf_mp"])
    assert bd() == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()                            # more than eight maps
    B.n_maps, B.cap = 1, api.FUSE_MAX_OPS + 1
    assert bd() == -3 and b"SLAMIT_FUSE_MAX_OPS" in err()
    B.cap, B.mp_cap = 4, n_mp - 1
    assert bd() == -1 and b"n_mp above mp_cap" in err()
    B.mp_cap = n_mp
    assert bd() == -1 and b"null array" in err()                                           # no list arrays
    X[0].obs_cap_out = -1
    assert bd() == -1 and b"negative obs_cap_out" in err()
    X[0].obs_cap_out, X[0].mp_replaced = cap, None
    assert bd() == -1 and b"null table" in err()
    X[0].mp_replaced, M[0].n_kf = xrec.mp_replaced, 65536
    assert bd() == -1 and b"SLAMIT_LOCAL_MAP_MAX_KF" in err()
    M[0].n_kf = n_kf
    one4 = np.zeros(4, np.int32)
    B.d_n = B.d_n_touched = B.d_n_obs_out = B.d_status = B.d_outcome = B.d_moved = B.d_erased = B.d_touched = B.d_ops = one4.ctypes.data
    assert bd() == -1 and b"null array" in err()                                           # d_n_fused
    B.d_n_fused = one4.ctypes.data                                                         # never read: the workspace is missing
    assert bd() == -1 and b"workspace" in err()
    B.d_workspace, B.workspace_bytes = one4.ctypes.data, api.map_fuse_workspace(1, 4, n_mp, len(t["kf_mp"])) - 1
    assert bd() == -1 and b"workspace" in err()
    Q = api.FuseListBatchRec()
    ld = lambda: L.slamit_fuse_list_batch_dev(0, C.byref(Q), None)
    assert ld() == 0                                                                       # no targets: nothing to do
    Q.q_cap = -1
    assert ld() == -1 and b"slamit_fuse_list_batch_dev: bad argument" in err()
    Q.nframes, Q.q_cap, Q.kp_cap, Q.cap = 2, 4, 4, 8
    assert ld() == -1 and b"n_maps outside" in err()
    Q.n_maps = 9
    assert ld() == -1 and b"n_maps outside" in err()
    Q.n_maps, Q.cap = 1, api.FUSE_MAX_OPS + 1
    assert ld() == -3 and b"SLAMIT_FUSE_MAX_OPS" in err()
    Q.cap = 8
    assert ld() == -1 and b"null array" in err()
    Q.d_m = Q.d_match_kp = Q.d_query_point = Q.d_frame_map = Q.d_frame_kf = Q.d_base = Q.d_ops = Q.d_n = Q.d_status = one4.ctypes.data
    assert ld() == -1 and b"null array" in err()                                           # keypoints to read the octave from
    Q.nframes = 65536
    assert ld() == -3 and b"65,535 frames" in err()
    del keep
