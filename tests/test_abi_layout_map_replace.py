"""Layout of the map-replace records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes before a
launch (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.map_replace_fixtures import by_name
from tests.map_replace_host import REPLACE_DTYPE, records

STRUCTS = (("slamit_replace_index", "ReplaceIndexRec"), ("slamit_map_replace_batch_rec", "MapReplaceBatchRec"), ("slamit_check_replaced_batch_rec", "CheckReplacedBatchRec"))
SYMBOLS = ("slamit_map_replace_apply", "slamit_map_replace_workspace", "slamit_map_replace_batch_dev", "slamit_check_replaced", "slamit_check_replaced_batch_dev")
MACROS = ("SLAMIT_REPLACE_REPLACE", "SLAMIT_REPLACE_ADD_OBS", "SLAMIT_REPLACE_OP_OVERFLOW", "SLAMIT_REPLACE_OBS_OVERFLOW", "SLAMIT_REPLACE_TABLE_OVERFLOW",
          "SLAMIT_REPLACE_BAD_SLOT", "SLAMIT_REPLACE_MAX_OPS", "SLAMIT_REPLACE_MAX_PER_POINT", "SLAMIT_CHECK_REPLACED_MAX_N", "SLAMIT_UPKEEP_MAX_OBS")
OP_FIELDS = ("kind", "a", "b", "idx", "octave", "weight", "pad")
WORKSPACE_BYTES = (((1, 0, 0, 0), 144), ((1, 1, 1, 1), 5408), ((1, 4, 7, 30), 36672), ((2, 64, 257, 1000), 1350992), ((8, 1000, 5000, 70000), 88097792),
                   ((8, 16384, 255, 3), 14229824))


def test_map_replace_struct_layouts_match_the_header(tmp_path):
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
    src += '    printf("%zu\\n", sizeof(slamit_map_replace));\n'
    want.append(api.REPLACE_DTYPE.itemsize)
    for f in OP_FIELDS:
        src += '    printf("%%zu\\n", offsetof(slamit_map_replace, %s));\n' % f
        want.append(api.REPLACE_DTYPE.fields[f][1])
    src += '    printf("%zu %zu %zu\\n", sizeof(slamit_map_index), sizeof(slamit_edit_index), sizeof(slamit_map_edit));\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.REPLACE_STATUS
    assert v[:len(MACROS)] == [api.REPLACE_REPLACE, api.REPLACE_ADD_OBS] + [st[k] for k in ("OP_OVERFLOW", "OBS_OVERFLOW", "TABLE_OVERFLOW", "BAD_SLOT")] + \
        [api.REPLACE_MAX_OPS, api.REPLACE_MAX_PER_POINT, api.CHECK_REPLACED_MAX_N, api.UPKEEP_MAX_OBS]
    assert v[len(MACROS):-3] == want
    assert v[-3:] == [120, C.sizeof(api.EditIndexRec), 24] and C.sizeof(api.MapIndexRec) == 120   # no existing record changes
    assert api.REPLACE_DTYPE == REPLACE_DTYPE and api.REPLACE_DTYPE.itemsize == 20 and api.REPLACE_MAX_OPS == 16384 and api.REPLACE_MAX_PER_POINT == 64
    assert api.REPLACE_REFUSED == st["OP_OVERFLOW"] | st["OBS_OVERFLOW"] | st["TABLE_OVERFLOW"]
    names = [f[0] for f in api.ReplaceIndexRec._fields_]
    assert names[:3] == [k for k, _ in api.EDIT_INDEX_COLUMNS] and names[3:9] == [k for k, _ in api.REPLACE_INDEX_INPLACE]
    assert names[9] == "obs_ptr_out" and names[10:14] == [k for k, _ in api.EDIT_INDEX_OUT]


def test_the_host_statement_has_the_c_abi_record(tmp_path):
    """csrc/map_replace.h is built without include/slamit.h: its MrOp / MrIndex are slamit_map_replace / slamit_replace_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.ReplaceIndexRec._fields_]
    pairs = [("MR_" + n, "SLAMIT_REPLACE_" + n) for n in ("REPLACE", "ADD_OBS", "OP_OVERFLOW", "OBS_OVERFLOW", "TABLE_OVERFLOW", "BAD_SLOT", "MAX_OPS", "MAX_PER_POINT")]
    pairs += [("MR_MAX_OBS", "SLAMIT_UPKEEP_MAX_OBS")]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "map_replace.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(MrIndex), sizeof(slamit_replace_index));\n    printf("%zu %zu\\n", sizeof(MrOp), sizeof(slamit_map_replace));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(MrIndex, %s), offsetof(slamit_replace_index, %s));\n' % (f, f)
    for f in OP_FIELDS:
        src += '    printf("%%zu %%zu\\n", offsetof(MrOp, %s), offsetof(slamit_map_replace, %s));\n' % (f, f)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (2 + len(names) + len(OP_FIELDS) + len(pairs))


def test_map_replace_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "map_replace.hip" in build.SOURCES and "map_replace.hip" not in build.PER_FILE     # nothing is float: no per-file flags
    for f in ("map_replace", "map_replace_batch_dev", "map_replace_workspace", "ReplaceIndex", "replace_records", "check_replaced", "check_replaced_batch_dev"):
        assert callable(getattr(api, f))
    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    src, rows = open(os.path.join(csrc, "map_replace.hip")).read(), open(os.path.join(csrc, "map_rows_dev.h")).read()
    assert '#include "map_rows_dev.h"' in src
    for text in (src, rows):                                                                  # the file and the shared device header, each on its own
        assert "getenv" not in text and "float" not in text.replace("Nothing here is float", "") and "double" not in text
        assert "while (" not in text.replace("while (lo < hi)", "").replace("while (mask)", "")   # no kernel waits: the bisection and the ballot's bits
        assert "agent" not in text and "__threadfence" not in text                            # workgroup scope only
    assert '#include "wave_ops.h"' in src and "wave_inclusive_scan_i32" in rows and "mr_walk_op(" in src and '#include "map_edit' not in src
    assert "round < n" in src                                                                 # the round loop is bounded by n
    assert "struct slamit_replace_index {" in hdr and "struct slamit_map_replace {" in hdr
    # the workspace's bytes, pinned before the rows moved into the shared layout: (n_maps, cap, mp_cap, kfmp_cap) -> bytes
    for dims, want in WORKSPACE_BYTES:
        assert api.map_replace_workspace(*dims) == want, dims
    assert api.map_replace_workspace(1, 0, 0, 0) > 0 and api.map_replace_workspace(0, 1, 1, 1) == 0 and api.map_replace_workspace(1, api.REPLACE_MAX_OPS + 1, 1, 1) == 0
    # the formula beside the declaration: the kf_mp words, six rows over the points, seven per op, a working row per involved point
    assert api.map_replace_workspace(8, 1000, 5000, 70000) >= 8 * (8 * 70000 + 6 * 4 * 5001 + 7 * 4 * 1000 + 2000 * (10 * 512 + 32))
    assert api.map_replace_workspace(8, 1000, 5000, 70000) <= 8 * (8 * 70000 + 6 * 4 * 5001 + 7 * 4 * 1000 + 2000 * (10 * 512 + 32)) + 8 * 1024


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

    fx = by_name("add_order")
    t, x, E = fx["t"], fx["x"], fx["ops"]
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    mr = lambda tables=t, index=x, ops=E, **kw: api.map_replace(tables, index, records(ops), **kw)
    w = "slamit_map_replace_apply: "
    for key in ("obs_ptr", "obs_kf", "kf_mp_ptr", "kf_mp", "mp_bad"):
        _refused(lambda: mr(dict(t, **{key: None})) if key != "obs_ptr" else api.map_replace(dict(t, obs_ptr=None), x, records(E), obs_cap_out=99), w + "null table")
    for key in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_found", "mp_visible", "mp_replaced"):
        _refused(lambda: mr(index=dict(x, **{key: None})), w + "null table")
    _refused(lambda: mr(obs_cap_out=-1), "negative obs_cap_out")
    _refused(lambda: mr(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: mr(dict(t, kf_mp_ptr=t["kf_mp_ptr"][::-1].copy())), "CSR pointer array")
    _refused(lambda: mr(dict(t, obs_ptr=t["obs_ptr"] + 1)), "CSR pointer array")
    _refused(lambda: mr(dict(t, obs_kf=np.where(t["obs_kf"] == 3, n_kf, t["obs_kf"]))), "obs_kf holds a keyframe slot outside")
    _refused(lambda: mr(index=dict(x, obs_idx=np.where(np.arange(len(x["obs_idx"])) == 1, 999, x["obs_idx"]))), "obs_idx holds a keypoint index outside")
    _refused(lambda: mr(index=dict(x, obs_weight=np.where(np.arange(len(x["obs_weight"])) == 2, 3, x["obs_weight"]))), "obs_weight holds a weight other than 1 or 2")
    add = next(e for e in E if e[0] == api.REPLACE_ADD_OBS)
    one = lambda **kw: [tuple(kw.get(f, v) for f, v in zip(OP_FIELDS, add))]
    _refused(lambda: mr(ops=one(kind=0)), "an op's kind outside 1..2")
    _refused(lambda: mr(ops=one(kind=3)), "an op's kind outside 1..2")
    _refused(lambda: mr(ops=one(a=n_mp)), "ops holds a point slot outside")
    _refused(lambda: mr(ops=one(a=-1)), "ops holds a point slot outside")
    _refused(lambda: mr(ops=one(kind=api.REPLACE_REPLACE, b=n_mp)), "ops holds a point slot outside")
    _refused(lambda: mr(ops=one(kind=api.REPLACE_REPLACE, b=-1)), "ops holds a point slot outside")
    _refused(lambda: mr(ops=one(b=n_kf)), "ops holds a keyframe slot outside")
    _refused(lambda: mr(ops=one(idx=int(t["kf_mp_ptr"][add[2] + 1] - t["kf_mp_ptr"][add[2]]))), "ops holds a keypoint index outside")
    _refused(lambda: mr(ops=one(idx=-1)), "ops holds a keypoint index outside")
    _refused(lambda: mr(ops=one(weight=0)), "an op's weight other than 1 or 2")
    _refused(lambda: mr(ops=one(weight=3)), "an op's weight other than 1 or 2")
    _refused(lambda: api.map_replace(t, x, np.zeros(api.REPLACE_MAX_OPS + 1, api.REPLACE_DTYPE), obs_cap_out=8), "SLAMIT_REPLACE_MAX_OPS", code=-3)
    _refused(lambda: api.check_replaced(x["mp_replaced"], [0, n_mp]), "frame_mp holds a point slot outside")
    _refused(lambda: api.check_replaced(x["mp_replaced"], [-2]), "frame_mp holds a point slot outside")
    _refused(lambda: api.check_replaced(x["mp_replaced"], np.zeros(api.CHECK_REPLACED_MAX_N + 1, np.int32)), "SLAMIT_CHECK_REPLACED_MAX_N", code=-3)
    # what a REPLACE does not read is not checked; without a device a valid call fails loudly and says why
    for ops in (one(kind=api.REPLACE_REPLACE, b=1, idx=-5, weight=9), E, []):
        if api.device_count() == 0:
            _refused(lambda: mr(ops=ops), "", code=-2)
        else:
            assert mr(ops=ops)["status"] == 0
    # a missing output through the raw entry point: the other outputs and the in-place arrays keep their bytes
    L = api.lib()
    err = lambda: L.slamit_last_error()
    rec, keep = api._map_index_host(t)
    arrs = {k: np.array(v) for k, v in list(x.items()) + [("mp_bad", t["mp_bad"]), ("kf_mp", t["kf_mp"])] if k != "mp_ref_kf"}
    cap = len(t["obs_kf"]) + 4
    outs = {"obs_ptr_out": np.full(n_mp + 1, 77, np.int32), "obs_kf_out": np.full(cap, 77, np.int32), "obs_idx_out": np.full(cap, 77, np.int32),
            "obs_octave_out": np.full(cap, 77, np.uint8), "obs_weight_out": np.full(cap, 77, np.uint8)}
    xrec = api.ReplaceIndexRec(obs_cap_out=cap, **{k: v.ctypes.data for k, v in list(arrs.items()) + list(outs.items())})
    ed = records(E)
    mv, er, tch, three = np.full(len(ed), 77, np.int32), np.full(len(ed), 77, np.int32), np.full(n_mp, 77, np.int32), np.full(3, 77, np.int32)
    p3 = [three[i:].ctypes.data for i in range(3)]
    call = lambda *a: L.slamit_map_replace_apply(0, *a)
    R, Xr, n, e, m, r, tc = C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, mv.ctypes.data, er.ctypes.data, tch.ctypes.data
    assert call(R, Xr, n, e, m, r, tc, p3[0], p3[1], None) == -1 and b"slamit_map_replace_apply: null array" in err()
    assert call(R, Xr, n, None, m, r, tc, *p3) == -1 and b"null array" in err()
    assert call(R, Xr, n, e, None, r, tc, *p3) == -1 and b"null array" in err()
    assert call(R, Xr, n, e, m, None, tc, *p3) == -1 and b"null array" in err()
    assert call(R, Xr, -1, e, m, r, tc, *p3) == -1 and b"negative n" in err()
    assert call(R, Xr, n, e, m, r, None, *p3) == -1 and b"null array" in err()
    assert call(None, Xr, n, e, m, r, tc, *p3) == -1 and b"null table" in err()
    assert call(R, None, n, e, m, r, tc, *p3) == -1 and b"null table" in err()
    xrec.obs_idx_out = None
    assert call(R, Xr, n, e, m, r, tc, *p3) == -1 and b"null table" in err()
    xrec.obs_idx_out = outs["obs_idx_out"].ctypes.data
    ed["a"][3] = n_mp
    assert call(R, Xr, n, e, m, r, tc, *p3) == -1 and b"slot outside" in err()
    assert np.all(mv == 77) and np.all(er == 77) and np.all(tch == 77) and np.all(three == 77) and all(np.all(v == 77) for v in outs.values())
    for k, v in arrs.items():
        assert np.array_equal(v, np.asarray(x[k] if k in x else t[k]).reshape(-1)), k
    # the resident form: what the host can see of a batch
    B = api.MapReplaceBatchRec()
    bd = lambda: L.slamit_map_replace_batch_dev(0, C.byref(B), None)
    assert bd() == 0                                                                       # no maps: nothing to do
    B.cap = -1
    assert bd() == -1 and b"slamit_map_replace_batch_dev: bad argument" in err()
    M, X = (api.MapIndexRec * 9)(*([rec] * 9)), (api.ReplaceIndexRec * 9)(*([xrec] * 9))
    B.cap, B.n_maps, B.maps, B.index, B.mp_cap, B.kfmp_cap = 4, 9, M, X, n_mp, len(t["kf_mp"])
    assert bd() == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()                            # more than eight maps
    B.n_maps, B.cap = 1, api.REPLACE_MAX_OPS + 1
    assert bd() == -3 and b"SLAMIT_REPLACE_MAX_OPS" in err()
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
    B.d_n = B.d_n_touched = B.d_n_obs_out = B.d_status = B.d_moved = B.d_erased = B.d_touched = B.d_ops = one4.ctypes.data   # never read: the workspace is missing
    assert bd() == -1 and b"workspace" in err()
    B.d_workspace, B.workspace_bytes = one4.ctypes.data, api.map_replace_workspace(1, 4, n_mp, len(t["kf_mp"])) - 1
    assert bd() == -1 and b"workspace" in err()
    Q = api.CheckReplacedBatchRec()
    cd = lambda: L.slamit_check_replaced_batch_dev(0, C.byref(Q), None)
    assert cd() == 0                                                                       # no frames: nothing to do
    Q.nframes, Q.cap = 1, 4
    assert cd() == -1 and b"slamit_check_replaced_batch_dev: n_maps outside" in err()
    Q.n_maps, Q.n_mp, Q.d_mp_replaced = 1, (C.c_int32 * 1)(n_mp), (C.c_void_p * 1)(None)
    assert cd() == -1 and b"no mp_replaced" in err()
    Q.d_mp_replaced = (C.c_void_p * 1)(one4.ctypes.data)
    assert cd() == -1 and b"null array" in err()
    Q.cap = api.CHECK_REPLACED_MAX_N + 1
    assert cd() == -3 and b"SLAMIT_CHECK_REPLACED_MAX_N" in err()
    del keep
