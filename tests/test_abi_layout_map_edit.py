"""Layout of the map-edit records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes before a
launch (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.map_edit_fixtures import by_name
from tests.map_edit_host import EDIT_DTYPE, records

STRUCTS = (("slamit_edit_index", "EditIndexRec"), ("slamit_map_edit_batch_rec", "MapEditBatchRec"))
SYMBOLS = ("slamit_map_edit_apply", "slamit_map_edit_workspace", "slamit_map_edit_batch_dev")
MACROS = ("SLAMIT_EDIT_ADD_OBS", "SLAMIT_EDIT_ERASE_OBS", "SLAMIT_EDIT_SET_BAD", "SLAMIT_EDIT_MATCH", "SLAMIT_EDIT_REF_END", "SLAMIT_EDIT_EDIT_OVERFLOW",
          "SLAMIT_EDIT_OBS_OVERFLOW", "SLAMIT_EDIT_BAD_SLOT", "SLAMIT_EDIT_TABLE_OVERFLOW", "SLAMIT_EDIT_MAX_PER_POINT", "SLAMIT_EDIT_MAX_EDITS", "SLAMIT_UPKEEP_MAX_OBS")
EDIT_FIELDS = ("kind", "flags", "mp", "kf", "idx", "octave", "weight", "pad")


def test_map_edit_struct_layouts_match_the_header(tmp_path):
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
    src += '    printf("%zu\\n", sizeof(slamit_map_edit));\n'
    want.append(api.EDIT_DTYPE.itemsize)
    for f in EDIT_FIELDS:
        src += '    printf("%%zu\\n", offsetof(slamit_map_edit, %s));\n' % f
        want.append(api.EDIT_DTYPE.fields[f][1])
    src += '    printf("%zu\\n", sizeof(slamit_map_index));\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.EDIT_STATUS
    assert v[:len(MACROS)] == [api.EDIT_ADD_OBS, api.EDIT_ERASE_OBS, api.EDIT_SET_BAD, api.EDIT_MATCH] + \
        [st[k] for k in ("REF_END", "EDIT_OVERFLOW", "OBS_OVERFLOW", "BAD_SLOT", "TABLE_OVERFLOW")] + [api.EDIT_MAX_PER_POINT, api.EDIT_MAX_EDITS, api.UPKEEP_MAX_OBS]
    assert v[len(MACROS):-1] == want
    assert v[-1] == 120 == C.sizeof(api.MapIndexRec)                                       # the map record keeps its size
    assert api.EDIT_DTYPE == EDIT_DTYPE and api.EDIT_DTYPE.itemsize == 24 and api.EDIT_MAX_PER_POINT == 64 and api.EDIT_MAX_EDITS == 1 << 20
    names = [f[0] for f in api.EditIndexRec._fields_]
    assert names[:3] == [k for k, _ in api.EDIT_INDEX_COLUMNS] and names[3:7] == [k for k, _ in api.EDIT_INDEX_INPLACE]
    assert names[7] == "obs_ptr_out" and names[8:12] == [k for k, _ in api.EDIT_INDEX_OUT]


def test_the_host_restatement_has_the_c_abi_record(tmp_path):
    """csrc/map_edit.h is built without include/slamit.h: its MeEdit / MeIndex are slamit_map_edit / slamit_edit_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.EditIndexRec._fields_]
    pairs = [("ME_" + n, "SLAMIT_EDIT_" + n) for n in ("ADD_OBS", "ERASE_OBS", "SET_BAD", "MATCH", "REF_END", "EDIT_OVERFLOW", "OBS_OVERFLOW", "BAD_SLOT",
                                                       "TABLE_OVERFLOW", "MAX_PER_POINT", "MAX_EDITS")]
    pairs += [("ME_MAX_OBS", "SLAMIT_UPKEEP_MAX_OBS")]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "map_edit.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(MeIndex), sizeof(slamit_edit_index));\n    printf("%zu %zu\\n", sizeof(MeEdit), sizeof(slamit_map_edit));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(MeIndex, %s), offsetof(slamit_edit_index, %s));\n' % (f, f)
    for f in EDIT_FIELDS:
        src += '    printf("%%zu %%zu\\n", offsetof(MeEdit, %s), offsetof(slamit_map_edit, %s));\n' % (f, f)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (2 + len(names) + len(EDIT_FIELDS) + len(pairs))


def test_map_edit_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "map_edit.hip" in build.SOURCES and "map_edit.hip" not in build.PER_FILE           # nothing is float: no per-file flags
    for f in ("map_edit", "map_edit_batch_dev", "map_edit_workspace", "EditIndex", "edit_records"):
        assert callable(getattr(api, f))
    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    src = open(os.path.join(csrc, "map_edit.hip")).read()
    assert "getenv" not in src and '#include "wave_ops.h"' in src and "me_walk(" in src
    rows = open(os.path.join(csrc, "map_rows_dev.h")).read()                                  # the scan bodies, shared with map_replace and map_fuse
    assert all(body + "<ME_NT>(" in src for body in ("map_scan_sum", "map_scan_parts", "map_scan_add")) and "block_inclusive_scan_i32<NT>(" in rows
    ops = open(os.path.join(csrc, "wave_ops.h")).read()                                       # the workgroup scan stands on the DPP wave scan, no __shfl
    assert "wave_inclusive_scan_i32(v)" in ops.split("block_inclusive_scan_i32(int v, int& total) {")[1].split("\n}")[0] and "__shfl" not in ops.split("#ifndef")[1]
    assert "while (" not in src.replace("while (lo < hi)", "")                                # no kernel waits: the one loop is the bisection
    assert "struct slamit_edit_index {" in hdr and "struct slamit_map_edit {" in hdr
    assert api.map_edit_workspace(1, 0, 0, 0) > 0 and api.map_edit_workspace(0, 1, 1, 1) == 0
    assert api.map_edit_workspace(8, 1000, 5000, 70000) >= 8 * (8 * 70000 + 4 * 1000 + 8 * 4 * 5001)   # the kf_mp words, the buckets, eight rows over the points
    # the workspace's bytes, pinned when the scan and the row copy moved into the shared header: (n_maps, cap, mp_cap, kfmp_cap) -> bytes
    for dims, want in (((1, 0, 0, 0), 160), ((1, 1, 1, 1), 192), ((1, 4, 7, 30), 544), ((2, 64, 257, 1000), 33104), ((8, 1000, 5000, 70000), 5793728),
                       ((8, 16384, 255, 3), 590272)):
        assert api.map_edit_workspace(*dims) == want, dims


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

    fx = by_name("single")
    t, x, E = fx["t"], fx["x"], fx["edits"]
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    me = lambda tables=t, edit=x, edits=E, **kw: api.map_edit(tables, edit, records(edits), **kw)
    w = "slamit_map_edit_apply: "
    for key in ("obs_ptr", "obs_kf", "kf_mp_ptr", "kf_mp", "mp_bad"):
        _refused(lambda: me(dict(t, **{key: None})) if key != "obs_ptr" else api.map_edit(dict(t, obs_ptr=None), x, records(E), obs_cap_out=99), w + "null table")
    for key in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_ref_kf"):
        _refused(lambda: me(edit=dict(x, **{key: None})), w + "null table")
    _refused(lambda: me(obs_cap_out=-1), "negative obs_cap_out")
    _refused(lambda: me(dict(t, n_kf=65536)), "SLAMIT_LOCAL_MAP_MAX_KF")
    _refused(lambda: me(dict(t, kf_mp_ptr=t["kf_mp_ptr"][::-1].copy())), "CSR pointer array")
    _refused(lambda: me(dict(t, obs_ptr=t["obs_ptr"] + 1)), "CSR pointer array")
    _refused(lambda: me(dict(t, obs_kf=np.where(t["obs_kf"] == 7, n_kf, t["obs_kf"]))), "obs_kf holds a keyframe slot outside")
    _refused(lambda: me(edit=dict(x, obs_idx=np.where(np.arange(len(x["obs_idx"])) == 1, 999, x["obs_idx"]))), "obs_idx holds a keypoint index outside")
    _refused(lambda: me(edit=dict(x, obs_weight=np.where(np.arange(len(x["obs_weight"])) == 2, 3, x["obs_weight"]))), "obs_weight holds a weight other than 1 or 2")
    _refused(lambda: me(edit=dict(x, mp_ref_kf=np.where(np.arange(n_mp) == 2, n_kf, x["mp_ref_kf"]))), "mp_ref_kf holds a keyframe slot outside")
    _refused(lambda: me(edit=dict(x, mp_ref_kf=np.where(np.arange(n_mp) == 2, -2, x["mp_ref_kf"]))), "mp_ref_kf holds a keyframe slot outside")
    add = next(e for e in E if e[0] == api.EDIT_ADD_OBS)
    one = lambda **kw: [tuple(kw.get(f, v) for f, v in zip(EDIT_FIELDS, add))]
    _refused(lambda: me(edits=one(kind=0)), "an edit's kind outside 1..3")
    _refused(lambda: me(edits=one(kind=4)), "an edit's kind outside 1..3")
    _refused(lambda: me(edits=one(flags=2)), "an edit's flags outside 0..1")
    _refused(lambda: me(edits=one(mp=n_mp)), "edits holds a point slot outside")
    _refused(lambda: me(edits=one(mp=-1)), "edits holds a point slot outside")
    _refused(lambda: me(edits=one(kf=n_kf)), "edits holds a keyframe slot outside")
    _refused(lambda: me(edits=one(kind=api.EDIT_ERASE_OBS, kf=-1)), "edits holds a keyframe slot outside")
    _refused(lambda: me(edits=one(idx=int(t["kf_mp_ptr"][add[3] + 1] - t["kf_mp_ptr"][add[3]]))), "edits holds a keypoint index outside")
    _refused(lambda: me(edits=one(weight=0)), "an edit's weight other than 1 or 2")
    _refused(lambda: me(edits=one(weight=3)), "an edit's weight other than 1 or 2")
    _refused(lambda: api.map_edit(t, x, np.zeros(api.EDIT_MAX_EDITS + 1, api.EDIT_DTYPE), obs_cap_out=8), "SLAMIT_EDIT_MAX_EDITS", code=-3)
    # what SET_BAD and ERASE_OBS do not read is not checked; without a device a valid call fails loudly and says why
    for edits in (one(kind=api.EDIT_SET_BAD, kf=-5, idx=-5, weight=9), one(kind=api.EDIT_ERASE_OBS, idx=-5, weight=9), E, []):
        if api.device_count() == 0:
            _refused(lambda: me(edits=edits), "", code=-2)
        else:
            assert me(edits=edits)["status"] == 0
    # a missing output through the raw entry point: the other outputs and the in-place arrays keep their bytes
    L = api.lib()
    err = lambda: L.slamit_last_error()
    rec, keep = api._map_index_host(t)
    arrs = {k: np.array(v) for k, v in list(x.items()) + [("mp_bad", t["mp_bad"]), ("kf_mp", t["kf_mp"])]}
    cap = len(t["obs_kf"]) + 4
    outs = {"obs_ptr_out": np.full(n_mp + 1, 77, np.int32), "obs_kf_out": np.full(cap, 77, np.int32), "obs_idx_out": np.full(cap, 77, np.int32),
            "obs_octave_out": np.full(cap, 77, np.uint8), "obs_weight_out": np.full(cap, 77, np.uint8)}
    xrec = api.EditIndexRec(obs_cap_out=cap, **{k: v.ctypes.data for k, v in list(arrs.items()) + list(outs.items())})
    ed = records(E)
    st_mp, tch, three = np.full(n_mp, 77, np.int32), np.full(n_mp, 77, np.int32), np.full(3, 77, np.int32)
    p3 = [three[i:].ctypes.data for i in range(3)]
    call = lambda *a: L.slamit_map_edit_apply(0, *a)
    assert call(C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, p3[0], p3[1], None) == -1 and b"slamit_map_edit_apply: null array" in err()
    assert call(C.byref(rec), C.byref(xrec), len(ed), None, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"null array" in err()
    assert call(C.byref(rec), C.byref(xrec), -1, ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"negative n" in err()
    assert call(C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, None, tch.ctypes.data, *p3) == -1 and b"null array" in err()
    assert call(None, C.byref(xrec), len(ed), ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"null table" in err()
    assert call(C.byref(rec), None, len(ed), ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"null table" in err()
    xrec.obs_idx_out = None
    assert call(C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"null table" in err()
    xrec.obs_idx_out = outs["obs_idx_out"].ctypes.data
    ed["mp"][3] = n_mp
    assert call(C.byref(rec), C.byref(xrec), len(ed), ed.ctypes.data, st_mp.ctypes.data, tch.ctypes.data, *p3) == -1 and b"slot outside" in err()
    assert np.all(st_mp == 77) and np.all(tch == 77) and np.all(three == 77) and all(np.all(v == 77) for v in outs.values())
    for k, v in arrs.items():
        assert np.array_equal(v, np.asarray(x[k] if k in x else t[k]).reshape(-1)), k
    # the resident form: what the host can see of a batch
    B = api.MapEditBatchRec()
    bd = lambda: L.slamit_map_edit_batch_dev(0, C.byref(B), None)
    assert bd() == 0                                                                       # no maps: nothing to do
    B.cap = -1
    assert bd() == -1 and b"slamit_map_edit_batch_dev: bad argument" in err()
    M, X = (api.MapIndexRec * 9)(*([rec] * 9)), (api.EditIndexRec * 9)(*([xrec] * 9))
    B.cap, B.n_maps, B.maps, B.edit, B.mp_cap, B.kfmp_cap = 4, 9, M, X, n_mp, len(t["kf_mp"])
    assert bd() == -1 and b"SLAMIT_LOCAL_MAP_MAX_MAPS" in err()                            # more than eight maps
    B.n_maps, B.cap = 1, api.EDIT_MAX_EDITS + 1
    assert bd() == -3 and b"SLAMIT_EDIT_MAX_EDITS" in err()
    B.cap, B.mp_cap = 4, n_mp - 1
    assert bd() == -1 and b"n_mp above mp_cap" in err()
    B.mp_cap = n_mp
    assert bd() == -1 and b"null array" in err()                                           # no list arrays
    X[0].obs_cap_out = -1
    assert bd() == -1 and b"negative obs_cap_out" in err()
    X[0].obs_cap_out, X[0].obs_weight_out = cap, None
    assert bd() == -1 and b"null table" in err()
    X[0].obs_weight_out, M[0].n_kf = xrec.obs_weight_out, 65536
    assert bd() == -1 and b"SLAMIT_LOCAL_MAP_MAX_KF" in err()
    M[0].n_kf = n_kf
    one4 = np.zeros(4, np.int32)
    B.d_n = B.d_n_touched = B.d_n_obs_out = B.d_status = B.d_status_mp = B.d_touched = B.d_edits = one4.ctypes.data   # never read: the workspace is missing
    assert bd() == -1 and b"workspace" in err()
    B.d_workspace, B.workspace_bytes = one4.ctypes.data, api.map_edit_workspace(1, 4, n_mp, len(t["kf_mp"])) - 1
    assert bd() == -1 and b"workspace" in err()
    del keep
