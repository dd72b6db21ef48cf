"""Layout of the map-growth records against their ctypes mirrors and numpy records, the macros, the symbols, and every refusal the host
makes before a launch (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT
from tests.map_grow_host import INDEX, OP_DTYPE
from tests import map_grow_ref as ref

STRUCTS = (("slamit_grow_index", "GrowIndexRec"), ("slamit_grow_frame", "GrowFrameRec"), ("slamit_map_grow_batch_rec", "MapGrowBatchRec"))
SYMBOLS = ("slamit_map_grow_apply", "slamit_map_grow_workspace", "slamit_map_grow_batch_dev")
NAMES = ("NEW_KF", "NEW_POINT", "ASSOCIATE", "RECENT", "OP_REJECTED", "OP_BAD", "KF_OVERFLOW", "MP_OVERFLOW", "KFMP_OVERFLOW", "EDIT_OVERFLOW", "RECENT_OVERFLOW",
         "KP_OVERFLOW", "OPS_OVERFLOW", "BAD_SLOT", "REFUSED", "MAX_OPS", "MAX_FRAMES", "NEEDS")
OP_FIELDS = ("kind", "flags", "kf", "src", "kf_id", "cand", "kf_a", "idx_a", "kf_b", "idx_b", "weight_a", "weight_b", "pad", "pos")
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")]


def test_map_grow_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%s\\n", %s);\n' % (" ".join(["%d"] * len(NAMES)), ", ".join("SLAMIT_GROW_" + n for n in NAMES))
    want = []
    for cname, pname in STRUCTS:
        cls = getattr(api, pname)
        src += '    printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            src += '    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0])
            want.append(getattr(cls, f[0]).offset)
    src += '    printf("%zu\\n", sizeof(slamit_grow_op));\n'
    want.append(api.GROW_OP_DTYPE.itemsize)
    for f in OP_FIELDS:
        src += '    printf("%%zu\\n", offsetof(slamit_grow_op, %s));\n' % f
        want.append(api.GROW_OP_DTYPE.fields[f][1])
    src += '    printf("%zu %zu %zu %d\\n", sizeof(slamit_map_index), sizeof(slamit_covis_index), sizeof(slamit_map_edit), SLAMIT_FRAME_MAX_KP);\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.GROW_STATUS
    assert v[:len(NAMES)] == [api.GROW_NEW_KF, api.GROW_NEW_POINT, api.GROW_ASSOCIATE, api.GROW_RECENT, api.GROW_OP_REJECTED, api.GROW_OP_BAD] + \
        [st[k] for k in NAMES[6:14]] + [api.GROW_REFUSED, api.GROW_MAX_OPS, api.GROW_MAX_FRAMES, api.GROW_NEEDS]
    assert v[len(NAMES):-4] == want
    assert v[-4:] == [120, 120, 24, ref.MAX_KP] and C.sizeof(api.MapIndexRec) == 120                 # no existing record changes
    assert api.GROW_OP_DTYPE == OP_DTYPE and OP_DTYPE.itemsize == 56 and C.sizeof(api.GrowIndexRec) == 240 and C.sizeof(api.GrowFrameRec) == 56
    assert [k for k, _ in api.GROW_INDEX_ARRAYS] == [k for k, _, _ in INDEX] and [f[0] for f in api.GrowIndexRec._fields_][4:] == [k for k, _, _ in INDEX]
    assert api.GROW_REFUSED == sum(st[k] for k in NAMES[6:13]) and not api.GROW_REFUSED & st["BAD_SLOT"]
    assert (api.GROW_NEW_KF, api.GROW_NEW_POINT, api.GROW_ASSOCIATE, api.GROW_RECENT, api.GROW_OP_REJECTED, api.GROW_OP_BAD) == \
        (ref.NEW_KF, ref.NEW_POINT, ref.ASSOCIATE, ref.RECENT, ref.OP_REJECTED, ref.OP_BAD)
    assert [st[k] for k in NAMES[6:14]] == [ref.KF_OVERFLOW, ref.MP_OVERFLOW, ref.KFMP_OVERFLOW, ref.EDIT_OVERFLOW, ref.RECENT_OVERFLOW, ref.KP_OVERFLOW, ref.OPS_OVERFLOW, ref.BAD_SLOT]


def test_the_host_statement_has_the_c_abi_record(tmp_path):
    """csrc/map_grow.h is built without include/slamit.h: its MgOp / MgFrame / MgIndex are the C-ABI's records, its constants the header's."""
    from weiner_slamit_v2_amd import api

    pairs = [("MG_" + n, "SLAMIT_GROW_" + n) for n in NAMES if n != "NEEDS"] + [("MG_NNEED", "SLAMIT_GROW_NEEDS"), ("MG_MAX_KP", "SLAMIT_FRAME_MAX_KP")]
    recs = (("MgIndex", "slamit_grow_index", [f[0] for f in api.GrowIndexRec._fields_]), ("MgFrame", "slamit_grow_frame", [f[0] for f in api.GrowFrameRec._fields_]),
            ("MgOp", "slamit_grow_op", list(OP_FIELDS)))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "map_grow.h"\nint main() {\n'
    n = 0
    for a, b, fields in recs:
        src += '    printf("%%zu %%zu\\n", sizeof(%s), sizeof(%s));\n' % (a, b)
        for f in fields:
            src += '    printf("%%zu %%zu\\n", offsetof(%s, %s), offsetof(%s, %s));\n' % (a, f, b, f)
        n += 1 + len(fields)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11"] + INC + [c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (n + len(pairs))


def test_map_grow_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "map_grow.hip" in build.SOURCES and "map_grow.hip" not in build.PER_FILE     # mg_center is exact under the build's own -ffp-contract=off
    for f in ("map_grow", "map_grow_batch_dev", "map_grow_workspace", "grow_index_rec", "grow_frame_rec", "grow_op_records"):
        assert callable(getattr(api, f))
    assert "struct slamit_grow_index {" in hdr and "struct slamit_grow_op {" in hdr and "slamit_map_grow_batch_dev's" in hdr
    ws = api.map_grow_workspace
    assert ws(1, 0) > 0 and ws(0, 10) == 0 and ws(api.LOCAL_MAP_MAX_MAPS + 1, 10) == 0 and ws(1, -1) == 0
    assert 8 * 8 * 1000 <= ws(8, 1000) <= 8 * 8 * 1000 + 16 * 9                          # the formula beside the declaration


def test_the_host_form_refuses_before_a_launch():
    """What the resident form skips, slamit_map_grow_apply refuses with SLAMIT_ERR_ARG and a message; the same with and without a GPU."""
    import copy

    import numpy as np

    from tests.map_grow_fixtures import bad_fixtures, by_name, op
    from tests.map_grow_host import api_run, default_caps
    from weiner_slamit_v2_amd import api

    def refused(fx, word, code=-1, caps=None):
        try:
            api_run(fx, caps or default_caps(fx))
            raise AssertionError("accepted: " + word)
        except api.SlamitError as e:
            assert "(%d)" % code in str(e) and word in str(e), str(e)

    def with_ops(fx, ops):
        fx = copy.deepcopy(fx)
        fx["ops"] = ops
        return fx

    a, b = bad_fixtures()
    refused(a, "a NEW_KF op does not name the next free slot")
    refused(b, "kf_mp holds a point slot")                                 # its tables are looked at before its list
    refused(with_ops(by_name("associate_plain"), b["ops"]), "an op's src lies outside [0, n_frames)")
    base = by_name("associate_plain")                                      # 3 keyframes of 5, 6, 4 keypoints, 9 points, one frame record of 7
    pt = lambda **kw: op(ref.NEW_POINT, **dict(dict(kf=1, kf_id=1, kf_a=1, idx_a=0, pos=(1, 1, 1)), **kw))
    for ops, word in (([op(7, kf=1)], "kind outside 1..3"), ([op(ref.ASSOCIATE, kf=1, src=0)], "does not have its keyframe's keypoints"),
                      ([op(ref.ASSOCIATE, kf=3, src=0)], "an ASSOCIATE op whose keyframe"), ([pt(kf=3)], "a NEW_POINT op whose ref"), ([pt(idx_a=6)], "an observer's keyframe, index or weight"),
                      ([pt(weight_a=3)], "an observer's keyframe, index or weight"), ([pt(kf_b=0, idx_b=5)], "an observer's keyframe, index or weight"),
                      ([pt(cand=1000)], "cand lies outside")):
        refused(with_ops(base, ops), word)
    fx = copy.deepcopy(base)
    fx["frames"][0]["frame_mp"][1] = 50
    refused(fx, "frame_mp holds a point slot")
    fx = copy.deepcopy(base)
    fx["t"]["kf_mp"][2] = 9
    refused(fx, "kf_mp holds a point slot")
    fx = copy.deepcopy(base)
    fx["t"]["obs_kf"][0] = 3
    refused(fx, "obs_kf holds a keyframe slot")
    fx = copy.deepcopy(base)
    fx["t"]["kf_mp_ptr"] = np.array([0, 5, 4, 15], np.int32)
    refused(fx, "does not ascend from 0")
    fx = copy.deepcopy(base)
    fx["t"]["mp_found"] = None
    refused(fx, "null table")
    refused(with_ops(base, [pt()] * (api.GROW_MAX_OPS + 1)), "more than SLAMIT_GROW_MAX_OPS ops", code=-3)
    L = api.lib()
    assert L.slamit_map_grow_apply(0, None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, 0, None, None, None, None, None) == -1


def test_refusals_need_no_device():
    """Every refusal is made before a launch: the same with and without a GPU, with a message."""
    from weiner_slamit_v2_amd import api

    L = api.lib()
    go = lambda rec: L.slamit_map_grow_batch_dev(0, C.byref(rec), None)
    rec = api.MapGrowBatchRec(1, api.GROW_MAX_OPS + 1, 0, 0, 4, 4, 8)
    rec.maps, rec.grow = (api.MapIndexRec * 1)(), (api.GrowIndexRec * 1)()
    assert go(rec) == -3 and b"cap above SLAMIT_GROW_MAX_OPS" in L.slamit_last_error()
    rec.cap, rec.n_frames = 4, api.GROW_MAX_FRAMES + 1
    assert go(rec) == -3 and b"n_frames above SLAMIT_GROW_MAX_FRAMES" in L.slamit_last_error()
    rec.n_frames, rec.recent_cap = 0, api.UPKEEP_MAX_RECENT + 1
    assert go(rec) == -3 and b"recent_cap above SLAMIT_UPKEEP_MAX_RECENT" in L.slamit_last_error()
    rec.recent_cap, rec.edit_cap = api.UPKEEP_MAX_RECENT, api.EDIT_MAX_EDITS + 1
    assert go(rec) == -3 and b"edit_cap above SLAMIT_EDIT_MAX_EDITS" in L.slamit_last_error()
    rec.recent_cap, rec.edit_cap = 4, 4
    rec.n_frames = 1
    assert go(rec) == -1 and b"null array" in L.slamit_last_error()
    rec.frames = (api.GrowFrameRec * 1)(api.GrowFrameRec(-1, 0.0))
    assert go(rec) == -1 and b"negative n_kp" in L.slamit_last_error()
    rec.frames[0].n_kp = 3
    assert go(rec) == -1 and b"a frame record with a null array" in L.slamit_last_error()
    rec.n_frames = 0
    rec.grow[0].mp_cap = 9
    assert go(rec) == -1 and b"mp_cap outside" in L.slamit_last_error()
    rec.grow[0].mp_cap, rec.maps[0].n_kf = 8, 1
    assert go(rec) == -1 and b"n_kf outside [0, kf_cap]" in L.slamit_last_error()
    rec.maps[0].n_kf = 0
    assert go(rec) == -1 and b"null table" in L.slamit_last_error()
    rec.n_maps = api.LOCAL_MAP_MAX_MAPS + 1
    assert go(rec) == -1 and b"n_maps outside" in L.slamit_last_error()
    rec.n_maps = -1
    assert go(rec) == -1 and b"bad argument" in L.slamit_last_error()
    rec.n_maps = 0
    assert go(rec) == 0
    assert L.slamit_map_grow_batch_dev(0, None, None) == -1
