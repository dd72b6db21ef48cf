"""Layout of the SetBadFlag records against their ctypes mirrors, the macros, the symbols, and every refusal the host makes before a
launch (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.kf_erase_fixtures import by_name
from tests.kf_erase_host import KF_OP_DTYPE, records
from tests.kf_erase_ref import SET_BAD, SET_PARENT

STRUCTS = (("slamit_tree_index", "TreeIndexRec"), ("slamit_kf_erase_batch_rec", "KfEraseBatchRec"))
SYMBOLS = ("slamit_kf_erase_apply", "slamit_kf_erase_workspace", "slamit_kf_erase_batch_dev")
NAMES = ("SET_PARENT", "SET_BAD", "ORIGIN", "NOT_ERASE", "NO_PARENT", "BAD_SLOT", "ROW_OVERFLOW", "CHILD_OVERFLOW", "EDIT_OVERFLOW", "MAX_OPS", "MAX_CHILD")
OP_FIELDS = ("kind", "kf", "parent", "reserved")


def test_kf_erase_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%s\\n", %s);\n' % (" ".join(["%d"] * len(NAMES)), ", ".join("SLAMIT_KF_ERASE_" + n for n in NAMES))
    want = []
    for cname, pname in STRUCTS:
        cls = getattr(api, pname)
        src += '    printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            src += '    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0])
            want.append(getattr(cls, f[0]).offset)
    src += '    printf("%zu\\n", sizeof(slamit_kf_op));\n'
    want.append(api.KF_OP_DTYPE.itemsize)
    for f in OP_FIELDS:
        src += '    printf("%%zu\\n", offsetof(slamit_kf_op, %s));\n' % f
        want.append(api.KF_OP_DTYPE.fields[f][1])
    src += '    printf("%zu %zu %zu\\n", sizeof(slamit_map_index), sizeof(slamit_covis_index), sizeof(slamit_map_edit));\n    return 0;\n}\n'
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    st = api.KF_ERASE_STATUS
    assert v[:len(NAMES)] == [api.KF_ERASE_SET_PARENT, api.KF_ERASE_SET_BAD] + [st[k] for k in NAMES[2:9]] + [api.KF_ERASE_MAX_OPS, api.KF_ERASE_MAX_CHILD]
    assert v[len(NAMES):-3] == want
    assert v[-3:] == [120, 120, 24] and C.sizeof(api.MapIndexRec) == 120 and C.sizeof(api.CovisIndexRec) == 120   # no existing record changes (two int32, fourteen pointers)
    assert C.sizeof(api.TreeIndexRec) == 120 and api.KF_OP_DTYPE == KF_OP_DTYPE and api.KF_OP_DTYPE.itemsize == 16 and api.EDIT_DTYPE.itemsize == 24
    assert api.KF_ERASE_REFUSED == st["CHILD_OVERFLOW"] | st["EDIT_OVERFLOW"] and (api.KF_ERASE_SET_PARENT, api.KF_ERASE_SET_BAD) == (SET_PARENT, SET_BAD)
    names = [f[0] for f in api.TreeIndexRec._fields_]
    assert names[3:13] == [k for k, _ in api.TREE_INDEX_INPLACE] and names[6:13] == list(api.COVIS_GRAPH)


def test_the_host_statement_has_the_c_abi_record(tmp_path):
    """csrc/kf_erase.h is built without include/slamit.h: its KeOp / KeIndex are slamit_kf_op / slamit_tree_index, its constants the header's."""
    from weiner_slamit_v2_amd import api

    names = [f[0] for f in api.TreeIndexRec._fields_]
    pairs = [("KE_" + n, "SLAMIT_KF_ERASE_" + n) for n in NAMES]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\n#include "kf_erase.h"\nint main() {\n'
    src += '    printf("%zu %zu\\n", sizeof(KeIndex), sizeof(slamit_tree_index));\n    printf("%zu %zu\\n", sizeof(KeOp), sizeof(slamit_kf_op));\n'
    for f in names:
        src += '    printf("%%zu %%zu\\n", offsetof(KeIndex, %s), offsetof(slamit_tree_index, %s));\n' % (f, f)
    for f in OP_FIELDS:
        src += '    printf("%%zu %%zu\\n", offsetof(KeOp, %s), offsetof(slamit_kf_op, %s));\n' % (f, f)
    for a, b in pairs:
        src += '    printf("%%d %%d\\n", (int)%s, (int)%s);\n' % (a, b)
    src += '    const MeEdit e = ke_edit(5, 3);\n    printf("%d %d\\n", (int)me_edit_ok(LmMap{4, 6}, e), 1);\n'   # map_edit.h's own validation takes an emitted edit
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_rec.cc"), str(tmp_path / "_rec")
    open(c, "w").write(src)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0::2] == v[1::2] and len(v) == 2 * (3 + len(names) + len(OP_FIELDS) + len(pairs))


def test_kf_erase_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    lib_path = build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name) and getattr(api.lib(), name).argtypes is not None, name
        assert " T %s\n" % name in dyn, name
    assert "kf_erase.hip" in build.SOURCES and "kf_erase.hip" not in build.PER_FILE     # nothing is float: no per-file flags
    for f in ("kf_erase", "kf_erase_batch_dev", "kf_erase_workspace", "TreeIndex", "kf_op_records"):
        assert callable(getattr(api, f))
    csrc = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
    src = open(os.path.join(csrc, "kf_erase.hip")).read()
    assert "getenv" not in src and "float" not in src.replace("Nothing here is float", "") and "double" not in src
    assert '#include "wave_ops.h"' in src and "wave_inclusive_scan_i32" in src and "wave_min_u64" in src and "cv_place(" in src and "ke_pick_key(" in src
    assert "agent" not in src and "__threadfence" not in src                            # workgroup scope only: no workgroup waits on another
    assert "struct slamit_tree_index {" in hdr and "struct slamit_kf_op {" in hdr
    ws = api.kf_erase_workspace
    assert ws(1, 0, 0, 1, 0) > 0 and ws(0, 1, 1, 1, 1) == 0 and ws(1, api.KF_ERASE_MAX_OPS + 1, 1, 1, 1) == 0 and ws(1, 1, 1, api.COVIS_MAX_ROW + 1, 1) == 0
    # the formula beside the declaration
    per_map = 16 + 3 * 200 + 4 * (4 * 64 + 15) * 200 + 4 + 8 * (300 + 10 * 200) + 12 * 10 + 4
    assert 8 * per_map <= ws(8, 10, 200, 64, 300) <= 8 * per_map + 20 * 16 * 8


def _refused(call, word, code=-1):
    from weiner_slamit_v2_amd import api

    try:
        call()
        raise AssertionError("accepted: " + word)
    except api.SlamitError as e:
        assert "(%d)" % code in str(e) and word in str(e), str(e)


def test_refusals_need_no_device():
    """Every refusal is made before a launch: the same with and without a GPU, with a message."""
    from weiner_slamit_v2_amd import api

    fx = by_name("then_child")
    t, x, E = fx["t"], fx["x"], fx["ops"]
    n_kf = t["n_kf"]
    ke = lambda tables=t, tree=x, ops=E, **kw: api.kf_erase(dict(tables), tree, records(ops), **kw)
    changed = lambda d, key, fn: dict(d, **{key: fn(np.array(d[key]))})

    def put(a, at, v):
        a[at] = v
        return a

    # null tables
    for key in ("kf_mp_ptr", "kf_child_ptr", "kf_mp", "kf_child", "kf_parent", "kf_bad"):
        _refused(lambda: ke(tables=dict(t, **{key: None})), "null table")
    for key in ("kf_not_erase", "kf_to_be_erased", "cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n"):
        _refused(lambda: ke(tree=dict(x, **{key: None})), "null table")
    # slots and counts out of range
    _refused(lambda: ke(ops=[(SET_BAD, n_kf, -1)]), "ops holds a keyframe slot")
    _refused(lambda: ke(ops=[(SET_BAD, -1, -1)]), "ops holds a keyframe slot")
    _refused(lambda: ke(ops=[(SET_PARENT, 1, n_kf)]), "ops holds a keyframe slot")
    _refused(lambda: ke(ops=[(SET_PARENT, 1, -1)]), "ops holds a keyframe slot")
    _refused(lambda: ke(ops=[(0, 1, 0)]), "kind outside 1..2")
    _refused(lambda: ke(ops=[(3, 1, 0)]), "kind outside 1..2")
    _refused(lambda: ke(tables=changed(t, "kf_parent", lambda a: put(a, 2, n_kf))), "kf_parent holds a keyframe slot")
    _refused(lambda: ke(tables=changed(t, "kf_parent", lambda a: put(a, 2, -2))), "kf_parent holds a keyframe slot")
    _refused(lambda: ke(tables=changed(t, "kf_child", lambda a: put(a, 0, n_kf))), "kf_child holds a keyframe slot")
    _refused(lambda: ke(tables=changed(t, "kf_mp", lambda a: put(a, 1, t["n_mp"]))), "kf_mp holds a point slot")
    _refused(lambda: ke(tables=changed(t, "kf_mp", lambda a: put(a, 1, -2))), "kf_mp holds a point slot")
    _refused(lambda: ke(tree=changed(x, "cw_kf", lambda a: put(a, (1, 0), n_kf))), "cw_kf holds a keyframe slot")
    _refused(lambda: ke(tree=changed(x, "cw_kf", lambda a: put(a, (1, 0), 1))), "cw_kf holds a keyframe slot")      # a keyframe's own
    _refused(lambda: ke(tree=changed(x, "ord_kf", lambda a: put(a, (1, 0), -1))), "ord_kf holds a keyframe slot")
    _refused(lambda: ke(tree=changed(x, "cw_n", lambda a: put(a, 1, x["row_cap"] + 1))), "count outside [0, row_cap]")
    _refused(lambda: ke(tree=changed(x, "ord_n", lambda a: put(a, 1, -1))), "count outside [0, row_cap]")
    _refused(lambda: ke(tree=dict(x, origin_kf=n_kf)), "origin_kf holds a keyframe slot")
    _refused(lambda: ke(tree=dict(x, row_cap=0)), "row_cap outside")
    _refused(lambda: ke(tree=dict(x, row_cap=api.COVIS_MAX_ROW + 1)), "row_cap outside")
    # the children rows are std::set order; the pointer arrays ascend from 0
    assert t["kf_child"][:2].tolist() == [1, 5]
    _refused(lambda: ke(tables=changed(t, "kf_child", lambda a: put(put(a, 0, 5), 1, 1))), "a children row does not ascend")
    _refused(lambda: ke(tables=changed(t, "kf_child", lambda a: put(a, 1, 1))), "a children row does not ascend")   # an entry twice
    _refused(lambda: ke(tables=changed(t, "kf_child_ptr", lambda a: put(a, 0, 1))), "does not ascend from 0")
    _refused(lambda: ke(tables=changed(t, "kf_mp_ptr", lambda a: put(a, 2, 0))), "does not ascend from 0")
    # counts and the list's ceiling
    _refused(lambda: ke(child_cap_out=-1), "negative child_cap_out")
    _refused(lambda: ke(edit_cap=-1), "negative count")
    _refused(lambda: ke(tables=dict(t, n_kf=api.LOCAL_MAP_MAX_KF + 1)), "n_kf outside")
    _refused(lambda: ke(ops=[(SET_BAD, 1, -1)] * (api.KF_ERASE_MAX_OPS + 1)), "more than SLAMIT_KF_ERASE_MAX_OPS ops", code=-3)
    L = api.lib()
    assert L.slamit_kf_erase_apply(0, None, None, 0, None, None, 0, None, None, None, None) == -1
    # the resident form's record
    rec = api.KfEraseBatchRec(1, api.KF_ERASE_MAX_OPS + 1, 4, 8, 4, 4)
    rec.maps, rec.tree = (api.MapIndexRec * 1)(), (api.TreeIndexRec * 1)()
    assert L.slamit_kf_erase_batch_dev(0, C.byref(rec), None) == -3 and b"cap above SLAMIT_KF_ERASE_MAX_OPS" in L.slamit_last_error()
    rec.cap = 4
    assert L.slamit_kf_erase_batch_dev(0, C.byref(rec), None) == -1 and b"row_cap outside" in L.slamit_last_error()   # the map's own row_cap is 0
    rec.tree[0].row_cap = 8
    assert L.slamit_kf_erase_batch_dev(0, C.byref(rec), None) == -1 and b"null table" in L.slamit_last_error()
    rec.n_maps = api.LOCAL_MAP_MAX_MAPS + 1
    assert L.slamit_kf_erase_batch_dev(0, C.byref(rec), None) == -1 and b"n_maps outside" in L.slamit_last_error()
    rec.n_maps = 0
    assert L.slamit_kf_erase_batch_dev(0, C.byref(rec), None) == 0
    assert L.slamit_kf_erase_batch_dev(0, None, None) == -1
