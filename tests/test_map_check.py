"""csrc/map_check.h, the host-side statement of a valid map table, on the CPU: built with g++ behind a small C driver, first as a
shared library (one fault at a time, each message against its literal text), then with the driver's own main as a stand-alone program
under AddressSanitizer and UBSan over the same cases; and the six map modules' entry points against it: for a shared fault the
library's message is the entry point's name, ": " and the header's text for the same table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
MAX_KF = 65535   # SLAMIT_LOCAL_MAP_MAX_KF

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include "map_check.h"

enum { FN_CSR, FN_SLOTS, FN_SIZES, FN_BATCH_SIZES, FN_OBS, FN_GRAPH, FN_CHILDREN };

// h: n_kf n_mp row_cap a b c.  FN_CSR: a = 0 obs_ptr, 1 kf_mp_ptr, 2 kf_child_ptr.  FN_SLOTS: v[a] inside [b, c).
extern "C" const char* drv_check(int fn, const int32_t* h, const int32_t* obs_ptr, const int32_t* obs_kf, const int32_t* kf_mp_ptr, const int32_t* kf_child_ptr,
                                 const int32_t* kf_child, const int32_t* obs_idx, const uint8_t* obs_weight, const int32_t* cw_kf, const int32_t* cw_n,
                                 const int32_t* ord_kf, const int32_t* ord_n, const int32_t* v) {
    slamit_map_index M = slamit_map_index();
    M.n_kf = h[0]; M.n_mp = h[1];
    M.obs_ptr = obs_ptr; M.obs_kf = obs_kf; M.kf_mp_ptr = kf_mp_ptr; M.kf_child_ptr = kf_child_ptr; M.kf_child = kf_child;
    switch (fn) {
    case FN_CSR: return map_csr_ok(h[3] == 0 ? obs_ptr : h[3] == 1 ? kf_mp_ptr : kf_child_ptr, h[3] == 0 ? M.n_mp : M.n_kf) ? nullptr : "false";
    case FN_SLOTS: return map_slots_ok(v, (size_t)h[3], h[4], h[5]) ? nullptr : "false";
    case FN_SIZES: return map_sizes_error(&M);
    case FN_BATCH_SIZES: return map_batch_sizes_error(&M);
    case FN_OBS: return map_obs_error(&M, obs_idx, obs_weight);
    case FN_GRAPH: return map_graph_rows_error(M.n_kf, h[2], cw_kf, cw_n, ord_kf, ord_n);
    case FN_CHILDREN: return map_children_error(&M);
    }
    return "no such function";
}

#ifdef MAP_CHECK_MAIN
// cases from a file: fn, h[6], then the twelve arrays as (count or -1 for null, the bytes), each in an allocation of its own size
int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t fn, h[6];
    while (fread(&fn, 4, 1, f) == 1) {
        if (fread(h, 4, 6, f) != 6) return 2;
        void* a[12];
        for (int i = 0; i < 12; ++i) {
            int32_t n;
            if (fread(&n, 4, 1, f) != 1) return 2;
            const size_t bytes = n < 0 ? 0 : (size_t)n * (i == 6 ? 1 : 4);   // array 6 is obs_weight
            a[i] = n < 0 ? nullptr : malloc(bytes ? bytes : 1);
            if (bytes && fread(a[i], 1, bytes, f) != bytes) return 2;
        }
        const char* const r = drv_check(fn, h, (int32_t*)a[0], (int32_t*)a[1], (int32_t*)a[2], (int32_t*)a[3], (int32_t*)a[4], (int32_t*)a[5], (uint8_t*)a[6],
                                        (int32_t*)a[7], (int32_t*)a[8], (int32_t*)a[9], (int32_t*)a[10], (int32_t*)a[11]);
        printf("%s\n", r ? r : "-");
        for (int i = 0; i < 12; ++i) free(a[i]);
    }
    fclose(f);
    return 0;
}
#endif
'''

CSR, SLOTS, SIZES, BATCH_SIZES, OBS, GRAPH, CHILDREN = range(7)
ARRAYS = (("obs_ptr", np.int32), ("obs_kf", np.int32), ("kf_mp_ptr", np.int32), ("kf_child_ptr", np.int32), ("kf_child", np.int32), ("obs_idx", np.int32),
          ("obs_weight", np.uint8), ("cw_kf", np.int32), ("cw_n", np.int32), ("ord_kf", np.int32), ("ord_n", np.int32), ("v", np.int32))

T_CSR = None   # map_csr_ok and map_slots_ok say only yes or no; the text is the entry point's
T_SIZES = "n_kf outside [0, SLAMIT_LOCAL_MAP_MAX_KF] or negative n_mp"
T_OBS_KF = "obs_kf holds a keyframe slot outside [0, n_kf)"
T_OBS_IDX = "obs_idx holds a keypoint index outside its keyframe's row"
T_OBS_WEIGHT = "obs_weight holds a weight other than 1 or 2"
T_COUNT = "a graph row's count outside [0, row_cap]"
T_CW = "cw_kf holds a keyframe slot outside [0, n_kf) or a keyframe's own"
T_ORD = "ord_kf holds a keyframe slot outside [0, n_kf)"
T_CHILD = "kf_child holds a keyframe slot outside [0, n_kf)"
T_CHILD_ROW = "a children row does not ascend"


def base():
    """The smallest table with every array non-empty: 3 keyframes, 4 points, six observations (keypoint rows of two), one children
    row of two, graph rows of row_cap = 2.  Entries past a graph row's count are never read: they hold slots outside the map."""
    return {"n_kf": 3, "n_mp": 4, "row_cap": 2,
            "obs_ptr": [0, 2, 3, 5, 6], "obs_kf": [0, 1, 1, 0, 2, 2], "obs_idx": [0, 0, 1, 1, 0, 1], "obs_weight": [1, 2, 1, 1, 2, 1],
            "kf_mp_ptr": [0, 2, 4, 6], "kf_child_ptr": [0, 2, 2, 2], "kf_child": [1, 2],
            "cw_n": [2, 1, 1], "cw_kf": [1, 2, 0, 7, 0, 7], "ord_n": [2, 1, 0], "ord_kf": [2, 1, 0, 9, 9, 9]}


def empty():
    return {"n_kf": 0, "n_mp": 0, "row_cap": 2, "obs_ptr": [0], "kf_mp_ptr": [0], "kf_child_ptr": [0]}


def put(tab, key, at, value):
    out = dict(tab)
    out[key] = list(tab[key])
    out[key][at] = value
    return out


def cases():
    """(name, function, table, (a, b, c), the text or None).  False stands for the `false` of the two yes / no functions."""
    b, e = base(), empty()
    out = []
    add = lambda name, fn, tab, want, args=(0, 0, 0): out.append((name, fn, tab, args, want))
    for which in range(3):
        add("valid csr %d" % which, CSR, b, None, (which, 0, 0))
        add("empty csr %d" % which, CSR, e, None, (which, 0, 0))
    for fn in (SIZES, BATCH_SIZES, OBS, GRAPH, CHILDREN):
        add("valid %d" % fn, fn, b, None)
        add("empty %d" % fn, fn, e, None)
    add("ptr[0] != 0", CSR, put(b, "obs_ptr", 0, 1), False)
    add("a descending pointer", CSR, put(b, "kf_mp_ptr", 1, 5), False, (1, 0, 0))
    add("a descending last pointer", CSR, put(b, "kf_child_ptr", 3, 1), False, (2, 0, 0))
    slots = lambda v, lo, n: (dict(b, v=v), (len(v), lo, n))
    for name, v, lo, n, want in (("slots inside", [0, 2, 1], 0, 3, None), ("no slots", [], 0, 3, None), ("a slot at -1", [0, -1, 1], 0, 3, False),
                                 ("a slot at n", [0, 1, 3], 0, 3, False), ("-1 with lo = -1", [-1, 2], -1, 3, None), ("a slot at lo - 1", [2, -2], -1, 3, False)):
        tab, args = slots(v, lo, n)
        add(name, SLOTS, tab, want, args)
    add("null v, no count", SLOTS, b, None, (0, 0, 3))
    add("obs_kf at -1", OBS, put(b, "obs_kf", 3, -1), T_OBS_KF)
    add("obs_kf at n_kf", OBS, put(b, "obs_kf", 5, 3), T_OBS_KF)
    add("obs_idx equal to its row's length", OBS, put(b, "obs_idx", 2, 2), T_OBS_IDX)
    add("obs_idx at -1", OBS, put(b, "obs_idx", 0, -1), T_OBS_IDX)
    add("weight 0", OBS, put(b, "obs_weight", 4, 0), T_OBS_WEIGHT)
    add("weight 3", OBS, put(b, "obs_weight", 0, 3), T_OBS_WEIGHT)
    add("cw_n = row_cap + 1", GRAPH, put(b, "cw_n", 1, 3), T_COUNT)
    add("cw_n = -1", GRAPH, put(b, "cw_n", 0, -1), T_COUNT)
    add("ord_n = -1", GRAPH, put(b, "ord_n", 2, -1), T_COUNT)
    add("ord_n = row_cap + 1", GRAPH, put(b, "ord_n", 0, 3), T_COUNT)
    add("a keyframe's own slot in cw_kf", GRAPH, put(b, "cw_kf", 2, 1), T_CW)
    add("cw_kf at n_kf", GRAPH, put(b, "cw_kf", 1, 3), T_CW)
    add("ord_kf at -1", GRAPH, put(b, "ord_kf", 0, -1), T_ORD)
    add("ord_kf at n_kf in the last counted entry", GRAPH, put(b, "ord_kf", 2, 3), T_ORD)
    add("full rows", GRAPH, dict(b, cw_n=[2, 2, 2], cw_kf=[1, 2, 0, 2, 0, 1], ord_n=[2, 2, 2], ord_kf=[2, 1, 2, 0, 1, 0]), None)
    add("a children row holding an entry twice", CHILDREN, put(b, "kf_child", 1, 1), T_CHILD_ROW)
    add("a children row descending", CHILDREN, dict(b, kf_child=[2, 1]), T_CHILD_ROW)
    add("kf_child at n_kf", CHILDREN, put(b, "kf_child", 1, 3), T_CHILD)
    add("kf_child at -1", CHILDREN, put(b, "kf_child", 0, -1), T_CHILD)
    add("two rows, each ascending", CHILDREN, dict(b, kf_child_ptr=[0, 1, 2, 2], kf_child=[2, 0]), None)   # the test is per row
    for fn, lead in ((SIZES, ""), (BATCH_SIZES, "a map with ")):
        add("n_kf at the ceiling", fn, dict(e, n_kf=MAX_KF), None)
        add("n_kf one past it", fn, dict(e, n_kf=MAX_KF + 1), lead + T_SIZES)
        add("n_kf = -1", fn, dict(e, n_kf=-1), lead + T_SIZES)
        add("n_mp = -1", fn, dict(e, n_mp=-1), lead + T_SIZES)
        add("n_mp large", fn, dict(e, n_mp=0x7fffffff), None)
    # the null arguments of map_obs_error: what remains is checked, exactly
    both = put(put(b, "obs_idx", 2, 2), "obs_weight", 1, 0)                     # the weight's fault lies in front
    add("two faults", OBS, both, T_OBS_WEIGHT)
    add("two faults, no weights", OBS, dict(both, obs_weight=None), T_OBS_IDX)
    add("two faults, no indices", OBS, dict(both, obs_idx=None), T_OBS_WEIGHT)
    add("two faults, neither", OBS, dict(both, obs_idx=None, obs_weight=None), None)
    add("obs_kf alone", OBS, dict(put(both, "obs_kf", 5, 3), obs_idx=None, obs_weight=None), T_OBS_KF)
    add("an index fault unseen", OBS, dict(put(b, "obs_idx", 5, 2), obs_idx=None), None)
    add("a weight fault unseen", OBS, dict(put(b, "obs_weight", 5, 3), obs_weight=None), None)
    return out


def _build(tmp, name, extra):
    src = os.path.join(tmp, "map_check_driver.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    out = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-I", CSRC, src, "-o", out] + extra)   # the header alone: plain C++11, no HIP
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = C.CDLL(_build(str(tmp_path_factory.mktemp("map_check")), "libmap_check_driver.so", ["-shared", "-fPIC"]))
    L.drv_check.restype = C.c_char_p
    L.drv_check.argtypes = [C.c_int, C.c_void_p] + [C.c_void_p] * len(ARRAYS)
    return L


def _arrays(tab):
    return [None if tab.get(k) is None else np.ascontiguousarray(np.asarray(tab[k]).reshape(-1), dt) for k, dt in ARRAYS]


def check(L, fn, tab, args=(0, 0, 0)):
    """The header's answer for a table given as a dict of the C-ABI's field names (a missing or None array is NULL): None, the text, or
    False from the yes / no functions."""
    h = np.array([tab["n_kf"], tab["n_mp"], tab.get("row_cap", 0)] + list(args), np.int32)
    arrs = _arrays(tab)
    r = L.drv_check(fn, h.ctypes.data, *[None if a is None else a.ctypes.data for a in arrs])
    return None if r is None else False if r == b"false" else r.decode()


def test_one_fault_at_a_time(lib):
    names = [c[0] + "/%d" % c[1] for c in cases()]
    assert len(set(names)) == len(names)
    for name, fn, tab, args, want in cases():
        got = check(lib, fn, tab, args)
        assert got == want and type(got) is type(want), (name, got, want)


def test_the_same_cases_under_sanitizers(tmp_path):
    """The driver with its own main, every array in an allocation of exactly its size: one run over all cases, clean."""
    exe = _build(str(tmp_path), "map_check_driver", ["-DMAP_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    blob = b""
    for _, fn, tab, args, _ in cases():
        blob += np.array([fn, tab["n_kf"], tab["n_mp"], tab.get("row_cap", 0)] + list(args), np.int32).tobytes()
        for a in _arrays(tab):
            blob += np.int32(-1 if a is None else a.size).tobytes() + (b"" if a is None else a.tobytes())
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    want = ["-" if c[4] is None else "false" if c[4] is False else c[4] for c in cases()]
    assert r.stdout.decode().splitlines() == want


# ---- the six entry points say what the header says -------------------------------------------------------------------------------
def _message(call):
    """The library's message for a call that must be refused with SLAMIT_ERR_ARG."""
    from weiner_slamit_v2_amd import api

    with pytest.raises(api.SlamitError) as e:
        call()
    head, _, text = str(e.value).partition("(-1): ")
    assert head and text, str(e.value)
    return text


def _agree(lib, where, call, fn, tab, skip=()):
    """tab: the tables and index columns as the entry point got them; skip: the columns this entry point does not hand to map_check.h."""
    text = check(lib, fn, {k: v for k, v in tab.items() if k not in skip})
    assert isinstance(text, str)
    assert _message(call) == where + ": " + text, (where, text)


def _at(a, at, value):
    out = np.array(a)
    out[at] = value
    return out


def _over(t):
    return dict(t, n_kf=MAX_KF + 1)


def test_map_edit_and_map_replace_agree_with_the_header(lib):
    from weiner_slamit_v2_amd import api
    from tests import map_edit_fixtures, map_edit_host, map_replace_fixtures, map_replace_host

    fx = map_edit_fixtures.by_name("single")
    me = lambda t, x: api.map_edit(t, x, map_edit_host.records(fx["edits"]))
    fr = map_replace_fixtures.by_name("add_order")
    mr = lambda t, x: api.map_replace(t, x, map_replace_host.records(fr["ops"]))
    for where, call, t, x in (("slamit_map_edit_apply", me, fx["t"], fx["x"]), ("slamit_map_replace_apply", mr, fr["t"], fr["x"])):
        for fn, t1, x1 in ((OBS, dict(t, obs_kf=_at(t["obs_kf"], 4, t["n_kf"])), x), (OBS, dict(t, obs_kf=_at(t["obs_kf"], 0, -1)), x),
                           (OBS, t, dict(x, obs_idx=_at(x["obs_idx"], 1, 999))), (OBS, t, dict(x, obs_weight=_at(x["obs_weight"], 2, 3))),
                           (OBS, t, dict(x, obs_weight=_at(x["obs_weight"], 2, 0))), (SIZES, _over(t), x)):
            _agree(lib, where, lambda: call(t1, x1), fn, dict(t1, **x1))


def test_upkeep_covis_and_local_map_agree_with_the_header(lib):
    from weiner_slamit_v2_amd import api
    from tests.covis_fixtures import fixture as covis_fixture
    from tests.local_map_fixtures import fixture as local_map_fixture
    from tests.upkeep_fixtures import small_map

    fx = small_map()
    t, x = fx["t"], fx["x"]
    up = lambda t1, x1, what=3: api.update_points(t1, x1, (0, 1), what)
    where = "slamit_update_points"
    bad_kf, bad_idx = dict(t, obs_kf=_at(t["obs_kf"], 1, t["n_kf"])), dict(x, obs_idx=_at(x["obs_idx"], 1, 99))
    _agree(lib, where, lambda: up(bad_kf, x), OBS, dict(bad_kf, **x), skip=("obs_weight",))
    _agree(lib, where, lambda: up(t, bad_idx), OBS, dict(t, **bad_idx), skip=("obs_weight",))
    _agree(lib, where, lambda: up(_over(t), x), SIZES, _over(t))
    _agree(lib, "slamit_map_point_culling", lambda: api.map_point_culling(_over(t), x, 5, True, (0, 1)), SIZES, _over(t))
    if api.device_count() == 0:                                                 # without the descriptors obs_idx is not read: the call passes every check
        assert _message_code(lambda: up(t, bad_idx, 1)) == -2
    else:
        assert up(t, bad_idx, 1)["status"].shape == (2,)
    fc = covis_fixture("uc", "tie_below")
    t, x = fc["t"], fc["x"]
    bad_kf = dict(t, obs_kf=_at(t["obs_kf"], 0, t["n_kf"]))
    for where, call in (("slamit_update_connections", lambda t1: api.update_connections(t1, x, 2)), ("slamit_keyframe_culling", lambda t1: api.keyframe_culling(t1, x, 2, True))):
        _agree(lib, where, lambda: call(bad_kf), OBS, bad_kf)                   # the tables alone: no indices, no weights
        _agree(lib, where, lambda: call(_over(t)), SIZES, _over(t))
    fl = local_map_fixture("tie")
    t, mp = fl["maps"][0], fl["frames"][0]["frame_mp"]
    _agree(lib, "slamit_local_keyframes", lambda: api.local_keyframes(_over(t), mp), SIZES, _over(t))
    _agree(lib, "slamit_local_points", lambda: api.local_points(_over(t), mp, (0, 1)), SIZES, _over(t))


def _message_code(call):
    from weiner_slamit_v2_amd import api

    with pytest.raises(api.SlamitError) as e:
        call()
    return int(str(e.value).partition("(")[2].partition(")")[0])


def test_kf_erase_agrees_with_the_header(lib):
    from weiner_slamit_v2_amd import api
    from tests import kf_erase_fixtures, kf_erase_host

    fx = kf_erase_fixtures.by_name("then_child")
    t, x = fx["t"], fx["x"]
    n_kf, rc = t["n_kf"], x["row_cap"]
    assert np.asarray(t["kf_child"])[:2].tolist() == [1, 5]
    ke = lambda t1, x1: api.kf_erase(dict(t1), x1, kf_erase_host.records(fx["ops"]))
    where = "slamit_kf_erase_apply"
    for fn, t1, x1 in ((GRAPH, t, dict(x, cw_n=_at(x["cw_n"], 1, rc + 1))), (GRAPH, t, dict(x, ord_n=_at(x["ord_n"], 1, -1))),
                       (GRAPH, t, dict(x, cw_kf=_at(np.asarray(x["cw_kf"]).reshape(-1), rc, 1))), (GRAPH, t, dict(x, cw_kf=_at(np.asarray(x["cw_kf"]).reshape(-1), rc, n_kf))),
                       (GRAPH, t, dict(x, ord_kf=_at(np.asarray(x["ord_kf"]).reshape(-1), rc, -1))),
                       (CHILDREN, dict(t, kf_child=_at(t["kf_child"], 1, 1)), x), (CHILDREN, dict(t, kf_child=_at(_at(t["kf_child"], 0, 5), 1, 1)), x),
                       (CHILDREN, dict(t, kf_child=_at(t["kf_child"], 0, n_kf)), x), (SIZES, _over(t), x)):
        _agree(lib, where, lambda: ke(t1, x1), fn, dict(t1, **{k: v for k, v in x1.items() if k in ("row_cap", "cw_kf", "cw_n", "ord_kf", "ord_n")}))
