"""csrc/map_check.h, the host-side statement of a valid map table, on the CPU: built with g++ behind a small C driver, first as a
shared library (one fault at a time, each message against its literal text), then with the driver's own main as a stand-alone program
under AddressSanitizer and UBSan over the same cases; and the map modules' entry points against it: for a shared fault the
library's message is the entry point's name, ": " and the header's text for the same table.  The two functions over the pair
slamit_map_index + slamit_replace_index (the host and the resident form of map_replace and map_fuse) are cases of the same driver."""
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

enum { FN_CSR, FN_SLOTS, FN_SIZES, FN_BATCH_SIZES, FN_OBS, FN_GRAPH, FN_CHILDREN, FN_REPLACE_TABLES, FN_REPLACE_BATCH };

// The replace index of FN_REPLACE_TABLES / FN_REPLACE_BATCH.  nul: bit i set makes the record's i-th pointer null (bit 14 `touched`,
// bit 15 the map record, bit 16 the index record).  obs_idx and obs_weight are the case's arrays; every other pointer is only ever
// tested for null and points at one byte, so a read through it is the sanitizers' to find.
static const char* drv_replace(int fn, slamit_map_index& M, const int32_t* obs_idx, const uint8_t* obs_weight, int nul, int cap_out, int mp_cap) {
    static unsigned char one[1];
    void* const p = one;
    const auto get = [&](int bit, const void* have) { return (nul >> bit) & 1 ? nullptr : const_cast<void*>(have); };
    slamit_replace_index X = slamit_replace_index();
    X.obs_idx = (const int32_t*)get(0, obs_idx); X.obs_octave = (const uint8_t*)get(1, p); X.obs_weight = (const uint8_t*)get(2, obs_weight);
    X.mp_bad = (uint8_t*)get(3, p); X.mp_nobs = (int32_t*)get(4, p); X.mp_found = (int32_t*)get(5, p); X.mp_visible = (int32_t*)get(6, p);
    X.mp_replaced = (int32_t*)get(7, p); X.kf_mp = (int32_t*)get(8, p); X.obs_ptr_out = (int32_t*)get(9, p); X.obs_kf_out = (int32_t*)get(10, p);
    X.obs_idx_out = (int32_t*)get(11, p); X.obs_octave_out = (uint8_t*)get(12, p); X.obs_weight_out = (uint8_t*)get(13, p);
    X.obs_cap_out = cap_out;
    if (fn == FN_REPLACE_TABLES) return map_replace_tables_error((nul >> 15) & 1 ? nullptr : &M, (nul >> 16) & 1 ? nullptr : &X, (const int32_t*)get(14, p));
    // two maps: a clean one of one keyframe and one point in front of the case's, whose pointers the resident form does not read
    slamit_map_index maps[2] = {slamit_map_index(), M};
    slamit_replace_index index[2] = {X, X};
    maps[0].n_kf = maps[0].n_mp = 1;
    maps[0].obs_ptr = maps[0].obs_kf = maps[0].kf_mp_ptr = (const int32_t*)p;
    index[0].obs_idx = (const int32_t*)p; index[0].obs_octave = index[0].obs_weight = index[0].mp_bad = index[0].obs_octave_out = index[0].obs_weight_out = one;
    index[0].mp_nobs = index[0].mp_found = index[0].mp_visible = index[0].mp_replaced = index[0].kf_mp = index[0].obs_ptr_out = index[0].obs_kf_out =
        index[0].obs_idx_out = (int32_t*)p;
    index[0].obs_cap_out = 0;
    return map_replace_batch_error(2, mp_cap, maps, index);
}

// h: n_kf n_mp row_cap a b c.  FN_CSR: a = 0 obs_ptr, 1 kf_mp_ptr, 2 kf_child_ptr.  FN_SLOTS: v[a] inside [b, c).  FN_REPLACE_*: a = nul,
// b = obs_cap_out, c = mp_cap.
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
    case FN_REPLACE_TABLES: case FN_REPLACE_BATCH: return drv_replace(fn, M, obs_idx, obs_weight, h[3], h[4], h[5]);
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

CSR, SLOTS, SIZES, BATCH_SIZES, OBS, GRAPH, CHILDREN, REPLACE_TABLES, REPLACE_BATCH = range(9)
REPLACE_POINTERS = ("obs_idx", "obs_octave", "obs_weight", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "kf_mp", "obs_ptr_out", "obs_kf_out",
                    "obs_idx_out", "obs_octave_out", "obs_weight_out", "touched", "map", "index")   # the bits of the driver's `nul`
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
T_NULL_TABLE = "null table"
T_NULL_ARRAY = "null array or negative n"
T_CAP_OUT = "negative obs_cap_out"
T_CSR_ROWS = "a CSR pointer array does not ascend from 0"
T_MP_CAP = "a map with n_mp above mp_cap"


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
    # the pair map + replace index of a host form: clean tables, one fault at a time, and the order of two
    nul = lambda *names: sum(1 << REPLACE_POINTERS.index(k) for k in names)
    rt = lambda name, tab, want, bits=0, cap_out=6: add(name, REPLACE_TABLES, tab, want, (bits, cap_out, 0))
    rt("valid pair", b, None)
    rt("empty pair, every array null but obs_ptr_out", e, None, nul(*(k for k in REPLACE_POINTERS[:15] if k != "obs_ptr_out")), 0)
    rt("empty pair without obs_ptr_out", e, T_NULL_TABLE, nul("obs_ptr_out"), 0)
    rt("no room and no new table", b, None, nul("obs_kf_out", "obs_idx_out", "obs_octave_out", "obs_weight_out"), 0)
    rt("no map record", b, T_NULL_TABLE, nul("map"))
    rt("no index record", b, T_NULL_TABLE, nul("index"))
    rt("n_kf one past the ceiling", dict(e, n_kf=MAX_KF + 1), T_SIZES)
    rt("n_mp = -1", dict(e, n_mp=-1), T_SIZES)
    rt("no touched", b, T_NULL_ARRAY, nul("touched"))
    rt("obs_cap_out = -1", b, T_CAP_OUT, 0, -1)
    for key in ("obs_ptr", "kf_mp_ptr", "obs_kf"):
        rt("no " + key, dict(b, **{key: None}), T_NULL_TABLE)
    for key in REPLACE_POINTERS[:14]:
        rt("no " + key, b, T_NULL_TABLE, nul(key))
    rt("obs_ptr[0] != 0", put(b, "obs_ptr", 0, 1), T_CSR_ROWS)
    rt("kf_mp_ptr descending", put(b, "kf_mp_ptr", 1, 5), T_CSR_ROWS)
    rt("obs_kf at n_kf", put(b, "obs_kf", 5, 3), T_OBS_KF)
    rt("obs_idx equal to its row's length", put(b, "obs_idx", 2, 2), T_OBS_IDX)
    rt("weight 3", put(b, "obs_weight", 0, 3), T_OBS_WEIGHT)
    rt("sizes before touched", dict(b, n_kf=-1), T_SIZES, nul("touched"))
    rt("touched before obs_cap_out", b, T_NULL_ARRAY, nul("touched"), -1)
    rt("obs_cap_out before a null table", b, T_CAP_OUT, nul("kf_mp"), -1)
    rt("a null table before the rows", put(b, "obs_ptr", 0, 1), T_NULL_TABLE, nul("obs_ptr_out"))
    rt("the rows before the columns", put(b, "kf_mp_ptr", 1, 5), T_CSR_ROWS, nul("mp_nobs"))
    rt("the columns before the entries", put(b, "obs_kf", 0, -1), T_NULL_TABLE, nul("obs_octave"))
    # the same pair in a resident form: the second of two maps carries the case
    rb = lambda name, tab, want, bits=0, cap_out=6, mp_cap=4: add(name, REPLACE_BATCH, tab, want, (bits, cap_out, mp_cap))
    rb("valid maps", b, None)
    rb("n_mp = mp_cap", b, None, mp_cap=4)
    rb("n_mp above mp_cap", b, T_MP_CAP, mp_cap=3)
    rb("n_kf one past the ceiling", dict(b, n_kf=MAX_KF + 1), "a map with " + T_SIZES)
    rb("obs_cap_out = -1", b, T_CAP_OUT, 0, -1)
    rb("obs_cap_out = 0", b, None, 0, 0)
    for key in ("obs_ptr", "kf_mp_ptr", "obs_kf"):
        rb("no " + key, dict(b, **{key: None}), T_NULL_TABLE)
    for key in REPLACE_POINTERS[:14]:
        rb("no " + key, b, T_NULL_TABLE, nul(key))
    rb("an empty map still names its arrays", e, T_NULL_TABLE, nul("kf_mp"), 0, 1)
    rb("sizes before mp_cap", dict(b, n_kf=-1), "a map with " + T_SIZES, mp_cap=3)
    rb("mp_cap before obs_cap_out", b, T_MP_CAP, 0, -1, 3)
    rb("obs_cap_out before a null table", b, T_CAP_OUT, nul("mp_bad"), -1)
    rb("the pointers are not read", put(put(b, "obs_ptr", 0, 1), "obs_kf", 0, -1), None)
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


def test_map_replace_and_map_fuse_agree_with_the_pair_check(lib):
    """What slamit_map_replace_apply and slamit_map_fuse_apply refuse of their tables is map_replace_tables_error's text for the same pair."""
    from weiner_slamit_v2_amd import api
    from tests import map_fuse_fixtures, map_fuse_host, map_replace_fixtures, map_replace_host

    fr, ff = map_replace_fixtures.by_name("add_order"), map_fuse_fixtures.by_name("mixed")
    mr = lambda t, x, cap: api.map_replace(t, x, map_replace_host.records(fr["ops"]), obs_cap_out=cap)
    mf = lambda t, x, cap: api.map_fuse(t, x, map_fuse_host.records(ff["ops"]), obs_cap_out=cap)
    for where, call, t, x in (("slamit_map_replace_apply", mr, fr["t"], fr["x"]), ("slamit_map_fuse_apply", mf, ff["t"], ff["x"])):
        room = len(t["obs_kf"]) + len(fr["ops"]) + len(ff["ops"])
        faults = [(dict(t, n_kf=MAX_KF + 1), x, room), (dict(t, n_mp=-1), x, room), (t, x, -1), (dict(t, obs_ptr=None), x, room), (dict(t, kf_mp_ptr=None), x, room),
                  (dict(t, obs_ptr=_at(t["obs_ptr"], 0, 1)), x, room), (dict(t, kf_mp_ptr=np.asarray(t["kf_mp_ptr"])[::-1].copy()), x, room),
                  (dict(t, obs_kf=None), x, room), (dict(t, mp_bad=None), x, room), (dict(t, kf_mp=None), x, room),
                  (dict(t, obs_kf=_at(t["obs_kf"], 4, t["n_kf"])), x, room), (t, dict(x, obs_idx=_at(x["obs_idx"], 1, 999)), room),
                  (t, dict(x, obs_weight=_at(x["obs_weight"], 2, 3)), room), (dict(t, obs_ptr=_at(t["obs_ptr"], 0, 1)), dict(x, mp_nobs=None), -1)]
        faults += [(t, dict(x, **{key: None}), room) for key in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_found", "mp_visible", "mp_replaced")]
        for t1, x1, cap in faults:
            tab = dict(t1, **x1)
            bits = sum(1 << REPLACE_POINTERS.index(k) for k in REPLACE_POINTERS[:9] if tab.get(k) is None)
            text = check(lib, REPLACE_TABLES, tab, (bits, cap, 0))
            assert isinstance(text, str), (where, bits, cap)
            assert _message(lambda: call(t1, x1, cap)) == where + ": " + text, (where, text)
