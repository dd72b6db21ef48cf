"""The host-side packing of a vocabulary (csrc/voc_pack.cc) on the CPU: voc_pack.cc is built with g++ together with a small C driver;
the text loader, the validation and the device-order arrays are checked against tests/bow_voc_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import bow_voc_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")

DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include "voc_pack.h"

static VocArrays g_a;
static VocPacked g_p;
static std::string g_why;

extern "C" const char* drv_why() { return g_why.c_str(); }
// -> 1, or 0 with the reason in drv_why(); head = k L scoring weighting n_nodes
extern "C" int drv_load(const char* path, int32_t* head, const int32_t** parent, const uint8_t** is_leaf, const uint8_t** desc, const double** weight) {
    if (!voc_load_text(path, g_a, g_why)) return 0;
    head[0] = g_a.k; head[1] = g_a.L; head[2] = g_a.scoring; head[3] = g_a.weighting; head[4] = (int32_t)g_a.parent.size();
    *parent = g_a.parent.data(); *is_leaf = g_a.is_leaf.data(); *desc = g_a.desc.data(); *weight = g_a.weight.data();
    return 1;
}
// head = k L n_nodes n_words max_fanout depth
extern "C" int drv_pack(const slamit_voc_desc* d, int32_t* head, const int32_t** child_first, const int32_t** child_count, const uint8_t** desc,
                        const int32_t** orig_id, const int32_t** word_id, const double** weight) {
    if (!voc_pack(*d, g_p, g_why)) return 0;
    head[0] = g_p.k; head[1] = g_p.L; head[2] = g_p.n_nodes; head[3] = g_p.n_words; head[4] = g_p.max_fanout; head[5] = g_p.depth;
    *child_first = g_p.child_first.data(); *child_count = g_p.child_count.data(); *desc = g_p.desc.data();
    *orig_id = g_p.orig_id.data(); *word_id = g_p.word_id.data(); *weight = g_p.weight.data();
    return 1;
}
'''


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    from weiner_slamit_v2_amd import api   # the ctypes mirror of slamit_voc_desc

    d = tmp_path_factory.mktemp("voc_pack")
    src, so = str(d / "voc_driver.cc"), str(d / "libvoc_driver.so")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src,
                           os.path.join(CSRC, "voc_pack.cc"), "-o", so])   # no HIP in either file
    L = C.CDLL(so)
    L.drv_why.restype = C.c_char_p
    L.drv_load.argtypes = [C.c_char_p, C.c_void_p] + [C.c_void_p] * 4
    L.drv_pack.argtypes = [C.POINTER(api.VocDesc), C.c_void_p] + [C.c_void_p] * 6
    return L


def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype).copy() if n else np.zeros(0, dtype)


def load(drv, path):
    head = np.zeros(5, np.int32)
    p = [C.c_void_p() for _ in range(4)]
    if not drv.drv_load(os.fsencode(path), head.ctypes.data, *[C.byref(x) for x in p]):
        return None, drv.drv_why().decode()
    n = int(head[4])
    return {"k": int(head[0]), "L": int(head[1]), "scoring": int(head[2]), "weighting": int(head[3]), "parent": _arr(p[0], n, np.int32),
            "is_leaf": _arr(p[1], n, np.uint8), "desc": _arr(p[2], 32 * n, np.uint8).reshape(n, 32), "weight": _arr(p[3], n, np.float64)}, ""


def pack(drv, voc):
    from weiner_slamit_v2_amd import api

    keep = [np.ascontiguousarray(voc["parent"], np.int32), np.ascontiguousarray(voc["is_leaf"], np.uint8),
            np.ascontiguousarray(voc["desc"], np.uint8), np.ascontiguousarray(voc["weight"], np.float64)]
    d = api.VocDesc(voc["k"], voc["L"], voc["scoring"], voc["weighting"], len(keep[0]), *[a.ctypes.data for a in keep])
    head = np.zeros(6, np.int32)
    p = [C.c_void_p() for _ in range(6)]
    if not drv.drv_pack(C.byref(d), head.ctypes.data, *[C.byref(x) for x in p]):
        return None, drv.drv_why().decode()
    N = int(head[2]) + 1
    out = dict(zip(("k", "L", "n_nodes", "n_words", "max_fanout", "depth"), (int(v) for v in head)))
    out.update(child_first=_arr(p[0], N, np.int32), child_count=_arr(p[1], N, np.int32), desc=_arr(p[2], 32 * N, np.uint8).reshape(N, 32),
               orig_id=_arr(p[3], N, np.int32), word_id=_arr(p[4], N, np.int32), weight=_arr(p[5], N, np.float64))
    return out, ""


def _same(a, b):
    return all(a[k] == b[k] for k in ("k", "L", "scoring", "weighting")) and all(
        np.array_equal(a[k], b[k]) for k in ("parent", "is_leaf", "desc")) and np.array_equal(a["weight"].view(np.uint64), b["weight"].view(np.uint64))


@pytest.mark.parametrize("make", [lambda: ref.full_tree(3, 3, 1, stop_frac=0.2), lambda: ref.unbalanced_tree(2), lambda: ref.full_tree(20, 1, 3)])
def test_text_round_trip_equals_the_array_form(drv, tmp_path, make):
    voc = make()
    p = str(tmp_path / "voc.txt")
    ref.write_text(voc, p)
    got, why = load(drv, p)
    assert got is not None, why
    assert _same(got, voc)


def test_trailing_newline_does_not_add_a_node(drv, tmp_path):
    """The reference's while(!f.eof()) loop reads the empty last line as a node under the root (TemplatedVocabulary.h:1396); the
    loader skips empty lines, so a file loads the same with and without its final newline, and with blank lines and CR LF endings."""
    voc = ref.full_tree(2, 2, 4)
    a, b, c = (str(tmp_path / n) for n in ("a.txt", "b.txt", "c.txt"))
    ref.write_text(voc, a, trailing_newline=True)
    ref.write_text(voc, b, trailing_newline=False)
    open(c, "w").write(open(a).read().replace("\n", "\r\n") + "\r\n\r\n")
    va, vb, vc = load(drv, a)[0], load(drv, b)[0], load(drv, c)[0]
    assert len(va["parent"]) == 6 and _same(va, voc) and _same(vb, voc) and _same(vc, voc)


@pytest.mark.parametrize("make", [lambda: ref.full_tree(3, 3, 1), lambda: ref.unbalanced_tree(2), lambda: ref.full_tree(20, 2, 3), lambda: ref.full_tree(10, 3, 5)])
def test_device_order_keeps_siblings_adjacent_and_in_order(drv, make):
    voc = make()
    P, why = pack(drv, voc)
    assert P is not None, why
    v = ref.Vocabulary(voc)
    N = len(voc["parent"]) + 1
    assert P["n_nodes"] == N - 1 and P["n_words"] == v.n_words and P["max_fanout"] == max(len(c) for c in v.children)
    assert sorted(P["orig_id"].tolist()) == list(range(N)) and P["orig_id"][0] == 0      # a permutation, the root first
    for dev in range(N):
        oid = int(P["orig_id"][dev])
        first, cnt = int(P["child_first"][dev]), int(P["child_count"][dev])
        assert P["orig_id"][first:first + cnt].tolist() == v.children[oid] if cnt else not v.children[oid]
        assert cnt == 0 or 0 < first and first + cnt <= N                                   # what bounds the kernel's loads
        assert P["word_id"][dev] == v.word_id[oid]
        if oid:
            assert np.array_equal(P["desc"][dev], voc["desc"][oid - 1]) and P["weight"][dev] == voc["weight"][oid - 1]
    assert sorted(P["word_id"][P["word_id"] >= 0].tolist()) == list(range(v.n_words))


def _mut(voc, **kw):
    out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in voc.items()}
    out.update(kw)
    return out


def test_every_rejection(drv, tmp_path):
    base = ref.full_tree(3, 2, 7)

    def refused(voc, word):
        P, why = pack(drv, voc)
        assert P is None and word in why, (why, word)

    par = base["parent"].copy(); par[4] = 5                  # node 5 names itself
    refused(_mut(base, parent=par), "not smaller")
    par = base["parent"].copy(); par[2] = 9                  # a later node
    refused(_mut(base, parent=par), "not smaller")
    par = base["parent"].copy(); par[0] = -1
    refused(_mut(base, parent=par), "not smaller")
    wide = ref.tree_from_shape(20, 1, lambda nid, lev: 21 if lev == 0 else 0, 1)
    refused(wide, "SLAMIT_VOC_MAX_K")
    deep = ref.tree_from_shape(2, 10, lambda nid, lev: 1 if lev < 11 else 0, 1)
    refused(deep, "SLAMIT_VOC_MAX_L")
    ok10 = ref.tree_from_shape(2, 10, lambda nid, lev: 1 if lev < 10 else 0, 1)
    assert pack(drv, ok10)[0]["depth"] == 10
    leaf = base["is_leaf"].copy(); leaf[0] = 1               # an inner node marked as a leaf
    refused(_mut(base, is_leaf=leaf), "is_leaf")
    leaf = base["is_leaf"].copy(); leaf[-1] = 0              # a node without children not marked
    refused(_mut(base, is_leaf=leaf), "is_leaf")
    for w in (2, 3):
        refused(_mut(base, weighting=w), "weighting")
    assert pack(drv, _mut(base, weighting=1))[0] is not None
    for s in (1, 5):
        refused(_mut(base, scoring=s), "scoring")
    for bad in (dict(k=21), dict(k=-1), dict(L=0), dict(L=11), dict(scoring=6), dict(weighting=4)):
        refused(_mut(base, **bad), "out of bounds")
    refused(_mut(base, parent=base["parent"][:0], is_leaf=base["is_leaf"][:0], desc=base["desc"][:0], weight=base["weight"][:0]), "no nodes")
    # the same through the text loader: a bad header, a short line, a missing file
    p = str(tmp_path / "bad.txt")
    open(p, "w").write("10 6 0 2\n")
    assert load(drv, p) == (None, "vocabulary weighting is not TF_IDF (0) or TF (1): not built")
    open(p, "w").write("3 2 0 0\n0 0 1 2 3 0.5\n")
    got, why = load(drv, p)
    assert got is None and "line 2" in why
    got, why = load(drv, str(tmp_path / "absent.txt"))
    assert got is None and "cannot open" in why
