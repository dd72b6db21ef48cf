"""The octree pass from its path table alone (csrc/octree_table.h) on the CPU: the header is built with g++ together with a small C
driver that fills the depth-4 histogram and the per-bin best keys of a case with the header's own key -> (root, path) functions and
runs oct_table_seq, the sequential statement of octree_kernel's table path, on them.

On every OCTREE_CASES entry (tests/orb_ref_fixtures.py) the walk either ends inside the table, and then its keys and their order are
the reference's own (tests/golden/orb_ref_octree.npz), or it reports the pass that needed depth 5 and gives no result: the kernel then
walks the keys from the start."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import orb_ref_fixtures as fx
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
FD = 4

DRIVER = r'''
#include <math.h>
#include <vector>
#include "octree_table.h"

// keys: n x (x, y, response) with x, y relative to the detection border; bw, bh = maxBorder - minBorder.  Roots as orb_plan.cc lays
// them out.  out: per node (order index, response); info: n, passes, exit, left_at.
extern "C" int drv_octree(const float* keys, int n_keys, int bw, int bh, int N, int FD, int32_t* out, int out_cap, int32_t* info) {
    const int nIni = (int)round((float)bw / (float)bh);
    const float hX = (float)bw / nIni;
    const int HS = oct_table_ints(FD), nb = oct_bins(FD), cap = (N > 4 * nIni ? N : 4 * nIni) + 4;
    std::vector<int> hist((size_t)nIni * HS, 0);
    std::vector<unsigned long long> best((size_t)nIni * nb, 0ull);
    for (int k = 0; k < n_keys; ++k) {
        const int x = (int)keys[3 * k], y = (int)keys[3 * k + 1];
        const int r = oct_key_root(x, hX, nIni);
        Box16 b; b.x0 = (short)(int)(hX * (float)r); b.y0 = 0; b.x1 = (short)(int)(hX * (float)(r + 1)); b.y1 = (short)bh;
        const int path = oct_key_path(b, x, y, FD);
        ++hist[r * HS + oct_depth_off(FD) + path];
        const unsigned long long pk = oct_pick_key((unsigned)keys[3 * k + 2], (unsigned)k);
        if (pk > best[r * nb + path]) best[r * nb + path] = pk;
    }
    for (int r = 0; r < nIni; ++r) oct_table_sum_up(&hist[r * HS], FD);
    std::vector<int> code(2 * cap), work(8 * cap);
    std::vector<unsigned long long> key(cap);
    const OctSeqResult res = oct_table_seq(nIni, FD, hist.data(), best.data(), N, cap, code.data(), key.data(), work.data());
    info[0] = res.n; info[1] = res.passes; info[2] = res.exit; info[3] = res.left_at;
    if (res.n > out_cap) return -1;
    for (int i = 0; i < res.n; ++i) { out[2 * i] = (int32_t)oct_pick_order(key[i]); out[2 * i + 1] = (int32_t)oct_pick_response(key[i]); }
    return 0;
}
'''


@pytest.fixture(scope="module")
def olib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("octree_table"))
    drv, so = os.path.join(tmp, "octree_driver.cc"), os.path.join(tmp, "liboctree_driver.so")
    with open(drv, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, drv, "-o", so])
    L = C.CDLL(so)
    L.drv_octree.restype = C.c_int
    return L


def _run(L, case, fd=FD):
    keys = np.ascontiguousarray(case["keys"], np.float32)
    b = case["borders"]
    cap = max(case["n"], 16) + 8
    out, info = np.zeros((cap, 2), np.int32), np.zeros(4, np.int32)
    rc = L.drv_octree(keys.ctypes.data_as(C.c_void_p), len(keys), b[1] - b[0], b[3] - b[2], case["n"], fd,
                      out.ctypes.data_as(C.c_void_p), cap, info.ctypes.data_as(C.c_void_p))
    assert rc == 0
    n, passes, exit_kind, left_at = (int(v) for v in info)
    return out[:n], passes, exit_kind, left_at


@pytest.fixture(scope="module")
def results(olib):
    return {c["name"]: _run(olib, c) for c in fx.OCTREE_CASES}


@pytest.fixture(scope="module")
def golden():
    return fx.load_octree_golden()


def test_finished_cases_equal_the_reference(results, golden):
    finished = 0
    for c in fx.OCTREE_CASES:
        picks, passes, exit_kind, left_at = results[c["name"]]
        if left_at:
            continue
        finished += 1
        got = np.concatenate([c["keys"][picks[:, 0], :2], picks[:, 1:2].astype(np.float32)], 1).astype(np.float32)
        want = golden[c["name"]]
        assert got.shape == want.shape, "%s: %d keys, the reference keeps %d" % (c["name"], len(got), len(want))
        assert np.array_equal(got, want), "%s: keys or their order differ from the reference" % c["name"]
        assert np.array_equal(c["keys"][picks[:, 0], 2], picks[:, 1].astype(np.float32)), c["name"]
        assert passes >= 1
    assert finished >= 100, "only %d cases end inside the depth-%d table" % (finished, FD)
    print("octree table: %d of %d cases end inside the depth-%d table" % (finished, len(fx.OCTREE_CASES), FD))


def test_other_cases_report_the_pass_they_left_at(olib, results):
    """A case that leaves the table reports a pass p >= 1, gives no result, and p is where the walk first has to split a node of depth
    FD: with a table one level deeper the same walk is served at least one pass more, and with a shallower one it leaves no later."""
    left = 0
    for c in fx.OCTREE_CASES:
        picks, passes, exit_kind, left_at = results[c["name"]]
        if not left_at:
            assert exit_kind in (0, 1, 2), c["name"]
            continue
        left += 1
        assert len(picks) == 0 and exit_kind == -1, c["name"]
        assert left_at == passes + 1 and 1 <= left_at, c["name"]
        assert passes >= FD, "%s: left at pass %d, but no node can lie at depth %d before pass %d" % (c["name"], left_at, FD, FD + 1)
        shallower = _run(olib, c, FD - 1)
        assert shallower[3] and shallower[3] <= left_at, c["name"]
    assert left >= 50, "only %d cases leave the depth-%d table" % (left, FD)


def test_each_exit_is_taken_inside_the_table(results):
    exits, _ = fx.octree_premises()
    names = ("at_once", "sorted_stage", "exhausted")
    inside = {k: 0 for k in names}
    for c in fx.OCTREE_CASES:
        _, _, exit_kind, left_at = results[c["name"]]
        if left_at:
            continue
        assert names[exit_kind] == exits[c["name"]], "%s: ended by %s, the oracle by %s" % (c["name"], names[exit_kind], exits[c["name"]])
        inside[names[exit_kind]] += 1
    assert all(v >= 1 for v in inside.values()), inside
