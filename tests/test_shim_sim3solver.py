"""shim/Sim3Solver.h: the host logic on the CPU (sampler, SetRansacParameters, the acceptance scan, in C++ and in Python, against
the line-by-line restatements of tests/sim3_ransac_ref.py) and, on the GPU, the C++ class over the C-ABI against api.Sim3Solver."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import sim3_ransac_ref as ref
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")

HOST = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "Sim3Solver.h"
using namespace ORB_SLAM2;
static std::vector<unsigned> script; static size_t pos = 0;
static int scripted(int lo, int hi) { unsigned v = pos < script.size() ? script[pos] : 0u; ++pos; return lo + (int)(v % (unsigned)(hi - lo + 1)); }
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "sample")) {          // sample N count v0 v1 ...
        const int N = atoi(argv[2]), count = atoi(argv[3]);
        for (int i = 4; i < argc; ++i) script.push_back((unsigned)strtoul(argv[i], 0, 10));
        sim3solver::RandomInt() = scripted;
        std::vector<int> avail;
        for (int h = 0; h < count; ++h) { int t[3]; sim3solver::SampleTriple(N, avail, t); printf("%d %d %d\n", t[0], t[1], t[2]); }
    } else if (!strcmp(argv[1], "its")) {      // its N minInliers maxIts
        printf("%d\n", sim3solver::RansacIterations(atoi(argv[2]), 0.99, atoi(argv[3]), atoi(argv[4])));
    } else if (!strcmp(argv[1], "scan")) {     // scan minInliers maxIts chunk c0 c1 ... : one line per iterate(chunk) call
        const int minInl = atoi(argv[2]), maxIts = atoi(argv[3]), chunk = atoi(argv[4]);
        std::vector<int32_t> c;
        for (int i = 5; i < argc; ++i) c.push_back(atoi(argv[i]));
        sim3solver::ScanState st;
        for (;;) {
            bool noMore;
            const int h = sim3solver::Scan(c.data(), chunk, maxIts, minInl, st, noMore);
            printf("%d %d %d %d\n", h, noMore ? 1 : 0, st.best, st.mnBestInliers);
            if (h >= 0 || noMore) break;
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3solver_host")
    open(str(d / "host.cc"), "w").write(HOST)
    exe = str(d / "host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-I", SHIM, str(d / "host.cc"), "-o", exe])   # header only: no device, no library
    return lambda *a: [[int(v) for v in ln.split()] for ln in subprocess.check_output([exe] + [str(x) for x in a]).decode().splitlines()]


def _script(vals):
    it = iter(vals)
    return lambda lo, hi: lo + next(it) % (hi - lo + 1)


@pytest.mark.parametrize("N,vals", [(5, [4, 0, 2, 1, 1, 1, 0, 0, 0]), (4, [3, 3, 1, 2, 2, 0]), (10, [9, 9, 9, 3, 3, 3]), (7, list(range(20, 41)))])
def test_sampler_reproduces_the_reference_quirk(host, N, vals):
    """:163-177 on a scripted RandomInt stream: the C++ sampler, the binding's and the line-by-line restatement give the same triples."""
    from weiner_slamit_v2_amd import api

    count = len(vals) // 3
    want = ref.sample_triples(N, count, _script(vals))
    assert np.array_equal(np.array(host("sample", N, count, *vals)), want)
    assert np.array_equal(api.Sim3Solver.sample_triples(N, count, _script(vals)), want)
    assert want.min() >= 0 and want.max() < N


def test_a_scripted_stream_repeats_an_index_inside_a_triple():
    """N = 5, three draws of position 0.  The first takes 0 and stores back() = 4 into slot 0; the second takes that 4 and stores into
    slot 4 -- indexed by the VALUE, a slot already popped -- so slot 0 still holds 4 and the third draw takes it again.  Erasing
    [randi] would never give an index twice."""
    t = ref.sample_triples(5, 1, _script([0, 0, 0]))
    assert t.tolist() == [[0, 4, 4]]
    assert not ref.distinct(t)[0]


@pytest.mark.parametrize("N,minInl,maxIts", [(100, 20, 300), (100, 6, 300), (100, 60, 300), (40, 20, 300), (20, 20, 300), (20, 20, 1), (15, 20, 300),
                                              (0, 6, 300), (300, 299, 300), (64, 33, 5), (1000, 20, 300), (8, 6, 300)])
def test_ransac_parameters(host, N, minInl, maxIts):
    """SetRansacParameters (:114-138): float epsilon, ceil(log / log), N == minInliers, N < minInliers (log of a negative), the clamp."""
    from weiner_slamit_v2_amd import api

    want = ref.ransac_iterations(N, 0.99, minInl, maxIts)
    assert host("its", N, minInl, maxIts) == [[want]]
    assert api.Sim3Solver.ransac_iterations(N, 0.99, minInl, maxIts) == want
    assert 1 <= want <= max(1, maxIts)
    if N == minInl or N < minInl:
        assert want == 1


SCANS = [
    # (counts, minInliers, maxIts, expected accepted, expected best, why)
    ([3, 5, 5, 4, 9, 2], 8, 6, 4, 4, "accepted on a strict >"),
    ([3, 8, 8, 4, 8, 2], 8, 6, -1, 4, "count == minInliers is never accepted; ties move the best forward"),
    ([0, 0, 0], 8, 3, -1, 2, "the best starts from mnBestInliers = 0 and >= takes every zero"),
    ([7, 7, 6, 7, 1, 1, 1, 1, 1, 1, 1, 12], 10, 12, 11, 11, "accepted in the third chunk of five"),
    ([5, 4, 3, 2, 1, 9, 9], 8, 5, -1, 0, "mRansacMaxIts cuts the scan before the good hypothesis"),
    ([9], 8, 1, 0, 0, "a single hypothesis"),
]


@pytest.mark.parametrize("counts,minInl,maxIts,acc,best,why", SCANS)
def test_acceptance_scan(host, counts, minInl, maxIts, acc, best, why):
    """iterate()'s rule (:183-204), C++ and Python, fed whole and in chunks of 5: same accepted index, same best, same bNoMore."""
    from weiner_slamit_v2_amd import api

    for chunk in (5, maxIts):
        want = ref.Scan(len(counts) + 100, counts, minInl, maxIts)
        lines = host("scan", minInl, maxIts, chunk, *counts)
        st = dict(it=0, best_n=0, best=-1)
        for ln in lines:
            w = want.iterate(chunk)
            assert (ln[0], bool(ln[1])) == (w[0], w[1]) and ln[2] == want.best and ln[3] == want.mnBestInliers, why
            a, b, st["best_n"], st["it"], nm = api.Sim3Solver.scan(counts, st["it"], chunk, st["it"], maxIts, st["best_n"], minInl)
            st["best"] = b if b >= 0 else st["best"]
            assert (a, nm) == (w[0], w[1]) and st["best"] == want.best and st["best_n"] == want.mnBestInliers, why
        assert lines[-1][0] == acc and lines[-1][2] == best, why
        assert bool(lines[-1][1]) == (acc < 0), why       # bNoMore ends an unsuccessful scan, and only that


def test_scan_returns_at_once_below_min_inliers():
    s = ref.Scan(5, [9, 9], 6, 2)
    assert s.iterate(5) == (-1, True, 0)


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_header_keeps_the_reference_surface():
    _build()
    hdr = open(os.path.join(SHIM, "Sim3Solver.h")).read()
    for want in ("Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true",
                 "void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)",
                 "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)",
                 "cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers)", "cv::Mat GetEstimatedRotation()",
                 "cv::Mat GetEstimatedTranslation()", "float GetEstimatedScale()", "static int EvaluateAll(std::vector<Sim3Solver*>& vpSolvers)"):
        assert want in hdr, want


@pytest.mark.gpu
def test_shim_sim3solver_matches_the_binding(tmp_path):
    """shim_test sim3solver: six candidates' solvers through the C++ template over the C-ABI, EvaluateAll in one call, iterate(5) until
    accepted; api.Sim3Solver on the same data and the same RandomInt stream accepts the same hypothesis with the same count, T12 and flags."""
    from weiner_slamit_v2_amd import api

    _build()
    ks, lead = [3, 6, 8, 10, 12, 15], 2
    rand_int, u = ref.scripted_rand(4242, 6 * 2000)
    blob = struct.pack("<ii", len(ks), len(u)) + u.tobytes()
    solvers, probs = [], []
    for k in ks:
        pr = ref.fixture(k)
        n = len(pr["max_err1"])
        blob += struct.pack("<iiiii", n, lead, int(pr["fix_scale"]), pr["min_inliers"], 300) + pr["intr1"].tobytes() + pr["intr2"].tobytes()
        blob += pr["x1"].tobytes() + pr["x2"].tobytes() + pr["sigma2_1"].tobytes() + pr["sigma2_2"].tobytes()
        s = api.Sim3Solver(pr, rand_int)                       # draws for the default parameters, like the C++ constructor
        s.SetRansacParameters(0.99, pr["min_inliers"], 300)
        solvers.append(s)
        probs.append(pr)
    pin, pout = tmp_path / "s.bin", tmp_path / "o.bin"
    open(pin, "wb").write(blob)
    out = subprocess.check_output([EXE, "sim3solver", str(pin), str(pout)]).decode()
    assert out.count("accepted hypothesis") == len(ks)
    raw = open(pout, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == 0
    api.Sim3Solver.EvaluateAll(solvers)
    off = 4
    for s, pr in zip(solvers, probs):
        n = len(pr["max_err1"])
        acc, nin, ncalls, its = struct.unpack_from("<iiii", raw, off)
        f = np.frombuffer(raw, np.float32, 29, off + 16)
        vb = np.frombuffer(raw, np.uint8, lead + n, off + 16 + 116).astype(bool)
        off += 16 + 116 + lead + n
        T, calls = None, 0
        no_more = False
        while T is None and not no_more:
            T, no_more, flags, cnt = s.iterate(5)
            calls += 1
        assert its == s.mRansacMaxIts and (acc, nin, ncalls) == (s.accepted, cnt, calls) and acc >= 0
        assert np.array_equal(f[:16].reshape(4, 4), T)
        assert np.array_equal(f[16:25].reshape(3, 3), s.GetEstimatedRotation()) and np.array_equal(f[25:28], s.GetEstimatedTranslation()) and f[28] == np.float32(s.GetEstimatedScale())
        assert not vb[:lead].any() and np.array_equal(vb[lead:], flags)
