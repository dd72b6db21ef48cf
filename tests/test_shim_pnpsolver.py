"""shim/PnPsolver.h: the host logic on the CPU (SetRansacParameters, the sampler, the records and the scan with Refine(), in C++
against the line-by-line restatements of tests/pnp_ref.py) and, on the GPU, the C++ class over the C-ABI against api.PnPsolver."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pnp_ref as ref
from tests.helpers import ROOT
from tests.test_pnp_ref import PARAMS

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")

HOST = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "PnPsolver.h"
using namespace ORB_SLAM2;
static std::vector<unsigned> script; static size_t pos = 0;
static int scripted(int lo, int hi) { unsigned v = pos < script.size() ? script[pos] : 0u; ++pos; return lo + (int)(v % (unsigned)(hi - lo + 1)); }
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "sample")) {          // sample N count v0 v1 ...
        const int N = atoi(argv[2]), count = atoi(argv[3]);
        for (int i = 4; i < argc; ++i) script.push_back((unsigned)strtoul(argv[i], 0, 10));
        pnpsolver::RandomInt() = scripted;
        std::vector<int> avail;
        for (int h = 0; h < count; ++h) { int q[4]; pnpsolver::SampleQuad(N, avail, q); printf("%d %d %d %d\n", q[0], q[1], q[2], q[3]); }
    } else if (!strcmp(argv[1], "params")) {   // params N probability minInliers maxIts minSet epsilon
        const pnpsolver::Params P = pnpsolver::RansacParameters(atoi(argv[2]), atof(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), (float)atof(argv[7]));
        unsigned bits; memcpy(&bits, &P.epsilon, 4);
        printf("%d %d %u\n", P.minInliers, P.maxIts, bits);
    } else if (!strcmp(argv[1], "scan")) {     // scan minInliers maxIts chunk n c0 .. r0 .. : one line per iterate(chunk) call
        const int minInl = atoi(argv[2]), maxIts = atoi(argv[3]), chunk = atoi(argv[4]), n = atoi(argv[5]);
        std::vector<int32_t> c, r;
        for (int i = 0; i < n; ++i) c.push_back(atoi(argv[6 + i]));
        for (int i = 0; i < n; ++i) r.push_back(atoi(argv[6 + n + i]));
        const std::vector<int> rec = pnpsolver::Records(c.data(), 0, n, minInl, 0);
        printf("%d", (int)rec.size());
        for (size_t k = 0; k < rec.size(); ++k) printf(" %d", rec[k]);
        printf("\n");
        pnpsolver::ScanState st;
        for (int call = 0; call < 4; ++call) {
            bool noMore;
            if (pnpsolver::ScanNeeds(st, chunk, maxIts) > n) { printf("-1 -1 -1 -1 -1\n"); break; }
            const int what = pnpsolver::Scan(c.data(), r.data(), chunk, maxIts, minInl, st, noMore);
            printf("%d %d %d %d %d\n", what, noMore ? 1 : 0, st.best, st.mnBestInliers, st.mnIterations);
            if (what != pnpsolver::SCAN_NONE || noMore) break;
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("pnpsolver_host")
    open(str(d / "host.cc"), "w").write(HOST)
    exe = str(d / "host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-I", SHIM, "-I", os.path.join(ROOT, "include"), str(d / "host.cc"), "-o", exe])   # header only: no device, no library
    return lambda *a: [[int(v) for v in ln.split()] for ln in subprocess.check_output([exe] + [str(x) for x in a]).decode().splitlines()]


def _script(vals):
    it = iter(vals)
    return lambda lo, hi: lo + next(it) % (hi - lo + 1)


@pytest.mark.parametrize("N,vals", [(6, [0, 0, 0, 0, 5, 4, 3, 2]), (4, [3, 3, 1, 0, 2, 0, 1, 0]), (10, [9, 9, 9, 9, 3, 3, 3, 3]), (7, list(range(20, 48)))])
def test_sampler_reproduces_the_reference_quirk(host, N, vals):
    count = len(vals) // 4
    want = ref.sample_quads(N, count, _script(vals))
    assert np.array_equal(np.array(host("sample", N, count, *vals)), want)
    assert want.min() >= 0 and want.max() < N


@pytest.mark.parametrize("N,par,want", PARAMS)
def test_ransac_parameters(host, N, par, want):
    mi, its, eps = ref.set_ransac_parameters(N, *par)
    assert (mi, its) == want
    assert host("params", N, *par) == [[mi, its, int(np.float32(eps).view(np.uint32))]]


SCANS = [
    # (counts, refined count per hypothesis, minInliers, maxIts, chunk)
    ([0] * 8 + [30, 0, 0, 0], [0] * 8 + [31, 0, 0, 0], 20, 12, 5),            # the first iterate(5) runs to maxIts and accepts the 9th
    ([19, 20, 25, 25, 24, 40, 0, 0], [0, 20, 20, 0, 0, 41, 0, 0], 20, 8, 5),  # >= considers, > records, the refined count must exceed strictly
    ([22, 21, 0, 0, 0, 0], [20, 0, 0, 0, 0, 0], 20, 6, 5),                    # never accepted: the bNoMore tail returns the best
    ([5, 6, 7, 0, 0], [0] * 5, 20, 3, 5),                                     # maxIts < chunk: five hypotheses walked, nothing found
    ([5, 6, 7, 0, 0, 0, 30, 0, 0, 0], [0] * 6 + [40, 0, 0, 0], 20, 5, 5),     # a call after bNoMore takes its own hypotheses
]


@pytest.mark.parametrize("counts,refined,minInl,maxIts,chunk", SCANS)
def test_records_and_scan(host, counts, refined, minInl, maxIts, chunk):
    lines = host("scan", minInl, maxIts, chunk, len(counts), *(counts + refined))
    assert lines[0][1:] == ref.records(counts, minInl) and lines[0][0] == len(lines[0]) - 1
    s = ref.Solver(64, None, None, None, 0.99, minInl, maxIts, 4, 0.01, 5.991)
    assert (s.minInliers, s.maxIts) == (minInl, maxIts)
    s.quads = np.zeros((len(counts), 4), np.int32)
    s.counts, s.flags, s.pose = np.array(counts, np.int32), np.eye(len(counts), 64, dtype=bool), np.zeros((len(counts), 12))
    s.refine_fn = lambda sub: (np.zeros(12), refined[int(np.flatnonzero(sub)[0])], sub)
    kinds = {None: 0, "refined": 1, "best": 2}
    for ln in lines[1:]:
        if ln[0] < 0:
            break                                                              # the scripted counts are used up
        r = s.iterate(chunk)
        assert ln == [kinds[r["kind"]], int(r["bNoMore"]), s.best, s.mnBestInliers, s.mnIterations]


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_header_keeps_the_reference_surface():
    _build()
    hdr = open(os.path.join(SHIM, "PnPsolver.h")).read()
    for want in ("PnPsolver(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches",
                 "int SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991)",
                 "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)",
                 "cv::Mat find(std::vector<bool>& vbInliers, int& nInliers)", "static int EvaluateAll(std::vector<PnPsolver*>& vpSolvers)",
                 "another order than in the reference"):
        assert want in hdr, want
    assert '#include "PnPsolver.h"' in open(os.path.join(SHIM, "shim_main.cc")).read()


@pytest.mark.gpu
def test_shim_pnpsolver_matches_the_binding(tmp_path):
    """shim_test pnpsolver: the solvers of seven candidates through the C++ template over the C-ABI, EvaluateAll in two launches, iterate(5)
    until a pose or bNoMore; api.PnPsolver on the same data and the same RandomInt stream returns the same hypothesis, count, Tcw and flags.
    One more solver asks for minSet = 5 and is refused."""
    from weiner_slamit_v2_amd import api

    _build()
    names, lead = ["n12", "n64", "n65", "n257", "h300", "refine_fails_first", "never"], 3
    rand_int, u = ref.scripted_rand(4343, 8 * 2000)
    blob = struct.pack("<ii", len(names) + 1, len(u)) + u.tobytes()
    solvers = []
    for name in names + ["n40"]:
        pr = ref.fixture(name)
        _, mi, its, ms, eps, th2 = pr["params"]
        ms = 5 if name == "n40" else ms
        blob += struct.pack("<iiiiiff", pr["n"], lead, mi, its, ms, eps, th2) + np.asarray(pr["intr"], np.float32).tobytes()
        blob += pr["p3d"].tobytes() + pr["p2d"].tobytes() + pr["sigma2"].tobytes()
        if name != "n40":
            s = api.PnPsolver(pr, rand_int)
            s.SetRansacParameters(*pr["params"])
            solvers.append(s)
    pin, pout = tmp_path / "s.bin", tmp_path / "o.bin"
    open(pin, "wb").write(blob)
    subprocess.check_output([EXE, "pnpsolver", str(pin), str(pout)])
    raw = open(pout, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == 0
    api.PnPsolver.EvaluateAll(solvers)
    off, seen = 4, set()
    for name, s in zip(names, solvers):
        n = s.N
        st, acc, nin, ncalls, its, mi, nm = struct.unpack_from("<iiiiiii", raw, off)
        T = np.frombuffer(raw, np.float32, 16, off + 28).reshape(4, 4)
        vb = np.frombuffer(raw, np.uint8, lead + n, off + 28 + 64).astype(bool)
        off += 28 + 64 + lead + n
        Tp, calls, no_more = None, 0, False
        while Tp is None and not no_more:
            Tp, no_more, flags, cnt = s.iterate(5)
            calls += 1
        seen.add(s.kind)
        assert st == 0 and (its, mi) == (s.mRansacMaxIts, s.mRansacMinInliers)
        assert (acc, nin, ncalls, bool(nm)) == (s.accepted, cnt, calls, no_more), name
        assert np.array_equal(T, Tp if Tp is not None else np.zeros((4, 4), np.float32))
        assert not vb[:lead].any() and np.array_equal(vb[lead:], flags)
    assert seen == {"refined", "best"}
    st, acc, nin, ncalls, its, mi, nm = struct.unpack_from("<iiiiiii", raw, off)
    assert st == -1 and acc == -1 and nin == 0 and nm == 1                      # SLAMIT_ERR_ARG, and bNoMore at once
