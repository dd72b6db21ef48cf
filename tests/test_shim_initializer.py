"""shim/Initializer.h: the sampler on the CPU against the binding's, the class surface, and on the GPU the C++ class over the
C-ABI: InitializeAll of eight frame pairs equals eight Initialize calls and api.Initializer on the same RandomInt stream."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import initializer_ref as ref
from tests import pnp_ref
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")
PAIRS = ("general", "planar", "general_outliers", "rotation", "few", "ambiguous", "eight", "n65")

HOST = r'''
#include <stdio.h>
#include <stdlib.h>
#include "Initializer.h"
#include "PnPsolver.h"
using namespace ORB_SLAM2;
static std::vector<unsigned> script; static size_t pos = 0;
static int scripted(int lo, int hi) { unsigned v = pos < script.size() ? script[pos] : 0u; ++pos; return lo + (int)(v % (unsigned)(hi - lo + 1)); }
int main(int argc, char** argv) {   // N count v0 v1 ...
    const int N = atoi(argv[1]), count = atoi(argv[2]);
    for (int i = 3; i < argc; ++i) script.push_back((unsigned)strtoul(argv[i], 0, 10));
    pnpsolver::RandomInt() = scripted;          // one hook: what PnPsolver's name sets, the Initializer's sampler draws from
    if (shim::RandomInt() != scripted) return 1;
    std::vector<int> avail;
    for (int h = 0; h < count; ++h) {
        int32_t s[8];
        initializer::SampleSet(N, avail, s);
        for (int j = 0; j < 8; ++j) printf("%d ", s[j]);
        printf("\n");
    }
    return 0;
}
'''


def test_sampler_draws_without_replacement_from_the_shared_hook(tmp_path):
    from weiner_slamit_v2_amd import api

    open(str(tmp_path / "host.cc"), "w").write(HOST)
    exe = str(tmp_path / "host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-I", SHIM, "-I", os.path.join(ROOT, "include"), str(tmp_path / "host.cc"), "-o", exe])   # header only
    for N, count in ((8, 3), (9, 5), (150, 20)):
        rand_int, u = pnp_ref.scripted_rand(N, 8 * count)
        got = np.array([[int(v) for v in ln.split()] for ln in subprocess.check_output([exe, str(N), str(count)] + [str(int(v)) for v in u]).decode().splitlines()])
        want = api.Initializer.sample_sets(N, count, rand_int)
        assert np.array_equal(got, want)
        assert all(len(set(row)) == 8 and min(row) >= 0 and max(row) < N for row in got)


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_header_keeps_the_reference_surface():
    _build()
    hdr = open(os.path.join(SHIM, "Initializer.h")).read()
    for want in ("Initializer(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200",
                 "bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,",
                 "std::vector<bool>& vbTriangulated)", "static int InitializeAll(std::vector<Job>& jobs)", "SeedRandOnce(0)"):
        assert want in hdr, want
    assert '#include "Initializer.h"' in open(os.path.join(SHIM, "shim_main.cc")).read()
    common = open(os.path.join(SHIM, "shim_common.h")).read()
    assert "inline RandomIntFn& RandomInt()" in common and "using shim::RandomInt;" in open(os.path.join(SHIM, "PnPsolver.h")).read()


@pytest.mark.gpu
def test_shim_initializer_matches_the_binding(tmp_path):
    """shim_test initializer: eight frame pairs through the C++ template, once in one InitializeAll (two launches) and once pair by
    pair; api.Initializer on the same data and RandomInt stream returns the same verdict, model, motion, pose, points and flags."""
    from weiner_slamit_v2_amd import api

    _build()
    rand_int, u = pnp_ref.scripted_rand(77, 8 * 8 * 200)
    blob = struct.pack("<ii", len(PAIRS), len(u)) + u.tobytes()
    jobs = []
    for name in PAIRS:
        pr = ref.fixture(name)
        its = len(pr["sets"])
        blob += struct.pack("<iiif", len(pr["keys1"]), len(pr["keys2"]), its, pr["sigma"]) + np.asarray(pr["K"], np.float32).tobytes()
        blob += pr["keys1"].tobytes() + pr["keys2"].tobytes() + np.asarray(pr["vMatches12"], np.int32).tobytes()
        jobs.append((api.Initializer(pr["keys1"], pr["K"], pr["sigma"], its, rand_int), pr["keys2"], pr["vMatches12"]))
    pin, pout = tmp_path / "p.bin", tmp_path / "o.bin"
    open(pin, "wb").write(blob)
    subprocess.check_output([EXE, "initializer", str(pin), str(pout)])
    raw = open(pout, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == 0
    want = api.Initializer.InitializeAll(jobs)
    off, passes = 4, []
    for _ in range(2):
        got = []
        for name in PAIRS:
            n1 = len(ref.fixture(name)["keys1"])
            ok, kind, motion, nsets = struct.unpack_from("<iiii", raw, off)
            rt = np.frombuffer(raw, np.float32, 12, off + 16)
            p = np.frombuffer(raw, np.float32, 3 * n1, off + 64).reshape(n1, 3)
            vb = np.frombuffer(raw, np.uint8, n1, off + 64 + 12 * n1).astype(bool)
            sets = np.frombuffer(raw, np.int32, 8 * nsets, off + 64 + 13 * n1).reshape(nsets, 8)
            off += 64 + 13 * n1 + 32 * nsets
            got.append((ok, kind, motion, rt, p, vb, sets))
        passes.append(got)
    assert off == len(raw)
    seen = set()
    for (ini, _, _), a, b, w in zip(jobs, passes[0], passes[1], want):
        for x, y in zip(a, b):                                               # InitializeAll == Initialize, pair by pair
            assert np.array_equal(x, y)
        ok, kind, motion, rt, p, vb, sets = a
        assert np.array_equal(sets, ini.last["problem"]["sets"])
        assert (bool(ok), kind, motion) == (w[0], ini.last["kind"], ini.last["motion"])
        assert np.array_equal(rt[:9].view(np.uint32), w[1].reshape(9).view(np.uint32)) and np.array_equal(rt[9:].view(np.uint32), w[2].view(np.uint32))
        assert np.array_equal(p.view(np.uint32), w[3].view(np.uint32)) and np.array_equal(vb, w[4])
        seen.add((bool(ok), kind))
    assert {k for _, k in seen} == {0, 1} and {o for o, _ in seen} == {True, False}   # both models, both verdicts
