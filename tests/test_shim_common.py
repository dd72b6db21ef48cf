"""shim/shim_common.h on the CPU: the rotation histogram against a float32 restatement of the reference's binning and
ComputeThreeMaxima, and LastStatus() as the calling thread's own (two threads, ordered with promises; every call is one that is
refused or returns before the device, so the outcome is the same with and without a GPU)."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
LIBDIR = os.path.join(ROOT, "weiner_slamit_v2_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")   # as shim/Makefile's ROCM
F32 = np.float32
ERR_ARG = -1   # SLAMIT_ERR_ARG (include/slamit.h)

# ---- a. the histogram ---------------------------------------------------------------------------------------------------------

HISTO = r'''
#include <stdio.h>
#include "shim_common.h"
int main(int argc, char** argv) {   // pairs.bin: float32 angle1, angle2 per pair; the payload is the pair's index
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    ORB_SLAM2::shim::RotationHistogram h;
    float a[2];
    for (int i = 0; fread(a, 4, 2, f) == 2; ++i) h.add(a[0], a[1], i);
    fclose(f);
    h.reject([](int payload) { printf("%d\n", payload); });
    return 0;
}
'''


@pytest.fixture(scope="module")
def histo(tmp_path_factory):
    d = tmp_path_factory.mktemp("shim_common_histo")
    open(str(d / "histo.cc"), "w").write(HISTO)
    exe = str(d / "histo")
    # the shim's own flags; header only: no device, no library
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-I", SHIM, str(d / "histo.cc"), "-o", exe])

    def run(pairs):
        p = d / "pairs.bin"
        np.asarray(pairs, F32).reshape(-1, 2).tofile(str(p))
        return [int(v) for v in subprocess.check_output([exe, str(p)]).decode().split()]

    return run


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1605-1646): strict '>' in bin order, the 10 % rule in float32.  -> (i1, i2, i3)"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if max2 < F32(0.1) * F32(max1):
        i2 = i3 = -1
    elif max3 < F32(0.1) * F32(max1):
        i3 = -1
    return i1, i2, i3


def restate(pairs):
    """The reference's filter (ORBmatcher.cc:240-250, 271-289) in float32 at every step. -> (rejected payloads in order, kept bins, bin sizes)"""
    factor = F32(1) / F32(30)
    hist = [[] for _ in range(30)]
    for k, (a1, a2) in enumerate(np.asarray(pairs, F32).reshape(-1, 2)):
        rot = F32(a1 - a2)
        if rot < 0:
            rot = F32(rot + F32(360))
        x = F32(rot * factor)
        b = int(math.floor(float(x) + 0.5))   # roundf of a non-negative float32: the sum is exact in double
        if b == 30:
            b = 0
        if 0 <= b < 30:
            hist[b].append(k)
    sizes = [len(h) for h in hist]
    keep = three_maxima(sizes)
    return [k for b in range(30) if b not in keep for k in hist[b]], keep, sizes


def bins(*populations):
    """pairs whose difference sits in the middle of bin 1, 2, ... (30 degrees each), populations[i] of them in bin i + 1, interleaved"""
    out = []
    for j in range(max(populations)):
        for b, n in enumerate(populations):
            if j < n:
                out.append((30.0 * (b + 1) + 7.0, 7.0))
    return out


def _cases():
    rs = np.random.RandomState(5)
    halves = [(15, 0), (45, 0), (200, 185), (10, 325), (75, 30), (15, 0), (45, 0), (100, 100), (3, 2)]
    return {
        "random": rs.uniform(0, 360, (200, 2)).astype(F32),
        "equal_angles": [(a, a) for a in rs.uniform(0, 360, 20).astype(F32)] + bins(1, 1, 1, 1),
        "a1_below_a2": [(a, a + 100.0) for a in rs.uniform(0, 250, 12)] + [(10.0, 200.0), (0.0, 359.5), (5.0, 70.0), (5.0, 160.0)],
        "halves": halves,
        "equal_bins": bins(5, 5, 5, 5),
        "empty": [],
        "tenth_30_3_1": bins(30, 3, 1) + bins(0, 0, 0, 0, 1),   # 0.1f * 30 == 3 in float32: 3 < 3 is false, the second bin stays
        "tenth_10_1_1": bins(10, 1, 1) + bins(0, 0, 0, 0, 1),
        "tenth_30_2_1": bins(30, 2, 1),                          # 2 < 3: the second and the third go
        "tenth_40_5_3": bins(40, 5, 3),                          # 3 < 4: only the third goes
    }


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_histogram_rejects_what_the_reference_rejects(histo, name):
    want, _, _ = restate(CASES[name])
    assert histo(CASES[name]) == want   # lists: bins in ascending order, entries in insertion order


def test_histogram_cases_bite():
    """The premises: a restatement that trips one of them would let the comparison above pass vacuously."""
    res = {k: restate(v) for k, v in CASES.items()}
    assert sum(len(r[0]) > 0 for r in res.values()) >= 6 and len(res["random"][0]) > 50
    assert res["empty"][0] == []
    # equal sizes: the first three win, the fourth is rejected
    assert res["equal_bins"][1] == (1, 2, 3) and res["equal_bins"][0] == [3, 7, 11, 15, 19]
    # the boundary of the 10 % rule: kept when the product is rounded to float32 (0.1f * 30 == 3 and 0.1f * 10 == 1 exactly); a
    # restatement that multiplies the float32 constant in double drops them: 3 < 3.0000000447
    assert F32(0.1) * F32(30) == 3 and F32(0.1) * F32(10) == 1 and 3 < float(F32(0.1)) * 30.0 and 1 < float(F32(0.1)) * 10.0
    assert res["tenth_30_3_1"][1] == (1, 2, -1) and len(res["tenth_30_3_1"][0]) == 2   # the second stays, the third (1 < 3) goes
    assert res["tenth_10_1_1"][1] == (1, 2, 3) and len(res["tenth_10_1_1"][0]) == 1
    assert res["tenth_30_2_1"][1] == (1, -1, -1) and len(res["tenth_30_2_1"][0]) == 3
    assert res["tenth_40_5_3"][1] == (1, 2, -1) and len(res["tenth_40_5_3"][0]) == 3
    # 15 and 45 degrees are halves after scaling, and the +360 branch is taken
    factor = F32(1) / F32(30)
    assert any(abs(float(F32(F32(d) * factor)) % 1.0 - 0.5) < 1e-6 for d in (15, 45))
    assert any(a1 < a2 for a1, a2 in CASES["a1_below_a2"]) and sum(res["a1_below_a2"][2]) == len(CASES["a1_below_a2"])
    assert sum(res["halves"][2]) == len(CASES["halves"])


# ---- b. LastStatus() is the calling thread's ---------------------------------------------------------------------------------------

THREADS = r'''
#include <stdio.h>
#include <future>
#include <map>
#include <thread>
#include "LocalMapping.h"
#include "ORBmatcher.h"
using namespace ORB_SLAM2;

struct Point {
    bool mbTrackInView; int mnTrackScaleLevel; float mTrackViewCos, mTrackProjX, mTrackProjY;
    bool isBad() { return false; }
    int Observations() { return 1; }
    cv::Mat GetDescriptor() { return cv::Mat::zeros(1, 32, CV_8U); }
};
struct Frame {
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::vector<Point*> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors;
    float mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv;
};
struct KeyFrame {
    int N;
    std::map<unsigned, std::vector<unsigned> > mFeatVec;
    cv::Mat mDescriptors, m;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvScaleFactors, mvLevelSigma2;
    float fx, fy, cx, cy, invfx, invfy, mfScaleFactor;
    Point* GetMapPoint(size_t) { return 0; }
    cv::Mat GetCameraCenter() { return m; }
    cv::Mat GetRotation() { return m; }
    cv::Mat GetTranslation() { return m; }
    float ComputeSceneMedianDepth(int) { return 1.f; }
};

int main() {
    std::promise<void> aRefused, bDone;
    int a1 = 99, a2 = 99, aLM = 99, b1 = 99, b2 = 99, bLM = 99, b3 = 99, ret = 99;
    std::thread A([&] {
        Frame F;
        F.mvKeysUn.resize(2); F.mvpMapPoints.assign(2, (Point*)0); F.mvScaleFactors.assign(8, 1.f);
        F.mvuRight.assign(2, -1.f); F.mvuRight[0] = 5.f;   // a stereo keypoint: refused before any device call
        F.mnMinX = F.mnMinY = 0.f; F.mfGridElementWidthInv = F.mfGridElementHeightInv = 0.1f;
        std::vector<Point*> points;
        ORBmatcher matcher(0.8f);
        ret = matcher.SearchByProjection(F, points, 3.f);
        a1 = ORBmatcher::LastStatus();
        aRefused.set_value();
        bDone.get_future().wait();
        a2 = ORBmatcher::LastStatus();       // B's calls in between have not touched it
        aLM = LocalMapping::LastStatus();    // nor has B's refusal become A's
    });
    std::thread B([&] {
        aRefused.get_future().wait();
        b1 = ORBmatcher::LastStatus();       // B has made no call
        std::vector<cv::KeyPoint> keys;
        std::vector<uint8_t> taken;
        std::vector<int> matchKp;
        ORBmatcher::GuidedQueries none;      // zero queries: returns before the device
        ORBmatcher::GuidedSearch(keys, cv::Mat(), taken, 0.f, 0.f, 1.f, 1.f, none, ORBmatcher::TH_LOW, false, 0.6f, matchKp);
        b2 = ORBmatcher::LastStatus();
        KeyFrame cur;
        std::vector<KeyFrame*> neigh;
        LocalMapping::CreateNewMapPoints(&cur, neigh, /*monocular*/ false, [](const cv::Mat&, int, int, KeyFrame*) {});
        bLM = LocalMapping::LastStatus();
        b3 = ORBmatcher::LastStatus();
        bDone.set_value();
    });
    A.join(); B.join();
    printf("%d %d %d %d %d %d %d %d\n", ret, a1, b1, b2, bLM, b3, a2, aLM);
    return 0;
}
'''


def test_last_status_is_the_calling_threads(tmp_path):
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])
    src, exe = tmp_path / "threads.cc", tmp_path / "threads"
    src.write_text(THREADS)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-I", SHIM, str(src), "-o", str(exe), "-L" + SHIM, "-lslamit_shim",
                           "-L" + LIBDIR, "-lslamit_hip", "-L" + ROCM_LIB, "-Wl,-rpath-link," + ROCM_LIB, "-Wl,-rpath," + SHIM,
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB, "-lpthread"])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    ret, a1, b1, b2, b_lm, b3, a2, a_lm = [int(v) for v in p.stdout.decode().split()]
    assert ret == 0 and a1 == ERR_ARG                    # A: refused, with the named code
    assert b1 == 0 and b2 == 0                           # B: SLAMIT_OK before and after a search of its own
    assert b_lm == ERR_ARG and b3 == 0                   # B: its LocalMapping refusal, its matcher status untouched
    assert a2 == ERR_ARG and a_lm == 0                   # A: still its own refusal; B's is not A's
    assert b"only the monocular path is on the device" in p.stderr
