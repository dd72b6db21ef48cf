"""The compile-time choice of the shim's stereo paths (shim/shim_common.h's member detection): a translation unit whose types have
mTrackProjXR / mbf instantiates the three drivers with the right-image gate, and one whose types lack them still compiles, its
drivers being the monocular code that refuses stereo frames.  Compile only: no device, no library."""
import os
import subprocess

import pytest

from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")

TU = r'''
#include <set>
#include "ORBmatcher.h"
using namespace ORB_SLAM2;
struct KF;
struct Point {
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos, mTrackProjX, mTrackProjY;
#if STEREO_MEMBERS
    float mTrackProjXR;
#endif
    bool isBad() { return false; }
    bool IsInKeyFrame(KF*) { return false; }
    int Observations() { return 1; }
    cv::Mat GetDescriptor() { return cv::Mat(1, 32, CV_8U); }
    cv::Mat GetWorldPos() { return cv::Mat(3, 1, CV_32F); }
    cv::Mat GetNormal() { return cv::Mat(3, 1, CV_32F); }
    float GetMaxDistance() { return 1.f; }
    float GetMinDistance() { return 1.f; }
    float GetMaxDistanceInvariance() { return 1.f; }
    float GetMinDistanceInvariance() { return 1.f; }
    int PredictScale(const float&, const float&) { return 0; }
    void Replace(Point*) {}
    void AddObservation(KF*, size_t) {}
};
struct Frame {
    int N;
    cv::Mat mTcw, mDescriptors;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<Point*> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors;
    std::vector<bool> mvbOutlier;
    float fx, fy, cx, cy, mb, mfLogScaleFactor;
#if STEREO_MEMBERS
    float mbf;
#endif
    static float mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
};
struct KF {
    float fx, fy, cx, cy, mfLogScaleFactor;
#if STEREO_MEMBERS
    float mbf;
#endif
    float mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
    cv::Mat mDescriptors;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat GetRotation() { return cv::Mat(3, 3, CV_32F); }
    cv::Mat GetTranslation() { return cv::Mat(3, 1, CV_32F); }
    cv::Mat GetCameraCenter() { return cv::Mat(3, 1, CV_32F); }
    bool IsInImage(const float&, const float&) const { return true; }
    Point* GetMapPoint(size_t) { return 0; }
    void AddMapPoint(Point*, size_t) {}
};
static_assert(shim::has_member_mTrackProjXR<Point>::value == (STEREO_MEMBERS != 0), "mTrackProjXR on the map point");
static_assert(shim::has_member_mbf<Frame>::value == (STEREO_MEMBERS != 0), "mbf on the frame");
static_assert(shim::has_member_mbf<KF>::value == (STEREO_MEMBERS != 0), "mbf on the keyframe");
int drive(Frame& F, Frame& L, KF* K, std::vector<KF*>& targets, std::vector<Point*>& pts) {
    ORBmatcher host(0.8f, true), device(0.8f, true, true);
    return host.SearchByProjection(F, pts, 3.f) + host.SearchByProjection(F, L, 7.f, false) + device.SearchByProjection(F, L, 7.f, false) +
           host.Fuse(K, pts, 3.f) + device.Fuse(K, pts, 3.f) + host.Fuse(targets, pts, 3.f) + device.Fuse(targets, pts, 3.f);
}
'''


@pytest.mark.parametrize("stereo_members", (1, 0))
def test_three_drivers_instantiate(tmp_path, stereo_members):
    src = tmp_path / "tu.cc"
    src.write_text(TU)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-DSTEREO_MEMBERS=%d" % stereo_members,
                           "-I", SHIM, "-c", str(src), "-o", str(tmp_path / "tu.o")])
    names = subprocess.check_output(["nm", "-C", str(tmp_path / "tu.o")]).decode()
    assert "ORBmatcher::Fuse" in names and "SearchByProjection" in names
