// FrameOps.h — the three Frame member functions that sit between the extractor and the guided search, backed by
// libslamit_hip.so: Frame::ComputeImageBounds (ORB_SLAM2/src/Frame.cc:561-590), Frame::UndistortKeyPoints (:529-559)
// and Frame::AssignFeaturesToGrid (:336-357).  Frame itself (a data-model class) stays the caller's: these are
// templates over it, like shim/Optimizer.h, so the reference's Frame.cc can forward its three bodies here:
//
//     void Frame::UndistortKeyPoints()   { ORB_SLAM2::FrameOps::UndistortAndAssign(*this); }   // does both ...
//     void Frame::AssignFeaturesToGrid() {}                                                     // ... in one device call
//     void Frame::ComputeImageBounds(const cv::Mat& im) { ORB_SLAM2::FrameOps::ComputeImageBounds(*this, im); }
//
// Members used on the caller's type (all from include/Frame.h): N, mvKeys, mvKeysUn, mK (3x3 CV_32F), mDistCoef (4x1 or
// 5x1 CV_32F), mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS] (std::vector<std::size_t>), and the statics mnMinX, mnMaxX, mnMinY,
// mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv.
//
// Frame::ComputeStereoMatches (:591-763) forwards the same way:
//
//     void Frame::ComputeStereoMatches() { ORB_SLAM2::FrameOps::ComputeStereoMatches(*this); }
//
// It reads mvKeys, mvKeysRight, mDescriptors, mDescriptorsRight, mb, mbf and the two extractors (mpORBextractorLeft / Right, the
// shim's, whose last calls left both pyramids in HBM: no SetPyramidExport) and writes mvuRight and mvDepth.  include/slamit.h lists
// where the device walk departs from the reference (status 8: out-of-range octaves, rows and windows the reference reads anyway).
//
// Frame::ComputeStereoFromRGBD (:766-787) forwards the same way:
//
//     void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth) { ORB_SLAM2::FrameOps::ComputeStereoFromRGBD(*this, imDepth); }
//
// It reads mvKeys, mvKeysUn and mbf and writes mvuRight and mvDepth in one staged device call (csrc/unproject.h).  imDepth is the
// CV_32F image Tracking::GrabImageRGBD converted (factor 1), or the sensor's own 16-bit image with depthMapFactor = mDepthMapFactor,
// which saves the convertTo: the device multiplies as it reads.  A Frame type without mbf, mvDepth and mvKeys is refused on stderr
// with LastStatus() == SLAMIT_ERR_ARG, as the other stereo paths are chosen by the members the caller's type has.
#ifndef SLAMIT_SHIM_FRAMEOPS_H
#define SLAMIT_SHIM_FRAMEOPS_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#ifdef SLAMIT_USE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

#include "shim_common.h"

namespace ORB_SLAM2 {
namespace FrameOps {

struct Status {};   // FrameOps is a namespace: the tag of its per-thread status cell
inline int& lastStatus() { return shim::status<Status>(); }
inline int LastStatus() { return lastStatus(); }

template <class FrameT>
slamit_camera CameraOf(const FrameT& F) {
    slamit_camera c;
    c.fx = F.mK.template at<float>(0, 0); c.fy = F.mK.template at<float>(1, 1);
    c.cx = F.mK.template at<float>(0, 2); c.cy = F.mK.template at<float>(1, 2);
    c.k1 = F.mDistCoef.template at<float>(0, 0); c.k2 = F.mDistCoef.template at<float>(1, 0);
    c.p1 = F.mDistCoef.template at<float>(2, 0); c.p2 = F.mDistCoef.template at<float>(3, 0);
    c.k3 = F.mDistCoef.rows >= 5 ? F.mDistCoef.template at<float>(4, 0) : 0.f;
    return c;
}

// Frame::ComputeImageBounds (Frame.cc:561-590) + the grid constants of the first-frame branch (:113-118)
template <class FrameT>
void ComputeImageBounds(FrameT& F, const cv::Mat& imLeft) {
    if (F.mDistCoef.template at<float>(0, 0) != 0.0) {
        const slamit_camera c = CameraOf(F);
        const float in[8] = {0.f, 0.f, (float)imLeft.cols, 0.f, 0.f, (float)imLeft.rows, (float)imLeft.cols, (float)imLeft.rows};
        float out[8];
        lastStatus() = slamit_undistort_points(0, &c, in, 4, out);
        if (lastStatus() != SLAMIT_OK) return;
        FrameT::mnMinX = std::min(out[0], out[4]); FrameT::mnMaxX = std::max(out[2], out[6]);
        FrameT::mnMinY = std::min(out[1], out[3]); FrameT::mnMaxY = std::max(out[5], out[7]);
    } else {
        FrameT::mnMinX = 0.0f; FrameT::mnMaxX = imLeft.cols;
        FrameT::mnMinY = 0.0f; FrameT::mnMaxY = imLeft.rows;
    }
    FrameT::mfGridElementWidthInv = static_cast<float>(SLAMIT_FRAME_GRID_COLS) / (FrameT::mnMaxX - FrameT::mnMinX);
    FrameT::mfGridElementHeightInv = static_cast<float>(SLAMIT_FRAME_GRID_ROWS) / (FrameT::mnMaxY - FrameT::mnMinY);
}

// Frame::UndistortKeyPoints + Frame::AssignFeaturesToGrid in one device call: fills mvKeysUn and mGrid
template <class FrameT>
void UndistortAndAssign(FrameT& F) {
    const int n = (int)F.mvKeys.size();
    const slamit_camera c = CameraOf(F);
    static_assert(sizeof(cv::KeyPoint) == sizeof(slamit_kp), "cv::KeyPoint must be the 28-byte record");
    F.mvKeysUn.resize(n);
    std::vector<int32_t> start(SLAMIT_FRAME_GRID_CELLS + 1), items((size_t)std::max(n, 1));
    lastStatus() = slamit_frame_finish(0, &c, reinterpret_cast<const slamit_kp*>(F.mvKeys.data()), n, FrameT::mnMinX, FrameT::mnMinY,
                                       FrameT::mfGridElementWidthInv, FrameT::mfGridElementHeightInv,
                                       reinterpret_cast<slamit_kp*>(F.mvKeysUn.data()), start.data(), items.data());
    for (int x = 0; x < SLAMIT_FRAME_GRID_COLS; ++x)
        for (int y = 0; y < SLAMIT_FRAME_GRID_ROWS; ++y) {
            std::vector<std::size_t>& cell = F.mGrid[x][y];
            cell.clear();
            if (lastStatus() != SLAMIT_OK) continue;   // silent failure like the reference: an empty grid
            const int c0 = start[x * SLAMIT_FRAME_GRID_ROWS + y], c1 = start[x * SLAMIT_FRAME_GRID_ROWS + y + 1];
            cell.reserve(c1 - c0);
            for (int j = c0; j < c1; ++j) cell.push_back((std::size_t)items[j]);
        }
}

// Frame::ComputeStereoMatches: one staged device call on the two extractors' pyramids.  A failure leaves every keypoint unmatched
// (-1) and its code in LastStatus(); `status` (optional) receives the per-keypoint codes of include/slamit.h.
template <class FrameT>
void ComputeStereoMatches(FrameT& F, std::vector<uint8_t>* status = 0) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(slamit_kp), "cv::KeyPoint must be the 28-byte record");
    const int nl = (int)F.mvKeys.size(), nr = (int)F.mvKeysRight.size();
    F.mvuRight.assign(nl, -1.0f);
    F.mvDepth.assign(nl, -1.0f);
    if (status) status->assign(nl, 1);
    lastStatus() = SLAMIT_OK;
    if (nl == 0) return;
    if (!F.mpORBextractorLeft || !F.mpORBextractorRight || F.mDescriptors.rows != nl || F.mDescriptorsRight.rows != nr) {
        shim::refuse<Status>("FrameOps::ComputeStereoMatches: extractors or descriptors missing");
        return;
    }
    std::vector<uint8_t> dl((size_t)nl * 32), dr((size_t)std::max(nr, 1) * 32), st((size_t)nl);
    for (int i = 0; i < nl; ++i) memcpy(&dl[(size_t)i * 32], F.mDescriptors.ptr(i), 32);
    for (int i = 0; i < nr; ++i) memcpy(&dr[(size_t)i * 32], F.mDescriptorsRight.ptr(i), 32);
    std::vector<float> u(nl), d(nl);
    const int rc = slamit_stereo_match(F.mpORBextractorLeft->Handle(), F.mpORBextractorRight->Handle(), 0,
                                       reinterpret_cast<const slamit_kp*>(F.mvKeys.data()), dl.data(), nl,
                                       reinterpret_cast<const slamit_kp*>(F.mvKeysRight.data()), dr.data(), nr, F.mb, F.mbf, u.data(), d.data(),
                                       st.data(), 0, 0, 0, 0);
    if (rc != SLAMIT_OK) { shim::report<Status>("slamit_stereo_match", rc); return; }
    F.mvuRight.swap(u);
    F.mvDepth.swap(d);
    if (status) status->swap(st);
}

// Frame::ComputeStereoFromRGBD.  A failure leaves every keypoint without depth (-1) and its code in LastStatus(); `status`
// (optional) receives the per-keypoint codes of include/slamit.h (2 = the truncated pixel lies outside the image, the departure).
template <class FrameT>
void ComputeStereoFromRGBD(FrameT& F, const cv::Mat& imDepth, float depthMapFactor, std::vector<uint8_t>* status, shim::bool_tag<true>) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(slamit_kp), "cv::KeyPoint must be the 28-byte record");
    const int n = (int)F.mvKeys.size();
    F.mvuRight.assign(n, -1.0f);
    F.mvDepth.assign(n, -1.0f);
    if (status) status->assign(n, 0);
    lastStatus() = SLAMIT_OK;
    if (n == 0) return;
    if ((int)F.mvKeysUn.size() != n) { shim::refuse<Status>("FrameOps::ComputeStereoFromRGBD: mvKeysUn does not have one entry per keypoint"); return; }
    slamit_rgbd_problem P;
    P.plane.data = imDepth.data; P.plane.pitch = imDepth.step; P.plane.width = imDepth.cols; P.plane.height = imDepth.rows;
    if (imDepth.type() == CV_32F) P.plane.type = SLAMIT_DEPTH_F32;
    else if (imDepth.elemSize() == 2) P.plane.type = SLAMIT_DEPTH_U16;
    else { shim::refuse<Status>("FrameOps::ComputeStereoFromRGBD: the depth image is neither CV_32F nor 16-bit"); return; }
    P.plane.factor = depthMapFactor;
    P.mbf = F.mbf; P.n = n;
    P.kps = reinterpret_cast<const slamit_kp*>(F.mvKeys.data()); P.kps_un = reinterpret_cast<const slamit_kp*>(F.mvKeysUn.data());
    std::vector<float> u(n), d(n);
    std::vector<uint8_t> st(n);
    slamit_rgbd_result R;
    R.u_right = u.data(); R.depth = d.data(); R.status = st.data();
    const int rc = slamit_rgbd_depth(0, &P, &R);
    if (rc != SLAMIT_OK) { shim::report<Status>("slamit_rgbd_depth", rc); return; }
    F.mvuRight.swap(u);
    F.mvDepth.swap(d);
    if (status) status->swap(st);
}
template <class FrameT>
void ComputeStereoFromRGBD(FrameT&, const cv::Mat&, float, std::vector<uint8_t>*, shim::bool_tag<false>) {
    shim::refuse<Status>("FrameOps::ComputeStereoFromRGBD: the Frame type has no mbf / mvDepth / mvKeys");
}
template <class FrameT>
void ComputeStereoFromRGBD(FrameT& F, const cv::Mat& imDepth, float depthMapFactor = 1.0f, std::vector<uint8_t>* status = 0) {
    ComputeStereoFromRGBD(F, imDepth, depthMapFactor, status,
                          shim::bool_tag<shim::has_member_mbf<FrameT>::value && shim::has_member_mvDepth<FrameT>::value && shim::has_member_mvKeys<FrameT>::value>());
}

}  // namespace FrameOps
}  // namespace ORB_SLAM2

#endif
