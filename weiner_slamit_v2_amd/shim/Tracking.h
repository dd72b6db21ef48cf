// Tracking.h — Tracking::SearchLocalPoints (ORB_SLAM2/src/Tracking.cc:1409-1464) over the caller's Frame and MapPoint types,
// monocular, and the closest-point walks of a stereo or RGB-D frame (below).  The loop over the frame's own map points stays host code; Frame::isInFrustum with MapPoint::PredictScale
// (Frame.cc:389-445, MapPoint.cc:391-400) for ALL local map points is ONE slamit_frustum call (csrc/frustum.h), and the search that
// follows is the existing ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) (one slamit_guided_search call).
//
// Members used on the caller's types (on top of what ORBmatcher::SearchByProjection lists):
//   Frame    : mnId, mvpMapPoints, mRcw, mtcw, mOw (CV_32F), fx, fy, cx, cy, mbf, static mnMinX, mnMaxX, mnMinY, mnMaxY,
//              mfLogScaleFactor, mvScaleFactors
//   MapPoint : isBad(), IncreaseVisible(), mnLastFrameSeen, mbTrackInView, mTrackProjX, mTrackProjXR, mTrackProjY,
//              mnTrackScaleLevel, mTrackViewCos, GetWorldPos(), GetNormal(), and the RAW invariance distances
//              GetMaxDistance() / GetMinDistance() = mfMaxDistance / mfMinDistance under mMutexPos.  The reference's MapPoint keeps
//              those two protected and only hands out 1.2f * max and 0.8f * min (MapPoint.cc:379-389), but PredictScale divides the
//              raw one: the integration adds the two one-line accessors next to GetMaxDistanceInvariance().
//
// ONE DEPARTURE (csrc/frustum.h): this reference's PredictScale does not clamp, and a predicted level outside [0, n_levels) indexes
// mvScaleFactors out of bounds in the search.  Here such a point (status 7) gets mbTrackInView = false: it is not counted in
// nToMatch, IncreaseVisible is not called for it and it is not searched.
//
// A non-SLAMIT_OK status of a device call is reported on stderr with LastStatus() set, and ends the function: never a silent return.
//
// STEREO AND RGB-D: the closest-point walks of Tracking::UpdateLastFrame (Tracking.cc:1037-1091), of the stereo
// branch of CreateNewKeyFrame (:1327-1397) and of StereoInitialization (:712-727), and the two counts of NeedNewKeyFrame (:1244-1253).
// Each gathers `tracked` (mvpMapPoints[i] non-null with Observations() >= 1), makes ONE slamit_unproject_closest call (the sort by
// depth, the cut, Frame::UnprojectStereo and what the new point's constructor stores: csrc/unproject.h) and walks `order`, so the
// points are created in the reference's order and get the reference's mnId.  Members used on the caller's types:
//   Frame    : N, mvKeysUn, mvDepth, mvpMapPoints, mRwc, mOw (CV_32F), fx, fy, cx, cy, invfx, invfy, mvScaleFactors
//   MapPoint : Observations(); for keyframe points AddObservation(pKF, i), ComputeDistinctiveDescriptors(), UpdateNormalAndDepth()
//   KeyFrame : AddMapPoint(pMP, i);   Map : AddMapPoint(pMP)
// and one callable, make(const cv::Mat& x3D /* 3x1 CV_32F */, int i, const float normal[3], float max_dist, float min_dist), which
// returns the new MapPoint*: `new MapPoint(x3D, mpMap, &mLastFrame, i)` for a frame point, `new MapPoint(x3D, pKF, mpMap)` for a
// keyframe point.  normal / max_dist / min_dist are what that constructor (and UpdateNormalAndDepth with its one observer) computes,
// bit for bit; a caller may store them instead.  The bookkeeping around the call stays here, in the reference's order: the
// `mvpMapPoints[i] = NULL` of :1370, AddObservation / AddMapPoint / ComputeDistinctiveDescriptors / UpdateNormalAndDepth /
// Map::AddMapPoint for keyframe points, mlpTemporalPoints for frame points.
// ONE DEPARTURE (csrc/unproject.h): a visited keypoint whose octave lies outside [0, n_levels) (status 4) counts in the walk and gets
// no point, where the reference indexes mvScaleFactors out of bounds.
#ifndef SLAMIT_SHIM_TRACKING_H
#define SLAMIT_SHIM_TRACKING_H

#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "ORBmatcher.h"
#include "shim_common.h"

namespace ORB_SLAM2 {

class Tracking {
public:
    // th: 1, or 3 for RGBD, or 5 after a recent relocalisation (:1452-1460); nnratio 0.8 (:1451).  Returns the matches of the search
    // (0 when nothing is in view); LastInView() is nToMatch.
    template <class FrameT, class MapPointT>
    static int SearchLocalPoints(FrameT& F, std::vector<MapPointT*>& local, int th, float nnratio = 0.8f, int device = 0) {
        status() = SLAMIT_OK;
        inView() = 0;
        // Do not search map points already matched (:1412-1429)
        for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {
            MapPointT* pMP = F.mvpMapPoints[i];
            if (!pMP) continue;
            if (pMP->isBad()) {
                F.mvpMapPoints[i] = static_cast<MapPointT*>(NULL);
            } else {
                pMP->IncreaseVisible();
                pMP->mnLastFrameSeen = F.mnId;
                pMP->mbTrackInView = false;
            }
        }
        const int n = (int)local.size();
        if (n == 0) return 0;
        if (F.mvScaleFactors.size() < 1 || F.mvScaleFactors.size() > SLAMIT_MAX_LEVELS) return shim::refuse<Tracking>("SearchLocalPoints: mvScaleFactors outside [1, SLAMIT_MAX_LEVELS] levels");
        // Project points in frame and check its visibility (:1433-1447): every point in one call
        slamit_frustum_problem P;
        shim::load3x3(F.mRcw, P.frame.Rcw); shim::load3(F.mtcw, P.frame.tcw); shim::load3(F.mOw, P.frame.Ow);
        P.frame.fx = F.fx; P.frame.fy = F.fy; P.frame.cx = F.cx; P.frame.cy = F.cy; P.frame.bf = F.mbf;
        P.frame.min_x = F.mnMinX; P.frame.max_x = F.mnMaxX; P.frame.min_y = F.mnMinY; P.frame.max_y = F.mnMaxY;
        P.frame.view_cos_limit = 0.5f;
        P.frame.log_scale_factor = F.mfLogScaleFactor;
        P.frame.th = (float)th;
        P.frame.n_levels = (int32_t)F.mvScaleFactors.size();
        for (int l = 0; l < SLAMIT_MAX_LEVELS; ++l) P.frame.scale_factors[l] = l < P.frame.n_levels ? F.mvScaleFactors[l] : 0.f;
        std::vector<float> pos(3 * (size_t)n, 0.f), nrm(3 * (size_t)n, 0.f), maxd(n, 0.f), mind(n, 0.f);
        std::vector<uint8_t> skip(n, 0);
        for (int i = 0; i < n; ++i) {
            MapPointT* pMP = local[i];
            if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) { skip[i] = 1; continue; }
            const cv::Mat Pw = pMP->GetWorldPos(), Pn = pMP->GetNormal();
            shim::load3(Pw, &pos[3 * (size_t)i]); shim::load3(Pn, &nrm[3 * (size_t)i]);
            maxd[i] = pMP->GetMaxDistance(); mind[i] = pMP->GetMinDistance();
        }
        P.n = n; P.pos = pos.data(); P.normal = nrm.data(); P.max_dist = maxd.data(); P.min_dist = mind.data(); P.skip = skip.data();
        std::vector<uint8_t> st(n), valid(n);
        std::vector<float> proj(3 * (size_t)n), vc(n), uvr(3 * (size_t)n);
        std::vector<int32_t> level(n), l0(n), l1(n);
        slamit_frustum_result R;
        R.status = st.data(); R.proj = proj.data(); R.view_cos = vc.data(); R.level = level.data(); R.uvr = uvr.data();
        R.level_min = l0.data(); R.level_max = l1.data(); R.valid = valid.data(); R.n_in_view = 0;
        const int rc = slamit_frustum(device, &P, &R);
        if (rc != SLAMIT_OK) return shim::report<Tracking>("SearchLocalPoints: slamit_frustum", rc);
        int nToMatch = 0;
        for (int i = 0; i < n; ++i) {
            if (skip[i]) continue;                       // :1436-1440: the reference does not touch these
            MapPointT* pMP = local[i];
            pMP->mbTrackInView = st[i] == 0;             // Frame.cc:391; status 7 stays false (the departure)
            if (st[i] != 0) continue;
            pMP->mTrackProjX = proj[3 * (size_t)i]; pMP->mTrackProjY = proj[3 * (size_t)i + 1]; pMP->mTrackProjXR = proj[3 * (size_t)i + 2];
            pMP->mnTrackScaleLevel = level[i];
            pMP->mTrackViewCos = vc[i];
            pMP->IncreaseVisible();
            nToMatch++;
        }
        inView() = nToMatch;
        if (nToMatch != R.n_in_view) return shim::refuse<Tracking>("SearchLocalPoints: the device's count of points in view disagrees with its statuses");
        if (nToMatch == 0) return 0;
        ORBmatcher matcher(nnratio);
        const int nmatches = matcher.SearchByProjection(F, local, (float)th);
        if (ORBmatcher::LastStatus() != SLAMIT_OK) return shim::report<Tracking>("SearchLocalPoints: SearchByProjection", ORBmatcher::LastStatus());
        return nmatches;
    }

    // Tracking::UpdateLastFrame after the pose update and the two early returns (:1037-1091): the "visual odometry" points of the last
    // frame.  temporal is mlpTemporalPoints.  Returns the number of points created.
    template <class FrameT, class TemporalT, class MakeFn>
    static int UpdateLastFrame(FrameT& F, float thDepth, TemporalT& temporal, MakeFn&& make, int device = 0) {
        Walk W;
        if (!walk(F, thDepth, SLAMIT_UNPROJECT_CLOSEST, SLAMIT_UNPROJECT_CTOR_FRAME, device, "UpdateLastFrame", W)) return 0;
        int made = 0;
        for (int j = 0; j < W.counts.n_visited; ++j) {
            const int i = W.order[j];
            if (W.status[i] != 3) continue;
            auto* pNewMP = make(W.x3D(i), i, &W.normal[3 * (size_t)i], W.max_dist[i], W.min_dist[i]);
            F.mvpMapPoints[i] = pNewMP;
            temporal.push_back(pNewMP);
            ++made;
        }
        return made;
    }

    // The stereo / RGB-D branch of Tracking::CreateNewKeyFrame (:1327-1397) after UpdatePoseMatrices.  Returns the points created.
    template <class FrameT, class KeyFrameT, class MapT, class MakeFn>
    static int CreateNewKeyFramePoints(FrameT& F, KeyFrameT* pKF, MapT* pMap, float thDepth, MakeFn&& make, int device = 0) {
        Walk W;
        if (!walk(F, thDepth, SLAMIT_UNPROJECT_CLOSEST, SLAMIT_UNPROJECT_CTOR_KEYFRAME, device, "CreateNewKeyFramePoints", W)) return 0;
        int made = 0;
        for (int j = 0; j < W.counts.n_visited; ++j) {
            const int i = W.order[j];
            if (W.status[i] == 2) continue;
            if (F.mvpMapPoints[i]) F.mvpMapPoints[i] = NULL;   // :1365-1371: a point without observations is dropped from the frame
            if (W.status[i] != 3) continue;
            made += keyframePoint(F, pKF, pMap, W, i, make);
        }
        return made;
    }

    // The loop of Tracking::StereoInitialization (:712-727): every keypoint with a depth, in index order.  Returns the points created.
    template <class FrameT, class KeyFrameT, class MapT, class MakeFn>
    static int StereoInitializationPoints(FrameT& F, KeyFrameT* pKFini, MapT* pMap, MakeFn&& make, int device = 0) {
        Walk W;
        if (!walk(F, 0.f, SLAMIT_UNPROJECT_ALL, SLAMIT_UNPROJECT_CTOR_KEYFRAME, device, "StereoInitializationPoints", W)) return 0;
        int made = 0;
        for (int j = 0; j < W.counts.n_visited; ++j)
            if (W.status[W.order[j]] == 3) made += keyframePoint(F, pKFini, pMap, W, W.order[j], make);
        return made;
    }

    // The two counts of Tracking::NeedNewKeyFrame (:1238-1254): nTotal keypoints with 0 < depth < thDepth, nMap of them with a tracked
    // point.  false (and zeros) when the device call failed.
    template <class FrameT>
    static bool CloseRatio(FrameT& F, float thDepth, int& nMap, int& nTotal, int device = 0) {
        Walk W;
        nMap = nTotal = 0;
        if (!walk(F, thDepth, SLAMIT_UNPROJECT_CLOSEST, SLAMIT_UNPROJECT_CTOR_FRAME, device, "CloseRatio", W)) return status() == SLAMIT_OK;
        nMap = W.counts.n_map; nTotal = W.counts.n_total;
        return true;
    }

    static int LastStatus() { return status(); }
    static int LastInView() { return inView(); }
    static slamit_unproject_counts LastCounts() { return counts(); }   // of the last of the four calls above on this thread

private:
    static int& status() { return shim::status<Tracking>(); }
    static int& inView() { static thread_local int s = 0; return s; }
    static slamit_unproject_counts& counts() { static thread_local slamit_unproject_counts c = {0, 0, 0, 0, 0, 0}; return c; }

    struct Walk {
        std::vector<uint8_t> status;
        std::vector<int32_t> order;
        std::vector<float> pos, normal, max_dist, min_dist;
        slamit_unproject_counts counts;
        cv::Mat x3D(int i) const {
            cv::Mat m(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) m.at<float>(r, 0) = pos[3 * (size_t)i + r];
            return m;
        }
    };

    // one slamit_unproject_closest call on the frame; false = nothing to walk (no keypoints, or a failure that has been reported)
    template <class FrameT>
    static bool walk(FrameT& F, float thDepth, int mode, int ctor, int device, const char* who, Walk& W) {
        static_assert(sizeof(cv::KeyPoint) == sizeof(slamit_kp), "cv::KeyPoint must be the 28-byte record");
        status() = SLAMIT_OK;
        const slamit_unproject_counts zero = {0, 0, 0, 0, 0, 0};
        counts() = W.counts = zero;
        const int n = (int)F.mvKeysUn.size();
        if (n == 0) return false;
        char msg[160];
        if ((int)F.mvDepth.size() != n || (int)F.mvpMapPoints.size() != n) {
            snprintf(msg, sizeof(msg), "%s: mvDepth / mvpMapPoints do not have one entry per keypoint", who);
            shim::refuse<Tracking>(msg);
            return false;
        }
        if (F.mvScaleFactors.size() < 1 || F.mvScaleFactors.size() > SLAMIT_MAX_LEVELS) {
            snprintf(msg, sizeof(msg), "%s: mvScaleFactors outside [1, SLAMIT_MAX_LEVELS] levels", who);
            shim::refuse<Tracking>(msg);
            return false;
        }
        slamit_unproject_problem P;
        P.frame.fx = F.fx; P.frame.fy = F.fy; P.frame.cx = F.cx; P.frame.cy = F.cy; P.frame.invfx = F.invfx; P.frame.invfy = F.invfy;
        shim::load3x3(F.mRwc, P.frame.Rwc); shim::load3(F.mOw, P.frame.Ow);
        P.frame.th_depth = thDepth; P.frame.min_points = 100; P.frame.mode = mode; P.frame.ctor = ctor;
        P.frame.n_levels = (int32_t)F.mvScaleFactors.size();
        for (int l = 0; l < SLAMIT_MAX_LEVELS; ++l) P.frame.scale_factors[l] = l < P.frame.n_levels ? F.mvScaleFactors[l] : 0.f;
        std::vector<uint8_t> tracked(n, 0);
        for (int i = 0; i < n; ++i) tracked[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() >= 1 ? 1 : 0;
        P.n = n; P.kps_un = reinterpret_cast<const slamit_kp*>(F.mvKeysUn.data()); P.depth = F.mvDepth.data(); P.tracked = tracked.data();
        W.status.assign(n, 0); W.order.assign(n, -1); W.pos.assign(3 * (size_t)n, 0.f); W.normal.assign(3 * (size_t)n, 0.f);
        W.max_dist.assign(n, 0.f); W.min_dist.assign(n, 0.f);
        slamit_unproject_result R;
        R.status = W.status.data(); R.order = W.order.data(); R.pos = W.pos.data(); R.normal = W.normal.data();
        R.max_dist = W.max_dist.data(); R.min_dist = W.min_dist.data(); R.counts = zero;
        const int rc = slamit_unproject_closest(device, &P, &R);
        if (rc != SLAMIT_OK) {
            snprintf(msg, sizeof(msg), "%s: slamit_unproject_closest", who);
            shim::report<Tracking>(msg, rc);
            return false;
        }
        counts() = W.counts = R.counts;
        return true;
    }

    // :1376-1385 and :718-725
    template <class FrameT, class KeyFrameT, class MapT, class MakeFn>
    static int keyframePoint(FrameT& F, KeyFrameT* pKF, MapT* pMap, const Walk& W, int i, MakeFn&& make) {
        auto* pNewMP = make(W.x3D(i), i, &W.normal[3 * (size_t)i], W.max_dist[i], W.min_dist[i]);
        pNewMP->AddObservation(pKF, i);
        pKF->AddMapPoint(pNewMP, i);
        pNewMP->ComputeDistinctiveDescriptors();
        pNewMP->UpdateNormalAndDepth();
        pMap->AddMapPoint(pNewMP);
        F.mvpMapPoints[i] = pNewMP;
        return 1;
    }
};

}  // namespace ORB_SLAM2

#endif
