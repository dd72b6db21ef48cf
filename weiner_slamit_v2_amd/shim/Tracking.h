// Tracking.h — Tracking::SearchLocalPoints (ORB_SLAM2/src/Tracking.cc:1409-1464) over the caller's Frame and MapPoint types,
// monocular.  The loop over the frame's own map points stays host code; Frame::isInFrustum with MapPoint::PredictScale
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

    static int LastStatus() { return status(); }
    static int LastInView() { return inView(); }

private:
    static int& status() { return shim::status<Tracking>(); }
    static int& inView() { static thread_local int s = 0; return s; }
};

}  // namespace ORB_SLAM2

#endif
