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
// Tracking::UpdateLocalMap (:1467-1626) is documented at the function: slot tables built from the caller's objects, two calls
// (slamit_local_keyframes, slamit_local_points), for parity rather than speed.
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
#include <string.h>

#include <map>
#include <set>
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

    // Tracking::UpdateLocalMap (:1467-1626): UpdateLocalKeyFrames, then UpdateLocalPoints.  localKFs / refKF / localMPs are
    // mvpLocalKeyFrames / mpReferenceKF / mvpLocalMapPoints: in / out, since a frame in which no keyframe gets a vote keeps its list.
    // Writes them back with F.mvpMapPoints (bad points become NULL), F.mpReferenceKF and the mnTrackReferenceForFrame marks of the
    // listed keyframes and points.  Returns the number of local points.
    //
    // The keyframes that can matter -- the observers of the frame's points, their best ten, children and parent, and the list as it
    // stands -- are numbered by std::less<KeyFrameT*> and children are listed in set order, so slamit_local_keyframes' "ascending
    // slot, children as given" is the reference's address order on this run (csrc/local_map.h).
    // WHAT THIS COSTS: building the tables from host objects walks the same observers, neighbours and point lists as the host loop
    // itself, so this function is for parity and for integrations that want one code path; the gain is slamit_local_map_batch_dev
    // with the tables kept in HBM.  Members used: Frame mnId, mvpMapPoints, mpReferenceKF; MapPoint isBad(), GetObservations(),
    // mnTrackReferenceForFrame; KeyFrame isBad(), GetBestCovisibilityKeyFrames(int), GetChilds(), GetParent(), GetMapPointMatches(),
    // mnTrackReferenceForFrame.
    template <class FrameT, class KeyFrameT, class MapPointT>
    static int UpdateLocalMap(FrameT& F, std::vector<KeyFrameT*>& localKFs, std::vector<MapPointT*>& localMPs, KeyFrameT*& refKF, int device = 0) {
        status() = SLAMIT_OK;
        // the observers, then one hop; a std::set orders by std::less
        std::set<KeyFrameT*> observers, all;
        for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {
            MapPointT* pMP = F.mvpMapPoints[i];
            if (!pMP || pMP->isBad()) continue;
            const std::map<KeyFrameT*, size_t> obs = pMP->GetObservations();
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) observers.insert(it->first);
        }
        all = observers;
        for (typename std::set<KeyFrameT*>::const_iterator it = observers.begin(); it != observers.end(); ++it) {
            const std::vector<KeyFrameT*> best = (*it)->GetBestCovisibilityKeyFrames(SLAMIT_LOCAL_MAP_BEST);
            all.insert(best.begin(), best.end());
            const std::set<KeyFrameT*> childs = (*it)->GetChilds();
            all.insert(childs.begin(), childs.end());
            if ((*it)->GetParent()) all.insert((*it)->GetParent());
        }
        all.insert(localKFs.begin(), localKFs.end());
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<Tracking>("UpdateLocalMap: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the frame");
        // the points: the frame's, then every listed keyframe's, numbered as they come
        std::map<MapPointT*, int32_t> mpSlot;
        std::vector<MapPointT*> mps;
        std::vector<int32_t> frame_mp(F.mvpMapPoints.size(), -1);
        for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {
            MapPointT* pMP = F.mvpMapPoints[i];
            if (pMP) frame_mp[i] = slotOf(mpSlot, mps, pMP);
        }
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp, kf_best((size_t)n_kf * SLAMIT_LOCAL_MAP_BEST, -1), kf_child_ptr(n_kf + 1, 0), kf_child, kf_parent(n_kf, -1);
        std::vector<uint8_t> kf_bad(n_kf, 0);
        for (int k = 0; k < n_kf; ++k) {
            KeyFrameT* pKF = kfs[k];
            kf_bad[k] = pKF->isBad() ? 1 : 0;
            const std::vector<MapPointT*> vpMPs = pKF->GetMapPointMatches();
            for (size_t i = 0; i < vpMPs.size(); ++i) kf_mp.push_back(vpMPs[i] ? slotOf(mpSlot, mps, vpMPs[i]) : -1);
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
            if (observers.count(pKF)) {   // the walk visits voted keyframes only: the others' neighbours are never read
                const std::vector<KeyFrameT*> best = pKF->GetBestCovisibilityKeyFrames(SLAMIT_LOCAL_MAP_BEST);
                for (size_t b = 0; b < best.size() && b < SLAMIT_LOCAL_MAP_BEST; ++b) kf_best[(size_t)k * SLAMIT_LOCAL_MAP_BEST + b] = kfSlot[best[b]];
                const std::set<KeyFrameT*> childs = pKF->GetChilds();
                for (typename std::set<KeyFrameT*>::const_iterator c = childs.begin(); c != childs.end(); ++c) kf_child.push_back(kfSlot[*c]);
                if (pKF->GetParent()) kf_parent[k] = kfSlot[pKF->GetParent()];
            }
            kf_child_ptr[k + 1] = (int32_t)kf_child.size();
        }
        const int n_mp = (int)mps.size();
        std::vector<int32_t> obs_ptr(n_mp + 1, 0), obs_kf;
        std::vector<uint8_t> mp_bad(n_mp, 0);
        std::vector<uint8_t> inFrame(n_mp, 0);
        for (size_t i = 0; i < frame_mp.size(); ++i)
            if (frame_mp[i] >= 0) inFrame[frame_mp[i]] = 1;
        for (int p = 0; p < n_mp; ++p) {
            mp_bad[p] = mps[p]->isBad() ? 1 : 0;
            if (inFrame[p] && !mp_bad[p]) {   // only the frame's points vote
                const std::map<KeyFrameT*, size_t> obs = mps[p]->GetObservations();
                for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) obs_kf.push_back(kfSlot[it->first]);
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        uint8_t none8 = 0;
        int32_t none32 = -1;
        M.n_kf = n_kf; M.n_mp = n_mp;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.mp_bad = n_mp ? mp_bad.data() : &none8;
        M.kf_bad = n_kf ? kf_bad.data() : &none8; M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.empty() ? &none32 : kf_mp.data();
        M.kf_best = n_kf ? kf_best.data() : &none32; M.kf_child_ptr = kf_child_ptr.data(); M.kf_child = kf_child.empty() ? &none32 : kf_child.data();
        M.kf_parent = n_kf ? kf_parent.data() : &none32;
        // UpdateLocalKeyFrames
        const int kf_cap = n_kf > SLAMIT_LOCAL_MAP_MIN_KF_CAP ? n_kf : SLAMIT_LOCAL_MAP_MIN_KF_CAP;
        std::vector<int32_t> votes(n_kf + 1, 0), list(kf_cap, -1);
        for (size_t j = 0; j < localKFs.size(); ++j) list[j] = kfSlot[localKFs[j]];
        int32_t n_list = (int32_t)localKFs.size(), ref = -1, st = 0;
        int rc = slamit_local_keyframes(device, &M, (int32_t)frame_mp.size(), frame_mp.empty() ? &none32 : frame_mp.data(), votes.data(), kf_cap, list.data(),
                                        &n_list, &ref, &st);
        if (rc != SLAMIT_OK) return shim::report<Tracking>("UpdateLocalMap: slamit_local_keyframes", rc);
        if (st != 0 || n_list > kf_cap) return shim::refuse<Tracking>("UpdateLocalMap: slamit_local_keyframes reported a status on tables built here", SLAMIT_ERR_STATE);
        for (size_t i = 0; i < frame_mp.size(); ++i)
            if (frame_mp[i] < 0) F.mvpMapPoints[i] = static_cast<MapPointT*>(NULL);   // :1535
        bool voted = false;
        for (int k = 0; k < n_kf; ++k) voted = voted || votes[k] > 0;
        if (voted) {   // :1546-1619; without a vote the reference returned before clear()
            localKFs.clear();
            for (int j = 0; j < n_list; ++j) {
                localKFs.push_back(kfs[list[j]]);
                kfs[list[j]]->mnTrackReferenceForFrame = F.mnId;
            }
        }
        if (ref >= 0) {   // :1621-1625: pKFmax
            refKF = kfs[ref];
            F.mpReferenceKF = refKF;
        }
        // UpdateLocalPoints
        localMPs.clear();
        if (n_mp > SLAMIT_FRUSTUM_MAX_N) return shim::refuse<Tracking>("UpdateLocalMap: more than SLAMIT_FRUSTUM_MAX_N map points around the frame", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> local_mp(n_mp + 1, -1);
        std::vector<uint8_t> skip(n_mp + 1, 0);
        int32_t n_local = 0;
        rc = slamit_local_points(device, &M, (int32_t)frame_mp.size(), frame_mp.empty() ? &none32 : frame_mp.data(), 0, NULL, n_list, list.data(), n_mp,
                                 local_mp.data(), skip.data(), &n_local, &st);
        if (rc != SLAMIT_OK) return shim::report<Tracking>("UpdateLocalMap: slamit_local_points", rc);
        if (st != 0 || n_local > n_mp) return shim::refuse<Tracking>("UpdateLocalMap: slamit_local_points reported a status on tables built here", SLAMIT_ERR_STATE);
        for (int i = 0; i < n_local; ++i) {
            localMPs.push_back(mps[local_mp[i]]);
            mps[local_mp[i]]->mnTrackReferenceForFrame = F.mnId;
        }
        return n_local;
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

    // the slot of a map point in UpdateLocalMap's numbering: a new one on first sight
    template <class MapPointT>
    static int32_t slotOf(std::map<MapPointT*, int32_t>& slots, std::vector<MapPointT*>& mps, MapPointT* p) {
        typename std::map<MapPointT*, int32_t>::const_iterator it = slots.find(p);
        if (it != slots.end()) return it->second;
        const int32_t s = (int32_t)mps.size();
        slots[p] = s;
        mps.push_back(p);
        return s;
    }

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
