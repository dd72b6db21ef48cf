// LocalMapping.h — LocalMapping::CreateNewMapPoints (ORB_SLAM2/src/LocalMapping.cc:224-505) over the caller's KeyFrame type,
// monocular and stereo.  The loop over the neighbours, the baseline gate, ComputeF12 and the bookkeeping stay host code; the matcher is
// ORBmatcher::SearchForTriangulation (one slamit_bow_search call) and the per-pair body -- parallax, linear triangulation, depth,
// reprojection and scale gates (:348-483) -- is ONE slamit_triangulate call per neighbour (csrc/triangulate.h), or ONE
// slamit_triangulate_stereo call with the stereo branches of :335-465.
//
// Members used on the caller's type (on top of what ORBmatcher::SearchForTriangulation lists):
//   KeyFrame : N, mvKeysUn, mvuRight, mvScaleFactors, mvLevelSigma2, mfScaleFactor, fx, fy, cx, cy, invfx, invfy,
//              GetRotation(), GetTranslation(), GetCameraCenter(), ComputeSceneMedianDepth(q),
//              mFeatVec, mDescriptors, GetMapPoint(idx)
// and one callable, make(const cv::Mat& x3D /* 3x1 CV_32F */, int idx1, int idx2, KeyFrameT* pKF2), called for every accepted pair in
// pair order; it does what :486-500 does (new MapPoint, AddObservation on both keyframes, AddMapPoint on both keyframes,
// ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Map::AddMapPoint, mlpRecentAddedMapPoints).
//
// The neighbours are NOT merged into one launch: a point made for neighbour i gives keypoint idx1 of the current keyframe a map
// point, which removes it from neighbour i+1's SearchForTriangulation (:700-704) -- the reference's result depends on that order,
// so each neighbour's search runs after the previous neighbour's make() calls.  slamit_triangulate_batch is for callers that hold
// the keyframe pairs of several independent streams at once (the pipeline configuration), where no such dependency exists.
//
// The stereo path is chosen at compile time (shim_common.h's member detection): a KeyFrameT with all of
//   mb, mbf, mvDepth, mvKeys
// takes stereo keyframes and monocular == false.  There the baseline gate is baseline < pKF2->mb when !monocular (:278-283), the
// right-image side of every pair is mvuRight / mvDepth of its keypoints and the RAW keypoint mvKeys[idx].pt (KeyFrame::UnprojectStereo
// reads it, not mvKeysUn), mb of each keyframe, and the CURRENT keyframe's mbf for both reprojection gates (:430, :458).
// A KeyFrameT without these members keeps the monocular code: monocular == false, or a keyframe with a stereo coordinate
// (mvuRight >= 0), is refused on stderr with LastStatus() == SLAMIT_ERR_ARG and nothing is created.  Any other non-SLAMIT_OK status
// of a device call is reported the same way and ends the loop: never a silent return.
//
// KeyFrame::UpdateConnections (src/KeyFrame.cc:296-386) and LocalMapping::KeyFrameCulling (:686-752) are documented at the functions:
// slot tables built from the caller's objects, one call each (slamit_update_connections, slamit_keyframe_culling), the results
// written into the objects; for parity rather than speed.  UpdateMapPoints (MapPoint::UpdateNormalAndDepth and
// ::ComputeDistinctiveDescriptors for a list of points, src/MapPoint.cc:248-377) and MapPointCulling (:184-219) are built the same way
// over slamit_update_points and slamit_map_point_culling, ApplyMapEdits (MapPoint::AddObservation, ::EraseObservation
// and ::SetBadFlag for a list of edits, src/MapPoint.cc:104-174) over slamit_map_edit_apply (section 26), ReplaceMapPoints (MapPoint::Replace for a fuse list, :183-221) over
// slamit_map_replace_apply (section 27), SetBadFlagKeyFrames (KeyFrame::SetBadFlag for a list of keyframes, src/KeyFrame.cc:460-552) over
// slamit_kf_erase_apply and ApplyMapEdits (section 28), FuseMapPoints (the tail of ORBmatcher::Fuse for a list of matched points,
// src/ORBmatcher.cc:955-975) over slamit_map_fuse_apply (section 31).
#ifndef SLAMIT_SHIM_LOCALMAPPING_H
#define SLAMIT_SHIM_LOCALMAPPING_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "ORBmatcher.h"
#include "shim_common.h"

namespace ORB_SLAM2 {

class LocalMapping {
public:
    // K1^-T [t12]x R12 K2^-1 (:590-607) in float; K^-1 of a pinhole K is written out.
    template <class KeyFrameT>
    static cv::Mat ComputeF12(KeyFrameT* pKF1, KeyFrameT* pKF2) {
        const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        float R12[3][3], t12[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                R12[r][c] = R1w.template at<float>(r, 0) * R2w.template at<float>(c, 0) + R1w.template at<float>(r, 1) * R2w.template at<float>(c, 1) +
                            R1w.template at<float>(r, 2) * R2w.template at<float>(c, 2);
        for (int r = 0; r < 3; ++r)
            t12[r] = -(R12[r][0] * t2w.template at<float>(0, 0) + R12[r][1] * t2w.template at<float>(1, 0) + R12[r][2] * t2w.template at<float>(2, 0)) +
                     t1w.template at<float>(r, 0);
        const float tx[3][3] = {{0, -t12[2], t12[1]}, {t12[2], 0, -t12[0]}, {-t12[1], t12[0], 0}};
        const float K1i[3][3] = {{1.f / pKF1->fx, 0, -pKF1->cx / pKF1->fx}, {0, 1.f / pKF1->fy, -pKF1->cy / pKF1->fy}, {0, 0, 1}};
        const float K2i[3][3] = {{1.f / pKF2->fx, 0, -pKF2->cx / pKF2->fx}, {0, 1.f / pKF2->fy, -pKF2->cy / pKF2->fy}, {0, 0, 1}};
        float a[3][3], b[3][3];
        cv::Mat F(3, 3, CV_32F);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) a[r][c] = K1i[0][r] * tx[0][c] + K1i[1][r] * tx[1][c] + K1i[2][r] * tx[2][c];   // K1^-T [t]x
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) b[r][c] = a[r][0] * R12[0][c] + a[r][1] * R12[1][c] + a[r][2] * R12[2][c];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) F.at<float>(r, c) = b[r][0] * K2i[0][c] + b[r][1] * K2i[1][c] + b[r][2] * K2i[2][c];
        return F;
    }

    // The loop of :265-504.  stop() stands for CheckNewKeyFrames(): asked before every neighbour but the first (:267).
    // Returns the number of make() calls (nnew).
    template <class KeyFrameT, class NewPointFn, class StopFn>
    static int CreateNewMapPoints(KeyFrameT* cur, const std::vector<KeyFrameT*>& neigh, bool monocular, NewPointFn&& make, StopFn&& stop, int device = 0) {
        status() = SLAMIT_OK;
        const StereoTag<KeyFrameT> tag = StereoTag<KeyFrameT>();
        if (!accepts(cur, neigh, monocular, tag)) return 0;
        ORBmatcher matcher(0.6, false);
        slamit_triangulate_problem P;
        pose(cur, P.Tcw1, P.intr1);
        const cv::Mat Ow1 = cur->GetCameraCenter();
        P.ratio_factor = 1.5f * cur->mfScaleFactor;
        int nnew = 0;
        for (size_t i = 0; i < neigh.size(); i++) {
            if (i > 0 && stop()) return nnew;
            KeyFrameT* pKF2 = neigh[i];
            // baseline against the scene's median depth, or against the rig's baseline (:273-294)
            const cv::Mat Ow2 = pKF2->GetCameraCenter();
            const float vB[3] = {Ow2.template at<float>(0, 0) - Ow1.template at<float>(0, 0), Ow2.template at<float>(1, 0) - Ow1.template at<float>(1, 0),
                                 Ow2.template at<float>(2, 0) - Ow1.template at<float>(2, 0)};
            const float baseline = (float)sqrt((double)vB[0] * vB[0] + (double)vB[1] * vB[1] + (double)vB[2] * vB[2]);
            if (baselineTooShort(pKF2, baseline, monocular, tag)) continue;
            const cv::Mat F12 = ComputeF12(cur, pKF2);
            std::vector<std::pair<size_t, size_t> > vMatchedIndices;
            matcher.SearchForTriangulation(cur, pKF2, F12, vMatchedIndices, false);
            if (ORBmatcher::LastStatus() != SLAMIT_OK) {
                shim::report<LocalMapping>("CreateNewMapPoints: SearchForTriangulation", ORBmatcher::LastStatus());
                return nnew;
            }
            const int nmatches = (int)vMatchedIndices.size();
            if (nmatches == 0) continue;
            std::vector<float> kp1(2 * (size_t)nmatches), kp2(2 * (size_t)nmatches), x3d(3 * (size_t)nmatches);
            std::vector<int32_t> o1(nmatches), o2(nmatches);
            std::vector<uint8_t> st(nmatches);
            for (int k = 0; k < nmatches; ++k) {
                const cv::KeyPoint& a = cur->mvKeysUn[vMatchedIndices[k].first];
                const cv::KeyPoint& b = pKF2->mvKeysUn[vMatchedIndices[k].second];
                kp1[2 * k] = a.pt.x; kp1[2 * k + 1] = a.pt.y; o1[k] = a.octave;
                kp2[2 * k] = b.pt.x; kp2[2 * k + 1] = b.pt.y; o2[k] = b.octave;
            }
            pose(pKF2, P.Tcw2, P.intr2);
            P.n = nmatches;
            P.n_levels = (int32_t)cur->mvScaleFactors.size();
            if (pKF2->mvScaleFactors.size() != cur->mvScaleFactors.size() || cur->mvLevelSigma2.size() != cur->mvScaleFactors.size() ||
                pKF2->mvLevelSigma2.size() != cur->mvScaleFactors.size()) {
                shim::refuse<LocalMapping>("CreateNewMapPoints: the level tables of the two keyframes differ in length");
                return nnew;
            }
            P.kp1_xy = kp1.data(); P.kp2_xy = kp2.data(); P.octave1 = o1.data(); P.octave2 = o2.data();
            P.scale_factors1 = cur->mvScaleFactors.data(); P.level_sigma2_1 = cur->mvLevelSigma2.data();
            P.scale_factors2 = pKF2->mvScaleFactors.data(); P.level_sigma2_2 = pKF2->mvLevelSigma2.data();
            slamit_triangulate_result R;
            R.status = st.data(); R.x3d = x3d.data(); R.n_accepted = 0;
            const int rc = triangulate(cur, pKF2, vMatchedIndices, device, P, R, tag);
            if (rc != SLAMIT_OK) {
                shim::report<LocalMapping>("CreateNewMapPoints: slamit_triangulate", rc);
                return nnew;
            }
            for (int k = 0; k < nmatches; ++k) {
                if (st[k] != 0) continue;
                cv::Mat x3D(3, 1, CV_32F);
                for (int r = 0; r < 3; ++r) x3D.at<float>(r, 0) = x3d[3 * (size_t)k + r];
                make(x3D, (int)vMatchedIndices[k].first, (int)vMatchedIndices[k].second, pKF2);
                nnew++;
            }
        }
        return nnew;
    }

    template <class KeyFrameT, class NewPointFn>
    static int CreateNewMapPoints(KeyFrameT* cur, const std::vector<KeyFrameT*>& neigh, bool monocular, NewPointFn&& make) {
        return CreateNewMapPoints(cur, neigh, monocular, make, never);
    }

    // KeyFrame::UpdateConnections (KeyFrame.cc:296-386) for pKF.  Writes mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames and
    // mvOrderedWeights of pKF, calls AddConnection(pKF, weight) on the listed neighbours in the reference's order (ascending address,
    // so their own UpdateBestCovisibles runs as host code on the caller's type), and on a first connection of a keyframe other than
    // the origin sets mpParent, calls AddChild and clears mbFirstConnection.  Returns the number of listed keyframes; 0 with
    // LastStatus() == SLAMIT_OK when no other keyframe shares a point (the reference returns there too).
    //
    // The keyframes that can matter -- pKF and the observers of its points -- are numbered by std::less<KeyFrameT*>, so
    // slamit_update_connections' "ascending slot" and "within equal weight the higher slot first" are the reference's address order
    // and its sort of (weight, pointer) on this run (csrc/covis.h).  The neighbours' rows are passed empty: the call is asked for the
    // counter and pKF's own list only.
    // WHAT THIS COSTS: building the tables from host objects walks the same points and observers as the host loop itself, so this
    // function is for parity and for integrations that want one code path; the gain is slamit_update_connections_batch_dev with the
    // tables kept in HBM.  Members used: KeyFrame mnId, mbFirstConnection, mpParent, mConnectedKeyFrameWeights,
    // mvpOrderedConnectedKeyFrames, mvOrderedWeights, GetMapPointMatches(), AddConnection(KeyFrame*, const int&), AddChild(KeyFrame*);
    // MapPoint isBad(), GetObservations().
    template <class KeyFrameT>
    static int UpdateConnections(KeyFrameT* pKF, int device = 0) {
        status() = SLAMIT_OK;
        return updateConnections(pKF, pKF->GetMapPointMatches(), device);
    }

    // LocalMapping::KeyFrameCulling (LocalMapping.cc:686-752) for the current keyframe: the candidates are
    // cur->GetVectorCovisibleKeyFrames(); SetBadFlag() is called on the culled ones in order (a keyframe with mbNotErase gets the call
    // too: its own SetBadFlag marks it to be erased, as in the reference).  Returns the number of SetBadFlag() calls.
    //
    // The device call evaluates every candidate against the tables as they are at the start and carries the cascade itself (a culled
    // keyframe's observations are gone for the candidates behind it), so the SetBadFlag() calls are made after it, in order: the
    // caller's objects see the same sequence of calls as in the reference.  monocular == false needs mvDepth and mThDepth on the
    // keyframe type; a type without mvDepth is refused.
    // WHAT THIS COSTS: as above, the tables cost what the host loop costs; the gain is slamit_keyframe_culling_batch_dev.
    // Members used: KeyFrame mnId, mbNotErase, mvKeysUn, mvuRight, (mvDepth, mThDepth), GetVectorCovisibleKeyFrames(),
    // GetMapPointMatches(), SetBadFlag(); MapPoint isBad(), Observations(), GetObservations().
    template <class KeyFrameT>
    static int KeyFrameCulling(KeyFrameT* cur, bool monocular, int device = 0) {
        status() = SLAMIT_OK;
        if (!monocular && !shim::has_member_mvDepth<KeyFrameT>::value) return shim::refuse<LocalMapping>("KeyFrameCulling: monocular == false needs mvDepth and mThDepth on the keyframe type");
        const std::vector<KeyFrameT*> cands = cur->GetVectorCovisibleKeyFrames();
        if (cands.empty()) return 0;
        return keyFrameCulling(cur, cands, cands[0]->GetMapPointMatches(), monocular, device);
    }

    // MapPoint::UpdateNormalAndDepth (what & 1) and MapPoint::ComputeDistinctiveDescriptors (what & 2) (MapPoint.cc:248-377) for the
    // listed points (NULL entries are skipped) in ONE slamit_update_points call.  Writes mNormalVector, mfMaxDistance, mfMinDistance
    // and mDescriptor of the points the reference would have written.  Returns the number of points looked at.
    //
    // The keyframes that matter -- the observers and the reference keyframes of the listed points -- are numbered by
    // std::less<KeyFrameT*>, so slamit_update_points' "ascending slot" is the reference's iteration of mObservations on this run: the
    // float sum of the normal and the first least median come out in its order (csrc/upkeep.h).  A keyframe's row holds its keypoint 0
    // (what observations[pRefKF] default-inserts for a reference keyframe that does not observe the point) and then the listed points'
    // observations, so only the descriptors that can be read travel.  mnScaleLevels / mvScaleFactors are one keyframe's: the
    // reference's keyframes share them.
    // Where the reference would read out of bounds (no reference keyframe, a level outside mvScaleFactors) or a ceiling is passed
    // (SLAMIT_UPKEEP_MAX_OBS observers, SLAMIT_DISTINCTIVE_MAX good ones) the point keeps what the status names, the others are
    // written, and LastStatus() is SLAMIT_ERR_ARG / SLAMIT_ERR_CAPACITY with a line on stderr.
    // THROUGH THE SHIM THIS SAVES NOTHING: building the tables walks the same observations as the host loops and copies their
    // descriptors; it is for parity and for integrations that want one code path.  The gain is slamit_update_points_batch_dev with
    // the tables kept in HBM.  Members used: MapPoint isBad(), GetObservations(),
    // GetReferenceKeyFrame(), GetWorldPos(), mNormalVector, mfMaxDistance, mfMinDistance, mDescriptor; KeyFrame isBad(),
    // GetCameraCenter(), mvKeysUn, mDescriptors, mvScaleFactors, mnScaleLevels.
    template <class MapPointT>
    static int UpdateMapPoints(const std::vector<MapPointT*>& vpMP, int what, int device = 0) {
        status() = SLAMIT_OK;
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        std::vector<int32_t> points;
        for (size_t i = 0; i < vpMP.size(); ++i)
            if (vpMP[i]) points.push_back(slotOf(mpSlot, mps, vpMP[i]));
        if (points.empty()) return 0;
        return updateMapPoints(mps, points, mps[0]->GetObservations(), what, device);
    }

    // LocalMapping::MapPointCulling (LocalMapping.cc:184-219) over mlpRecentAddedMapPoints for the current keyframe: ONE
    // slamit_map_point_culling call gives every entry its verdict, then SetBadFlag() is called on the points the reference calls it on
    // and the list is erased from, both in list order.  Returns the number of SetBadFlag() calls.
    // GetFoundRatio() < 0.25f is evaluated here, on the caller's own float, and travels as found / visible = 0 / 1 or 1 / 1: the
    // counters behind it are not public in the reference.
    // THROUGH THE SHIM THIS SAVES NOTHING: the predicate is five loads and three compares per point.  The gain is
    // slamit_map_point_culling_batch_dev beside the other resident steps.  Members used: MapPoint isBad(), GetFoundRatio(),
    // Observations(), mnFirstKFid, SetBadFlag(); KeyFrame mnId.
    template <class ListT, class KeyFrameT>
    static int MapPointCulling(ListT& mlpRecentAddedMapPoints, KeyFrameT* pCurrentKF, bool mbMonocular, int device = 0) {
        status() = SLAMIT_OK;
        const int n = (int)mlpRecentAddedMapPoints.size();
        if (n == 0) return 0;
        if (n > SLAMIT_UPKEEP_MAX_RECENT) return shim::refuse<LocalMapping>("MapPointCulling: more than SLAMIT_UPKEEP_MAX_RECENT recent points", SLAMIT_ERR_CAPACITY);
        std::vector<uint8_t> mp_bad(n), verdict(n, 0);
        std::vector<int32_t> found(n), visible(n, 1), first(n), nobs(n), recent(n), kept(n, -1);
        int j = 0;
        for (typename ListT::iterator lit = mlpRecentAddedMapPoints.begin(); lit != mlpRecentAddedMapPoints.end(); ++lit, ++j) {
            mp_bad[j] = (*lit)->isBad() ? 1 : 0;
            found[j] = (*lit)->GetFoundRatio() < 0.25f ? 0 : 1;
            first[j] = (int32_t)(*lit)->mnFirstKFid;
            nobs[j] = (*lit)->Observations();
            recent[j] = j;
        }
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = 0; M.n_mp = n; M.mp_bad = mp_bad.data();
        slamit_point_index X;
        memset(&X, 0, sizeof(X));
        X.mp_nobs = nobs.data(); X.mp_found = found.data(); X.mp_visible = visible.data(); X.mp_first_kf = first.data();
        int32_t n_kept = 0, st = 0;
        const int rc = slamit_map_point_culling(device, &M, &X, (int32_t)pCurrentKF->mnId, mbMonocular ? 1 : 0, n, recent.data(), verdict.data(), kept.data(), &n_kept, &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("MapPointCulling: slamit_map_point_culling", rc);
        if (st != 0) return shim::refuse<LocalMapping>("MapPointCulling: slamit_map_point_culling reported a status on tables built here", SLAMIT_ERR_STATE);
        int calls = 0;
        j = 0;
        for (typename ListT::iterator lit = mlpRecentAddedMapPoints.begin(); lit != mlpRecentAddedMapPoints.end(); ++j) {
            if (verdict[j] == SLAMIT_UPKEEP_KEPT) { ++lit; continue; }
            if (verdict[j] == SLAMIT_UPKEEP_LOW_RATIO || verdict[j] == SLAMIT_UPKEEP_FEW_OBS) { (*lit)->SetBadFlag(); ++calls; }   // :206, :211
            lit = mlpRecentAddedMapPoints.erase(lit);
        }
        return calls;
    }

    // One edit of ApplyMapEdits over the caller's objects: kind SLAMIT_EDIT_ADD_OBS (pMP->AddObservation(pKF, idx), with flags &
    // SLAMIT_EDIT_MATCH also pKF->AddMapPoint(pMP, idx)), SLAMIT_EDIT_ERASE_OBS (with MATCH first pKF->EraseMapPointMatch(pMP), then
    // pMP->EraseObservation(pKF)) or SLAMIT_EDIT_SET_BAD (pMP->SetBadFlag()).
    template <class MapPointT, class KeyFrameT>
    struct MapEdit {
        int kind, flags;
        MapPointT* pMP;
        KeyFrameT* pKF;
        size_t idx;
    };

    // The point-side mutators of the map (MapPoint.cc:104-174 with KeyFrame.cc:215-234) for a LIST of edits, applied as if one after the
    // other in ONE slamit_map_edit_apply call.  Writes back mObservations, nObs, mbBad and mpRefKF of the points the edits name and the
    // changed entries of mvpMapPoints of the keyframes around them, and calls pMap->EraseMapPoint on the points turned bad.  Returns the
    // number of edits.  Keyframes -- the ones the edits name, the observers and the reference keyframes of the named points -- are
    // numbered by std::less<KeyFrameT*>, so "the remaining observer with the smallest slot" is mObservations.begin() on this run.  Every
    // point stored in those keyframes' mvpMapPoints gets a slot (an unnamed one an empty row), so that a SetBadFlag that erases by index
    // erases whatever is stored there.  Where the reference reads end() (the reference keyframe erased as the last observer) mpRefKF
    // becomes NULL.  A point with more than SLAMIT_EDIT_MAX_PER_POINT edits or SLAMIT_UPKEEP_MAX_OBS observers is left as it was, the
    // others are written, and LastStatus() is SLAMIT_ERR_CAPACITY with a line on stderr.
    // IT SAVES NOTHING THROUGH THE SHIM: building the tables walks the observations and the keyframes' rows that the three mutators
    // touch a few entries of.  It is for parity and for integrations that want one code path; the gain is slamit_map_edit_batch_dev with
    // the tables kept in HBM.  Members used (a friend declaration in the reference's classes): MapPoint mObservations, nObs, mbBad,
    // mpRefKF; KeyFrame mvpMapPoints, mvuRight, mvKeysUn; Map EraseMapPoint().
    template <class MapPointT, class KeyFrameT, class MapT>
    static int ApplyMapEdits(const std::vector<MapEdit<MapPointT, KeyFrameT> >& edits, MapT* pMap, int device = 0) {
        typedef typename std::map<KeyFrameT*, size_t>::const_iterator ObsIt;
        status() = SLAMIT_OK;
        const int n = (int)edits.size();
        if (n == 0) return 0;
        if (n > SLAMIT_EDIT_MAX_EDITS) return shim::refuse<LocalMapping>("ApplyMapEdits: more than SLAMIT_EDIT_MAX_EDITS edits", SLAMIT_ERR_CAPACITY);
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        std::set<KeyFrameT*> all;
        for (int i = 0; i < n; ++i) {
            if (!edits[i].pMP || (edits[i].kind != SLAMIT_EDIT_SET_BAD && !edits[i].pKF)) return shim::refuse<LocalMapping>("ApplyMapEdits: an edit without its point or keyframe");
            slotOf(mpSlot, mps, edits[i].pMP);
            if (edits[i].kind != SLAMIT_EDIT_SET_BAD) all.insert(edits[i].pKF);
        }
        const int n_named = (int)mps.size();
        for (int p = 0; p < n_named; ++p) {
            if (mps[p]->mpRefKF) all.insert(mps[p]->mpRefKF);
            for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) all.insert(it->first);
        }
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("ApplyMapEdits: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the points", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp;
        for (int k = 0; k < n_kf; ++k) {
            for (size_t i = 0; i < kfs[k]->mvpMapPoints.size(); ++i) kf_mp.push_back(kfs[k]->mvpMapPoints[i] ? slotOf(mpSlot, mps, kfs[k]->mvpMapPoints[i]) : -1);
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        const int n_mp = (int)mps.size();
        std::vector<int32_t> obs_ptr(n_mp + 1, 0), obs_kf, obs_idx, mp_nobs(n_mp, 0), mp_ref(n_mp, -1);
        std::vector<uint8_t> obs_octave, obs_weight, mp_bad(n_mp, 0);
        for (int p = 0; p < n_mp; ++p) {
            if (p < n_named) {
                mp_bad[p] = mps[p]->mbBad ? 1 : 0; mp_nobs[p] = mps[p]->nObs;
                if (mps[p]->mpRefKF) mp_ref[p] = kfSlot[mps[p]->mpRefKF];
                for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) {
                    KeyFrameT* kf = it->first;
                    obs_kf.push_back(kfSlot[kf]); obs_idx.push_back((int32_t)it->second);
                    obs_octave.push_back(it->second < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[it->second].octave : 0);
                    obs_weight.push_back(it->second < kf->mvuRight.size() && kf->mvuRight[it->second] >= 0 ? 2 : 1);
                }
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        std::vector<slamit_map_edit> list(n);
        for (int i = 0; i < n; ++i) {
            slamit_map_edit& e = list[i];
            memset(&e, 0, sizeof(e));
            e.kind = edits[i].kind; e.flags = edits[i].flags; e.mp = mpSlot[edits[i].pMP];
            if (e.kind == SLAMIT_EDIT_SET_BAD) continue;
            KeyFrameT* kf = edits[i].pKF;
            e.kf = kfSlot[kf]; e.idx = (int32_t)edits[i].idx;
            if (e.kind == SLAMIT_EDIT_ADD_OBS) {
                e.octave = edits[i].idx < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[edits[i].idx].octave : 0;
                e.weight = edits[i].idx < kf->mvuRight.size() && kf->mvuRight[edits[i].idx] >= 0 ? 2 : 1;
            }
        }
        const size_t cap = obs_kf.size() + (size_t)n;
        std::vector<int32_t> optr(n_mp + 1, 0), okf(cap, 0), oidx(cap, 0), st_mp(n_mp, 0), touched(n_mp, -1), kf_mp_new(kf_mp);
        std::vector<uint8_t> ooct(cap, 0), owgt(cap, 0), bad_new(mp_bad);
        std::vector<int32_t> nobs_new(mp_nobs), ref_new(mp_ref);
        int32_t none32 = -1;
        uint8_t none8 = 0;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp; M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.kf_mp_ptr = kf_mp_ptr.data();
        slamit_edit_index X;
        memset(&X, 0, sizeof(X));
        X.obs_idx = obs_idx.empty() ? &none32 : obs_idx.data(); X.obs_octave = obs_octave.empty() ? &none8 : obs_octave.data();
        X.obs_weight = obs_weight.empty() ? &none8 : obs_weight.data();
        X.mp_bad = bad_new.data(); X.mp_nobs = nobs_new.data(); X.mp_ref_kf = ref_new.data(); X.kf_mp = kf_mp_new.empty() ? &none32 : kf_mp_new.data();
        X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
        X.obs_cap_out = (int32_t)cap;
        int32_t n_touched = 0, n_obs_out = 0, st = 0;
        const int rc = slamit_map_edit_apply(device, &M, &X, n, list.data(), st_mp.data(), touched.data(), &n_touched, &n_obs_out, &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("ApplyMapEdits: slamit_map_edit_apply", rc);
        if (st != 0) return shim::refuse<LocalMapping>("ApplyMapEdits: slamit_map_edit_apply reported a status on tables built here", SLAMIT_ERR_STATE);
        int any = 0;
        for (int p = 0; p < n_named; ++p) {
            any |= st_mp[p];
            if (st_mp[p] & (SLAMIT_EDIT_EDIT_OVERFLOW | SLAMIT_EDIT_OBS_OVERFLOW)) continue;
            MapPointT* pMP = mps[p];
            pMP->mObservations.clear();
            for (int o = optr[p]; o < optr[p + 1]; ++o) pMP->mObservations[kfs[okf[o]]] = (size_t)oidx[o];
            pMP->nObs = nobs_new[p];
            pMP->mpRefKF = ref_new[p] < 0 ? (KeyFrameT*)0 : kfs[ref_new[p]];
            const bool turned = bad_new[p] && !mp_bad[p];
            pMP->mbBad = bad_new[p] != 0;
            if (turned) pMap->EraseMapPoint(pMP);                          // MapPoint.cc:173
        }
        for (int k = 0; k < n_kf; ++k)
            for (int e = kf_mp_ptr[k]; e < kf_mp_ptr[k + 1]; ++e)
                if (kf_mp_new[e] != kf_mp[e]) kfs[k]->mvpMapPoints[e - kf_mp_ptr[k]] = kf_mp_new[e] < 0 ? (MapPointT*)0 : mps[kf_mp_new[e]];
        if (any & (SLAMIT_EDIT_EDIT_OVERFLOW | SLAMIT_EDIT_OBS_OVERFLOW))
            shim::refuse<LocalMapping>("ApplyMapEdits: a point above SLAMIT_EDIT_MAX_PER_POINT edits or SLAMIT_UPKEEP_MAX_OBS observers was left as it was", SLAMIT_ERR_CAPACITY);
        return n;
    }

    // One op of ReplaceMapPoints over the caller's objects: kind SLAMIT_REPLACE_REPLACE (pMP->Replace(pRep)) or SLAMIT_REPLACE_ADD_OBS
    // (pMP->AddObservation(pKF, idx) and pKF->AddMapPoint(pMP, idx), the other branch of ORBmatcher::Fuse's tail).
    template <class MapPointT, class KeyFrameT>
    struct ReplaceOp {
        int kind;
        MapPointT* pMP;
        MapPointT* pRep;   // REPLACE
        KeyFrameT* pKF;    // ADD_OBS
        size_t idx;        // ADD_OBS
    };

    // MapPoint::Replace (MapPoint.cc:183-221) for a LIST of ops as ORBmatcher::Fuse's tail, LoopClosing::SearchAndFuse and ::CorrectLoop
    // issue them, applied as if one after the other in ONE slamit_map_replace_apply call.  Writes back mObservations, nObs, mbBad,
    // mpReplaced, mnFound and mnVisible of the points the ops name and the changed entries of mvpMapPoints of the keyframes around
    // them, and calls pMap->EraseMapPoint on every replaced point (:220).  Returns the number of ops.  ComputeDistinctiveDescriptors of
    // the receivers (:218) is UpdateMapPoints' work and stays the caller's next call.  Keyframes -- the ones the ops name and the
    // observers of the named points -- are numbered by std::less<KeyFrameT*>, so "ascending slot" is the std::map order of this run.
    // The ceilings are all-or-nothing: a point named by more than SLAMIT_REPLACE_MAX_PER_POINT ops or a row past
    // SLAMIT_UPKEEP_MAX_OBS observers leaves EVERYTHING as it was, LastStatus() is SLAMIT_ERR_CAPACITY with a line on stderr.
    // IT SAVES NOTHING THROUGH THE SHIM: building the tables walks the observations and the keyframes' rows that Replace touches a few
    // entries of.  It is for parity and for integrations that want one code path; the gain is slamit_map_replace_batch_dev with the
    // tables kept in HBM.  Members used (a friend declaration in the reference's classes): MapPoint mObservations, nObs, mbBad,
    // mpReplaced, mnFound, mnVisible; KeyFrame mvpMapPoints, mvuRight, mvKeysUn; Map EraseMapPoint().
    template <class MapPointT, class KeyFrameT, class MapT>
    static int ReplaceMapPoints(const std::vector<ReplaceOp<MapPointT, KeyFrameT> >& ops, MapT* pMap, int device = 0) {
        typedef typename std::map<KeyFrameT*, size_t>::const_iterator ObsIt;
        status() = SLAMIT_OK;
        const int n = (int)ops.size();
        if (n == 0) return 0;
        if (n > SLAMIT_REPLACE_MAX_OPS) return shim::refuse<LocalMapping>("ReplaceMapPoints: more than SLAMIT_REPLACE_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        std::set<KeyFrameT*> all;
        for (int i = 0; i < n; ++i) {
            const bool rep = ops[i].kind == SLAMIT_REPLACE_REPLACE;
            if (!rep && ops[i].kind != SLAMIT_REPLACE_ADD_OBS) return shim::refuse<LocalMapping>("ReplaceMapPoints: an op's kind outside 1..2");
            if (!ops[i].pMP || (rep ? !ops[i].pRep : !ops[i].pKF)) return shim::refuse<LocalMapping>("ReplaceMapPoints: an op without its point, replacement or keyframe");
            slotOf(mpSlot, mps, ops[i].pMP);
            if (rep) slotOf(mpSlot, mps, ops[i].pRep); else all.insert(ops[i].pKF);
        }
        const int n_named = (int)mps.size();
        for (int p = 0; p < n_named; ++p)
            for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) all.insert(it->first);
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("ReplaceMapPoints: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the points", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp;
        for (int k = 0; k < n_kf; ++k) {                                       // every stored point gets a slot: a changed entry is found by comparing
            for (size_t i = 0; i < kfs[k]->mvpMapPoints.size(); ++i) kf_mp.push_back(kfs[k]->mvpMapPoints[i] ? slotOf(mpSlot, mps, kfs[k]->mvpMapPoints[i]) : -1);
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        std::vector<int32_t> rep_named(n_named, -1);
        for (int p = 0; p < n_named; ++p)
            if (mps[p]->mpReplaced) rep_named[p] = slotOf(mpSlot, mps, mps[p]->mpReplaced);
        const int n_mp = (int)mps.size();
        std::vector<int32_t> obs_ptr(n_mp + 1, 0), obs_kf, obs_idx, mp_nobs(n_mp, 0), mp_found(n_mp, 0), mp_visible(n_mp, 0), mp_replaced(n_mp, -1);
        std::vector<uint8_t> obs_octave, obs_weight, mp_bad(n_mp, 0);
        for (int p = 0; p < n_mp; ++p) {
            if (p < n_named) {
                mp_bad[p] = mps[p]->mbBad ? 1 : 0; mp_nobs[p] = mps[p]->nObs; mp_found[p] = mps[p]->mnFound; mp_visible[p] = mps[p]->mnVisible; mp_replaced[p] = rep_named[p];
                for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) {
                    KeyFrameT* kf = it->first;
                    obs_kf.push_back(kfSlot[kf]); obs_idx.push_back((int32_t)it->second);
                    obs_octave.push_back(it->second < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[it->second].octave : 0);
                    obs_weight.push_back(it->second < kf->mvuRight.size() && kf->mvuRight[it->second] >= 0 ? 2 : 1);
                }
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        std::vector<slamit_map_replace> list(n);
        size_t adds = 0;
        for (int i = 0; i < n; ++i) {
            slamit_map_replace& e = list[i];
            memset(&e, 0, sizeof(e));
            e.kind = ops[i].kind; e.a = mpSlot[ops[i].pMP];
            if (e.kind == SLAMIT_REPLACE_REPLACE) { e.b = mpSlot[ops[i].pRep]; continue; }
            KeyFrameT* kf = ops[i].pKF;
            e.b = kfSlot[kf]; e.idx = (int32_t)ops[i].idx;
            e.octave = ops[i].idx < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[ops[i].idx].octave : 0;
            e.weight = ops[i].idx < kf->mvuRight.size() && kf->mvuRight[ops[i].idx] >= 0 ? 2 : 1;
            ++adds;
        }
        const size_t cap = obs_kf.size() + adds;                               // Replace never creates an observation
        std::vector<int32_t> optr(n_mp + 1, 0), okf(cap + 1, 0), oidx(cap + 1, 0), moved(n, 0), erased(n, 0), touched(n_mp, -1), kf_mp_new(kf_mp);
        std::vector<uint8_t> ooct(cap + 1, 0), owgt(cap + 1, 0), bad_new(mp_bad);
        std::vector<int32_t> nobs_new(mp_nobs), found_new(mp_found), visible_new(mp_visible), rep_new(mp_replaced);
        int32_t none32 = -1;
        uint8_t none8 = 0;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp; M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.kf_mp_ptr = kf_mp_ptr.data();
        slamit_replace_index X;
        memset(&X, 0, sizeof(X));
        X.obs_idx = obs_idx.empty() ? &none32 : obs_idx.data(); X.obs_octave = obs_octave.empty() ? &none8 : obs_octave.data();
        X.obs_weight = obs_weight.empty() ? &none8 : obs_weight.data();
        X.mp_bad = bad_new.data(); X.mp_nobs = nobs_new.data(); X.mp_found = found_new.data(); X.mp_visible = visible_new.data(); X.mp_replaced = rep_new.data();
        X.kf_mp = kf_mp_new.empty() ? &none32 : kf_mp_new.data();
        X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
        X.obs_cap_out = (int32_t)cap;
        int32_t n_touched = 0, n_obs_out = 0, st = 0;
        const int rc = slamit_map_replace_apply(device, &M, &X, n, list.data(), moved.data(), erased.data(), touched.data(), &n_touched, &n_obs_out, &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("ReplaceMapPoints: slamit_map_replace_apply", rc);
        if (st & (SLAMIT_REPLACE_OP_OVERFLOW | SLAMIT_REPLACE_OBS_OVERFLOW))
            return shim::refuse<LocalMapping>("ReplaceMapPoints: a point named by more than SLAMIT_REPLACE_MAX_PER_POINT ops or a row past SLAMIT_UPKEEP_MAX_OBS observers: nothing was changed",
                                              SLAMIT_ERR_CAPACITY);
        if (st != 0) return shim::refuse<LocalMapping>("ReplaceMapPoints: slamit_map_replace_apply reported a status on tables built here", SLAMIT_ERR_STATE);
        for (int p = 0; p < n_named; ++p) {
            MapPointT* pMP = mps[p];
            pMP->mObservations.clear();
            for (int o = optr[p]; o < optr[p + 1]; ++o) pMP->mObservations[kfs[okf[o]]] = (size_t)oidx[o];
            pMP->nObs = nobs_new[p]; pMP->mnFound = found_new[p]; pMP->mnVisible = visible_new[p];
            pMP->mbBad = bad_new[p] != 0;
            if (rep_new[p] != mp_replaced[p]) pMP->mpReplaced = mps[rep_new[p]];
        }
        for (int k = 0; k < n_kf; ++k)
            for (int e = kf_mp_ptr[k]; e < kf_mp_ptr[k + 1]; ++e)
                if (kf_mp_new[e] != kf_mp[e]) kfs[k]->mvpMapPoints[e - kf_mp_ptr[k]] = kf_mp_new[e] < 0 ? (MapPointT*)0 : mps[kf_mp_new[e]];
        for (int i = 0; i < n; ++i)
            if (ops[i].kind == SLAMIT_REPLACE_REPLACE && ops[i].pMP != ops[i].pRep) pMap->EraseMapPoint(ops[i].pMP);   // MapPoint.cc:220
        return n;
    }

    // One op of FuseMapPoints over the caller's objects: the point pMP that ORBmatcher::Fuse projected into pKF and the keypoint its
    // search ended with (bestIdx < 0, or a null pMP: bestDist > TH_LOW, nothing happens).
    template <class MapPointT, class KeyFrameT>
    struct FuseOp {
        MapPointT* pMP;
        KeyFrameT* pKF;
        int bestIdx;
    };

    // The tail of ORBmatcher::Fuse (ORBmatcher.cc:853, :955-975) for a LIST of (point, keyframe, matched keypoint) as the searches of
    // SearchInNeighbors end, applied as if one after the other in ONE slamit_map_fuse_apply call: which way a Replace goes, or whether
    // the observation is added, is decided by the library from the state the earlier ops of the list left.  Writes back what
    // ReplaceMapPoints writes back (mObservations, nObs, mbBad, mpReplaced, mnFound, mnVisible of the points the ops name and of the
    // points that stood at the matched keypoints; the changed entries of mvpMapPoints) and calls pMap->EraseMapPoint on every point that
    // was replaced.  Returns nFused, the reference's return value summed over the list.  A row past SLAMIT_UPKEEP_MAX_OBS observers
    // leaves EVERYTHING as it was, LastStatus() is SLAMIT_ERR_CAPACITY with a line on stderr.  NOTHING IS SAVED THROUGH THE SHIM, as
    // ReplaceMapPoints: the gain is slamit_fuse_list_batch_dev + slamit_map_fuse_batch_dev with the tables kept in HBM.  ORBmatcher::Fuse
    // in shim/ORBmatcher.h stays as it is.  Members used: those of ReplaceMapPoints.
    template <class MapPointT, class KeyFrameT, class MapT>
    static int FuseMapPoints(const std::vector<FuseOp<MapPointT, KeyFrameT> >& ops, MapT* pMap, int device = 0) {
        typedef typename std::map<KeyFrameT*, size_t>::const_iterator ObsIt;
        status() = SLAMIT_OK;
        const int n = (int)ops.size();
        if (n == 0) return 0;
        if (n > SLAMIT_FUSE_MAX_OPS) return shim::refuse<LocalMapping>("FuseMapPoints: more than SLAMIT_FUSE_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        std::set<KeyFrameT*> all;
        for (int i = 0; i < n; ++i) {                                          // the involved points: P and whoever stands at the matched keypoint NOW
            if (!ops[i].pMP || ops[i].bestIdx < 0) continue;
            if (!ops[i].pKF || (size_t)ops[i].bestIdx >= ops[i].pKF->mvpMapPoints.size()) return shim::refuse<LocalMapping>("FuseMapPoints: an op without its keyframe or with a keypoint outside it");
            slotOf(mpSlot, mps, ops[i].pMP);
            if (ops[i].pKF->mvpMapPoints[ops[i].bestIdx]) slotOf(mpSlot, mps, ops[i].pKF->mvpMapPoints[ops[i].bestIdx]);
            all.insert(ops[i].pKF);
        }
        const int n_named = (int)mps.size();
        if (n_named == 0) return 0;
        for (int p = 0; p < n_named; ++p)
            for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) all.insert(it->first);
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("FuseMapPoints: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the points", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp;
        for (int k = 0; k < n_kf; ++k) {                                       // every stored point gets a slot: a changed entry is found by comparing
            for (size_t i = 0; i < kfs[k]->mvpMapPoints.size(); ++i) kf_mp.push_back(kfs[k]->mvpMapPoints[i] ? slotOf(mpSlot, mps, kfs[k]->mvpMapPoints[i]) : -1);
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        std::vector<int32_t> rep_named(n_named, -1);
        for (int p = 0; p < n_named; ++p)
            if (mps[p]->mpReplaced) rep_named[p] = slotOf(mpSlot, mps, mps[p]->mpReplaced);
        const int n_mp = (int)mps.size();
        std::vector<int32_t> obs_ptr(n_mp + 1, 0), obs_kf, obs_idx, mp_nobs(n_mp, 0), mp_found(n_mp, 0), mp_visible(n_mp, 0), mp_replaced(n_mp, -1);
        std::vector<uint8_t> obs_octave, obs_weight, mp_bad(n_mp, 0);
        for (int p = 0; p < n_mp; ++p) {
            if (p < n_named) {
                mp_bad[p] = mps[p]->mbBad ? 1 : 0; mp_nobs[p] = mps[p]->nObs; mp_found[p] = mps[p]->mnFound; mp_visible[p] = mps[p]->mnVisible; mp_replaced[p] = rep_named[p];
                for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it) {
                    KeyFrameT* kf = it->first;
                    obs_kf.push_back(kfSlot[kf]); obs_idx.push_back((int32_t)it->second);
                    obs_octave.push_back(it->second < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[it->second].octave : 0);
                    obs_weight.push_back(it->second < kf->mvuRight.size() && kf->mvuRight[it->second] >= 0 ? 2 : 1);
                }
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        std::vector<slamit_map_replace> list(n);
        for (int i = 0; i < n; ++i) {
            slamit_map_replace& e = list[i];
            memset(&e, 0, sizeof(e));
            e.kind = SLAMIT_FUSE_FUSE; e.idx = -1;
            if (!ops[i].pMP || ops[i].bestIdx < 0) continue;
            KeyFrameT* kf = ops[i].pKF;
            const size_t idx = (size_t)ops[i].bestIdx;
            e.a = mpSlot[ops[i].pMP]; e.b = kfSlot[kf]; e.idx = ops[i].bestIdx;
            e.octave = idx < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[idx].octave : 0;
            e.weight = idx < kf->mvuRight.size() && kf->mvuRight[idx] >= 0 ? 2 : 1;
        }
        const size_t cap = obs_kf.size() + (size_t)n;                          // an observation is created by an add alone
        std::vector<int32_t> optr(n_mp + 1, 0), okf(cap + 1, 0), oidx(cap + 1, 0), outcome(n, 0), moved(n, 0), erased(n, 0), touched(n_mp, -1), kf_mp_new(kf_mp);
        std::vector<uint8_t> ooct(cap + 1, 0), owgt(cap + 1, 0), bad_new(mp_bad);
        std::vector<int32_t> nobs_new(mp_nobs), found_new(mp_found), visible_new(mp_visible), rep_new(mp_replaced);
        int32_t none32 = -1;
        uint8_t none8 = 0;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp; M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.kf_mp_ptr = kf_mp_ptr.data();
        slamit_replace_index X;
        memset(&X, 0, sizeof(X));
        X.obs_idx = obs_idx.empty() ? &none32 : obs_idx.data(); X.obs_octave = obs_octave.empty() ? &none8 : obs_octave.data();
        X.obs_weight = obs_weight.empty() ? &none8 : obs_weight.data();
        X.mp_bad = bad_new.data(); X.mp_nobs = nobs_new.data(); X.mp_found = found_new.data(); X.mp_visible = visible_new.data(); X.mp_replaced = rep_new.data();
        X.kf_mp = kf_mp_new.empty() ? &none32 : kf_mp_new.data();
        X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
        X.obs_cap_out = (int32_t)cap;
        int32_t n_touched = 0, n_fused = 0, n_obs_out = 0, st = 0;
        const int rc = slamit_map_fuse_apply(device, &M, &X, n, list.data(), outcome.data(), moved.data(), erased.data(), touched.data(), &n_touched, &n_fused, &n_obs_out, &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("FuseMapPoints: slamit_map_fuse_apply", rc);
        if (st & SLAMIT_FUSE_OBS_OVERFLOW) return shim::refuse<LocalMapping>("FuseMapPoints: a row past SLAMIT_UPKEEP_MAX_OBS observers: nothing was changed", SLAMIT_ERR_CAPACITY);
        if (st != 0) return shim::refuse<LocalMapping>("FuseMapPoints: slamit_map_fuse_apply reported a status on tables built here", SLAMIT_ERR_STATE);
        for (int p = 0; p < n_named; ++p) {
            MapPointT* pMP = mps[p];
            pMP->mObservations.clear();
            for (int o = optr[p]; o < optr[p + 1]; ++o) pMP->mObservations[kfs[okf[o]]] = (size_t)oidx[o];
            pMP->nObs = nobs_new[p]; pMP->mnFound = found_new[p]; pMP->mnVisible = visible_new[p];
            pMP->mbBad = bad_new[p] != 0;
            if (rep_new[p] != mp_replaced[p]) { pMP->mpReplaced = mps[rep_new[p]]; pMap->EraseMapPoint(pMP); }   // MapPoint.cc:220
        }
        for (int k = 0; k < n_kf; ++k)
            for (int e = kf_mp_ptr[k]; e < kf_mp_ptr[k + 1]; ++e)
                if (kf_mp_new[e] != kf_mp[e]) kfs[k]->mvpMapPoints[e - kf_mp_ptr[k]] = kf_mp_new[e] < 0 ? (MapPointT*)0 : mps[kf_mp_new[e]];
        return n_fused;
    }

    // KeyFrame::SetBadFlag (KeyFrame.cc:460-552) for a LIST of keyframes, applied as if one after the other: ONE slamit_kf_erase_apply call
    // for the graph rows and the spanning tree plus ONE ApplyMapEdits call with the list it emitted for the point side.  Writes back
    // mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights, mspChildrens, mpParent, mbBad and mbToBeErased of the
    // listed keyframes, their neighbours, children and parents (mvOrderedWeights of a keyframe that turned bad is emptied with its
    // keyframes, where the reference leaves the stale weights), and through ApplyMapEdits the points' side.  Returns the number of
    // keyframes that turned bad.  Keyframes are numbered by std::less<KeyFrameT*>, so "ascending slot" is the std::map / std::set order of
    // this run.  A listed keyframe without a parent that is not the origin is skipped whole, where the reference dereferences NULL.  mTcp
    // (read mpParent), Map::EraseKeyFrame, KeyFrameDatabase::erase, SetErase() and the loop edges stay the caller's.  A keyframe above
    // SLAMIT_KF_ERASE_MAX_CHILD children is left as it was and LastStatus() is SLAMIT_ERR_CAPACITY with a line on stderr.
    // THROUGH THE SHIM IT SAVES NOTHING: building the tables walks every row the walk touches a few entries of.  It is for parity and for
    // integrations that want one code path; the gain is slamit_kf_erase_batch_dev with the tables kept in HBM.  Members used (a friend
    // declaration in the reference's classes): KeyFrame mnId, mbNotErase, mbToBeErased, mbBad, mpParent, mspChildrens,
    // mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights, mvpMapPoints, and what ApplyMapEdits names.
    template <class MapPointT, class KeyFrameT, class MapT>
    static int SetBadFlagKeyFrames(const std::vector<KeyFrameT*>& list, MapT* pMap, int device = 0) {
        typedef typename std::map<KeyFrameT*, int>::const_iterator CwIt;
        typedef typename std::set<KeyFrameT*>::const_iterator SetIt;
        status() = SLAMIT_OK;
        const int n = (int)list.size();
        if (n == 0) return 0;
        if (n > SLAMIT_KF_ERASE_MAX_OPS) return shim::refuse<LocalMapping>("SetBadFlagKeyFrames: more than SLAMIT_KF_ERASE_MAX_OPS keyframes", SLAMIT_ERR_CAPACITY);
        // the keyframes whose rows the walk may touch: the listed, their neighbours, children and parents ...
        std::set<KeyFrameT*> active;
        for (int i = 0; i < n; ++i) {
            KeyFrameT* k = list[i];
            if (!k) return shim::refuse<LocalMapping>("SetBadFlagKeyFrames: a null keyframe");
            active.insert(k);
            if (k->mpParent) active.insert(k->mpParent);
            for (CwIt it = k->mConnectedKeyFrameWeights.begin(); it != k->mConnectedKeyFrameWeights.end(); ++it) active.insert(it->first);
            for (SetIt it = k->mspChildrens.begin(); it != k->mspChildrens.end(); ++it) active.insert(*it);
        }
        // ... and the ones their rows name, which get a slot and empty rows
        std::set<KeyFrameT*> all(active);
        for (SetIt a = active.begin(); a != active.end(); ++a) {
            KeyFrameT* k = *a;
            if (k->mpParent) all.insert(k->mpParent);
            for (CwIt it = k->mConnectedKeyFrameWeights.begin(); it != k->mConnectedKeyFrameWeights.end(); ++it) all.insert(it->first);
            for (SetIt it = k->mspChildrens.begin(); it != k->mspChildrens.end(); ++it) all.insert(*it);
            for (size_t e = 0; e < k->mvpOrderedConnectedKeyFrames.size(); ++e) all.insert(k->mvpOrderedConnectedKeyFrames[e]);
        }
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("SetBadFlagKeyFrames: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the list", SLAMIT_ERR_CAPACITY);
        size_t rc = 1;
        for (SetIt a = active.begin(); a != active.end(); ++a) rc = std::max(rc, std::max((*a)->mConnectedKeyFrameWeights.size(), (*a)->mvpOrderedConnectedKeyFrames.size()));
        if (rc > SLAMIT_COVIS_MAX_ROW) return shim::refuse<LocalMapping>("SetBadFlagKeyFrames: a keyframe with more than SLAMIT_COVIS_MAX_ROW connections", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> cw_kf(n_kf * rc, -1), cw_w(n_kf * rc, 0), cw_n(n_kf, 0), ord_kf(n_kf * rc, -1), ord_w(n_kf * rc, 0), ord_n(n_kf, 0);
        std::vector<int32_t> parent(n_kf, -1), child_ptr(n_kf + 1, 0), child, kf_mp_ptr(n_kf + 1, 0), kf_mp;
        std::vector<uint8_t> bad(n_kf, 0), tbe(n_kf, 0), not_erase(n_kf, 0), is_active(n_kf, 0), is_listed(n_kf, 0);
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        int32_t origin = -1;
        for (int i = 0; i < n; ++i) is_listed[kfSlot[list[i]]] = 1;
        for (int k = 0; k < n_kf; ++k) {
            KeyFrameT* kf = kfs[k];
            if (kf->mnId == 0) origin = k;
            bad[k] = kf->mbBad ? 1 : 0; tbe[k] = kf->mbToBeErased ? 1 : 0; not_erase[k] = kf->mbNotErase ? 1 : 0;
            if (active.count(kf)) {
                is_active[k] = 1;
                if (kf->mpParent) parent[k] = kfSlot[kf->mpParent];
                size_t e = 0;
                for (CwIt it = kf->mConnectedKeyFrameWeights.begin(); it != kf->mConnectedKeyFrameWeights.end(); ++it, ++e) { cw_kf[k * rc + e] = kfSlot[it->first]; cw_w[k * rc + e] = it->second; }
                cw_n[k] = (int32_t)e;
                const size_t no = kf->mvpOrderedConnectedKeyFrames.size();
                for (e = 0; e < no; ++e) { ord_kf[k * rc + e] = kfSlot[kf->mvpOrderedConnectedKeyFrames[e]]; ord_w[k * rc + e] = e < kf->mvOrderedWeights.size() ? kf->mvOrderedWeights[e] : 0; }
                ord_n[k] = (int32_t)no;
                for (SetIt it = kf->mspChildrens.begin(); it != kf->mspChildrens.end(); ++it) child.push_back(kfSlot[*it]);   // set order = ascending slot
            }
            child_ptr[k + 1] = (int32_t)child.size();
            if (is_listed[k])
                for (size_t i = 0; i < kf->mvpMapPoints.size(); ++i) kf_mp.push_back(kf->mvpMapPoints[i] ? slotOf(mpSlot, mps, kf->mvpMapPoints[i]) : -1);
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        std::vector<slamit_kf_op> ops(n);
        for (int i = 0; i < n; ++i) {
            memset(&ops[i], 0, sizeof(ops[i]));
            ops[i].kind = SLAMIT_KF_ERASE_SET_BAD; ops[i].kf = kfSlot[list[i]]; ops[i].parent = -1;
        }
        const size_t child_cap = child.size() + (size_t)n * (size_t)n_kf;   // an op inserts each of its keyframe's children once at the most
        const size_t edit_cap = kf_mp.size();
        std::vector<int32_t> child_ptr_new(n_kf + 1, 0), child_new(child_cap + 1, -1), op_status(n, 0);
        std::vector<slamit_map_edit> emitted(edit_cap + 1);
        std::vector<int32_t> cw_kf2(cw_kf), cw_w2(cw_w), cw_n2(cw_n), ord_kf2(ord_kf), ord_w2(ord_w), ord_n2(ord_n), parent2(parent);
        std::vector<uint8_t> bad2(bad), tbe2(tbe);
        int32_t none32 = -1;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = (int32_t)mps.size(); M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.empty() ? &none32 : kf_mp.data();
        M.kf_child_ptr = child_ptr.data(); M.kf_child = child.empty() ? &none32 : child.data();
        slamit_tree_index X;
        memset(&X, 0, sizeof(X));
        X.row_cap = (int32_t)rc; X.origin_kf = origin; X.kf_not_erase = not_erase.data();
        X.kf_bad = bad2.data(); X.kf_parent = parent2.data(); X.kf_to_be_erased = tbe2.data();
        X.cw_kf = cw_kf2.data(); X.cw_w = cw_w2.data(); X.cw_n = cw_n2.data(); X.ord_kf = ord_kf2.data(); X.ord_w = ord_w2.data(); X.ord_n = ord_n2.data();
        X.child_ptr_out = child_ptr_new.data(); X.child_out = child_new.data(); X.child_cap_out = (int32_t)child_cap;
        int32_t n_edits = 0, n_child = 0, st = 0;
        const int rcode = slamit_kf_erase_apply(device, &M, &X, n, ops.data(), op_status.data(), (int32_t)edit_cap, emitted.data(), &n_edits, &n_child, &st);
        if (rcode != SLAMIT_OK) return shim::report<LocalMapping>("SetBadFlagKeyFrames: slamit_kf_erase_apply", rcode);
        if (st & ~SLAMIT_KF_ERASE_ROW_OVERFLOW) return shim::refuse<LocalMapping>("SetBadFlagKeyFrames: slamit_kf_erase_apply reported a status on tables built here", SLAMIT_ERR_STATE);
        int turned = 0;
        for (int k = 0; k < n_kf; ++k) {
            if (!is_active[k]) continue;
            KeyFrameT* kf = kfs[k];
            turned += bad2[k] && !bad[k];
            kf->mbBad = bad2[k] != 0; kf->mbToBeErased = tbe2[k] != 0;
            kf->mpParent = parent2[k] < 0 ? (KeyFrameT*)0 : kfs[parent2[k]];
            kf->mspChildrens.clear();
            for (int e = child_ptr_new[k]; e < child_ptr_new[k + 1]; ++e) kf->mspChildrens.insert(kfs[child_new[e]]);
            if (cw_n2[k] == cw_n[k] && ord_n2[k] == ord_n[k]) continue;     // a row the walk rewrites loses an entry
            kf->mConnectedKeyFrameWeights.clear();
            for (int e = 0; e < cw_n2[k]; ++e) kf->mConnectedKeyFrameWeights[kfs[cw_kf2[k * rc + e]]] = cw_w2[k * rc + e];
            kf->mvpOrderedConnectedKeyFrames.clear();
            kf->mvOrderedWeights.clear();                                    // of a keyframe that turned bad too, where :484 leaves stale weights
            for (int e = 0; e < ord_n2[k]; ++e) { kf->mvpOrderedConnectedKeyFrames.push_back(kfs[ord_kf2[k * rc + e]]); kf->mvOrderedWeights.push_back(ord_w2[k * rc + e]); }
        }
        std::vector<MapEdit<MapPointT, KeyFrameT> > edits((size_t)n_edits);
        for (int i = 0; i < n_edits; ++i) {
            edits[i].kind = SLAMIT_EDIT_ERASE_OBS; edits[i].flags = 0; edits[i].pMP = mps[emitted[i].mp]; edits[i].pKF = kfs[emitted[i].kf]; edits[i].idx = 0;
        }
        ApplyMapEdits(edits, pMap, device);
        if (status() != SLAMIT_OK) return turned;
        if (st & SLAMIT_KF_ERASE_ROW_OVERFLOW)
            shim::refuse<LocalMapping>("SetBadFlagKeyFrames: a keyframe above SLAMIT_KF_ERASE_MAX_CHILD children was left as it was", SLAMIT_ERR_CAPACITY);
        return turned;
    }

    // One op of GrowMap over the caller's objects.  SLAMIT_GROW_NEW_KF: pKF is a keyframe the caller has constructed from its frame
    // (KeyFrame::KeyFrame(Frame&, ...): mvpMapPoints, mvKeysUn, mvuRight are the frame's) and that no object of the map names yet.
    // SLAMIT_GROW_ASSOCIATE: pKF is the keyframe whose row ProcessNewKeyFrame walks.  SLAMIT_GROW_NEW_POINT: pKF is pRefKF, (pKFa, idxA) and
    // (pKFb, idxB) the observers (pKFb null: the one-observer stereo point), accepted what the triangulation said, pos the point, recent
    // whether CreateNewMapPoints would push it to mlpRecentAddedMapPoints.
    template <class KeyFrameT>
    struct GrowOp {
        int kind;
        KeyFrameT* pKF;
        KeyFrameT* pKFa; size_t idxA;
        KeyFrameT* pKFb; size_t idxB;
        bool accepted, recent;
        float pos[3];
    };

    // The places where the map grows -- Map::AddKeyFrame of a new keyframe, MapPoint::MapPoint(Pos, pRefKF, pMap) with AddObservation /
    // AddMapPoint on one or two keyframes and Map::AddMapPoint (LocalMapping.cc:486-500, Tracking.cc:1376-1383, :718-723, :875-891), the loop
    // of ProcessNewKeyFrame (:156-175) -- for a LIST of ops applied as if one after the other: ONE slamit_map_grow_apply call, then ONE
    // ApplyMapEdits call (one slamit_map_edit_apply) with the ADD_OBS list it emitted.  make(pos, pRefKF) constructs a map point; it is called
    // for the accepted points in slot order, which is list order, so the points get the reference's mnId.  Writes back the changed entries
    // of mvpMapPoints, through ApplyMapEdits mObservations / nObs, calls pMap->AddKeyFrame / pMap->AddMapPoint, and appends to `recent`
    // what the reference appends to mlpRecentAddedMapPoints.  Returns the number of points created.  Existing keyframes are numbered by
    // std::less<KeyFrameT*>, the new ones behind them in list order.  UpdateNormalAndDepth, ComputeDistinctiveDescriptors, ComputeBoW and
    // UpdateConnections stay the caller's next calls.  At most SLAMIT_GROW_MAX_FRAMES keyframes may be named by NEW_KF and ASSOCIATE ops.
    // THROUGH THE SHIM IT SAVES NOTHING: building the tables walks every row the ops touch a few entries of.  It is for parity and for
    // integrations that want one code path; the gain is slamit_map_grow_batch_dev with the tables kept in HBM.  Members used (a friend
    // declaration in the reference's classes): KeyFrame mvpMapPoints, mvKeysUn, mvuRight; MapPoint mObservations, mbBad, and what
    // ApplyMapEdits names.
    template <class MapPointT, class KeyFrameT, class MapT, class RecentT, class MakeT>
    static int GrowMap(const std::vector<GrowOp<KeyFrameT> >& ops, MapT* pMap, RecentT& recent, MakeT make, int device = 0) {
        typedef typename std::map<KeyFrameT*, size_t>::const_iterator ObsIt;
        status() = SLAMIT_OK;
        const int n = (int)ops.size();
        if (n == 0) return 0;
        if (n > SLAMIT_GROW_MAX_OPS) return shim::refuse<LocalMapping>("GrowMap: more than SLAMIT_GROW_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
        std::set<KeyFrameT*> fresh, named;
        std::vector<KeyFrameT*> fresh_order, framed;                          // the new keyframes in list order; the keyframes that need a frame record
        std::map<KeyFrameT*, int32_t> frameOf;
        for (int i = 0; i < n; ++i) {
            const GrowOp<KeyFrameT>& e = ops[i];
            if (!e.pKF || (e.kind == SLAMIT_GROW_NEW_POINT && !e.pKFa)) return shim::refuse<LocalMapping>("GrowMap: an op without its keyframe");
            if (e.kind == SLAMIT_GROW_NEW_KF) {
                if (!fresh.insert(e.pKF).second || named.count(e.pKF)) return shim::refuse<LocalMapping>("GrowMap: a NEW_KF op names a keyframe an earlier op named");
                fresh_order.push_back(e.pKF);
            } else if (e.kind == SLAMIT_GROW_ASSOCIATE || e.kind == SLAMIT_GROW_NEW_POINT) {
                KeyFrameT* const ks[3] = {e.pKF, e.kind == SLAMIT_GROW_NEW_POINT ? e.pKFa : (KeyFrameT*)0, e.kind == SLAMIT_GROW_NEW_POINT ? e.pKFb : (KeyFrameT*)0};
                for (int q = 0; q < 3; ++q)
                    if (ks[q] && !fresh.count(ks[q])) named.insert(ks[q]);
            } else return shim::refuse<LocalMapping>("GrowMap: an op's kind outside 1..3");
            if (e.kind != SLAMIT_GROW_NEW_POINT && !frameOf.count(e.pKF)) { frameOf[e.pKF] = (int32_t)framed.size(); framed.push_back(e.pKF); }
        }
        if (framed.size() > SLAMIT_GROW_MAX_FRAMES) return shim::refuse<LocalMapping>("GrowMap: more than SLAMIT_GROW_MAX_FRAMES keyframes named by NEW_KF and ASSOCIATE ops", SLAMIT_ERR_CAPACITY);
        // the points the rows of the named and the new keyframes hold, and the keyframes that observe them
        std::vector<MapPointT*> mps;
        std::map<MapPointT*, int32_t> mpSlot;
        std::set<KeyFrameT*> old(named);
        for (int pass = 0; pass < 2; ++pass) {
            const std::vector<KeyFrameT*> rows(pass ? fresh_order : std::vector<KeyFrameT*>(named.begin(), named.end()));
            for (size_t k = 0; k < rows.size(); ++k)
                for (size_t i = 0; i < rows[k]->mvpMapPoints.size(); ++i) {
                    MapPointT* p = rows[k]->mvpMapPoints[i];
                    if (!p) continue;
                    slotOf(mpSlot, mps, p);
                    for (ObsIt it = p->mObservations.begin(); it != p->mObservations.end(); ++it)
                        if (!fresh.count(it->first)) old.insert(it->first);
                }
        }
        std::vector<KeyFrameT*> kfs(old.begin(), old.end());                  // a std::set orders by std::less
        const int n_kf = (int)kfs.size(), n_mp = (int)mps.size();
        kfs.insert(kfs.end(), fresh_order.begin(), fresh_order.end());        // the new ones behind them, in list order
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        if (kfs.size() > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("GrowMap: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the ops", SLAMIT_ERR_CAPACITY);
        int P = 0, n_rec_ops = 0;
        size_t kp_new = 0, kp_assoc = 0;
        for (int i = 0; i < n; ++i) {
            if (ops[i].kind == SLAMIT_GROW_NEW_POINT) { ++P; n_rec_ops += ops[i].recent; }
            else (ops[i].kind == SLAMIT_GROW_NEW_KF ? kp_new : kp_assoc) += ops[i].pKF->mvpMapPoints.size();
        }
        const int kf_cap = (int)kfs.size(), mp_cap = n_mp + P;
        // the tables: the rows of the old keyframes that are named (the others: empty rows), the observers of every point
        std::vector<int32_t> kf_mp_ptr(kf_cap + 1, 0), kf_mp;
        std::vector<uint8_t> kf_octave;
        for (int k = 0; k < n_kf; ++k) {
            if (named.count(kfs[k]))
                for (size_t i = 0; i < kfs[k]->mvpMapPoints.size(); ++i) {
                    kf_mp.push_back(kfs[k]->mvpMapPoints[i] ? mpSlot[kfs[k]->mvpMapPoints[i]] : -1);
                    kf_octave.push_back(i < kfs[k]->mvKeysUn.size() ? (uint8_t)kfs[k]->mvKeysUn[i].octave : 0);
                }
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        const std::vector<int32_t> kf_mp_old(kf_mp);
        const size_t kfmp_cap = kf_mp.size() + kp_new;
        kf_mp.resize(kfmp_cap + 1, -1); kf_octave.resize(kfmp_cap + 1, 0);
        std::vector<int32_t> obs_ptr(mp_cap + 1, 0), obs_kf;
        std::vector<uint8_t> mp_bad(mp_cap + 1, 0);
        for (int p = 0; p < n_mp; ++p) {
            mp_bad[p] = mps[p]->mbBad ? 1 : 0;
            for (ObsIt it = mps[p]->mObservations.begin(); it != mps[p]->mObservations.end(); ++it)
                if (!fresh.count(it->first)) obs_kf.push_back(kfSlot[it->first]);
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        // the frame records: what KeyFrame::KeyFrame copies from the frame is what the keyframe object holds
        std::vector<std::vector<int32_t> > f_mp(framed.size());
        std::vector<std::vector<uint8_t> > f_oct(framed.size()), f_desc(framed.size());
        std::vector<std::vector<float> > f_ur(framed.size());
        const float eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        std::vector<slamit_grow_frame> frames(framed.size());
        for (size_t f = 0; f < framed.size(); ++f) {
            KeyFrameT* kf = framed[f];
            const size_t nk = kf->mvpMapPoints.size();
            f_mp[f].resize(nk + 1, -1); f_oct[f].resize(nk + 1, 0); f_desc[f].resize(32 * nk + 32, 0); f_ur[f].resize(nk + 1, -1.f);
            for (size_t i = 0; i < nk; ++i) {
                f_mp[f][i] = kf->mvpMapPoints[i] ? mpSlot[kf->mvpMapPoints[i]] : -1;
                f_oct[f][i] = i < kf->mvKeysUn.size() ? (uint8_t)kf->mvKeysUn[i].octave : 0;
                f_ur[f][i] = i < kf->mvuRight.size() ? kf->mvuRight[i] : -1.f;
            }
            memset(&frames[f], 0, sizeof(frames[f]));
            frames[f].n_kp = (int32_t)nk; frames[f].frame_mp = f_mp[f].data(); frames[f].octave = f_oct[f].data(); frames[f].desc = f_desc[f].data();
            frames[f].uright = f_ur[f].data(); frames[f].Tcw = eye;
        }
        std::vector<slamit_grow_op> list(n);
        for (int i = 0; i < n; ++i) {
            const GrowOp<KeyFrameT>& e = ops[i];
            slamit_grow_op& o = list[i];
            memset(&o, 0, sizeof(o));
            o.kind = e.kind; o.kf = kfSlot[e.pKF]; o.cand = -1; o.kf_b = -1;
            if (e.kind != SLAMIT_GROW_NEW_POINT) { o.src = frameOf[e.pKF]; continue; }
            o.flags = e.recent ? SLAMIT_GROW_RECENT : 0; o.cand = e.accepted ? -1 : 0;
            o.kf_a = kfSlot[e.pKFa]; o.idx_a = (int32_t)e.idxA; o.weight_a = e.idxA < e.pKFa->mvuRight.size() && e.pKFa->mvuRight[e.idxA] >= 0 ? 2 : 1;
            if (e.pKFb) { o.kf_b = kfSlot[e.pKFb]; o.idx_b = (int32_t)e.idxB; o.weight_b = e.idxB < e.pKFb->mvuRight.size() && e.pKFb->mvuRight[e.idxB] >= 0 ? 2 : 1; }
            for (int c = 0; c < 3; ++c) o.pos[c] = e.pos[c];
        }
        const uint8_t rejected = 1;                                           // candidate 0: the status of every op that is not accepted
        const float no_pos[3] = {0, 0, 0};
        // the columns the call appends to and the caller's objects already hold or do not keep: scratch
        const size_t K = (size_t)kf_cap + 1, Q = (size_t)mp_cap + 1;
        std::vector<uint8_t> kf_desc(32 * (kfmp_cap + 1), 0), kf_bad(K, 0), kf_tbe(K, 0), kf_ne(K, 0), mp_desc(32 * Q, 0);
        std::vector<int32_t> kf_parent(K, -1), kf_best(SLAMIT_LOCAL_MAP_BEST * K, -1), cw_n(K, 0), ord_n(K, 0), child_ptr(K + 1, 0), mp_nobs(Q, 0), mp_ref(Q, -1), mp_found(Q, 0),
            mp_visible(Q, 0), mp_first(Q, 0), mp_replaced(Q, -1);
        std::vector<float> kf_center(3 * K, 0.f), mp_pos(3 * Q, 0.f), mp_normal(3 * Q, 0.f), mp_max(Q, 0.f), mp_min(Q, 0.f);
        int32_t none32 = -1;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp; M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data();
        slamit_grow_index X;
        memset(&X, 0, sizeof(X));
        X.kf_cap = kf_cap; X.mp_cap = mp_cap; X.kfmp_cap = (int32_t)kfmp_cap;
        X.kf_mp_ptr = kf_mp_ptr.data(); X.kf_mp = kf_mp.data(); X.kf_octave = kf_octave.data(); X.kf_desc = kf_desc.data(); X.kf_bad = kf_bad.data(); X.kf_parent = kf_parent.data();
        X.kf_to_be_erased = kf_tbe.data(); X.kf_not_erase = kf_ne.data(); X.kf_best = kf_best.data(); X.cw_n = cw_n.data(); X.ord_n = ord_n.data(); X.kf_child_ptr = child_ptr.data();
        X.kf_center = kf_center.data(); X.mp_pos = mp_pos.data(); X.mp_normal = mp_normal.data(); X.mp_max_dist = mp_max.data(); X.mp_min_dist = mp_min.data(); X.mp_bad = mp_bad.data();
        X.mp_nobs = mp_nobs.data(); X.mp_ref_kf = mp_ref.data(); X.mp_found = mp_found.data(); X.mp_visible = mp_visible.data(); X.mp_first_kf = mp_first.data();
        X.mp_replaced = mp_replaced.data(); X.mp_desc = mp_desc.data(); X.obs_ptr = obs_ptr.data();
        const size_t edit_cap = 2 * (size_t)P + kp_assoc, recent_cap = (size_t)n_rec_ops + kp_assoc;
        if (edit_cap > SLAMIT_EDIT_MAX_EDITS || recent_cap > SLAMIT_UPKEEP_MAX_RECENT) return shim::refuse<LocalMapping>("GrowMap: the ops may emit more edits or recent entries than a list holds", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> op_status(n, 0), rec_slots(recent_cap + 1, -1);
        std::vector<slamit_map_edit> emitted(edit_cap + 1);
        int32_t n_edits = 0, n_recent = 0, n_new = 0, need[SLAMIT_GROW_NEEDS], st = 0;
        const int rcode = slamit_map_grow_apply(device, &M, &X, (int32_t)frames.size(), frames.data(), n, list.data(), 1, &rejected, no_pos, op_status.data(), (int32_t)edit_cap,
                                                emitted.data(), &n_edits, (int32_t)recent_cap, rec_slots.data(), &n_recent, &n_new, need, &st);
        if (rcode != SLAMIT_OK) return shim::report<LocalMapping>("GrowMap: slamit_map_grow_apply", rcode);
        if (st != 0) return shim::refuse<LocalMapping>("GrowMap: slamit_map_grow_apply reported a status on tables built here", SLAMIT_ERR_STATE);
        // write back: the new objects in slot order, the rows, the map, the recent list; then the observations through ApplyMapEdits
        for (int i = 0; i < n; ++i) {
            if (ops[i].kind == SLAMIT_GROW_NEW_KF) pMap->AddKeyFrame(ops[i].pKF);
            if (ops[i].kind != SLAMIT_GROW_NEW_POINT || op_status[i] < 0) continue;
            if (op_status[i] != (int32_t)mps.size()) return shim::refuse<LocalMapping>("GrowMap: the slots of the new points do not ascend in list order", SLAMIT_ERR_STATE);
            MapPointT* pMP = make(ops[i].pos, ops[i].pKF);
            mps.push_back(pMP);
            pMap->AddMapPoint(pMP);
        }
        for (size_t k = 0; k < kfs.size(); ++k) {
            const bool is_new = (int)k >= n_kf;
            if (!is_new && !named.count(kfs[k])) continue;
            for (int e = kf_mp_ptr[k]; e < kf_mp_ptr[k + 1]; ++e) {
                MapPointT* now = kf_mp[e] < 0 ? (MapPointT*)0 : mps[kf_mp[e]];
                if (kfs[k]->mvpMapPoints[e - kf_mp_ptr[k]] != now) kfs[k]->mvpMapPoints[e - kf_mp_ptr[k]] = now;
            }
        }
        for (int r = 0; r < n_recent; ++r) recent.push_back(mps[rec_slots[r]]);
        std::vector<MapEdit<MapPointT, KeyFrameT> > edits((size_t)n_edits);
        for (int i = 0; i < n_edits; ++i) {
            edits[i].kind = SLAMIT_EDIT_ADD_OBS; edits[i].flags = 0; edits[i].pMP = mps[emitted[i].mp]; edits[i].pKF = kfs[emitted[i].kf]; edits[i].idx = (size_t)emitted[i].idx;
        }
        ApplyMapEdits(edits, pMap, device);
        return n_new;
    }

    static int LastStatus() { return status(); }

private:
    // a new slot for a pointer on first sight
    template <class T>
    static int32_t slotOf(std::map<T*, int32_t>& slots, std::vector<T*>& all, T* p) {
        typename std::map<T*, int32_t>::const_iterator it = slots.find(p);
        if (it != slots.end()) return it->second;
        const int32_t s = (int32_t)all.size();
        slots[p] = s;
        all.push_back(p);
        return s;
    }

    template <class KeyFrameT, class MapPointT>
    static int updateConnections(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMP, int device) {
        std::set<KeyFrameT*> all;
        all.insert(pKF);
        for (size_t i = 0; i < vpMP.size(); ++i) {
            if (!vpMP[i] || vpMP[i]->isBad()) continue;
            const std::map<KeyFrameT*, size_t> obs = vpMP[i]->GetObservations();
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) all.insert(it->first);
        }
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size(), k = kfSlot[pKF];
        if (n_kf - 1 > SLAMIT_COVIS_MAX_ROW) return shim::refuse<LocalMapping>("UpdateConnections: more than SLAMIT_COVIS_MAX_ROW keyframes share a point with this one", SLAMIT_ERR_CAPACITY);
        const int row_cap = n_kf > 1 ? n_kf - 1 : 1, n_mp = (int)vpMP.size();
        // one row of points (pKF's), one point per keypoint; only pKF's own points vote
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp(vpMP.size(), -1), obs_ptr(n_mp + 1, 0), obs_kf;
        std::vector<uint8_t> mp_bad(n_mp + 1, 0);
        for (int i = 0; i < n_mp; ++i) {
            if (vpMP[i]) {
                kf_mp[i] = i;
                mp_bad[i] = vpMP[i]->isBad() ? 1 : 0;
                if (!mp_bad[i]) {
                    const std::map<KeyFrameT*, size_t> obs = vpMP[i]->GetObservations();
                    for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) obs_kf.push_back(kfSlot[it->first]);
                }
            }
            obs_ptr[i + 1] = (int32_t)obs_kf.size();
        }
        for (int j = k + 1; j <= n_kf; ++j) kf_mp_ptr[j] = n_mp;
        int32_t none32 = -1;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.mp_bad = mp_bad.data();
        M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.empty() ? &none32 : kf_mp.data();
        const size_t rows = (size_t)n_kf * row_cap;
        std::vector<int32_t> cw_kf(rows, -1), cw_w(rows, 0), cw_n(n_kf, 0), ord_kf(rows, -1), ord_w(rows, 0), ord_n(n_kf, 0), counts(n_kf, 0);
        slamit_covis_index X;
        memset(&X, 0, sizeof(X));
        X.row_cap = row_cap; X.origin_kf = pKF->mnId == 0 ? k : -1;
        X.cw_kf = cw_kf.data(); X.cw_w = cw_w.data(); X.cw_n = cw_n.data(); X.ord_kf = ord_kf.data(); X.ord_w = ord_w.data(); X.ord_n = ord_n.data();
        int32_t n_counted = 0, n_listed = 0, parent = -1, st = 0;
        const int rc = slamit_update_connections(device, &M, &X, k, pKF->mbFirstConnection ? 1 : 0, counts.data(), &n_counted, &n_listed, &parent, &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("UpdateConnections: slamit_update_connections", rc);
        if (st == SLAMIT_COVIS_NO_OBSERVER) return 0;   // :331
        if (st != 0) return shim::refuse<LocalMapping>("UpdateConnections: slamit_update_connections reported a status on tables built here", SLAMIT_ERR_STATE);
        // :347-358: AddConnection on the listed neighbours, in map (address) order
        std::map<KeyFrameT*, int> KFcounter;
        bool any = false;
        for (int j = 0; j < n_kf; ++j) {
            if (counts[j] <= 0) continue;
            KFcounter[kfs[j]] = counts[j];
            if (counts[j] >= SLAMIT_COVIS_TH) { kfs[j]->AddConnection(pKF, counts[j]); any = true; }
        }
        if (!any) kfs[ord_kf[(size_t)k * row_cap]]->AddConnection(pKF, ord_w[(size_t)k * row_cap]);
        pKF->mConnectedKeyFrameWeights = KFcounter;
        pKF->mvpOrderedConnectedKeyFrames.clear();
        pKF->mvOrderedWeights.clear();
        for (int e = 0; e < n_listed; ++e) {
            pKF->mvpOrderedConnectedKeyFrames.push_back(kfs[ord_kf[(size_t)k * row_cap + e]]);
            pKF->mvOrderedWeights.push_back(ord_w[(size_t)k * row_cap + e]);
        }
        if (parent >= 0) {   // :374-379: mbFirstConnection && mnId != 0
            pKF->mpParent = kfs[parent];
            pKF->mpParent->AddChild(pKF);
            pKF->mbFirstConnection = false;
        }
        return n_listed;
    }

    // mvDepth / mThDepth of a keyframe type that has them
    template <class KeyFrameT>
    static float depthOf(KeyFrameT* kf, size_t i, shim::bool_tag<true>) { return kf->mvDepth[i]; }
    template <class KeyFrameT>
    static float depthOf(KeyFrameT*, size_t, shim::bool_tag<false>) { return 0.f; }
    template <class KeyFrameT>
    static float thDepthOf(KeyFrameT* kf, shim::bool_tag<true>) { return kf->mThDepth; }
    template <class KeyFrameT>
    static float thDepthOf(KeyFrameT*, shim::bool_tag<false>) { return 0.f; }

    template <class KeyFrameT, class MapPointT>
    static int keyFrameCulling(KeyFrameT* cur, const std::vector<KeyFrameT*>& cands, const std::vector<MapPointT*>&, bool monocular, int device) {
        const shim::bool_tag<shim::has_member_mvDepth<KeyFrameT>::value> depthTag = shim::bool_tag<shim::has_member_mvDepth<KeyFrameT>::value>();
        if (cands.size() > SLAMIT_COVIS_MAX_ROW) return shim::refuse<LocalMapping>("KeyFrameCulling: more than SLAMIT_COVIS_MAX_ROW covisible keyframes", SLAMIT_ERR_CAPACITY);
        // the keyframes that can matter: the current one, the candidates and the observers of the candidates' points
        std::set<KeyFrameT*> all(cands.begin(), cands.end());
        all.insert(cur);
        std::map<MapPointT*, int32_t> mpSlot;
        std::vector<MapPointT*> mps;
        std::vector<std::vector<MapPointT*> > rowsOf(cands.size());
        for (size_t c = 0; c < cands.size(); ++c) {
            rowsOf[c] = cands[c]->GetMapPointMatches();
            for (size_t i = 0; i < rowsOf[c].size(); ++i) {
                MapPointT* pMP = rowsOf[c][i];
                if (!pMP) continue;
                const size_t before = mps.size();
                slotOf(mpSlot, mps, pMP);
                if (mps.size() == before || pMP->isBad()) continue;
                const std::map<KeyFrameT*, size_t> obs = pMP->GetObservations();
                for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) all.insert(it->first);
            }
        }
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size(), n_mp = (int)mps.size(), row_cap = (int)cands.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("KeyFrameCulling: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the candidates", SLAMIT_ERR_CAPACITY);
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0), kf_mp, obs_ptr(n_mp + 1, 0), obs_kf, mp_nobs(n_mp + 1, 0);
        std::vector<uint8_t> kf_octave, mp_bad(n_mp + 1, 0), obs_octave, obs_weight, kf_not_erase(n_kf, 0);
        std::vector<float> kf_depth, kf_th_depth(n_kf, 0.f);
        std::map<KeyFrameT*, size_t> candOf;
        for (size_t c = 0; c < cands.size(); ++c) candOf[cands[c]] = c;
        int origin = -1;
        for (int k = 0; k < n_kf; ++k) {
            KeyFrameT* pKF = kfs[k];
            if (pKF->mnId == 0) origin = k;
            kf_not_erase[k] = pKF->mbNotErase ? 1 : 0;
            kf_th_depth[k] = thDepthOf(pKF, depthTag);
            typename std::map<KeyFrameT*, size_t>::const_iterator c = candOf.find(pKF);
            if (c != candOf.end()) {   // only the candidates' rows are read
                const std::vector<MapPointT*>& row = rowsOf[c->second];
                for (size_t i = 0; i < row.size(); ++i) {
                    kf_mp.push_back(row[i] ? mpSlot[row[i]] : -1);
                    kf_octave.push_back((uint8_t)pKF->mvKeysUn[i].octave);
                    kf_depth.push_back(depthOf(pKF, i, depthTag));
                }
            }
            kf_mp_ptr[k + 1] = (int32_t)kf_mp.size();
        }
        for (int p = 0; p < n_mp; ++p) {
            mp_bad[p] = mps[p]->isBad() ? 1 : 0;
            mp_nobs[p] = mps[p]->Observations();
            if (!mp_bad[p]) {
                const std::map<KeyFrameT*, size_t> obs = mps[p]->GetObservations();
                for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) {
                    obs_kf.push_back(kfSlot[it->first]);
                    obs_octave.push_back((uint8_t)it->first->mvKeysUn[it->second].octave);
                    obs_weight.push_back(it->first->mvuRight[it->second] >= 0 ? 2 : 1);
                }
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        int32_t none32 = -1;
        uint8_t none8 = 0;
        float nonef = 0.f;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.mp_bad = mp_bad.data();
        M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.empty() ? &none32 : kf_mp.data();
        const int c = kfSlot[cur];
        std::vector<int32_t> ord_kf((size_t)n_kf * row_cap, -1), ord_n(n_kf, 0);
        for (size_t e = 0; e < cands.size(); ++e) ord_kf[(size_t)c * row_cap + e] = kfSlot[cands[e]];
        ord_n[c] = row_cap;
        slamit_covis_index X;
        memset(&X, 0, sizeof(X));
        X.row_cap = row_cap; X.origin_kf = origin;
        X.obs_octave = obs_octave.empty() ? &none8 : obs_octave.data(); X.obs_weight = obs_weight.empty() ? &none8 : obs_weight.data();
        X.mp_nobs = mp_nobs.data(); X.kf_octave = kf_octave.empty() ? &none8 : kf_octave.data();
        X.kf_depth = kf_depth.empty() ? &nonef : kf_depth.data(); X.kf_th_depth = kf_th_depth.data(); X.kf_not_erase = kf_not_erase.data();
        X.ord_kf = ord_kf.data(); X.ord_n = ord_n.data();
        std::vector<uint8_t> verdict(row_cap, 0), turned(n_mp + 1, 0);
        std::vector<int32_t> n_mps(row_cap, 0), n_red(row_cap, 0);
        int32_t n_cand = 0, st = 0;
        const int rc = slamit_keyframe_culling(device, &M, &X, c, monocular ? 1 : 0, verdict.data(), n_mps.data(), n_red.data(), &n_cand, turned.data(), &st);
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("KeyFrameCulling: slamit_keyframe_culling", rc);
        if (st != 0 || n_cand != row_cap) return shim::refuse<LocalMapping>("KeyFrameCulling: slamit_keyframe_culling reported a status on tables built here", SLAMIT_ERR_STATE);
        int calls = 0;
        for (int e = 0; e < n_cand; ++e)
            if (verdict[e] == SLAMIT_COVIS_CULLED || verdict[e] == SLAMIT_COVIS_TO_BE_ERASED) {   // :749-750
                cands[e]->SetBadFlag();
                ++calls;
            }
        return calls;
    }

    // mps: the distinct listed points; points: the list as slots of mps; the third argument names the keyframe type
    template <class MapPointT, class KeyFrameT>
    static int updateMapPoints(const std::vector<MapPointT*>& mps, const std::vector<int32_t>& points, const std::map<KeyFrameT*, size_t>&, int what, int device) {
        typedef typename std::map<KeyFrameT*, size_t>::const_iterator ObsIt;
        if (what < 1 || what > 3) return shim::refuse<LocalMapping>("UpdateMapPoints: `what` outside 1..3");
        if (points.size() > (size_t)SLAMIT_UPKEEP_MAX_POINTS) return shim::refuse<LocalMapping>("UpdateMapPoints: more than SLAMIT_UPKEEP_MAX_POINTS points", SLAMIT_ERR_CAPACITY);
        const int n_mp = (int)mps.size();
        std::vector<std::map<KeyFrameT*, size_t> > obsOf(n_mp);
        std::vector<KeyFrameT*> refOf(n_mp, (KeyFrameT*)0);
        std::set<KeyFrameT*> all;
        for (int p = 0; p < n_mp; ++p) {
            obsOf[p] = mps[p]->GetObservations();
            refOf[p] = mps[p]->GetReferenceKeyFrame();
            if (refOf[p]) all.insert(refOf[p]);
            for (ObsIt it = obsOf[p].begin(); it != obsOf[p].end(); ++it) all.insert(it->first);
        }
        if (all.empty()) return (int)points.size();   // nothing observed, no reference keyframe: the reference returns at :262 / :351
        const std::vector<KeyFrameT*> kfs(all.begin(), all.end());   // a std::set orders by std::less
        std::map<KeyFrameT*, int32_t> kfSlot;
        for (size_t k = 0; k < kfs.size(); ++k) kfSlot[kfs[k]] = (int32_t)k;
        const int n_kf = (int)kfs.size();
        if (n_kf > SLAMIT_LOCAL_MAP_MAX_KF) return shim::refuse<LocalMapping>("UpdateMapPoints: more than SLAMIT_LOCAL_MAP_MAX_KF keyframes around the points", SLAMIT_ERR_CAPACITY);
        // a keyframe's row: its keypoint 0, then the listed points' observations in the order met
        std::vector<std::vector<size_t> > rowOf(n_kf);
        for (int k = 0; k < n_kf; ++k)
            if (!kfs[k]->mvKeysUn.empty()) rowOf[k].push_back(0);
        std::vector<int32_t> obs_ptr(n_mp + 1, 0), obs_kf, obs_idx, mp_ref(n_mp, -1);
        std::vector<uint8_t> mp_bad(n_mp, 0), kf_bad(n_kf, 0), mp_desc((size_t)n_mp * 32, 0);
        std::vector<int> good(n_mp, 0);
        std::vector<float> mp_pos((size_t)n_mp * 3), mp_normal((size_t)n_mp * 3, 0.f), mp_max(n_mp, 0.f), mp_min(n_mp, 0.f);
        for (int k = 0; k < n_kf; ++k) kf_bad[k] = kfs[k]->isBad() ? 1 : 0;
        for (int p = 0; p < n_mp; ++p) {
            mp_bad[p] = mps[p]->isBad() ? 1 : 0;
            if (refOf[p]) mp_ref[p] = kfSlot[refOf[p]];
            shim::load3(mps[p]->GetWorldPos(), &mp_pos[3 * (size_t)p]);
            for (ObsIt it = obsOf[p].begin(); it != obsOf[p].end(); ++it) {
                const int k = kfSlot[it->first];
                obs_kf.push_back(k);
                obs_idx.push_back((int32_t)rowOf[k].size());
                rowOf[k].push_back(it->second);
                good[p] += !kf_bad[k];
            }
            obs_ptr[p + 1] = (int32_t)obs_kf.size();
        }
        std::vector<int32_t> kf_mp_ptr(n_kf + 1, 0);
        std::vector<uint8_t> kf_octave, kf_desc, obs_octave(obs_kf.size(), 0);
        std::vector<float> kf_center((size_t)n_kf * 3);
        for (int k = 0; k < n_kf; ++k) {
            shim::load3(kfs[k]->GetCameraCenter(), &kf_center[3 * (size_t)k]);
            for (size_t e = 0; e < rowOf[k].size(); ++e) {
                const size_t i = rowOf[k][e];
                kf_octave.push_back((uint8_t)kfs[k]->mvKeysUn[i].octave);
                const size_t at = kf_desc.size();
                kf_desc.resize(at + 32, 0);
                if ((int)i < kfs[k]->mDescriptors.rows) memcpy(&kf_desc[at], kfs[k]->mDescriptors.ptr((int)i), 32);
            }
            kf_mp_ptr[k + 1] = (int32_t)kf_octave.size();
        }
        for (size_t o = 0; o < obs_kf.size(); ++o) obs_octave[o] = kf_octave[(size_t)kf_mp_ptr[obs_kf[o]] + obs_idx[o]];
        int32_t none32 = -1;
        uint8_t none8 = 0;
        slamit_map_index M;
        memset(&M, 0, sizeof(M));
        M.n_kf = n_kf; M.n_mp = n_mp;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.empty() ? &none32 : obs_kf.data(); M.mp_bad = mp_bad.data(); M.kf_bad = kf_bad.data();
        M.kf_mp_ptr = kf_mp_ptr.data(); M.mp_pos = mp_pos.data();
        slamit_point_index X;
        memset(&X, 0, sizeof(X));
        X.n_levels = kfs[0]->mnScaleLevels;
        for (int l = 0; l < SLAMIT_MAX_LEVELS && l < (int)kfs[0]->mvScaleFactors.size(); ++l) X.scale_factors[l] = kfs[0]->mvScaleFactors[l];
        X.obs_idx = obs_idx.empty() ? &none32 : obs_idx.data(); X.obs_octave = obs_octave.empty() ? &none8 : obs_octave.data();
        X.kf_octave = kf_octave.empty() ? &none8 : kf_octave.data(); X.kf_center = kf_center.data(); X.kf_desc = kf_desc.empty() ? &none8 : kf_desc.data();
        X.mp_ref_kf = mp_ref.data(); X.mp_normal = mp_normal.data(); X.mp_max_dist = mp_max.data(); X.mp_min_dist = mp_min.data(); X.mp_desc = mp_desc.data();
        std::vector<int32_t> st(points.size(), 0);
        const int rc = slamit_update_points(device, &M, &X, (int32_t)points.size(), points.data(), what, st.data());
        if (rc != SLAMIT_OK) return shim::report<LocalMapping>("UpdateMapPoints: slamit_update_points", rc);
        const int keeps_normal = SLAMIT_UPKEEP_NO_REF | SLAMIT_UPKEEP_REF_NO_KP | SLAMIT_UPKEEP_OCTAVE | SLAMIT_UPKEEP_OBS_OVERFLOW;
        int any = 0;
        for (size_t j = 0; j < points.size(); ++j) {
            const int p = points[j];
            MapPointT* pMP = mps[p];
            any |= st[j];
            if (mp_bad[p] || obsOf[p].empty() || (st[j] & SLAMIT_UPKEEP_OBS_OVERFLOW)) continue;   // :257, :262, :344, :351
            if ((what & SLAMIT_UPKEEP_NORMAL) && !(st[j] & keeps_normal)) {
                cv::Mat nrm(3, 1, CV_32F);
                for (int r = 0; r < 3; ++r) nrm.at<float>(r, 0) = mp_normal[3 * (size_t)p + r];
                pMP->mNormalVector = nrm;
                pMP->mfMaxDistance = mp_max[p];
                pMP->mfMinDistance = mp_min[p];
            }
            if ((what & SLAMIT_UPKEEP_DESC) && good[p] > 0 && !(st[j] & SLAMIT_UPKEEP_DESC_OVERFLOW)) {   // :275
                cv::Mat d(1, 32, CV_8U);
                memcpy(d.ptr(0), &mp_desc[32 * (size_t)p], 32);
                pMP->mDescriptor = d;
            }
        }
        if (any & (SLAMIT_UPKEEP_OBS_OVERFLOW | SLAMIT_UPKEEP_DESC_OVERFLOW))
            shim::refuse<LocalMapping>("UpdateMapPoints: a point above SLAMIT_UPKEEP_MAX_OBS observers or SLAMIT_DISTINCTIVE_MAX good ones was left as it was", SLAMIT_ERR_CAPACITY);
        else if (any & (keeps_normal | SLAMIT_UPKEEP_BAD_SLOT))
            shim::refuse<LocalMapping>("UpdateMapPoints: a point without a usable reference keyframe or level kept its normal and distances");
        return (int)points.size();
    }

    static bool never() { return false; }
    static int& status() { return shim::status<LocalMapping>(); }
    template <class KeyFrameT>
    struct StereoTag : shim::bool_tag<shim::has_member_mb<KeyFrameT>::value && shim::has_member_mbf<KeyFrameT>::value &&
                                      shim::has_member_mvDepth<KeyFrameT>::value && shim::has_member_mvKeys<KeyFrameT>::value> {};

    // a keyframe type without the stereo members: the monocular path only
    template <class KeyFrameT>
    static bool accepts(KeyFrameT* cur, const std::vector<KeyFrameT*>& neigh, bool monocular, shim::bool_tag<false>) {
        if (!monocular) { shim::refuse<LocalMapping>("CreateNewMapPoints: only the monocular path is on the device"); return false; }
        if (hasStereo(cur)) { shim::refuse<LocalMapping>("CreateNewMapPoints: the current keyframe carries stereo coordinates (mvuRight >= 0)"); return false; }
        for (size_t i = 0; i < neigh.size(); ++i)
            if (hasStereo(neigh[i])) { shim::refuse<LocalMapping>("CreateNewMapPoints: a neighbour keyframe carries stereo coordinates (mvuRight >= 0)"); return false; }
        return true;
    }
    template <class KeyFrameT>
    static bool accepts(KeyFrameT*, const std::vector<KeyFrameT*>&, bool, shim::bool_tag<true>) { return true; }

    // :273-294
    template <class KeyFrameT>
    static bool baselineTooShort(KeyFrameT* pKF2, float baseline, bool, shim::bool_tag<false>) {
        const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        return ratioBaselineDepth < 0.01;
    }
    template <class KeyFrameT>
    static bool baselineTooShort(KeyFrameT* pKF2, float baseline, bool monocular, shim::bool_tag<true>) {
        if (!monocular) return baseline < pKF2->mb;
        return baselineTooShort(pKF2, baseline, monocular, shim::bool_tag<false>());
    }

    // the device call of one neighbour: the monocular entry point, or the stereo one with the right-image side of every pair
    template <class KeyFrameT>
    static int triangulate(KeyFrameT*, KeyFrameT*, const std::vector<std::pair<size_t, size_t> >&, int device, slamit_triangulate_problem& P,
                           slamit_triangulate_result& R, shim::bool_tag<false>) {
        return slamit_triangulate(device, &P, &R);
    }
    template <class KeyFrameT>
    static int triangulate(KeyFrameT* cur, KeyFrameT* pKF2, const std::vector<std::pair<size_t, size_t> >& pairs, int device, slamit_triangulate_problem& P,
                           slamit_triangulate_result& R, shim::bool_tag<true>) {
        const size_t n = pairs.size();
        std::vector<float> ur1(n), ur2(n), depth1(n), depth2(n), raw1(2 * n), raw2(2 * n);
        for (size_t k = 0; k < n; ++k) {
            const size_t i1 = pairs[k].first, i2 = pairs[k].second;
            ur1[k] = cur->mvuRight[i1]; depth1[k] = cur->mvDepth[i1];
            ur2[k] = pKF2->mvuRight[i2]; depth2[k] = pKF2->mvDepth[i2];
            raw1[2 * k] = cur->mvKeys[i1].pt.x; raw1[2 * k + 1] = cur->mvKeys[i1].pt.y;      // KeyFrame::UnprojectStereo reads mvKeys
            raw2[2 * k] = pKF2->mvKeys[i2].pt.x; raw2[2 * k + 1] = pKF2->mvKeys[i2].pt.y;
        }
        slamit_triangulate_stereo_rec T;
        T.ur1 = ur1.data(); T.ur2 = ur2.data(); T.depth1 = depth1.data(); T.depth2 = depth2.data(); T.raw1_xy = raw1.data(); T.raw2_xy = raw2.data();
        T.mb1 = cur->mb; T.mb2 = pKF2->mb;
        T.bf = cur->mbf;                                                                       // :430 and :458: the current keyframe's
        return slamit_triangulate_stereo(device, &P, &T, &R, NULL);
    }

    template <class KeyFrameT>
    static bool hasStereo(KeyFrameT* kf) {
        for (size_t i = 0; i < kf->mvuRight.size(); ++i)
            if (kf->mvuRight[i] >= 0) return true;
        return false;
    }
    template <class KeyFrameT>
    static void pose(KeyFrameT* kf, float T[12], float K[6]) {
        const cv::Mat R = kf->GetRotation(), t = kf->GetTranslation();
        shim::load3x3(R, T, 4); shim::load3(t, T + 3, 0, 4);
        K[0] = kf->fx; K[1] = kf->fy; K[2] = kf->cx; K[3] = kf->cy; K[4] = kf->invfx; K[5] = kf->invfy;
    }
};

}  // namespace ORB_SLAM2

#endif
