// PnPsolver.h — ORB_SLAM2::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) above the C-ABI, as a template over the caller's
// Frame / MapPoint types like Sim3Solver.h.  What the caller's types must offer:
//   FrameT:    mvKeysUn (cv::KeyPoint: pt, octave), mvLevelSigma2, fx, fy, cx, cy
//   MapPointT: isBad(), GetWorldPos() (3x1 CV_32F)
//
// The constructor gathers what the reference's gathers (:67-118).  SetRansacParameters (:129-165) keeps the truncated float product
// N * epsilon, the two clamps, the epsilon update in float, pow(epsilon, 3) (3 although the set is 4), the mRansacMinInliers == N case
// and the final clamp, and then DRAWS ALL mRansacMaxIts QUADRUPLES with the reference's sampler (:196-209, including its quirk: it
// overwrites vAvailableIndices[idx], indexed by the value drawn, so an index can come twice in a quadruple).  The call the
// constructor makes for the default parameters draws nothing: Tracking sets its own parameters right after it.  minSet other than 4
// is refused with SLAMIT_ERR_ARG (the device solves four-point sets only); the solver then returns bNoMore at once.
//
// The first iterate() sends the quadruples to the device in one slamit_pnp_ransac_batch call.  The hypotheses iterate() can record
// as best (:217-232) are the strict prefix maxima among the counts >= mRansacMinInliers, known from the counts alone, and Refine()
// (:268-313) on an unchanged best is the same computation with the same failing answer: so the inliers of every such record go to
// one slamit_pnp_refine_batch call, and iterate()'s loop -- with its `||` condition, by which the first iterate(5) runs to
// mRansacMaxIts unless it accepts earlier, and its bNoMore tail that returns the unrefined best pose -- is a scan over both result
// sets that runs here.  EvaluateAll() does both launches for every candidate keyframe at once: Tracking::Relocalization then costs
// two launches for all its solvers.  A call to iterate() after bNoMore draws and evaluates its nIterations further hypotheses in
// calls of their own; Tracking never does, because bNoMore discards the candidate.
// The process RNG is therefore used in another order than in the reference (all draws of a solver at once instead of
// interleaved with the other candidates'); the reference is not reproducible there either, rand() being shared across threads.
#ifndef SLAMIT_SHIM_PNPSOLVER_H
#define SLAMIT_SHIM_PNPSOLVER_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <vector>

#ifdef SLAMIT_USE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

#include "shim_common.h"

namespace ORB_SLAM2 {

// ---- host logic, free of the device and of the caller's types (tests/test_shim_pnpsolver.py drives it on the CPU) ----
namespace pnpsolver {

// DUtils::Random::RandomInt(min, max) over rand(); RandomInt() lets a caller (or a test) put its own source in (shim_common.h:
// the Initializer draws from the same hook)
using shim::DefaultRandomInt;
using shim::RandomIntFn;
using shim::RandomInt;

struct Params { int minInliers, maxIts; float epsilon; };

// mRansacMinInliers, mRansacMaxIts and mRansacEpsilon after SetRansacParameters (:137-160)
inline Params RansacParameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon) {
    Params P;
    float mRansacEpsilon = epsilon;
    const float prod = N * mRansacEpsilon;
    int nMinInliers = (prod == prod && prod > -2147483649.0f && prod < 2147483648.0f) ? (int)prod : std::numeric_limits<int>::min();
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    if (mRansacEpsilon < (float)nMinInliers / N) mRansacEpsilon = (float)nMinInliers / N;
    int nIterations;
    if (nMinInliers == N) {
        nIterations = 1;
    } else {
        const double v = ceil(log(1 - probability) / log(1 - pow(mRansacEpsilon, 3)));
        // (int) of a NaN or of a double outside int is INT_MIN on x86-64 (N < minInliers gives log of a negative number)
        nIterations = (v == v && v > -2147483649.0 && v < 2147483648.0) ? (int)v : std::numeric_limits<int>::min();
    }
    P.minInliers = nMinInliers;
    P.maxIts = std::max(1, std::min(nIterations, maxIterations));
    P.epsilon = mRansacEpsilon;
    return P;
}

// One pass of the sampler (:196-209).  `avail` plays vAvailableIndices: pop_back() lowers the size and keeps the storage, so the
// store at [idx] -- idx is the VALUE drawn, not the position randi -- may land in an already popped slot; nothing reads it again.
inline void SampleQuad(int N, std::vector<int>& avail, int out[4]) {
    avail.resize(N);
    for (int i = 0; i < N; ++i) avail[i] = i;
    int size = N;
    for (short i = 0; i < 4; ++i) {
        const int randi = RandomInt()(0, size - 1);
        const int idx = avail[randi];
        out[i] = idx;
        avail[idx] = avail[size - 1];
        --size;
    }
}

// The hypotheses of counts[first, count) that iterate() records as best: the strict prefix maxima among counts >= minInliers
inline std::vector<int> Records(const int32_t* counts, int first, int count, int minInliers, int best) {
    std::vector<int> out;
    for (int h = first; h < count; ++h)
        if (counts[h] >= minInliers && counts[h] > best) { best = counts[h]; out.push_back(h); }
    return out;
}

struct ScanState {
    int mnIterations, mnBestInliers, best;   // best: the hypothesis that holds mBestTcw, -1 before the first record
    ScanState() : mnIterations(0), mnBestInliers(0), best(-1) {}
};

enum { SCAN_NONE = 0, SCAN_REFINED = 1, SCAN_BEST = 2 };

// The loop of iterate() (:190-263) over counts[h] = mnInliersi of hypothesis h and refined[h] = mnRefinedInliers of Refine() on the
// inliers of h (read for recorded h only).  SCAN_REFINED: Refine() of st.best was accepted; SCAN_BEST: the bNoMore tail returns the
// unrefined pose of st.best; SCAN_NONE: an empty matrix.  counts must hold mnIterations + max(maxIts - mnIterations, nIterations).
inline int Scan(const int32_t* counts, const int32_t* refined, int nIterations, int mRansacMaxIts, int mRansacMinInliers, ScanState& st, bool& bNoMore) {
    bNoMore = false;
    int nCurrentIterations = 0;
    while (st.mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
        nCurrentIterations++;
        const int h = st.mnIterations++;
        if (counts[h] >= mRansacMinInliers) {
            if (counts[h] > st.mnBestInliers) {
                st.mnBestInliers = counts[h];
                st.best = h;
            }
            if (refined[st.best] > mRansacMinInliers) return SCAN_REFINED;
        }
    }
    if (st.mnIterations >= mRansacMaxIts) {
        bNoMore = true;
        if (st.mnBestInliers >= mRansacMinInliers) return SCAN_BEST;
    }
    return SCAN_NONE;
}

// hypotheses iterate(nIterations) walks through if it accepts none
inline int ScanNeeds(const ScanState& st, int nIterations, int mRansacMaxIts) { return st.mnIterations + std::max(mRansacMaxIts - st.mnIterations, nIterations); }

}  // namespace pnpsolver

template <class FrameT, class MapPointT>
class PnPsolver {
public:
    PnPsolver(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches, int device = 0) : mDevice(device), mnMatches((int)vpMapPointMatches.size()) {
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPointT* pMP = vpMapPointMatches[i];
            if (!pMP) continue;
            if (pMP->isBad()) continue;
            const cv::KeyPoint& kp = F.mvKeysUn[i];
            mvP2D.push_back(kp.pt.x); mvP2D.push_back(kp.pt.y);
            mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
            cv::Mat Pos = pMP->GetWorldPos();
            for (int r = 0; r < 3; ++r) mvP3Dw.push_back(Pos.at<float>(r, 0));
            mvKeyPointIndices.push_back((int)i);
        }
        mIntr[0] = F.fx; mIntr[1] = F.fy; mIntr[2] = F.cx; mIntr[3] = F.cy;   // doubles holding the frame's floats
        Set(0.99, 8, 300, 4, 0.4f, 5.991f, false);
    }

    // SLAMIT_OK, or SLAMIT_ERR_ARG for a minSet other than 4 (also in LastStatus()); the reference returns void
    int SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991) {
        return Set(probability, minInliers, maxIterations, minSet, epsilon, th2, true);
    }

    // What the next iterate() of every solver can need, in two device calls: the hypotheses drawn and not yet evaluated, then Refine()
    // of every hypothesis those scans can record as best.  SLAMIT_OK or the failing call's error (also in LastStatus()).
    static int EvaluateAll(std::vector<PnPsolver*>& vpSolvers) {
        std::vector<PnPsolver*> todo;
        int device = 0;
        for (size_t k = 0; k < vpSolvers.size(); ++k) {
            PnPsolver* s = vpSolvers[k];
            if (!s || s->mbRefused || s->N < s->mRansacMinInliers) continue;
            if ((int)s->mvQuads.size() / 4 < s->mRansacMaxIts) s->Draw(s->mRansacMaxIts);
            todo.push_back(s);
            device = s->mDevice;
        }
        // hypotheses, SLAMIT_PNP_MAX_HYP per problem and call
        for (;;) {
            std::vector<slamit_pnp_problem> P;
            std::vector<slamit_pnp_result> R;
            std::vector<PnPsolver*> who;
            std::vector<int> cnt;
            for (size_t k = 0; k < todo.size(); ++k) {
                PnPsolver* s = todo[k];
                const int have = (int)s->mvCounts.size(), want = (int)s->mvQuads.size() / 4;
                if (have >= want) continue;
                const int m = std::min(want - have, (int)SLAMIT_PNP_MAX_HYP), w = (s->N + 31) / 32;
                s->mvPose.resize(12 * (size_t)(have + m)); s->mvCounts.resize(have + m); s->mvBits.resize((size_t)(have + m) * w);
                s->mvRefinedCount.resize(have + m, -1); s->mvRefinedSlot.resize(have + m, -1);
                who.push_back(s); cnt.push_back(m);
            }
            if (who.empty()) break;
            for (size_t k = 0; k < who.size(); ++k) {   // pointers after every resize
                PnPsolver* s = who[k];
                const int have = (int)s->mvCounts.size() - cnt[k], w = (s->N + 31) / 32;
                slamit_pnp_problem p;
                s->Fill(p);
                p.n_hyp = cnt[k]; p.quads = &s->mvQuads[4 * (size_t)have];
                slamit_pnp_result r;
                r.pose = &s->mvPose[12 * (size_t)have]; r.n_inliers = &s->mvCounts[have]; r.inlier_bits = &s->mvBits[(size_t)have * w];
                P.push_back(p); R.push_back(r);
            }
            const int rc = slamit_pnp_ransac_batch(device, (int)P.size(), P.data(), R.data());
            if (rc != SLAMIT_OK) {
                for (size_t k = 0; k < who.size(); ++k) who[k]->Shrink((int)who[k]->mvCounts.size() - cnt[k]);
                return lastStatus() = rc;
            }
        }
        // Refine() of every record ahead of the scans
        std::vector<slamit_pnp_refine_problem> P;
        std::vector<slamit_pnp_refine_result> R;
        std::vector<std::pair<PnPsolver*, int> > jobs;
        for (size_t k = 0; k < todo.size(); ++k) {
            PnPsolver* s = todo[k];
            const int w = (s->N + 31) / 32;
            const std::vector<int> rec = pnpsolver::Records(s->mvCounts.data(), s->mScan.mnIterations, (int)s->mvCounts.size(), s->mRansacMinInliers, s->mScan.mnBestInliers);
            for (size_t j = 0; j < rec.size(); ++j) {
                if (s->mvRefinedSlot[rec[j]] >= 0) continue;
                s->mvRefinedSlot[rec[j]] = (int)(s->mvRefinedPose.size() / 12);
                s->mvRefinedPose.resize(s->mvRefinedPose.size() + 12);
                s->mvRefinedBits.resize(s->mvRefinedBits.size() + w);
                jobs.push_back(std::make_pair(s, rec[j]));
            }
        }
        if (jobs.empty()) return lastStatus() = SLAMIT_OK;
        for (size_t j = 0; j < jobs.size(); ++j) {
            PnPsolver* s = jobs[j].first;
            const int h = jobs[j].second, w = (s->N + 31) / 32;
            slamit_pnp_problem q;
            s->Fill(q);
            slamit_pnp_refine_problem p;
            p.n = q.n; p.p3d = q.p3d; p.p2d = q.p2d; p.max_err = q.max_err;
            for (int i = 0; i < 4; ++i) p.intr[i] = q.intr[i];
            p.subset_bits = &s->mvBits[(size_t)h * w];
            slamit_pnp_refine_result r;
            r.n_inliers = 0; r.inlier_bits = &s->mvRefinedBits[(size_t)s->mvRefinedSlot[h] * w];
            P.push_back(p); R.push_back(r);
        }
        const int rc = slamit_pnp_refine_batch(device, (int)P.size(), P.data(), R.data());
        for (size_t j = 0; j < jobs.size(); ++j) {
            PnPsolver* s = jobs[j].first;
            const int h = jobs[j].second;
            if (rc != SLAMIT_OK) { s->mvRefinedSlot[h] = -1; continue; }   // (the slots' storage stays; a later call takes new ones)
            s->mvRefinedCount[h] = R[j].n_inliers;
            for (int i = 0; i < 12; ++i) s->mvRefinedPose[12 * (size_t)s->mvRefinedSlot[h] + i] = R[j].pose[i];
        }
        return lastStatus() = rc;
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (mbRefused || N < mRansacMinInliers) { bNoMore = true; return cv::Mat(); }
        const int need = pnpsolver::ScanNeeds(mScan, nIterations, mRansacMaxIts);
        if (need > (int)mvQuads.size() / 4) Draw(need);
        std::vector<PnPsolver*> me(1, this);
        if (EvaluateAll(me) != SLAMIT_OK) { bNoMore = true; return cv::Mat(); }   // the error is in LastStatus() / slamit_last_error()
        const int what = pnpsolver::Scan(mvCounts.data(), mvRefinedCount.data(), nIterations, mRansacMaxIts, mRansacMinInliers, mScan, bNoMore);
        if (what == pnpsolver::SCAN_NONE) return cv::Mat();
        const int h = mScan.best, w = (N + 31) / 32;
        mnAccepted = h;
        const uint32_t* bits = what == pnpsolver::SCAN_REFINED ? &mvRefinedBits[(size_t)mvRefinedSlot[h] * w] : &mvBits[(size_t)h * w];
        const double* pose = what == pnpsolver::SCAN_REFINED ? &mvRefinedPose[12 * (size_t)mvRefinedSlot[h]] : &mvPose[12 * (size_t)h];
        nInliers = what == pnpsolver::SCAN_REFINED ? mvRefinedCount[h] : mScan.mnBestInliers;
        vbInliers = std::vector<bool>(mnMatches, false);
        for (int i = 0; i < N; i++)
            if ((bits[i >> 5] >> (i & 31)) & 1u) vbInliers[mvKeyPointIndices[i]] = true;
        cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);   // eye(4, 4), rows 0..2 from the double pose converted to CV_32F (:225-231, :302-308)
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)pose[3 * r + c];
            T.at<float>(r, 3) = (float)pose[9 + r];
        }
        T.at<float>(3, 3) = 1.f;
        return T;
    }

    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    // beyond the reference's surface
    static int LastStatus() { return lastStatus(); }
    int AcceptedHypothesis() const { return mnAccepted; }   // the hypothesis whose refined or own pose iterate() returned, -1 if none yet
    int GetRansacMaxIts() const { return mRansacMaxIts; }
    int GetRansacMinInliers() const { return mRansacMinInliers; }

private:
    static int& lastStatus() { return shim::status<PnPsolver>(); }
    int Set(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2, bool draw) {
        N = (int)mvSigma2.size();
        mbRefused = minSet != 4;
        const pnpsolver::Params P = pnpsolver::RansacParameters(N, probability, minInliers, maxIterations, mbRefused ? 4 : minSet, epsilon);
        mRansacProb = probability; mRansacMinInliers = P.minInliers; mRansacMaxIts = P.maxIts; mRansacEpsilon = P.epsilon;
        mvMaxError.resize(N);
        for (int i = 0; i < N; ++i) mvMaxError[i] = mvSigma2[i] * th2;
        mScan = pnpsolver::ScanState();
        mnAccepted = -1;
        mvQuads.clear();
        Shrink(0);
        mvRefinedPose.clear(); mvRefinedBits.clear();
        if (mbRefused) {
            shim::refuse<PnPsolver>("PnPsolver::SetRansacParameters: minSet must be 4, the device solves four-point sets only");
            return SLAMIT_ERR_ARG;
        }
        if (draw && N >= mRansacMinInliers) Draw(mRansacMaxIts);
        return lastStatus() = SLAMIT_OK;
    }
    void Draw(int upto) {
        std::vector<int> avail;
        for (int h = (int)mvQuads.size() / 4; h < upto; ++h) {
            int q[4];
            pnpsolver::SampleQuad(N, avail, q);
            for (int k = 0; k < 4; ++k) mvQuads.push_back(q[k]);
        }
    }
    void Shrink(int nhyp) {
        mvPose.resize(12 * (size_t)nhyp); mvCounts.resize(nhyp); mvBits.resize((size_t)nhyp * ((N + 31) / 32));
        mvRefinedCount.resize(nhyp); mvRefinedSlot.resize(nhyp);
    }
    void Fill(slamit_pnp_problem& p) const {
        p.n = N; p.p3d = mvP3Dw.data(); p.p2d = mvP2D.data(); p.max_err = mvMaxError.data();
        for (int i = 0; i < 4; ++i) p.intr[i] = mIntr[i];
        p.n_hyp = 0; p.quads = 0;
    }

    std::vector<float> mvP2D, mvP3Dw, mvSigma2, mvMaxError;
    std::vector<int> mvKeyPointIndices;
    double mIntr[4];
    int N, mDevice, mnMatches;
    bool mbRefused;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    float mRansacEpsilon;
    std::vector<int32_t> mvQuads, mvCounts, mvRefinedCount, mvRefinedSlot;
    std::vector<double> mvPose, mvRefinedPose;
    std::vector<uint32_t> mvBits, mvRefinedBits;
    int mnAccepted;
    pnpsolver::ScanState mScan;
};

}  // namespace ORB_SLAM2

#endif
