// Initializer.h — ORB_SLAM2::Initializer (include/Initializer.h, src/Initializer.cc) above the C-ABI, as a template over the
// caller's Frame type like PnPsolver.h.  What the caller's type must offer:
//   FrameT: mvKeysUn (cv::KeyPoint: pt), mK (3x3 CV_32F)
//
// The constructor keeps what the reference's keeps (:38-47): mK, the reference frame's mvKeysUn, sigma, the iteration count.
// Initialize (:49-130) gathers mvMatches12 from vMatches12, seeds once per process (DUtils::Random::SeedRandOnce(0)) and draws the
// mMaxIterations sets of eight without replacement (:91-106) from the RandomInt() hook of shim_common.h, the one PnPsolver draws
// from.  FindHomography and FindFundamental for all sets are ONE slamit_init_hyp_batch call; the strict > scan over the scores, RH
// and, after ONE slamit_init_reconstruct_batch call for the eight or four motions of the kept model, ReconstructH's best /
// second-best rule or ReconstructF's cascade run here through the scan functions of include/slamit.h.  InitializeAll() does both
// launches for a batch of frame pairs at once, in the role EvaluateAll has in PnPsolver.h.
//
// vP3D and vbTriangulated are sized and indexed by frame 1's keypoints, as in the reference; on failure they are left empty, R21 and
// t21 are released.  Fewer than eight matches return false before anything is drawn (the reference's sampler would index an empty
// vector).  Tracking::CreateInitialMapMonocular stays with the caller.
#ifndef SLAMIT_SHIM_INITIALIZER_H
#define SLAMIT_SHIM_INITIALIZER_H

#include <stdint.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#ifdef SLAMIT_USE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

#include "shim_common.h"

namespace ORB_SLAM2 {

// ---- host logic, free of the device and of the caller's types (tests/test_shim_initializer.py drives it on the CPU) ----
namespace initializer {

// DUtils::Random::SeedRandOnce(seed): srand once per process
inline void SeedRandOnce(int seed) {
    static bool seeded = false;
    if (!seeded) { srand(seed); seeded = true; }
}

// One pass of the sampler (:93-105): eight draws without replacement
inline void SampleSet(int N, std::vector<int>& avail, int32_t out[8]) {
    avail.resize(N);
    for (int i = 0; i < N; ++i) avail[i] = i;
    for (size_t j = 0; j < 8; ++j) {
        const int randi = shim::RandomInt()(0, (int)avail.size() - 1);
        out[j] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
    }
}

struct Choice { int kind, best, n_inliers; };   // the model Initialize reconstructs from, its kept hypothesis (-1: no score above 0)

// :121-127 over the scores of one slamit_init_result (the n_hyp homographies first, then the fundamentals)
inline Choice Choose(int n_hyp, const float* score, const int32_t* n_inliers) {
    const int bh = slamit_init_best_hypothesis(n_hyp, score), bf = slamit_init_best_hypothesis(n_hyp, score + n_hyp);
    const float SH = bh >= 0 ? score[bh] : 0.f, SF = bf >= 0 ? score[n_hyp + bf] : 0.f;
    Choice c;
    c.kind = slamit_init_choose_h(SH, SF) ? SLAMIT_INIT_H : SLAMIT_INIT_F;
    c.best = c.kind == SLAMIT_INIT_H ? bh : bf;
    c.n_inliers = c.best >= 0 ? n_inliers[(size_t)c.kind * n_hyp + c.best] : 0;
    return c;
}

// The winning motion of a reconstruct result (-1: rejected), minParallax 1.0 and minTriangulated 50 as Initialize passes them
inline int Winner(int kind, const slamit_init_reconstruct_result& r, int n_inliers, float minParallax = 1.0f, int minTriangulated = 50) {
    if (!r.decomposable) return -1;
    float par[8];
    for (int k = 0; k < r.n_motions; ++k) par[k] = slamit_init_parallax_deg(r.n_good[k], r.cos_sel[k]);
    return kind == SLAMIT_INIT_H ? slamit_init_pick_h(r.n_good, par, n_inliers, minParallax, minTriangulated)
                                 : slamit_init_pick_f(r.n_good, par, n_inliers, minParallax, minTriangulated);
}

}  // namespace initializer

template <class FrameT>
class Initializer {
public:
    struct Tag {};
    static int LastStatus() { return shim::status<Tag>(); }

    // one frame pair of InitializeAll: the outputs are Initialize's
    struct Job {
        Initializer* init;
        const FrameT* CurrentFrame;
        const std::vector<int>* vMatches12;
        cv::Mat R21, t21;
        std::vector<cv::Point3f> vP3D;
        std::vector<bool> vbTriangulated;
        bool ok;
        Job(Initializer* i, const FrameT& F, const std::vector<int>& m) : init(i), CurrentFrame(&F), vMatches12(&m), ok(false) {}
    };

    Initializer(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200, int device = 0) : mDevice(device) {
        shim::load3x3(ReferenceFrame.mK, mK);
        mvKeys1 = ReferenceFrame.mvKeysUn;
        mSigma = sigma;
        mMaxIterations = iterations;
        mKind = -1; mMotion = -1;
    }

    bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated) {
        std::vector<Job> jobs(1, Job(this, CurrentFrame, vMatches12));
        InitializeAll(jobs);
        R21 = jobs[0].R21; t21 = jobs[0].t21;
        vP3D.swap(jobs[0].vP3D); vbTriangulated.swap(jobs[0].vbTriangulated);
        return jobs[0].ok;
    }

    // Every frame pair of `jobs` in two launches.  Returns LastStatus().
    static int InitializeAll(std::vector<Job>& jobs) {
        shim::status<Tag>() = SLAMIT_OK;
        const int device = jobs.empty() ? 0 : jobs[0].init->mDevice;
        std::vector<Job*> live;
        for (size_t j = 0; j < jobs.size(); ++j) {
            jobs[j].ok = false;
            if (jobs[j].init->Gather(*jobs[j].CurrentFrame, *jobs[j].vMatches12)) live.push_back(&jobs[j]);
        }
        if (live.empty()) return SLAMIT_OK;
        const size_t m = live.size();
        std::vector<slamit_init_problem> P(m);
        std::vector<slamit_init_result> R(m);
        for (size_t k = 0; k < m; ++k) {
            Initializer& I = *live[k]->init;
            const size_t nh = (size_t)I.mMaxIterations, words = ((size_t)I.N() + 31) / 32;
            I.mModel.resize(2 * 9 * nh); I.mScore.resize(2 * nh); I.mCount.resize(2 * nh); I.mBits.resize(2 * nh * words);
            slamit_init_problem& p = P[k];
            p.n1 = (int32_t)I.mvKeys1.size(); p.keys1 = I.mXY1.data(); p.n2 = (int32_t)(I.mXY2.size() / 2); p.keys2 = I.mXY2.data();
            p.n = I.N(); p.matches = I.mMatches.data(); p.sigma = I.mSigma; p.n_hyp = I.mMaxIterations; p.sets = I.mSets.data();
            R[k].model = I.mModel.data(); R[k].score = I.mScore.data(); R[k].n_inliers = I.mCount.data(); R[k].inlier_bits = I.mBits.data();
        }
        int rc = slamit_init_hyp_batch(device, (int)m, P.data(), R.data());
        if (rc != SLAMIT_OK) { shim::report<Tag>("slamit_init_hyp_batch", rc); return rc; }
        std::vector<slamit_init_reconstruct_problem> Q(m);
        std::vector<slamit_init_reconstruct_result> S(m);
        std::vector<initializer::Choice> choice(m);
        std::vector<std::vector<uint32_t> > none(m);
        for (size_t k = 0; k < m; ++k) {
            Initializer& I = *live[k]->init;
            const size_t nh = (size_t)I.mMaxIterations, n = (size_t)I.N(), words = (n + 31) / 32;
            const initializer::Choice c = choice[k] = initializer::Choose((int)nh, I.mScore.data(), I.mCount.data());
            const size_t slot = (size_t)c.kind * nh + (c.best >= 0 ? c.best : 0);
            slamit_init_reconstruct_problem& q = Q[k];
            q.n1 = P[k].n1; q.keys1 = P[k].keys1; q.n2 = P[k].n2; q.keys2 = P[k].keys2; q.n = P[k].n; q.matches = P[k].matches; q.sigma = I.mSigma;
            q.kind = c.kind;
            for (int i = 0; i < 9; ++i) { q.model[i] = c.best >= 0 ? I.mModel[9 * slot + i] : 0.f; q.K[i] = I.mK[i]; }
            none[k].assign(words, 0u);   // no score above 0: no model was kept and no match is an inlier
            q.subset_bits = c.best >= 0 ? &I.mBits[slot * words] : none[k].data();
            I.mStatus.resize(8 * n); I.mPoints.resize(3 * 8 * n); I.mGood.resize(8 * words);
            S[k].status = I.mStatus.data(); S[k].points = I.mPoints.data(); S[k].good_bits = I.mGood.data();
        }
        rc = slamit_init_reconstruct_batch(device, (int)m, Q.data(), S.data());
        if (rc != SLAMIT_OK) { shim::report<Tag>("slamit_init_reconstruct_batch", rc); return rc; }
        for (size_t k = 0; k < m; ++k) {
            Job& J = *live[k];
            Initializer& I = *J.init;
            const size_t n = (size_t)I.N(), words = (n + 31) / 32;
            I.mKind = choice[k].kind;
            const int mo = I.mMotion = initializer::Winner(choice[k].kind, S[k], choice[k].n_inliers);
            if (mo < 0) continue;
            J.ok = true;
            J.R21.create(3, 3, CV_32F); J.t21.create(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) J.R21.template at<float>(r, c) = S[k].R[9 * mo + 3 * r + c];
                J.t21.template at<float>(r, 0) = S[k].t[3 * mo + r];
            }
            J.vP3D.assign(I.mvKeys1.size(), cv::Point3f()); J.vbTriangulated.assign(I.mvKeys1.size(), false);
            for (size_t i = 0; i < n; ++i) {
                const size_t at = (size_t)mo * n + i, i1 = (size_t)I.mMatches[2 * i];
                if (I.mStatus[at] == 0) J.vP3D[i1] = cv::Point3f(I.mPoints[3 * at], I.mPoints[3 * at + 1], I.mPoints[3 * at + 2]);
                if ((I.mGood[(size_t)mo * words + (i >> 5)] >> (i & 31)) & 1u) J.vbTriangulated[i1] = true;
            }
        }
        return SLAMIT_OK;
    }

    int N() const { return (int)(mMatches.size() / 2); }
    int Kind() const { return mKind; }       // SLAMIT_INIT_H / SLAMIT_INIT_F of the last Initialize, -1 before
    int Motion() const { return mMotion; }   // its winning motion, -1 = rejected
    const std::vector<int32_t>& Sets() const { return mSets; }

private:
    // :56-106: the matches, the flat keypoint tables and the sets.  false = fewer than eight matches.
    bool Gather(const FrameT& CurrentFrame, const std::vector<int>& vMatches12) {
        mKind = -1; mMotion = -1;
        mMatches.clear();
        for (size_t i = 0, iend = vMatches12.size(); i < iend && i < mvKeys1.size(); i++)
            if (vMatches12[i] >= 0) { mMatches.push_back((int32_t)i); mMatches.push_back(vMatches12[i]); }
        const int n = N();
        if (n < 8) return false;
        mXY1.resize(2 * mvKeys1.size());
        for (size_t i = 0; i < mvKeys1.size(); ++i) { mXY1[2 * i] = mvKeys1[i].pt.x; mXY1[2 * i + 1] = mvKeys1[i].pt.y; }
        mXY2.resize(2 * CurrentFrame.mvKeysUn.size());
        for (size_t i = 0; i < CurrentFrame.mvKeysUn.size(); ++i) { mXY2[2 * i] = CurrentFrame.mvKeysUn[i].pt.x; mXY2[2 * i + 1] = CurrentFrame.mvKeysUn[i].pt.y; }
        initializer::SeedRandOnce(0);
        mSets.resize(8 * (size_t)mMaxIterations);
        std::vector<int> avail;
        for (int it = 0; it < mMaxIterations; it++) initializer::SampleSet(n, avail, &mSets[8 * (size_t)it]);
        return true;
    }

    int mDevice;
    float mK[9];
    std::vector<cv::KeyPoint> mvKeys1;
    float mSigma;
    int mMaxIterations, mKind, mMotion;
    std::vector<float> mXY1, mXY2;
    std::vector<int32_t> mMatches, mSets;
    std::vector<float> mModel, mScore, mPoints;
    std::vector<int32_t> mCount;
    std::vector<uint32_t> mBits, mGood;
    std::vector<uint8_t> mStatus;
};

}  // namespace ORB_SLAM2

#endif
