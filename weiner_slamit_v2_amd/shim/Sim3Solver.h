// Sim3Solver.h — ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) above the C-ABI, as a template over the
// caller's KeyFrame / MapPoint types like ORBmatcher.h.  What the caller's types must offer:
//   KeyFrameT: GetMapPointMatches(), GetRotation(), GetTranslation() (CV_32F), mvKeysUn, mvLevelSigma2, mK (3x3 CV_32F)
//   MapPointT: isBad(), GetIndexInKeyFrame(KeyFrameT*), GetWorldPos() (3x1 CV_32F)
//
// The constructor gathers what the reference's gathers (:37-112).  SetRansacParameters (:114-138) keeps the float epsilon, the
// ceil(log / log), the mRansacMinInliers == N case and the clamp, and then DRAWS ALL mRansacMaxIts TRIPLES with the reference's
// sampler (:163-177, including its quirk: it overwrites vAvailableIndices[idx], indexed by the value drawn, so an index can come
// twice in a triple).  The first iterate() sends them to the device in one slamit_sim3_ransac_batch call; iterate()'s
// acceptance rule (:183-204) is a sequential scan and runs here over the device's counts, so later iterate(5) calls only scan.
// EvaluateAll() puts the solvers of every loop candidate into one call: LoopClosing::ComputeSim3 then costs one launch.
// The process RNG is therefore used in another order than in the reference (all draws of a solver at once instead of
// interleaved with the other candidates'); the reference is not reproducible there either, rand() being shared across threads.
#ifndef SLAMIT_SHIM_SIM3SOLVER_H
#define SLAMIT_SHIM_SIM3SOLVER_H

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

// ---- host logic, free of the device and of the caller's types (tests/test_shim_sim3solver.py drives it on the CPU) ----
namespace sim3solver {

// DUtils::Random::RandomInt(min, max) over rand(); Sim3SolverRandomInt() lets a caller (or a test) put its own source in
inline int DefaultRandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}
typedef int (*RandomIntFn)(int, int);
inline RandomIntFn& RandomInt() { static RandomIntFn fn = DefaultRandomInt; return fn; }

// mRansacMaxIts after SetRansacParameters (:120-135)
inline int RansacIterations(int N, double probability, int minInliers, int maxIterations) {
    float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N) {
        nIterations = 1;
    } else {
        const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        // (int) of a NaN or of a double outside int is INT_MIN on x86-64 (N < minInliers gives log of a negative number)
        nIterations = (v == v && v > -2147483649.0 && v < 2147483648.0) ? (int)v : std::numeric_limits<int>::min();
    }
    return std::max(1, std::min(nIterations, maxIterations));
}

// One pass of the sampler (:163-177).  `avail` plays vAvailableIndices: pop_back() lowers the size and keeps the storage, so the
// store at [idx] -- idx is the VALUE drawn, not the position randi -- may land in an already popped slot; nothing reads it again.
inline void SampleTriple(int N, std::vector<int>& avail, int out[3]) {
    avail.resize(N);
    for (int i = 0; i < N; ++i) avail[i] = i;
    int size = N;
    for (short i = 0; i < 3; ++i) {
        const int randi = RandomInt()(0, size - 1);
        const int idx = avail[randi];
        out[i] = idx;
        avail[idx] = avail[size - 1];
        --size;
    }
}

struct ScanState {
    int mnIterations, mnBestInliers, best;   // best: the hypothesis that holds mBestT12, -1 before the first update
    ScanState() : mnIterations(0), mnBestInliers(0), best(-1) {}
};

// The loop of iterate() (:158-204) over counts[h] = mnInliersi of hypothesis h: the accepted hypothesis or -1
inline int Scan(const int32_t* counts, int nIterations, int mRansacMaxIts, int mRansacMinInliers, ScanState& st, bool& bNoMore) {
    bNoMore = false;
    int nCurrentIterations = 0;
    while (st.mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
        nCurrentIterations++;
        const int h = st.mnIterations++;
        if (counts[h] >= st.mnBestInliers) {
            st.mnBestInliers = counts[h];
            st.best = h;
            if (counts[h] > mRansacMinInliers) return h;
        }
    }
    if (st.mnIterations >= mRansacMaxIts) bNoMore = true;
    return -1;
}

inline float GemmRow3(const float r0, const float r1, const float r2, const float X, const float Y, const float Z, const float t) {
    const float t0 = r0 * X + r1 * Y + r2 * Z;   // Rcw * X3Dw + tcw as ORBmatcher.h states cv::gemm on CV_32F
    return (float)((double)t0 + (double)t);
}

}  // namespace sim3solver

template <class KeyFrameT, class MapPointT>
class Sim3Solver {
public:
    Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true, int device = 0)
        : mbFixScale(bFixScale), mDevice(device), mbEvaluated(false), mnAccepted(-1) {
        std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPointT* pMP1 = vpKeyFrameMP1[i1];
            MapPointT* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
            const float sigmaSquare2 = pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave];
            // mvnMaxError1/2 are vector<size_t>: the bound is truncated before it meets the float error
            mvMaxError1.push_back((float)(size_t)(9.210 * sigmaSquare1));
            mvMaxError2.push_back((float)(size_t)(9.210 * sigmaSquare2));
            mvnIndices1.push_back(i1);
            Push(mvX3Dc1, Rcw1, tcw1, pMP1->GetWorldPos());
            Push(mvX3Dc2, Rcw2, tcw2, pMP2->GetWorldPos());
        }
        Intrinsics(pKF1->mK, mK1);
        Intrinsics(pKF2->mK, mK2);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        N = (int)mvnIndices1.size();
        mRansacMaxIts = sim3solver::RansacIterations(N, probability, minInliers, maxIterations);
        mScan = sim3solver::ScanState();
        mbEvaluated = false;
        mnAccepted = -1;
        mvTriples.clear();
        if (N < mRansacMinInliers || N < 3) return;   // iterate() returns at once; nothing to draw
        const int nhyp = std::min(mRansacMaxIts, (int)SLAMIT_SIM3_RANSAC_MAX_HYP);
        std::vector<int> avail;
        mvTriples.resize(3 * (size_t)nhyp);
        for (int h = 0; h < nhyp; ++h) {
            int tri[3];
            sim3solver::SampleTriple(N, avail, tri);
            for (int k = 0; k < 3; ++k) mvTriples[3 * h + k] = tri[k];
        }
    }

    // every solver that has not been evaluated yet, in one device call; SLAMIT_OK or the call's error (also in LastStatus())
    static int EvaluateAll(std::vector<Sim3Solver*>& vpSolvers) {
        std::vector<slamit_sim3_ransac_problem> P;
        std::vector<slamit_sim3_ransac_result> R;
        std::vector<Sim3Solver*> todo;
        int device = 0;
        for (size_t k = 0; k < vpSolvers.size(); ++k) {
            Sim3Solver* s = vpSolvers[k];
            if (!s || s->mbEvaluated || s->mvTriples.empty()) continue;
            const int nhyp = (int)(s->mvTriples.size() / 3);
            s->mvT12.assign(13 * (size_t)nhyp, 0.f);
            s->mvCounts.assign(nhyp, 0);
            s->mvBits.assign((size_t)nhyp * ((s->N + 31) / 32), 0u);
            slamit_sim3_ransac_problem p;
            p.n = s->N; p.x1 = s->mvX3Dc1.data(); p.x2 = s->mvX3Dc2.data(); p.max_err1 = s->mvMaxError1.data(); p.max_err2 = s->mvMaxError2.data();
            for (int i = 0; i < 4; ++i) { p.intr1[i] = s->mK1[i]; p.intr2[i] = s->mK2[i]; }
            p.fix_scale = s->mbFixScale ? 1 : 0; p.n_hyp = nhyp; p.triples = s->mvTriples.data();
            slamit_sim3_ransac_result r;
            r.t12 = s->mvT12.data(); r.n_inliers = s->mvCounts.data(); r.inlier_bits = s->mvBits.data();
            P.push_back(p); R.push_back(r); todo.push_back(s);
            device = s->mDevice;
        }
        if (todo.empty()) return lastStatus() = SLAMIT_OK;
        const int rc = slamit_sim3_ransac_batch(device, (int)P.size(), P.data(), R.data());
        if (rc == SLAMIT_OK) for (size_t k = 0; k < todo.size(); ++k) todo[k]->mbEvaluated = true;
        return lastStatus() = rc;
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers || N < 3) { bNoMore = true; return cv::Mat(); }
        if (!mbEvaluated) {
            std::vector<Sim3Solver*> me(1, this);
            if (EvaluateAll(me) != SLAMIT_OK) { bNoMore = true; return cv::Mat(); }   // the error is in LastStatus() / slamit_last_error()
        }
        const int maxIts = std::min(mRansacMaxIts, (int)mvCounts.size());
        const int h = sim3solver::Scan(mvCounts.data(), nIterations, maxIts, mRansacMinInliers, mScan, bNoMore);
        if (h < 0) return cv::Mat();
        mnAccepted = h;
        nInliers = mvCounts[h];
        const uint32_t* bits = &mvBits[(size_t)h * ((N + 31) / 32)];
        for (int i = 0; i < N; i++)
            if ((bits[i >> 5] >> (i & 31)) & 1u) vbInliers[mvnIndices1[i]] = true;
        return T12(h);
    }

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    cv::Mat GetEstimatedRotation() {
        cv::Mat R(3, 3, CV_32F);
        for (int i = 0; i < 9; ++i) R.at<float>(i / 3, i % 3) = mScan.best < 0 ? 0.f : mvT12[13 * (size_t)mScan.best + i];
        return R;
    }
    cv::Mat GetEstimatedTranslation() {
        cv::Mat t(3, 1, CV_32F);
        for (int i = 0; i < 3; ++i) t.at<float>(i, 0) = mScan.best < 0 ? 0.f : mvT12[13 * (size_t)mScan.best + 9 + i];
        return t;
    }
    float GetEstimatedScale() { return mScan.best < 0 ? 0.f : mvT12[13 * (size_t)mScan.best + 12]; }

    // beyond the reference's surface
    static int LastStatus() { return lastStatus(); }
    int AcceptedHypothesis() const { return mnAccepted; }   // index of the hypothesis iterate() returned, -1 if none yet
    int GetRansacMaxIts() const { return mRansacMaxIts; }

private:
    static int& lastStatus() { return shim::status<Sim3Solver>(); }
    static void Push(std::vector<float>& v, const cv::Mat& R, const cv::Mat& t, const cv::Mat& X) {
        const float x = X.at<float>(0, 0), y = X.at<float>(1, 0), z = X.at<float>(2, 0);
        for (int r = 0; r < 3; ++r) v.push_back(sim3solver::GemmRow3(R.at<float>(r, 0), R.at<float>(r, 1), R.at<float>(r, 2), x, y, z, t.at<float>(r, 0)));
    }
    static void Intrinsics(const cv::Mat& K, float out[4]) {
        out[0] = K.at<float>(0, 0); out[1] = K.at<float>(1, 1); out[2] = K.at<float>(0, 2); out[3] = K.at<float>(1, 2);
    }
    cv::Mat T12(int h) const {   // mT12i: [s R | t; 0 0 0 1]
        cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
        const float* v = &mvT12[13 * (size_t)h];
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T.at<float>(r, c) = v[12] * v[3 * r + c]; T.at<float>(r, 3) = v[9 + r]; }
        T.at<float>(3, 3) = 1.f;
        return T;
    }

    std::vector<float> mvX3Dc1, mvX3Dc2, mvMaxError1, mvMaxError2;
    std::vector<int> mvnIndices1;
    float mK1[4], mK2[4];
    int N, mN1;
    bool mbFixScale;
    int mDevice;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    std::vector<int32_t> mvTriples, mvCounts;
    std::vector<float> mvT12;
    std::vector<uint32_t> mvBits;
    bool mbEvaluated;
    int mnAccepted;
    sim3solver::ScanState mScan;
};

}  // namespace ORB_SLAM2

#endif
