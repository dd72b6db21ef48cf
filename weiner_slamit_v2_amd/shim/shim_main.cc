// shim_main.cc — exercises the three class surfaces the way the reference's callers do, with
// mock KeyFrame / MapPoint / Map types standing in for the reference's data model (which is out
// of scope and is not copied).  Driven by tests/test_shim.py:
//     shim_test orb   <in.raw> <w> <h> <out.bin>
//     shim_test match <descA.bin> <nA> <descB.bin> <nB> <out.bin>
//     shim_test ba    <problem.bin> <out.bin>
//     shim_test pose  <problem.bin> <out.bin>
//     shim_test search <problem.bin> <out.bin>
//     shim_test frame <problem.bin> <out.bin>
//     shim_test fuse <problem.bin> <out.bin>
//     shim_test init <problem.bin> <out.bin>
//     shim_test bow <problem.bin> <out.bin>
//     shim_test sim3 <problem.bin> <out.bin>
//     shim_test osim3 <problem.bin> <out.bin>
//     shim_test essential <problem.bin> <out.bin>
//     shim_test sim3solver <problem.bin> <out.bin>
//     shim_test pnpsolver <problem.bin> <out.bin>
//     shim_test initializer <pairs.bin> <out.bin>
//     shim_test triangulate <problem.bin> <out.bin>
//     shim_test triangulate_stereo <problem.bin> <out.bin>
//     shim_test frustum <problem.bin> <out.bin>
//     shim_test stereo <pair.bin> <out.bin>
//     shim_test unproject <problem.bin> <out.bin>
//     shim_test local_map <seed> <keyframes> <points> <keypoints>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "Optimizer.h"
#include "FrameOps.h"
#include "PnPsolver.h"
#include "Initializer.h"
#include "Sim3Solver.h"
#include "ORBVocabulary.h"
#include "KeyFrameDatabase.h"
#include "LocalMapping.h"
#include "Tracking.h"
#include "../csrc/frustum.h"   // fru_predict_scale for the mocks

using namespace ORB_SLAM2;

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(n);
    if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
    fclose(f);
    return v;
}

// ---- mock data model: just the members Optimizer.h documents --------------------------------
// The projection drivers' commands (search 1 / 2, fuse, fuse_targets, sim3) take a trailing "host" or "device": the matcher is then
// built without or with deviceProjection, the blob's maxd / mind are the RAW mfMaxDistance / mfMinDistance, and the mocks' PredictScale is
// the real formula (MapPoint.cc:391-400) over csrc/frustum.h's fru_logf, so both paths must agree exactly.  Without it the mocks return
// the blob's stored level and its distances are the invariance bounds, as before.
static bool g_real_scale = false, g_device_projection = false;
static void projection_mode(int argc, char** argv, int at) {
    g_real_scale = argc > at;
    g_device_projection = argc > at && std::string(argv[at]) == "device";
}
static int mock_predict_scale(int stored, float rawMax, float dist, float logScaleFactor) {
    if (!g_real_scale) return stored;
    int level;
    fru_predict_scale(rawMax, dist, logScaleFactor, level);
    return level;
}

struct MockKeyFrame;
struct MockMapPoint {
    long unsigned int mnId, mnBALocalForKF;
    cv::Mat pos;
    std::map<MockKeyFrame*, size_t> obs;
    bool bad;
    int normalUpdates;
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF;
    MockMapPoint() : mnId(0), mnBALocalForKF(~0ul), bad(false), normalUpdates(0), mnBAGlobalForKF(0) {}
    bool isBad() { return bad; }
    std::map<MockKeyFrame*, size_t> GetObservations() { return obs; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    void SetWorldPos(const cv::Mat& p) { pos = p.clone(); }
    void UpdateNormalAndDepth() { ++normalUpdates; }
    void EraseObservation(MockKeyFrame* kf) { obs.erase(kf); }
};
struct MockKeyFrame {
    long unsigned int mnId, mnBALocalForKF, mnBAFixedForKF, mnBAGlobalForKF;
    cv::Mat Tcw, mTcwGBA;
    float fx, fy, cx, cy, mbf;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MockMapPoint*> matches;
    std::vector<MockKeyFrame*> covisible;
    int erased;
    MockKeyFrame() : mnId(0), mnBALocalForKF(~0ul), mnBAFixedForKF(~0ul), mnBAGlobalForKF(0), mbf(0.f), erased(0) {}
    bool isBad() { return false; }
    std::vector<MockKeyFrame*> GetVectorCovisibleKeyFrames() { return covisible; }
    std::vector<MockMapPoint*> GetMapPointMatches() { return matches; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& T) { Tcw = T.clone(); }
    void EraseMapPointMatch(MockMapPoint* mp) {
        for (size_t i = 0; i < matches.size(); ++i) if (matches[i] == mp) { matches[i] = 0; ++erased; }
    }
};
struct MockMap {
    std::mutex mMutexMapUpdate;
    std::vector<MockKeyFrame*> kfs;
    std::vector<MockMapPoint*> mps;
    std::vector<MockKeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<MockMapPoint*> GetAllMapPoints() { return mps; }
};

static int run_orb(int argc, char** argv) {
    if (argc < 6) return 2;
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    std::vector<unsigned char> raw = slurp(argv[2]);
    cv::Mat im(h, w, CV_8UC1, raw.data());
    ORBextractor ext(1000, 1.2f, 8, 20, 7);     // Tracking.cc:149-156
    ext.SetPyramidExport(true);
    std::vector<cv::KeyPoint> keys;
    cv::Mat desc;
    ext(im, cv::Mat(), keys, desc);
    if (!ext.ok()) { fprintf(stderr, "extract failed: %s\n", ext.lastError()); return 1; }
    FILE* f = fopen(argv[5], "wb");
    int n = (int)keys.size();
    fwrite(&n, 4, 1, f);
    if (n) fwrite(&keys[0], sizeof(cv::KeyPoint), n, f);
    for (int i = 0; i < n; ++i) fwrite(desc.ptr(i), 1, 32, f);
    // the mvImagePyramid member: ROI inside a REFLECT_101-padded plane
    int nl = ext.GetLevels();
    fwrite(&nl, 4, 1, f);
    for (int l = 0; l < nl; ++l) {
        const cv::Mat& m = ext.mvImagePyramid[l];
        int dims[2] = {m.cols, m.rows};
        fwrite(dims, 4, 2, f);
        unsigned sum = 0;  // checksum over ROI plus its 19-px frame, read through the ROI pointer
        for (int y = -19; y < m.rows + 19; ++y)
            for (int x = -19; x < m.cols + 19; ++x) sum = sum * 31u + m.data[(long)y * (long)m.step + x];
        fwrite(&sum, 4, 1, f);
    }
    std::vector<float> sf = ext.GetScaleFactors(), isig = ext.GetInverseScaleSigmaSquares();
    fwrite(sf.data(), 4, nl, f);
    fwrite(isig.data(), 4, nl, f);
    fclose(f);
    return 0;
}

static int run_match(int argc, char** argv) {
    if (argc < 7) return 2;
    std::vector<unsigned char> a = slurp(argv[2]), b = slurp(argv[4]);
    const int na = atoi(argv[3]), nb = atoi(argv[5]);
    cv::Mat da(na, 32, CV_8U, a.data()), db(nb, 32, CV_8U, b.data());
    std::vector<int> idx, best, second;
    if (!ORBmatcher::BestTwo(da, db, idx, best, second)) return 1;
    ORBmatcher m(0.9f, false);
    std::vector<cv::KeyPoint> none;
    std::vector<int> m12;
    int nm = m.SearchBruteForce(none, da, none, db, m12);
    int d00 = ORBmatcher::DescriptorDistance(da.row(0), db.row(0));
    FILE* f = fopen(argv[6], "wb");
    fwrite(idx.data(), 4, na, f); fwrite(best.data(), 4, na, f); fwrite(second.data(), 4, na, f);
    fwrite(m12.data(), 4, na, f); fwrite(&nm, 4, 1, f); fwrite(&d00, 4, 1, f);
    fclose(f);
    return 0;
}

// problem.bin: int32 n_kf n_pt n_edge | float pose[n_kf*12] | u8 fixed[n_kf] (padded to 4) |
//              float intr[4] | float pts[n_pt*3] | int32 ekf[] | int32 ept[] | float uv[2e] | float invsig[e]
//              [ | float bf | float ur[e] ]   (a window with stereo observations: KeyFrame::mbf and mvuRight, -1 = monocular)
static int run_ba(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    const unsigned char* p = raw.data();
    int hdr[3];
    memcpy(hdr, p, 12); p += 12;
    const int K = hdr[0], P = hdr[1], E = hdr[2];
    const float* pose = (const float*)p; p += 4 * 12 * K;
    const unsigned char* fixed = p; p += (K + 3) / 4 * 4;
    const float* intr = (const float*)p; p += 16;
    const float* pts = (const float*)p; p += 4 * 3 * P;
    const int* ekf = (const int*)p; p += 4 * E;
    const int* ept = (const int*)p; p += 4 * E;
    const float* uv = (const float*)p; p += 8 * E;
    const float* isg = (const float*)p; p += 4 * E;
    const bool stereo = (size_t)(p - raw.data()) + 4 + 4 * (size_t)E <= raw.size();
    const float bf = stereo ? *(const float*)p : 0.f;
    const float* ur = stereo ? (const float*)(p + 4) : 0;
    std::vector<MockKeyFrame> kfs(K);
    std::vector<MockMapPoint> mps(P);
    for (int k = 0; k < K; ++k) {
        MockKeyFrame& kf = kfs[k];
        // keyframe 0 of the file plays mnId 0 (fixed by id); further fixed ones are non-covisible observers
        kf.mnId = k;
        kf.Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) kf.Tcw.at<float>(r, c) = pose[12 * k + 3 * r + c]; kf.Tcw.at<float>(r, 3) = pose[12 * k + 9 + r]; kf.Tcw.at<float>(3, r) = 0; }
        kf.Tcw.at<float>(3, 3) = 1;
        kf.fx = intr[0]; kf.fy = intr[1]; kf.cx = intr[2]; kf.cy = intr[3]; kf.mbf = bf;
        kf.mvInvLevelSigma2.assign(1, 1.0f);
    }
    for (int q = 0; q < P; ++q) {
        mps[q].mnId = q;
        mps[q].pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) mps[q].pos.at<float>(r, 0) = pts[3 * q + r];
    }
    for (int e = 0; e < E; ++e) {
        MockKeyFrame& kf = kfs[ekf[e]];
        size_t slot = kf.mvKeysUn.size();
        cv::KeyPoint kp(uv[2 * e], uv[2 * e + 1], 31.f);
        kp.octave = (int)kf.mvInvLevelSigma2.size();   // one sigma entry per observation keeps invSigma2 exact
        kf.mvInvLevelSigma2.push_back(isg[e]);
        kf.mvKeysUn.push_back(kp);
        kf.mvuRight.push_back(ur ? ur[e] : -1.f);
        kf.matches.push_back(&mps[ept[e]]);
        mps[ept[e]].obs[&kf] = slot;
    }
    // the current keyframe is the last non-fixed one; every other non-fixed keyframe is covisible
    int cur = -1;
    for (int k = 0; k < K; ++k) if (!fixed[k] || k == 0) cur = k;
    for (int k = 0; k < K; ++k) if (k != cur && (!fixed[k] || k == 0)) kfs[cur].covisible.push_back(&kfs[k]);
    MockMap map;
    bool stop = false;
    // shim_test ba <problem> <out> [global <nIterations> <nLoopKF> <bRobust>]: GlobalBundleAdjustemnt over the same data
    const bool global = argc >= 8 && std::string(argv[4]) == "global";
    const unsigned long nLoopKF = global ? (unsigned long)atoi(argv[6]) : 0;
    if (global) {
        for (int k = 0; k < K; ++k) map.kfs.push_back(&kfs[k]);
        for (int q = 0; q < P; ++q) map.mps.push_back(&mps[q]);
        Optimizer::GlobalBundleAdjustemnt(&map, atoi(argv[5]), &stop, nLoopKF, atoi(argv[7]) != 0);
        if (nLoopKF) {   // results went to mTcwGBA / mPosGBA: fold them back so that the output format stays the same
            for (int k = 0; k < K; ++k) if (kfs[k].mnBAGlobalForKF == nLoopKF) kfs[k].Tcw = kfs[k].mTcwGBA.clone();
            for (int q = 0; q < P; ++q) if (mps[q].mnBAGlobalForKF == nLoopKF) { mps[q].pos = mps[q].mPosGBA.clone(); mps[q].normalUpdates = -1; }
        }
    } else {
        Optimizer::LocalBundleAdjustment(&kfs[cur], &stop, &map);
    }
    if (Optimizer::LastStatus() != 0) { fprintf(stderr, "BA failed: %s\n", slamit_last_error()); return 1; }
    FILE* f = fopen(argv[3], "wb");
    for (int k = 0; k < K; ++k)
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) fwrite(&kfs[k].Tcw.at<float>(r, c), 4, 1, f); }
    for (int k = 0; k < K; ++k) for (int r = 0; r < 3; ++r) fwrite(&kfs[k].Tcw.at<float>(r, 3), 4, 1, f);
    for (int q = 0; q < P; ++q) for (int r = 0; r < 3; ++r) fwrite(&mps[q].pos.at<float>(r, 0), 4, 1, f);
    int erased = 0, updates = 0;
    for (int k = 0; k < K; ++k) erased += kfs[k].erased;
    for (int q = 0; q < P; ++q) updates += mps[q].normalUpdates;
    fwrite(&erased, 4, 1, f); fwrite(&updates, 4, 1, f);
    fclose(f);
    return 0;
}

// pose.bin: int32 n | float pose[12] | float intr[4] | float xw[3n] | float uv[2n] | float invsig[n] [ | float bf | float ur[n] ]
struct MockFrame {
    int N;
    cv::Mat mTcw;
    float fx, fy, cx, cy, mbf;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<bool> mvbOutlier;
    std::vector<cv::KeyPoint> mvKeysUn;
    void SetPose(const cv::Mat& T) { mTcw = T.clone(); }
};

static int run_pose(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    const unsigned char* p = raw.data();
    int n;
    memcpy(&n, p, 4); p += 4;
    const float* pose = (const float*)p; p += 48;
    const float* intr = (const float*)p; p += 16;
    const float* xw = (const float*)p; p += 12 * n;
    const float* uv = (const float*)p; p += 8 * n;
    const float* isg = (const float*)p; p += 4 * n;
    // optional tail: float bf | float ur[n]  (a frame with stereo keypoints: Frame::mbf, mvuRight)
    const bool stereo = (size_t)(p - raw.data()) + 4 + 4 * (size_t)n <= raw.size();
    const float* ur = stereo ? (const float*)(p + 4) : 0;
    MockFrame F;
    F.mbf = stereo ? *(const float*)p : 0.f;
    std::vector<MockMapPoint> mps(n);
    F.N = n + 5;  // a few keypoints without a map point, like a real frame
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) F.mTcw.at<float>(r, c) = pose[3 * r + c]; F.mTcw.at<float>(r, 3) = pose[9 + r]; F.mTcw.at<float>(3, r) = 0; }
    F.mTcw.at<float>(3, 3) = 1;
    F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3];
    F.mvpMapPoints.assign(F.N, (MockMapPoint*)0); F.mvuRight.assign(F.N, -1.f); F.mvbOutlier.assign(F.N, false);
    F.mvKeysUn.resize(F.N); F.mvInvLevelSigma2.assign(1, 1.f);
    for (int i = 0; i < n; ++i) {
        mps[i].pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) mps[i].pos.at<float>(r, 0) = xw[3 * i + r];
        F.mvpMapPoints[i] = &mps[i];
        if (ur) F.mvuRight[i] = ur[i];
        F.mvKeysUn[i] = cv::KeyPoint(uv[2 * i], uv[2 * i + 1], 31.f);
        F.mvKeysUn[i].octave = (int)F.mvInvLevelSigma2.size();
        F.mvInvLevelSigma2.push_back(isg[i]);
    }
    int inl = Optimizer::PoseOptimization(&F);
    if (Optimizer::LastStatus() != 0) { fprintf(stderr, "pose failed: %s\n", slamit_last_error()); return 1; }
    FILE* f = fopen(argv[3], "wb");
    fwrite(&inl, 4, 1, f);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) fwrite(&F.mTcw.at<float>(r, c), 4, 1, f);
    for (int i = 0; i < n; ++i) { unsigned char o = F.mvbOutlier[i]; fwrite(&o, 1, 1, f); }
    fclose(f);
    return 0;
}

// ---- guided search: mock Frame / MapPoint with the members ORBmatcher.h documents -------------------
struct MockTrackPoint {
    bool mbTrackInView, bad;
    int mnTrackScaleLevel, nobs, id;
    float mTrackViewCos, mTrackProjX, mTrackProjXR, mTrackProjY, maxd, mind;
    cv::Mat desc, pos;
    MockTrackPoint() : mTrackProjXR(0.f) {}
    float GetMaxDistance() { return maxd; }   // raw (projection mode only)
    float GetMinDistance() { return mind; }
    float GetMaxDistanceInvariance() { return g_real_scale ? 1.2f * maxd : maxd; }
    float GetMinDistanceInvariance() { return g_real_scale ? 0.8f * mind : mind; }
    int PredictScale(const float& dist, const float& lsf) { return mock_predict_scale(mnTrackScaleLevel, maxd, dist, lsf); }   // the caller's method
    bool isBad() { return bad; }
    int Observations() { return nobs; }
    cv::Mat GetDescriptor() { return desc.clone(); }
    cv::Mat GetWorldPos() { return pos.clone(); }
};
struct MockSearchFrame {
    int N;
    cv::Mat mTcw, mDescriptors;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<MockTrackPoint*> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors;
    std::vector<bool> mvbOutlier;
    float fx, fy, cx, cy, mb, mbf, mfLogScaleFactor;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
};
struct MockRelocKF {
    std::vector<MockTrackPoint*> matches;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MockTrackPoint*> GetMapPointMatches() { return matches; }
};
float MockSearchFrame::mnMinX, MockSearchFrame::mnMaxX, MockSearchFrame::mnMinY, MockSearchFrame::mnMaxY;
float MockSearchFrame::mfGridElementWidthInv, MockSearchFrame::mfGridElementHeightInv;

struct Reader {
    const unsigned char* p;
    template <class T> T get() { T v; memcpy(&v, p, sizeof(T)); p += sizeof(T); return v; }
    template <class T> const T* arr(size_t n) { const T* a = (const T*)p; p += n * sizeof(T); return a; }
};

static cv::Mat mat_from(const float* v, int rows) {
    cv::Mat m(rows, 1, CV_32F);
    for (int r = 0; r < rows; ++r) m.at<float>(r, 0) = v[r];
    return m;
}
static cv::Mat pose_from(const float* p12) {   // R row-major (9) then t (3)
    cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T.at<float>(r, c) = p12[3 * r + c]; T.at<float>(r, 3) = p12[9 + r]; }
    T.at<float>(3, 3) = 1;
    return T;
}

// problem.bin (all little-endian, 4-byte aligned arrays first):
//   int32 variant n m ; float th nnratio ; float minx maxx miny maxy invw invh ; float scale[8]
//   current frame: float xy[2n] ; int32 octave[n] ; float angle[n] ; int32 state[n] (0 none, 1 map point with
//   observations, 2 map point without) ; u8 desc[32n]
//   variant 0 (map points): float proj[2m] viewcos[m] ; int32 level[m] inview[m] bad[m] nobs[m] ; u8 desc[32m]
//   variant 1 (last frame): float Tcw[12] Tlw[12] intr[5] ; int32 mono ; float world[3m] angle[m] ;
//                           int32 has[m] outlier[m] octave[m] nobs[m] ; u8 desc[32m]
//   variant 2 (relocalization, keyframe map points): float Tcw[12] intr[4] ; int32 orbdist ; float world[3m] angle[m] maxd[m]
//                           mind[m] ; int32 has[m] bad[m] found[m] level[m] ; u8 desc[32m]
//   optional tail, a stereo frame: variant 0: float mvuRight[n] ; float mTrackProjXR[m].  variant 1: float mbf ; float mvuRight[n]
// out.bin: int32 status nmatches ; int32 owner[n] (-1 none, -2 the frame's own earlier point, else query index)
static int run_search(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const unsigned char* const end = raw.data() + raw.size();
    const int variant = R.get<int>(), n = R.get<int>(), m = R.get<int>();
    const float th = R.get<float>(), nnratio = R.get<float>();
    projection_mode(argc, argv, 4);
    MockSearchFrame::mnMinX = R.get<float>(); MockSearchFrame::mnMaxX = R.get<float>();
    MockSearchFrame::mnMinY = R.get<float>(); MockSearchFrame::mnMaxY = R.get<float>();
    MockSearchFrame::mfGridElementWidthInv = R.get<float>(); MockSearchFrame::mfGridElementHeightInv = R.get<float>();
    const float* scale = R.arr<float>(8);
    const float* xy = R.arr<float>(2 * (size_t)n);
    const int* oct = R.arr<int>(n);
    const float* ang = R.arr<float>(n);
    const int* state = R.arr<int>(n);
    const unsigned char* desc = R.arr<unsigned char>(32 * (size_t)n);
    MockSearchFrame F;
    F.N = n;
    F.mfLogScaleFactor = 0.18232f;
    F.mvScaleFactors.assign(scale, scale + 8);
    F.mDescriptors = cv::Mat(n, 32, CV_8U);
    F.mvKeysUn.resize(n); F.mvuRight.assign(n, -1.f); F.mvpMapPoints.assign(n, (MockTrackPoint*)0); F.mvbOutlier.assign(n, false);
    MockTrackPoint own1, own2;
    own1.nobs = 3; own2.nobs = 0; own1.id = own2.id = -2;
    for (int i = 0; i < n; ++i) {
        F.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, ang[i], 0, oct[i]);
        memcpy(F.mDescriptors.ptr(i), desc + 32 * (size_t)i, 32);
        if (state[i] == 1) F.mvpMapPoints[i] = &own1;
        if (state[i] == 2) F.mvpMapPoints[i] = &own2;
    }
    F.mvKeys = F.mvKeysUn;
    std::vector<MockTrackPoint> mps(m);
    int nm = 0;
    if (variant == 0) {
        const float* proj = R.arr<float>(2 * (size_t)m);
        const float* vc = R.arr<float>(m);
        const int* level = R.arr<int>(m); const int* inview = R.arr<int>(m); const int* bad = R.arr<int>(m); const int* nobs = R.arr<int>(m);
        const unsigned char* qd = R.arr<unsigned char>(32 * (size_t)m);
        std::vector<MockTrackPoint*> vp(m);
        for (int q = 0; q < m; ++q) {
            MockTrackPoint& p = mps[q];
            p.id = q; p.mbTrackInView = inview[q] != 0; p.bad = bad[q] != 0; p.mnTrackScaleLevel = level[q]; p.nobs = nobs[q];
            p.mTrackViewCos = vc[q]; p.mTrackProjX = proj[2 * q]; p.mTrackProjY = proj[2 * q + 1];
            p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), qd + 32 * (size_t)q, 32);
            vp[q] = &p;
        }
        if (R.p < end) {
            const float* ur = R.arr<float>(n); const float* xr = R.arr<float>(m);
            F.mvuRight.assign(ur, ur + n);
            for (int q = 0; q < m; ++q) mps[q].mTrackProjXR = xr[q];
        }
        ORBmatcher matcher(nnratio, true);
        nm = matcher.SearchByProjection(F, vp, th);
    } else if (variant == 2) {
        const float* Tcw = R.arr<float>(12); const float* intr = R.arr<float>(4);
        const int orbdist = R.get<int>();
        const float* world = R.arr<float>(3 * (size_t)m); const float* kang = R.arr<float>(m);
        const float* maxd = R.arr<float>(m); const float* mind = R.arr<float>(m);
        const int* has = R.arr<int>(m); const int* bad = R.arr<int>(m); const int* found = R.arr<int>(m); const int* level = R.arr<int>(m);
        const unsigned char* qd = R.arr<unsigned char>(32 * (size_t)m);
        F.mTcw = pose_from(Tcw);
        F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; F.mfLogScaleFactor = 0.18232f;
        MockRelocKF KF;
        KF.matches.assign(m, (MockTrackPoint*)0); KF.mvKeysUn.resize(m);
        std::set<MockTrackPoint*> sFound;
        for (int q = 0; q < m; ++q) {
            MockTrackPoint& p = mps[q];
            p.id = q; p.bad = bad[q] != 0; p.mnTrackScaleLevel = level[q]; p.maxd = maxd[q]; p.mind = mind[q]; p.nobs = 1;
            p.pos = mat_from(world + 3 * (size_t)q, 3);
            p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), qd + 32 * (size_t)q, 32);
            KF.mvKeysUn[q] = cv::KeyPoint(0.f, 0.f, 31.f, kang[q], 0, 0);
            if (has[q]) KF.matches[q] = &p;
            if (found[q]) sFound.insert(&p);
        }
        ORBmatcher matcher(0.9f, true, g_device_projection);
        nm = matcher.SearchByProjection(F, &KF, sFound, th, orbdist);
    } else {
        const float* Tcw = R.arr<float>(12); const float* Tlw = R.arr<float>(12); const float* intr = R.arr<float>(5);
        const int mono = R.get<int>();
        const float* world = R.arr<float>(3 * (size_t)m); const float* lang = R.arr<float>(m);
        const int* has = R.arr<int>(m); const int* outl = R.arr<int>(m); const int* loct = R.arr<int>(m); const int* nobs = R.arr<int>(m);
        const unsigned char* qd = R.arr<unsigned char>(32 * (size_t)m);
        MockSearchFrame L;
        L.N = m; L.mTcw = pose_from(Tlw); F.mTcw = pose_from(Tcw);
        F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; F.mb = intr[4];
        L.mvKeys.resize(m); L.mvpMapPoints.assign(m, (MockTrackPoint*)0); L.mvbOutlier.assign(m, false);
        for (int q = 0; q < m; ++q) {
            MockTrackPoint& p = mps[q];
            p.id = q; p.nobs = nobs[q]; p.pos = mat_from(world + 3 * (size_t)q, 3);
            p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), qd + 32 * (size_t)q, 32);
            L.mvKeys[q] = cv::KeyPoint(0.f, 0.f, 31.f, lang[q], 0, loct[q]);
            if (has[q]) L.mvpMapPoints[q] = &p;
            L.mvbOutlier[q] = outl[q] != 0;
        }
        L.mvKeysUn = L.mvKeys;
        F.mbf = 0.f;
        if (R.p < end) {
            F.mbf = R.get<float>();
            const float* ur = R.arr<float>(n);
            F.mvuRight.assign(ur, ur + n);
        }
        ORBmatcher matcher(0.9f, true, g_device_projection);
        nm = matcher.SearchByProjection(F, L, th, mono != 0);
    }
    const int status = ORBmatcher::LastStatus();
    if (status != 0) fprintf(stderr, "search failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nm, 4, 1, f);
    for (int i = 0; i < n; ++i) { int o = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->id : -1; fwrite(&o, 4, 1, f); }
    fclose(f);
    return 0;
}

// ---- Frame epilogue: mock Frame with the members FrameOps.h documents -----------------------------------
struct MockEpiFrame {
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat mK, mDistCoef;
    std::vector<std::size_t> mGrid[SLAMIT_FRAME_GRID_COLS][SLAMIT_FRAME_GRID_ROWS];
    static float mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
};
float MockEpiFrame::mnMinX, MockEpiFrame::mnMaxX, MockEpiFrame::mnMinY, MockEpiFrame::mnMaxY;
float MockEpiFrame::mfGridElementWidthInv, MockEpiFrame::mfGridElementHeightInv;

// problem.bin: int32 n cols rows ; float cam[9] ; slamit_kp kps[n]
// out.bin: int32 status ; float bounds[6] ; slamit_kp kps_un[n] ; int32 counts[64*48] ; int32 items[sum counts]
static int run_frame(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int n = R.get<int>(), cols = R.get<int>(), rows = R.get<int>();
    const float* cam = R.arr<float>(9);
    const cv::KeyPoint* kps = R.arr<cv::KeyPoint>(n);
    MockEpiFrame F;
    F.N = n;
    F.mvKeys.assign(kps, kps + n);
    F.mK = cv::Mat::zeros(3, 3, CV_32F);
    F.mK.at<float>(0, 0) = cam[0]; F.mK.at<float>(1, 1) = cam[1]; F.mK.at<float>(0, 2) = cam[2]; F.mK.at<float>(1, 2) = cam[3];
    F.mK.at<float>(2, 2) = 1.f;
    F.mDistCoef = cv::Mat(5, 1, CV_32F);
    for (int i = 0; i < 5; ++i) F.mDistCoef.at<float>(i, 0) = cam[4 + i];
    cv::Mat im(rows, cols, CV_8U);
    FrameOps::ComputeImageBounds(F, im);
    int status = FrameOps::LastStatus();
    if (status == 0) { FrameOps::UndistortAndAssign(F); status = FrameOps::LastStatus(); }
    if (status != 0) fprintf(stderr, "frame failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f);
    const float b[6] = {MockEpiFrame::mnMinX, MockEpiFrame::mnMaxX, MockEpiFrame::mnMinY, MockEpiFrame::mnMaxY,
                        MockEpiFrame::mfGridElementWidthInv, MockEpiFrame::mfGridElementHeightInv};
    fwrite(b, 4, 6, f);
    fwrite(F.mvKeysUn.data(), sizeof(cv::KeyPoint), F.mvKeysUn.size(), f);
    for (int x = 0; x < SLAMIT_FRAME_GRID_COLS; ++x)
        for (int y = 0; y < SLAMIT_FRAME_GRID_ROWS; ++y) { int c = (int)F.mGrid[x][y].size(); fwrite(&c, 4, 1, f); }
    for (int x = 0; x < SLAMIT_FRAME_GRID_COLS; ++x)
        for (int y = 0; y < SLAMIT_FRAME_GRID_ROWS; ++y)
            for (size_t j = 0; j < F.mGrid[x][y].size(); ++j) { int v = (int)F.mGrid[x][y][j]; fwrite(&v, 4, 1, f); }
    fclose(f);
    return 0;
}

// ---- Fuse: mock KeyFrame / MapPoint with the members ORBmatcher.h documents ---------------------------------
struct MockFuseKF;
struct MockFusePoint {
    int id, nobs, level;
    bool bad, inKF;
    float maxd, mind;
    cv::Mat pos, normal, desc;
    MockFusePoint* replacedBy;
    int addedAt, idxInKF2;
    MockFusePoint() : id(-1), nobs(0), level(0), bad(false), inKF(false), maxd(0), mind(0), replacedBy(0), addedAt(-1), idxInKF2(-1) {}
    int GetIndexInKeyFrame(MockFuseKF*) { return idxInKF2; }
    bool isBad() { return bad; }
    bool IsInKeyFrame(MockFuseKF*) { return inKF; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetNormal() { return normal.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    float GetMaxDistance() { return maxd; }   // raw (projection mode only)
    float GetMinDistance() { return mind; }
    float GetMaxDistanceInvariance() { return g_real_scale ? 1.2f * maxd : maxd; }
    float GetMinDistanceInvariance() { return g_real_scale ? 0.8f * mind : mind; }
    int PredictScale(const float& dist, const float& lsf) { return mock_predict_scale(level, maxd, dist, lsf); }   // the caller's method
    int Observations() { return nobs; }
    void Replace(MockFusePoint* p) {
        replacedBy = p; bad = true;
        // projection mode: the survivor's descriptor changes, as ComputeDistinctiveDescriptors may change it (it takes over bytes 0 .. 15; the plain fuse command's own points carry no descriptor)
        if (g_real_scale && p->desc.rows > 0 && desc.rows > 0) { p->desc = p->desc.clone(); memcpy(p->desc.ptr(0), desc.ptr(0), 16); p->nobs += nobs; }
    }
    void AddObservation(MockFuseKF*, size_t idx) { addedAt = (int)idx; inKF = true; ++nobs; }
};
struct MockFuseKF {
    cv::Mat R, t, O, mDescriptors, mK;
    float fx, fy, cx, cy, mbf, mfLogScaleFactor;
    float mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvLevelSigma2, mvuRight;
    MockFuseKF() : mbf(0.f) {}
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MockFusePoint*> mps;
    cv::Mat GetRotation() { return R.clone(); }
    cv::Mat GetTranslation() { return t.clone(); }
    cv::Mat GetCameraCenter() { return O.clone(); }
    bool IsInImage(const float& x, const float& y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    MockFusePoint* GetMapPoint(size_t idx) { return mps[idx]; }
    void AddMapPoint(MockFusePoint* p, size_t idx) { mps[idx] = p; }
    std::vector<MockFusePoint*> GetMapPointMatches() { return mps; }
    std::set<MockFusePoint*> GetMapPoints() { std::set<MockFusePoint*> r; for (size_t i = 0; i < mps.size(); ++i) if (mps[i]) r.insert(mps[i]); return r; }
};

// problem.bin: int32 n m ; float th ; float R[9] t[3] O[3] ; float intr[4] ; float bounds[6] (minx maxx miny maxy invw invh) ;
//   float scale[8] invsig[8] ; keypoints: float xy[2n], int32 octave[n], int32 kf_state[n] (0 none, k>0: own point with k-1
//   observations), u8 desc[32n] ; map points: float pos[3m] normal[3m] maxd[m] mind[m], int32 level[m] nobs[m] bad[m] inkf[m]
//   null[m], u8 desc[32m] ; optional tail, a stereo keyframe: float mbf ; float mvuRight[n]
// out.bin: int32 status nFused ; per map point int32 addedAt, replacedBy (-1 none, -2 a keyframe-own point, else id), bad ;
//   per keypoint int32 owner (-1 none, -2 own, else map point id)
static int run_fuse(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const unsigned char* const end = raw.data() + raw.size();
    const int n = Rd.get<int>(), m = Rd.get<int>();
    const float th = Rd.get<float>();
    projection_mode(argc, argv, 4);
    const float* Rv = Rd.arr<float>(9); const float* tv = Rd.arr<float>(3); const float* Ov = Rd.arr<float>(3);
    const float* intr = Rd.arr<float>(4); const float* b = Rd.arr<float>(6);
    const float* scale = Rd.arr<float>(8); const float* invsig = Rd.arr<float>(8);
    const float* xy = Rd.arr<float>(2 * (size_t)n); const int* oct = Rd.arr<int>(n); const int* kfs = Rd.arr<int>(n);
    const unsigned char* kd = Rd.arr<unsigned char>(32 * (size_t)n);
    const float* pos = Rd.arr<float>(3 * (size_t)m); const float* nrm = Rd.arr<float>(3 * (size_t)m);
    const float* maxd = Rd.arr<float>(m); const float* mind = Rd.arr<float>(m);
    const int* level = Rd.arr<int>(m); const int* nobs = Rd.arr<int>(m); const int* bad = Rd.arr<int>(m); const int* inkf = Rd.arr<int>(m);
    const int* isnull = Rd.arr<int>(m);
    const unsigned char* md = Rd.arr<unsigned char>(32 * (size_t)m);
    MockFuseKF KF;
    KF.R = cv::Mat(3, 3, CV_32F); KF.t = cv::Mat(3, 1, CV_32F); KF.O = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) KF.R.at<float>(r, c) = Rv[3 * r + c]; KF.t.at<float>(r, 0) = tv[r]; KF.O.at<float>(r, 0) = Ov[r]; }
    KF.fx = intr[0]; KF.fy = intr[1]; KF.cx = intr[2]; KF.cy = intr[3]; KF.mfLogScaleFactor = 0.18232f;
    KF.mnMinX = b[0]; KF.mnMaxX = b[1]; KF.mnMinY = b[2]; KF.mnMaxY = b[3]; KF.mfGridElementWidthInv = b[4]; KF.mfGridElementHeightInv = b[5];
    KF.mvScaleFactors.assign(scale, scale + 8); KF.mvInvLevelSigma2.assign(invsig, invsig + 8);
    KF.mvuRight.assign(n, -1.f); KF.mvKeysUn.resize(n); KF.mps.assign(n, (MockFusePoint*)0);
    KF.mDescriptors = cv::Mat(n, 32, CV_8U);
    std::vector<MockFusePoint> own(n), pts(m);
    for (int i = 0; i < n; ++i) {
        KF.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, -1.f, 0, oct[i]);
        memcpy(KF.mDescriptors.ptr(i), kd + 32 * (size_t)i, 32);
        if (kfs[i] > 0) { own[i].id = -2; own[i].nobs = kfs[i] - 1; KF.mps[i] = &own[i]; }
    }
    std::vector<MockFusePoint*> vp(m);
    for (int j = 0; j < m; ++j) {
        MockFusePoint& p = pts[j];
        p.id = j; p.nobs = nobs[j]; p.level = level[j]; p.bad = bad[j] != 0; p.inKF = inkf[j] != 0; p.maxd = maxd[j]; p.mind = mind[j];
        p.pos = mat_from(pos + 3 * (size_t)j, 3); p.normal = mat_from(nrm + 3 * (size_t)j, 3);
        p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), md + 32 * (size_t)j, 32);
        vp[j] = isnull[j] ? (MockFusePoint*)0 : &p;
    }
    if (Rd.p < end) {
        KF.mbf = Rd.get<float>();
        const float* ur = Rd.arr<float>(n);
        KF.mvuRight.assign(ur, ur + n);
    }
    ORBmatcher matcher(0.6f, true, g_device_projection);
    const int nf = matcher.Fuse(&KF, vp, th);
    const int status = ORBmatcher::LastStatus();
    if (status != 0) fprintf(stderr, "fuse failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nf, 4, 1, f);
    for (int j = 0; j < m; ++j) {
        int a = pts[j].addedAt, r = pts[j].replacedBy ? pts[j].replacedBy->id : -1, bd = pts[j].bad ? 1 : 0;
        fwrite(&a, 4, 1, f); fwrite(&r, 4, 1, f); fwrite(&bd, 4, 1, f);
    }
    for (int i = 0; i < n; ++i) { int o = KF.mps[i] ? KF.mps[i]->id : -1; fwrite(&o, 4, 1, f); }
    for (int i = 0; i < n; ++i) { int r = own[i].replacedBy ? own[i].replacedBy->id : -1; fwrite(&r, 4, 1, f); }
    fclose(f);
    return 0;
}

// The multi-target Fuse (the first loop of LocalMapping::SearchInNeighbors).  fuse_targets <in> <out> host|device batch|single:
// `batch` is ONE Fuse(targets, points, th) call, `single` the loop of per-target calls.
// problem.bin: int32 nkf m ; float th ; map points: float pos[3m] normal[3m] maxd[m] mind[m] (raw), int32 nobs[m], u8 desc[32m] ;
//   per target: float R[9] t[3] O[3] intr[4] bounds[6] scale[8] invsig[8] ; int32 n ; float xy[2n] ; int32 octave[n] kf_state[n]
//   (0 none, k > 0: a point of the target's own with k - 1 observations) ; u8 desc[32n]
//   optional tail, stereo keyframes: per target float mbf ; float mvuRight[n]
// out.bin: int32 status nFused ; per map point int32 addedAt replacedBy (-1 none, -2 a target's own point, else id) bad nobs, u8 desc[32] ;
//   per target per keypoint int32 owner, int32 own point replacedBy
static int run_fuse_targets(int argc, char** argv) {
    if (argc < 6) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const unsigned char* const end = raw.data() + raw.size();
    const int nkf = Rd.get<int>(), m = Rd.get<int>();
    const float th = Rd.get<float>();
    projection_mode(argc, argv, 4);
    const bool batch = std::string(argv[5]) == "batch";
    const float* pos = Rd.arr<float>(3 * (size_t)m); const float* nrm = Rd.arr<float>(3 * (size_t)m);
    const float* maxd = Rd.arr<float>(m); const float* mind = Rd.arr<float>(m);
    const int* nobs = Rd.arr<int>(m);
    const unsigned char* md = Rd.arr<unsigned char>(32 * (size_t)m);
    std::vector<MockFusePoint> pts(m);
    std::vector<MockFusePoint*> vp(m);
    for (int j = 0; j < m; ++j) {
        MockFusePoint& p = pts[j];
        p.id = j; p.nobs = nobs[j]; p.maxd = maxd[j]; p.mind = mind[j];
        p.pos = mat_from(pos + 3 * (size_t)j, 3); p.normal = mat_from(nrm + 3 * (size_t)j, 3);
        p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), md + 32 * (size_t)j, 32);
        vp[j] = &p;
    }
    std::vector<MockFuseKF> KF(nkf);
    std::vector<std::vector<MockFusePoint> > own(nkf);
    std::vector<MockFuseKF*> targets(nkf);
    for (int k = 0; k < nkf; ++k) {
        const float* Rv = Rd.arr<float>(9); const float* tv = Rd.arr<float>(3); const float* Ov = Rd.arr<float>(3);
        const float* intr = Rd.arr<float>(4); const float* b = Rd.arr<float>(6);
        const float* scale = Rd.arr<float>(8); const float* invsig = Rd.arr<float>(8);
        const int n = Rd.get<int>();
        const float* xy = Rd.arr<float>(2 * (size_t)n); const int* oct = Rd.arr<int>(n); const int* kfs = Rd.arr<int>(n);
        const unsigned char* kd = Rd.arr<unsigned char>(32 * (size_t)n);
        MockFuseKF& K = KF[k];
        K.R = cv::Mat(3, 3, CV_32F); K.t = mat_from(tv, 3); K.O = mat_from(Ov, 3);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K.R.at<float>(r, c) = Rv[3 * r + c];
        K.fx = intr[0]; K.fy = intr[1]; K.cx = intr[2]; K.cy = intr[3]; K.mfLogScaleFactor = 0.18232f;
        K.mnMinX = b[0]; K.mnMaxX = b[1]; K.mnMinY = b[2]; K.mnMaxY = b[3]; K.mfGridElementWidthInv = b[4]; K.mfGridElementHeightInv = b[5];
        K.mvScaleFactors.assign(scale, scale + 8); K.mvInvLevelSigma2.assign(invsig, invsig + 8);
        K.mvuRight.assign(n, -1.f); K.mvKeysUn.resize(n); K.mps.assign(n, (MockFusePoint*)0);
        K.mDescriptors = cv::Mat(n, 32, CV_8U);
        own[k].resize(n);
        for (int i = 0; i < n; ++i) {
            K.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, -1.f, 0, oct[i]);
            memcpy(K.mDescriptors.ptr(i), kd + 32 * (size_t)i, 32);
            if (kfs[i] > 0) {
                MockFusePoint& o = own[k][i];
                o.id = -2; o.nobs = kfs[i] - 1; o.desc = cv::Mat(1, 32, CV_8U); memcpy(o.desc.ptr(0), kd + 32 * (size_t)i, 32);
                K.mps[i] = &o;
            }
        }
        targets[k] = &K;
    }
    if (Rd.p < end)
        for (int k = 0; k < nkf; ++k) {
            KF[k].mbf = Rd.get<float>();
            const float* ur = Rd.arr<float>(KF[k].mvKeysUn.size());
            KF[k].mvuRight.assign(ur, ur + KF[k].mvKeysUn.size());
        }
    ORBmatcher matcher(0.6f, true, g_device_projection);
    int nf = 0, status = 0;
    if (batch) { nf = matcher.Fuse(targets, vp, th); status = ORBmatcher::LastStatus(); }
    else
        for (int k = 0; k < nkf && status == 0; ++k) { nf += matcher.Fuse(targets[k], vp, th); status = ORBmatcher::LastStatus(); }
    if (status != 0) fprintf(stderr, "fuse_targets failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nf, 4, 1, f);
    for (int j = 0; j < m; ++j) {
        int v[4] = {pts[j].addedAt, pts[j].replacedBy ? pts[j].replacedBy->id : -1, pts[j].bad ? 1 : 0, pts[j].nobs};
        fwrite(v, 4, 4, f); fwrite(pts[j].desc.ptr(0), 1, 32, f);
    }
    for (int k = 0; k < nkf; ++k)
        for (size_t i = 0; i < KF[k].mps.size(); ++i) {
            int v[2] = {KF[k].mps[i] ? KF[k].mps[i]->id : -1, own[k][i].replacedBy ? own[k][i].replacedBy->id : -1};
            fwrite(v, 4, 2, f);
        }
    fclose(f);
    return 0;
}

// problem.bin: int32 n1 n2 window ; float nnratio ; float bounds[6] ; F1: int32 octave[n1], float angle[n1], float prev[2 n1],
//   u8 desc[32 n1] ; F2: float xy[2 n2], int32 octave[n2], float angle[n2], u8 desc[32 n2]
// out.bin: int32 status nmatches ; int32 vnMatches12[n1] ; float prev[2 n1]
static int run_init(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int n1 = R.get<int>(), n2 = R.get<int>(), window = R.get<int>();
    const float nnratio = R.get<float>();
    MockSearchFrame::mnMinX = R.get<float>(); MockSearchFrame::mnMaxX = R.get<float>();
    MockSearchFrame::mnMinY = R.get<float>(); MockSearchFrame::mnMaxY = R.get<float>();
    MockSearchFrame::mfGridElementWidthInv = R.get<float>(); MockSearchFrame::mfGridElementHeightInv = R.get<float>();
    const int* o1 = R.arr<int>(n1); const float* a1 = R.arr<float>(n1); const float* prev = R.arr<float>(2 * (size_t)n1);
    const unsigned char* d1 = R.arr<unsigned char>(32 * (size_t)n1);
    const float* xy2 = R.arr<float>(2 * (size_t)n2); const int* o2 = R.arr<int>(n2); const float* a2 = R.arr<float>(n2);
    const unsigned char* d2 = R.arr<unsigned char>(32 * (size_t)n2);
    MockSearchFrame F1, F2;
    F1.N = n1; F2.N = n2;
    F1.mDescriptors = cv::Mat(n1, 32, CV_8U); F2.mDescriptors = cv::Mat(n2, 32, CV_8U);
    F1.mvKeysUn.resize(n1); F2.mvKeysUn.resize(n2);
    for (int i = 0; i < n1; ++i) { F1.mvKeysUn[i] = cv::KeyPoint(0.f, 0.f, 31.f, a1[i], 0, o1[i]); memcpy(F1.mDescriptors.ptr(i), d1 + 32 * (size_t)i, 32); }
    for (int i = 0; i < n2; ++i) { F2.mvKeysUn[i] = cv::KeyPoint(xy2[2 * i], xy2[2 * i + 1], 31.f, a2[i], 0, o2[i]); memcpy(F2.mDescriptors.ptr(i), d2 + 32 * (size_t)i, 32); }
    std::vector<cv::Point2f> vbPrevMatched(n1);
    for (int i = 0; i < n1; ++i) vbPrevMatched[i] = cv::Point2f(prev[2 * i], prev[2 * i + 1]);
    std::vector<int> vnMatches12;
    ORBmatcher matcher(nnratio, true);
    const int nm = matcher.SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, window);
    const int status = ORBmatcher::LastStatus();
    if (status != 0) fprintf(stderr, "init failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nm, 4, 1, f);
    fwrite(vnMatches12.data(), 4, n1, f);
    for (int i = 0; i < n1; ++i) { fwrite(&vbPrevMatched[i].x, 4, 1, f); fwrite(&vbPrevMatched[i].y, 4, 1, f); }
    fclose(f);
    return 0;
}

// ---- SearchByBoW / SearchForTriangulation through the templates ----------------------------------------------------
struct MockBowPoint {
    int id; bool bad;
    bool isBad() const { return bad; }
};
struct MockBowKF {   // doubles as the Frame of SearchByBoW(KeyFrame*, Frame&)
    int N;
    std::map<unsigned, std::vector<unsigned> > mFeatVec;   // the shape of DBoW2::FeatureVector
    cv::Mat mDescriptors, Ow, Rcw, tcw;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<MockBowPoint*> matches;
    std::vector<float> mvuRight, mvScaleFactors, mvLevelSigma2;
    float fx, fy, cx, cy;
    std::vector<MockBowPoint*> GetMapPointMatches() { return matches; }
    MockBowPoint* GetMapPoint(size_t i) { return matches[i]; }
    cv::Mat GetCameraCenter() { return Ow; }
    cv::Mat GetRotation() { return Rcw; }
    cv::Mat GetTranslation() { return tcw; }
};
// problem.bin: int32 variant (0 KeyFrame/Frame, 1 KeyFrame/KeyFrame, 2 triangulation) n1 n2 ; float nnratio ;
//   per side: u8 desc[32 n], float angle[n], int32 node[n], int32 mp[n] (0 none, 1 good, 2 bad), float xy[2 n], int32 octave[n] ;
//   float F12[9] Cw[3] R2w[9] t2w[3] intr[4] scale[8] sigma2[8]
// out.bin: int32 status nmatches ; variant 0: int32[n2] (side-1 index of the map point given to frame feature i, or -1),
//   variant 1: int32[n1] (side-2 index whose map point was matched, or -1), variant 2: int32 npairs, then int32 pairs[2 npairs]
static void fill_side(Reader& R, int n, MockBowKF& K, std::vector<MockBowPoint>& pts) {
    const unsigned char* d = R.arr<unsigned char>(32 * (size_t)n);
    const float* ang = R.arr<float>(n); const int* node = R.arr<int>(n); const int* mp = R.arr<int>(n);
    const float* xy = R.arr<float>(2 * (size_t)n); const int* oct = R.arr<int>(n);
    K.N = n; K.mDescriptors = cv::Mat(n, 32, CV_8U); K.mvKeysUn.resize(n); K.matches.assign(n, (MockBowPoint*)0); K.mvuRight.assign(n, -1.f);
    pts.resize(n);
    for (int i = 0; i < n; ++i) {
        memcpy(K.mDescriptors.ptr(i), d + 32 * (size_t)i, 32);
        K.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, ang[i], 0, oct[i]);
        K.mFeatVec[(unsigned)node[i]].push_back((unsigned)i);
        pts[i].id = i; pts[i].bad = mp[i] == 2;
        if (mp[i]) K.matches[i] = &pts[i];
    }
    K.mvKeys = K.mvKeysUn;
}
static int run_bow(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int variant = R.get<int>(), n1 = R.get<int>(), n2 = R.get<int>();
    const float nnratio = R.get<float>();
    MockBowKF K1, K2;
    std::vector<MockBowPoint> p1, p2;
    fill_side(R, n1, K1, p1);
    fill_side(R, n2, K2, p2);
    const float* F = R.arr<float>(9); const float* Cw = R.arr<float>(3); const float* R2 = R.arr<float>(9); const float* t2 = R.arr<float>(3);
    const float* intr = R.arr<float>(4); const float* scale = R.arr<float>(8); const float* sig = R.arr<float>(8);
    K1.Ow = mat_from(Cw, 3);
    K2.Rcw = cv::Mat(3, 3, CV_32F); K2.tcw = mat_from(t2, 3);
    cv::Mat F12(3, 3, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { K2.Rcw.at<float>(r, c) = R2[3 * r + c]; F12.at<float>(r, c) = F[3 * r + c]; }
    K2.fx = intr[0]; K2.fy = intr[1]; K2.cx = intr[2]; K2.cy = intr[3];
    K2.mvScaleFactors.assign(scale, scale + 8); K2.mvLevelSigma2.assign(sig, sig + 8);
    ORBmatcher matcher(nnratio, true);
    int nm = 0;
    std::vector<int> out;
    if (variant == 0) {
        std::vector<MockBowPoint*> got;
        nm = matcher.SearchByBoW(&K1, K2, got);
        out.assign(n2, -1);
        for (int i = 0; i < n2 && i < (int)got.size(); ++i) if (got[i]) out[i] = got[i]->id;
    } else if (variant == 1) {
        std::vector<MockBowPoint*> got;
        nm = matcher.SearchByBoW(&K1, &K2, got);
        out.assign(n1, -1);
        for (int i = 0; i < n1 && i < (int)got.size(); ++i) if (got[i]) out[i] = got[i]->id;
    } else {
        std::vector<std::pair<size_t, size_t> > pairs;
        nm = matcher.SearchForTriangulation(&K1, &K2, F12, pairs, false);
        out.push_back((int)pairs.size());
        for (size_t k = 0; k < pairs.size(); ++k) { out.push_back((int)pairs[k].first); out.push_back((int)pairs[k].second); }
    }
    const int status = ORBmatcher::LastStatus();
    if (status != 0) fprintf(stderr, "bow failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nm, 4, 1, f);
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}

// ---- the Sim3 drivers through the templates -----------------------------------------------------------------------
// problem.bin: int32 variant (0 SearchByProjection(pKF, Scw, ...), 1 Fuse(pKF, Scw, ...), 2 SearchBySim3) nkf ; float th ;
//   map points: int32 m ; float pos[3m] normal[3m] maxd[m] mind[m] ; int32 level[m] bad[m] idx_in_kf2[m] ; u8 desc[32m]
//   per keyframe (nkf of them): float R[9] t[3] intr[4] bounds[6] scale[8] ; int32 n ; float xy[2n] ; int32 octave[n] mp[n] (map point
//     id sitting at the keypoint or -1) ; u8 desc[32n]
//   variant 0/1: float Scw[12] (rows 0..2 of the 4x4) ; variant 0: int32 matched[n] ; variant 2: float s12 R12[9] t12[3] ; int32 matches12[n1]
// out.bin: int32 status count ; variant 0: int32 matched[n] ; variant 1: int32 replace[m] addedAt[m] owner[n] ; variant 2: int32 matches12[n1]
static void read_kf(Reader& Rd, MockFuseKF& KF, std::vector<MockFusePoint>& pts) {
    const float* Rv = Rd.arr<float>(9); const float* tv = Rd.arr<float>(3); const float* intr = Rd.arr<float>(4);
    const float* b = Rd.arr<float>(6); const float* scale = Rd.arr<float>(8);
    const int n = Rd.get<int>();
    const float* xy = Rd.arr<float>(2 * (size_t)n); const int* oct = Rd.arr<int>(n); const int* mp = Rd.arr<int>(n);
    const unsigned char* kd = Rd.arr<unsigned char>(32 * (size_t)n);
    KF.R = cv::Mat(3, 3, CV_32F); KF.t = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) KF.R.at<float>(r, c) = Rv[3 * r + c]; KF.t.at<float>(r, 0) = tv[r]; }
    KF.fx = intr[0]; KF.fy = intr[1]; KF.cx = intr[2]; KF.cy = intr[3]; KF.mfLogScaleFactor = 0.18232f;
    KF.mnMinX = b[0]; KF.mnMaxX = b[1]; KF.mnMinY = b[2]; KF.mnMaxY = b[3]; KF.mfGridElementWidthInv = b[4]; KF.mfGridElementHeightInv = b[5];
    KF.mvScaleFactors.assign(scale, scale + 8);
    KF.mvuRight.assign(n, -1.f); KF.mvKeysUn.resize(n); KF.mps.assign(n, (MockFusePoint*)0);
    KF.mDescriptors = cv::Mat(n, 32, CV_8U);
    for (int i = 0; i < n; ++i) {
        KF.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, -1.f, 0, oct[i]);
        memcpy(KF.mDescriptors.ptr(i), kd + 32 * (size_t)i, 32);
        if (mp[i] >= 0) KF.mps[i] = &pts[mp[i]];
    }
}
static int run_sim3(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int variant = Rd.get<int>(), nkf = Rd.get<int>();
    const float th = Rd.get<float>();
    projection_mode(argc, argv, 4);
    const int m = Rd.get<int>();
    const float* pos = Rd.arr<float>(3 * (size_t)m); const float* nrm = Rd.arr<float>(3 * (size_t)m);
    const float* maxd = Rd.arr<float>(m); const float* mind = Rd.arr<float>(m);
    const int* level = Rd.arr<int>(m); const int* bad = Rd.arr<int>(m); const int* idx2 = Rd.arr<int>(m);
    const unsigned char* md = Rd.arr<unsigned char>(32 * (size_t)m);
    std::vector<MockFusePoint> pts(m);
    for (int j = 0; j < m; ++j) {
        MockFusePoint& p = pts[j];
        p.id = j; p.level = level[j]; p.bad = bad[j] != 0; p.maxd = maxd[j]; p.mind = mind[j]; p.idxInKF2 = idx2[j];
        p.pos = mat_from(pos + 3 * (size_t)j, 3); p.normal = mat_from(nrm + 3 * (size_t)j, 3);
        p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), md + 32 * (size_t)j, 32);
    }
    MockFuseKF KF[2];
    for (int k = 0; k < nkf && k < 2; ++k) read_kf(Rd, KF[k], pts);
    ORBmatcher matcher(0.75f, true, g_device_projection);
    std::vector<int> out;
    int count = 0;
    if (variant == 0 || variant == 1) {
        const float* S = Rd.arr<float>(12);
        cv::Mat Scw = cv::Mat::zeros(4, 4, CV_32F);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) Scw.at<float>(r, c) = S[4 * r + c];
        Scw.at<float>(3, 3) = 1.f;
        std::vector<MockFusePoint*> vp(m);
        for (int j = 0; j < m; ++j) vp[j] = &pts[j];
        const int n = (int)KF[0].mvKeysUn.size();
        if (variant == 0) {
            const int* init = Rd.arr<int>(n);
            std::vector<MockFusePoint*> vpMatched(n, (MockFusePoint*)0);
            for (int i = 0; i < n; ++i) if (init[i] >= 0) vpMatched[i] = &pts[init[i]];
            count = matcher.SearchByProjection(&KF[0], Scw, vp, vpMatched, (int)th);
            for (int i = 0; i < n; ++i) out.push_back(vpMatched[i] ? vpMatched[i]->id : -1);
        } else {
            std::vector<MockFusePoint*> vpReplace(m, (MockFusePoint*)0);
            count = matcher.Fuse(&KF[0], Scw, vp, th, vpReplace);
            for (int j = 0; j < m; ++j) out.push_back(vpReplace[j] ? vpReplace[j]->id : -1);
            for (int j = 0; j < m; ++j) out.push_back(pts[j].addedAt);
            for (int i = 0; i < n; ++i) out.push_back(KF[0].mps[i] ? KF[0].mps[i]->id : -1);
        }
    } else {
        const float s12 = Rd.get<float>();
        const float* Rv = Rd.arr<float>(9); const float* tv = Rd.arr<float>(3);
        cv::Mat R12(3, 3, CV_32F), t12 = mat_from(tv, 3);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R12.at<float>(r, c) = Rv[3 * r + c];
        const int n1 = (int)KF[0].mvKeysUn.size();
        const int* init = Rd.arr<int>(n1);
        std::vector<MockFusePoint*> vpMatches12(n1, (MockFusePoint*)0);
        for (int i = 0; i < n1; ++i) if (init[i] >= 0) vpMatches12[i] = &pts[init[i]];
        count = matcher.SearchBySim3(&KF[0], &KF[1], vpMatches12, s12, R12, t12, th);
        for (int i = 0; i < n1; ++i) out.push_back(vpMatches12[i] ? vpMatches12[i]->id : -1);
    }
    const int status = ORBmatcher::LastStatus();
    if (status != 0) fprintf(stderr, "sim3 failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&count, 4, 1, f);
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}

// ---- Optimizer::OptimizeSim3 through the template ----------------------------------------------------------------
struct MockSim3 { double R[9], t[3], s; };
inline void slamit_shim_sim3_get(const MockSim3& S, double R[9], double t[3], double& s) { memcpy(R, S.R, 72); memcpy(t, S.t, 24); s = S.s; }
inline void slamit_shim_sim3_set(MockSim3& S, const double R[9], const double t[3], double s) { memcpy(S.R, R, 72); memcpy(S.t, t, 24); S.s = s; }
// problem.bin: int32 n1 n2 m fix_scale ; float th2 ; double S12[13] (R, t, s) ; per keyframe: float K[4] (fx fy cx cy) R[9] t[3] invsig[8],
//   keypoints float xy[2n] int32 octave[n] int32 mp[n] (own map point id or -1) ; map points: float pos[3m], int32 bad[m] idx_in_kf2[m] ;
//   int32 matches1[n1] (map point id of the KF2 point matched to keypoint i of KF1, or -1)
// out.bin: int32 status n_inliers ; int32 matches1[n1] ; double S12[13]
static int run_osim3(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int n[2] = {Rd.get<int>(), Rd.get<int>()};
    const int m = Rd.get<int>(), fix = Rd.get<int>();
    const float th2 = Rd.get<float>();
    MockSim3 S12;
    { const double* v = Rd.arr<double>(13); memcpy(S12.R, v, 72); memcpy(S12.t, v + 9, 24); S12.s = v[12]; }
    MockFuseKF KF[2];
    const int* mpk[2];
    for (int k = 0; k < 2; ++k) {
        const float* K = Rd.arr<float>(4); const float* Rv = Rd.arr<float>(9); const float* tv = Rd.arr<float>(3); const float* isg = Rd.arr<float>(8);
        const float* xy = Rd.arr<float>(2 * (size_t)n[k]); const int* oct = Rd.arr<int>(n[k]); mpk[k] = Rd.arr<int>(n[k]);
        KF[k].mK = cv::Mat::zeros(3, 3, CV_32F);
        KF[k].mK.at<float>(0, 0) = K[0]; KF[k].mK.at<float>(1, 1) = K[1]; KF[k].mK.at<float>(0, 2) = K[2]; KF[k].mK.at<float>(1, 2) = K[3]; KF[k].mK.at<float>(2, 2) = 1.f;
        KF[k].R = cv::Mat(3, 3, CV_32F); KF[k].t = mat_from(tv, 3);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) KF[k].R.at<float>(r, c) = Rv[3 * r + c];
        KF[k].mvInvLevelSigma2.assign(isg, isg + 8);
        KF[k].mvKeysUn.resize(n[k]);
        for (int i = 0; i < n[k]; ++i) KF[k].mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, -1.f, 0, oct[i]);
    }
    const float* pos = Rd.arr<float>(3 * (size_t)m); const int* bad = Rd.arr<int>(m); const int* idx2 = Rd.arr<int>(m);
    std::vector<MockFusePoint> pts(m);
    for (int j = 0; j < m; ++j) { pts[j].id = j; pts[j].bad = bad[j] != 0; pts[j].idxInKF2 = idx2[j]; pts[j].pos = mat_from(pos + 3 * (size_t)j, 3); }
    for (int k = 0; k < 2; ++k) { KF[k].mps.assign(n[k], (MockFusePoint*)0); for (int i = 0; i < n[k]; ++i) if (mpk[k][i] >= 0) KF[k].mps[i] = &pts[mpk[k][i]]; }
    const int* m1 = Rd.arr<int>(n[0]);
    std::vector<MockFusePoint*> vpMatches1(n[0], (MockFusePoint*)0);
    for (int i = 0; i < n[0]; ++i) if (m1[i] >= 0) vpMatches1[i] = &pts[m1[i]];
    const int nin = Optimizer::OptimizeSim3(&KF[0], &KF[1], vpMatches1, S12, th2, fix != 0);
    const int status = Optimizer::LastStatus();
    if (status != 0) fprintf(stderr, "osim3 failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nin, 4, 1, f);
    for (int i = 0; i < n[0]; ++i) { int id = vpMatches1[i] ? vpMatches1[i]->id : -1; fwrite(&id, 4, 1, f); }
    fwrite(S12.R, 8, 9, f); fwrite(S12.t, 8, 3, f); fwrite(&S12.s, 8, 1, f);
    fclose(f);
    return 0;
}

// ---- Sim3Solver through the template: the candidates of one loop query, one EvaluateAll -----------------------------------
// problem.bin: int32 nsolvers nrand ; uint32 rand[nrand] (RandomInt(lo, hi) = lo + rand[k++] % (hi - lo + 1), one stream for all
//   solvers in order: each constructor draws for the default parameters, each SetRansacParameters draws again) ; per solver:
//   int32 n lead fix min_inliers max_its ; float K1[4] K2[4] x1[3n] x2[3n] sigma2_1[n] sigma2_2[n]
//   (keyframe 1 holds `lead` keypoints without a match in front of the n matched ones; both keyframes sit at the identity pose)
// out.bin: int32 status ; per solver: int32 accepted n_inliers ncalls max_its ; float T12[16] R[9] t[3] s ; u8 vbInliers[lead + n]
static std::vector<uint32_t> g_script;
static size_t g_script_pos = 0;
static int scripted_random_int(int lo, int hi) {
    const uint32_t v = g_script_pos < g_script.size() ? g_script[g_script_pos] : 0u;
    ++g_script_pos;
    return lo + (int)(v % (uint32_t)(hi - lo + 1));
}
static int run_sim3solver(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int ns = Rd.get<int>(), nrand = Rd.get<int>();
    { const uint32_t* r = Rd.arr<uint32_t>(nrand); g_script.assign(r, r + nrand); }
    sim3solver::RandomInt() = scripted_random_int;
    typedef Sim3Solver<MockFuseKF, MockFusePoint> Solver;
    std::vector<MockFuseKF> kfs(2 * (size_t)ns);
    std::vector<std::vector<MockFusePoint> > pts(2 * (size_t)ns);
    std::vector<Solver*> solvers;
    std::vector<int> total(ns);
    for (int k = 0; k < ns; ++k) {
        const int n = Rd.get<int>(), ld = Rd.get<int>(), fix = Rd.get<int>(), minInl = Rd.get<int>(), maxIts = Rd.get<int>();
        const float* K[2]; K[0] = Rd.arr<float>(4); K[1] = Rd.arr<float>(4);
        const float* x[2]; x[0] = Rd.arr<float>(3 * (size_t)n); x[1] = Rd.arr<float>(3 * (size_t)n);
        const float* sg[2]; sg[0] = Rd.arr<float>(n); sg[1] = Rd.arr<float>(n);
        total[k] = ld + n;
        for (int c = 0; c < 2; ++c) {
            MockFuseKF& KF = kfs[2 * k + c];
            KF.mK = cv::Mat::zeros(3, 3, CV_32F);
            KF.mK.at<float>(0, 0) = K[c][0]; KF.mK.at<float>(1, 1) = K[c][1]; KF.mK.at<float>(0, 2) = K[c][2]; KF.mK.at<float>(1, 2) = K[c][3]; KF.mK.at<float>(2, 2) = 1.f;
            KF.R = cv::Mat::zeros(3, 3, CV_32F); KF.t = cv::Mat::zeros(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) KF.R.at<float>(r, r) = 1.f;
            const int off = c == 0 ? ld : 0;
            KF.mvKeysUn.resize(off + n); KF.mps.assign(off + n, (MockFusePoint*)0); KF.mvLevelSigma2.assign(sg[c], sg[c] + n);
            pts[2 * k + c].resize(n);
            for (int i = 0; i < n; ++i) {
                MockFusePoint& p = pts[2 * k + c][i];
                p.id = i; p.idxInKF2 = off + i; p.pos = mat_from(x[c] + 3 * (size_t)i, 3);
                KF.mvKeysUn[off + i] = cv::KeyPoint(0.f, 0.f, 31.f, -1.f, 0, i);   // one sigma entry per keypoint keeps sigma2 exact
                KF.mps[off + i] = &p;
            }
        }
        std::vector<MockFusePoint*> vpMatched12(ld + n, (MockFusePoint*)0);
        for (int i = 0; i < n; ++i) vpMatched12[ld + i] = &pts[2 * k + 1][i];
        Solver* s = new Solver(&kfs[2 * k], &kfs[2 * k + 1], vpMatched12, fix != 0);
        s->SetRansacParameters(0.99, minInl, maxIts);   // LoopClosing.cc:276
        solvers.push_back(s);
    }
    int status = Solver::EvaluateAll(solvers);   // every candidate in one launch
    if (status != 0) fprintf(stderr, "sim3solver failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f);
    for (int k = 0; k < ns && status == 0; ++k) {
        Solver* s = solvers[k];
        std::vector<bool> vbInliers(total[k], false);
        int nInliers = 0, ncalls = 0;
        bool bNoMore = false;
        cv::Mat T;
        while (T.empty() && !bNoMore) { T = s->iterate(5, bNoMore, vbInliers, nInliers); ++ncalls; }   // LoopClosing.cc:311
        const int acc = s->AcceptedHypothesis(), its = s->GetRansacMaxIts();
        fwrite(&acc, 4, 1, f); fwrite(&nInliers, 4, 1, f); fwrite(&ncalls, 4, 1, f); fwrite(&its, 4, 1, f);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { const float v = T.empty() ? 0.f : T.at<float>(r, c); fwrite(&v, 4, 1, f); }
        cv::Mat Re = s->GetEstimatedRotation(), te = s->GetEstimatedTranslation();
        const float se = s->GetEstimatedScale();
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) fwrite(&Re.at<float>(r, c), 4, 1, f);
        for (int r = 0; r < 3; ++r) fwrite(&te.at<float>(r, 0), 4, 1, f);
        fwrite(&se, 4, 1, f);
        for (int i = 0; i < total[k]; ++i) { const unsigned char b = vbInliers[i]; fwrite(&b, 1, 1, f); }
        printf("solver %d: accepted hypothesis %d, %d inliers, T12 row 0 = %g %g %g %g\n", k, acc, nInliers, T.empty() ? 0.f : T.at<float>(0, 0),
               T.empty() ? 0.f : T.at<float>(0, 1), T.empty() ? 0.f : T.at<float>(0, 2), T.empty() ? 0.f : T.at<float>(0, 3));
    }
    fclose(f);
    for (size_t k = 0; k < solvers.size(); ++k) delete solvers[k];
    return status == 0 ? 0 : 1;
}

// ---- LocalMapping::CreateNewMapPoints through the template -----------------------------------------------------------------------
struct MockMapKF : MockBowKF {   // the members LocalMapping.h lists on top of the matcher's
    float invfx, invfy, mfScaleFactor, medianDepth;
    float ComputeSceneMedianDepth(int) { return medianDepth; }
};
// problem.bin: int32 nkf (the current keyframe, then its neighbours in covisibility order) stereo_kf (-1, or the keyframe whose
//   keypoint 0 gets a right-image coordinate) monocular ; float scale[8] sigma2[8] ; per keyframe: int32 n ; float R[9] t[3] intr[4]
//   median_depth ; then the side layout of `bow`: u8 desc[32 n], float angle[n], int32 node[n], int32 mp[n], float xy[2 n], int32 octave[n]
// out.bin: int32 status nnew ; per make() call: int32 neighbour idx1 idx2 ; float x3D[3]
static int run_triangulate(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int nkf = R.get<int>(), stereo_kf = R.get<int>(), monocular = R.get<int>();
    const float* scale = R.arr<float>(8); const float* sig = R.arr<float>(8);
    std::vector<MockMapKF> kfs(nkf);
    std::vector<std::vector<MockBowPoint> > pts(nkf);
    for (int k = 0; k < nkf; ++k) {
        MockMapKF& K = kfs[k];
        const int n = R.get<int>();
        const float* Rm = R.arr<float>(9); const float* t = R.arr<float>(3); const float* intr = R.arr<float>(4);
        K.medianDepth = R.get<float>();
        fill_side(R, n, K, pts[k]);
        K.Rcw = cv::Mat(3, 3, CV_32F); K.tcw = mat_from(t, 3);
        float Ow[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) K.Rcw.at<float>(r, c) = Rm[3 * r + c];
            Ow[r] = -((Rm[r] * t[0] + Rm[3 + r] * t[1]) + Rm[6 + r] * t[2]);   // KeyFrame::SetPose: Ow = -Rwc * tcw
        }
        K.Ow = mat_from(Ow, 3);
        K.fx = intr[0]; K.fy = intr[1]; K.cx = intr[2]; K.cy = intr[3]; K.invfx = 1.0f / K.fx; K.invfy = 1.0f / K.fy;
        K.mfScaleFactor = scale[1];
        K.mvScaleFactors.assign(scale, scale + 8); K.mvLevelSigma2.assign(sig, sig + 8);
        if (k == stereo_kf && n > 0) K.mvuRight[0] = K.mvKeysUn[0].pt.x - 3.0f;
    }
    std::vector<MockMapKF*> neigh;
    for (int k = 1; k < nkf; ++k) neigh.push_back(&kfs[k]);
    std::vector<int> rec;
    std::vector<float> xs;
    std::vector<MockBowPoint*> made;
    // what :486-500 does to the two keyframes: the new point sits at idx1 and idx2 from here on
    auto make = [&](const cv::Mat& x3D, int idx1, int idx2, MockMapKF* pKF2) {
        MockBowPoint* p = new MockBowPoint();
        p->id = (int)made.size(); p->bad = false;
        made.push_back(p);
        kfs[0].matches[idx1] = p; pKF2->matches[idx2] = p;
        rec.push_back((int)(pKF2 - &kfs[0]) - 1); rec.push_back(idx1); rec.push_back(idx2);
        for (int r = 0; r < 3; ++r) xs.push_back(x3D.at<float>(r, 0));
    };
    const int nnew = LocalMapping::CreateNewMapPoints(&kfs[0], neigh, monocular != 0, make);
    const int status = LocalMapping::LastStatus();
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nnew, 4, 1, f);
    for (int k = 0; k < nnew; ++k) { fwrite(&rec[3 * k], 4, 3, f); fwrite(&xs[3 * k], 4, 3, f); }
    fclose(f);
    for (size_t k = 0; k < made.size(); ++k) delete made[k];
    return 0;
}

// ---- LocalMapping::CreateNewMapPoints on stereo keyframes -------------------------------------------------------------------------
struct MockStereoMapKF : MockMapKF {   // the four members that choose LocalMapping.h's stereo path
    float mb, mbf;
    std::vector<float> mvDepth;
};
// problem.bin: int32 nkf monocular ; float scale[8] sigma2[8] ; per keyframe: int32 n ; float R[9] t[3] intr[4] median_depth mb mbf ;
//   the side layout of `bow` (xy = mvKeysUn) ; float ur[n] depth[n] raw_xy[2 n] (mvuRight, mvDepth, mvKeys: the distorted keypoints)
// out.bin: as `triangulate`
static int run_triangulate_stereo(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int nkf = R.get<int>(), monocular = R.get<int>();
    const float* scale = R.arr<float>(8); const float* sig = R.arr<float>(8);
    std::vector<MockStereoMapKF> kfs(nkf);
    std::vector<std::vector<MockBowPoint> > pts(nkf);
    for (int k = 0; k < nkf; ++k) {
        MockStereoMapKF& K = kfs[k];
        const int n = R.get<int>();
        const float* Rm = R.arr<float>(9); const float* t = R.arr<float>(3); const float* intr = R.arr<float>(4);
        K.medianDepth = R.get<float>(); K.mb = R.get<float>(); K.mbf = R.get<float>();
        fill_side(R, n, K, pts[k]);
        const float* ur = R.arr<float>(n); const float* depth = R.arr<float>(n); const float* rawxy = R.arr<float>(2 * (size_t)n);
        K.mvuRight.assign(ur, ur + n); K.mvDepth.assign(depth, depth + n);
        for (int i = 0; i < n; ++i) { K.mvKeys[i].pt.x = rawxy[2 * i]; K.mvKeys[i].pt.y = rawxy[2 * i + 1]; }
        K.Rcw = cv::Mat(3, 3, CV_32F); K.tcw = mat_from(t, 3);
        float Ow[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) K.Rcw.at<float>(r, c) = Rm[3 * r + c];
            Ow[r] = -((Rm[r] * t[0] + Rm[3 + r] * t[1]) + Rm[6 + r] * t[2]);   // KeyFrame::SetPose: Ow = -Rwc * tcw
        }
        K.Ow = mat_from(Ow, 3);
        K.fx = intr[0]; K.fy = intr[1]; K.cx = intr[2]; K.cy = intr[3]; K.invfx = 1.0f / K.fx; K.invfy = 1.0f / K.fy;
        K.mfScaleFactor = scale[1];
        K.mvScaleFactors.assign(scale, scale + 8); K.mvLevelSigma2.assign(sig, sig + 8);
    }
    std::vector<MockStereoMapKF*> neigh;
    for (int k = 1; k < nkf; ++k) neigh.push_back(&kfs[k]);
    std::vector<int> rec;
    std::vector<float> xs;
    std::vector<MockBowPoint*> made;
    auto make = [&](const cv::Mat& x3D, int idx1, int idx2, MockStereoMapKF* pKF2) {
        MockBowPoint* p = new MockBowPoint();
        p->id = (int)made.size(); p->bad = false;
        made.push_back(p);
        kfs[0].matches[idx1] = p; pKF2->matches[idx2] = p;
        rec.push_back((int)(pKF2 - &kfs[0]) - 1); rec.push_back(idx1); rec.push_back(idx2);
        for (int r = 0; r < 3; ++r) xs.push_back(x3D.at<float>(r, 0));
    };
    const int nnew = LocalMapping::CreateNewMapPoints(&kfs[0], neigh, monocular != 0, make);
    const int status = LocalMapping::LastStatus();
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nnew, 4, 1, f);
    for (int k = 0; k < nnew; ++k) { fwrite(&rec[3 * k], 4, 3, f); fwrite(&xs[3 * k], 4, 3, f); }
    fclose(f);
    for (size_t k = 0; k < made.size(); ++k) delete made[k];
    return 0;
}

// ---- Tracking::SearchLocalPoints through the template -----------------------------------------------------------------------------
struct MockLocalPoint {   // the members Tracking.h lists on top of the search's
    bool mbTrackInView, bad;
    long unsigned int mnLastFrameSeen;
    int mnTrackScaleLevel, nobs, id, visible;
    float mTrackViewCos, mTrackProjX, mTrackProjXR, mTrackProjY, maxd, mind;
    cv::Mat desc, pos, normal;
    MockLocalPoint() : mbTrackInView(true), bad(false), mnLastFrameSeen(0), mnTrackScaleLevel(-77), nobs(1), id(-1), visible(0), mTrackViewCos(-7.f),
                       mTrackProjX(-7.f), mTrackProjXR(-7.f), mTrackProjY(-7.f), maxd(0.f), mind(0.f) {}
    bool isBad() { return bad; }
    void IncreaseVisible() { ++visible; }
    int Observations() { return nobs; }
    float GetMaxDistance() { return maxd; }
    float GetMinDistance() { return mind; }
    cv::Mat GetDescriptor() { return desc.clone(); }
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetNormal() { return normal.clone(); }
};
struct MockLocalFrame {
    long unsigned int mnId;
    cv::Mat mRcw, mtcw, mOw, mDescriptors;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MockLocalPoint*> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors;
    float fx, fy, cx, cy, mbf, mfLogScaleFactor;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
};
float MockLocalFrame::mnMinX, MockLocalFrame::mnMaxX, MockLocalFrame::mnMinY, MockLocalFrame::mnMaxY;
float MockLocalFrame::mfGridElementWidthInv, MockLocalFrame::mfGridElementHeightInv;

// problem.bin: int32 n ; slamit_frustum_frame ; float pos[3 n] normal[3 n] max_dist[n] min_dist[n] ; u8 skip[n] (0, 1 = bad, 2 = seen in this
//   frame), padded to 4 ; int32 nobs[n] ; u8 desc[32 n] ; int32 nkp ; float nnratio invw invh ; float xy[2 nkp] ; int32 octave[nkp]
//   state[nkp] (0 none, 1 the frame's own point with observations, 2 its own point without, 3 its own BAD point) ; u8 desc[32 nkp]
//   optional tail, a stereo frame: float mvuRight[nkp]
// out.bin: int32 status nmatches ninview ; per local point: int32 inview level visible, float projx projy projxr viewcos ;
//   per keypoint int32 owner (-1 none, -2 / -3 the frame's own point with / without observations, else local index) ;
//   int32 visible of the two own points, int32 their mnLastFrameSeen == mnId
static int run_frustum(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const unsigned char* const end = raw.data() + raw.size();
    const int n = R.get<int>();
    const slamit_frustum_frame fr = R.get<slamit_frustum_frame>();
    const float* pos = R.arr<float>(3 * (size_t)n); const float* nrm = R.arr<float>(3 * (size_t)n);
    const float* maxd = R.arr<float>(n); const float* mind = R.arr<float>(n);
    const unsigned char* skip = R.arr<unsigned char>(n);
    R.p += (4 - n % 4) % 4;
    const int* nobs = R.arr<int>(n);
    const unsigned char* qd = R.arr<unsigned char>(32 * (size_t)n);
    const int nkp = R.get<int>();
    const float nnratio = R.get<float>();
    MockLocalFrame::mfGridElementWidthInv = R.get<float>(); MockLocalFrame::mfGridElementHeightInv = R.get<float>();
    const float* xy = R.arr<float>(2 * (size_t)nkp); const int* oct = R.arr<int>(nkp); const int* state = R.arr<int>(nkp);
    const unsigned char* kd = R.arr<unsigned char>(32 * (size_t)nkp);
    MockLocalFrame F;
    F.mnId = 41;
    MockLocalFrame::mnMinX = fr.min_x; MockLocalFrame::mnMaxX = fr.max_x; MockLocalFrame::mnMinY = fr.min_y; MockLocalFrame::mnMaxY = fr.max_y;
    F.mRcw = cv::Mat(3, 3, CV_32F); F.mtcw = mat_from(fr.tcw, 3); F.mOw = mat_from(fr.Ow, 3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F.mRcw.at<float>(r, c) = fr.Rcw[3 * r + c];
    F.fx = fr.fx; F.fy = fr.fy; F.cx = fr.cx; F.cy = fr.cy; F.mbf = fr.bf; F.mfLogScaleFactor = fr.log_scale_factor;
    F.mvScaleFactors.assign(fr.scale_factors, fr.scale_factors + fr.n_levels);
    F.mDescriptors = cv::Mat(nkp, 32, CV_8U);
    F.mvKeysUn.resize(nkp); F.mvuRight.assign(nkp, -1.f); F.mvpMapPoints.assign(nkp, (MockLocalPoint*)0);
    MockLocalPoint own1, own2, ownBad;
    own1.nobs = 3; own1.id = -2; own2.nobs = 0; own2.id = -3; ownBad.bad = true; ownBad.id = -4;
    for (int i = 0; i < nkp; ++i) {
        F.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f, -1.f, 0, oct[i]);
        memcpy(F.mDescriptors.ptr(i), kd + 32 * (size_t)i, 32);
        if (state[i] == 1) F.mvpMapPoints[i] = &own1;
        if (state[i] == 2) F.mvpMapPoints[i] = &own2;
        if (state[i] == 3) F.mvpMapPoints[i] = &ownBad;
    }
    if (R.p < end) {
        const float* ur = R.arr<float>(nkp);
        F.mvuRight.assign(ur, ur + nkp);
    }
    std::vector<MockLocalPoint> mps(n);
    std::vector<MockLocalPoint*> local(n);
    for (int i = 0; i < n; ++i) {
        MockLocalPoint& p = mps[i];
        p.id = i; p.bad = skip[i] == 1; p.mnLastFrameSeen = skip[i] == 2 ? F.mnId : 7; p.nobs = nobs[i]; p.maxd = maxd[i]; p.mind = mind[i];
        // A point seen in this frame is one of the frame's own, and the loop over those has already cleared its flag (Tracking.cc:1426); a bad
        // point keeps a stale `true`, which the search must get past by isBad() alone.  Every other point starts `true` too: isInFrustum clears it.
        if (skip[i] == 2) p.mbTrackInView = false;
        p.pos = mat_from(pos + 3 * (size_t)i, 3); p.normal = mat_from(nrm + 3 * (size_t)i, 3);
        p.desc = cv::Mat(1, 32, CV_8U); memcpy(p.desc.ptr(0), qd + 32 * (size_t)i, 32);
        local[i] = &p;
    }
    const int nm = Tracking::SearchLocalPoints(F, local, (int)fr.th, nnratio);
    const int status = Tracking::LastStatus(), ninview = Tracking::LastInView();
    if (status != 0) fprintf(stderr, "frustum failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f); fwrite(&nm, 4, 1, f); fwrite(&ninview, 4, 1, f);
    for (int i = 0; i < n; ++i) {
        const MockLocalPoint& p = mps[i];
        const int a[3] = {p.mbTrackInView ? 1 : 0, p.mnTrackScaleLevel, p.visible};
        const float b[4] = {p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR, p.mTrackViewCos};
        fwrite(a, 4, 3, f); fwrite(b, 4, 4, f);
    }
    for (int i = 0; i < nkp; ++i) { int o = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->id : -1; fwrite(&o, 4, 1, f); }
    const int tail[4] = {own1.visible, own2.visible, own1.mnLastFrameSeen == F.mnId, own2.mnLastFrameSeen == F.mnId};
    fwrite(tail, 4, 4, f);
    fclose(f);
    return 0;
}

// Frame::ComputeStereoMatches through FrameOps.h: a mock Frame with the members the reference's has, two shim extractors, no pyramid export.
// pair.bin: int32 w h nfeatures nlevels ; float mb mbf ; u8 left[w h] right[w h]
// out.bin: int32 status nL nR ; cv::KeyPoint left[nL] ; u8 desc[32 nL] ; cv::KeyPoint right[nR] ; u8 desc[32 nR] ; float mvuRight[nL] mvDepth[nL] ;
//   u8 status[nL]
struct MockStereoFrame {
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    cv::Mat mDescriptors, mDescriptorsRight;
    float mb, mbf;
    ORBextractor* mpORBextractorLeft;
    ORBextractor* mpORBextractorRight;
    std::vector<float> mvuRight, mvDepth;
};

static int run_stereo(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int w = R.get<int>(), h = R.get<int>(), nfeatures = R.get<int>(), nlevels = R.get<int>();
    MockStereoFrame F;
    F.mb = R.get<float>(); F.mbf = R.get<float>();
    if (raw.size() != 24 + 2 * (size_t)w * h) return 2;
    cv::Mat imL(h, w, CV_8UC1, (void*)R.arr<unsigned char>((size_t)w * h)), imR(h, w, CV_8UC1, (void*)R.arr<unsigned char>((size_t)w * h));
    ORBextractor left(nfeatures, 1.2f, nlevels, 20, 7), right(nfeatures, 1.2f, nlevels, 20, 7);   // Tracking.cc:149-159
    F.mpORBextractorLeft = &left; F.mpORBextractorRight = &right;
    left(imL, cv::Mat(), F.mvKeys, F.mDescriptors);                                                // Frame.cc:93-96, without the threads
    right(imR, cv::Mat(), F.mvKeysRight, F.mDescriptorsRight);
    if (!left.ok() || !right.ok()) { fprintf(stderr, "extract failed: %s\n", left.lastError()); return 1; }
    std::vector<uint8_t> st;
    FrameOps::ComputeStereoMatches(F, &st);
    const int status = FrameOps::LastStatus(), nL = (int)F.mvKeys.size(), nR = (int)F.mvKeysRight.size();
    if (status != 0) fprintf(stderr, "stereo failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    fwrite(&status, 4, 1, f); fwrite(&nL, 4, 1, f); fwrite(&nR, 4, 1, f);
    if (nL) fwrite(&F.mvKeys[0], sizeof(cv::KeyPoint), nL, f);
    for (int i = 0; i < nL; ++i) fwrite(F.mDescriptors.ptr(i), 1, 32, f);
    if (nR) fwrite(&F.mvKeysRight[0], sizeof(cv::KeyPoint), nR, f);
    for (int i = 0; i < nR; ++i) fwrite(F.mDescriptorsRight.ptr(i), 1, 32, f);
    fwrite(F.mvuRight.data(), 4, nL, f); fwrite(F.mvDepth.data(), 4, nL, f); fwrite(st.data(), 1, nL, f);
    fclose(f);
    return 0;
}

// ---- Initializer through the template: a batch of frame pairs in one InitializeAll (two launches), then one Initialize each --------
// pairs.bin: int32 npairs nrand ; uint32 rand[nrand] (one RandomInt stream, read from its start by each of the two passes) ; per pair:
//   int32 n1 n2 iterations ; float sigma K[9] keys1[2 n1] keys2[2 n2] ; int32 vMatches12[n1]
// out.bin: int32 status ; two passes (InitializeAll, then Initialize pair by pair), each per pair: int32 ok kind motion nsets ;
//   float R21[9] t21[3] (zeros when empty) vP3D[3 n1] ; u8 vbTriangulated[n1] (zeros when empty) ; int32 sets[8 nsets]
struct MockInitFrame {
    cv::Mat mK;
    std::vector<cv::KeyPoint> mvKeysUn;
};
static int run_initializer(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int np = Rd.get<int>(), nrand = Rd.get<int>();
    { const uint32_t* r = Rd.arr<uint32_t>(nrand); g_script.assign(r, r + nrand); g_script_pos = 0; }
    shim::RandomInt() = scripted_random_int;
    typedef Initializer<MockInitFrame> Init;
    std::vector<MockInitFrame> ref(np), cur(np);
    std::vector<std::vector<int> > vm(np);
    std::vector<int> its(np);
    std::vector<float> sigma(np);
    for (int k = 0; k < np; ++k) {
        const int n1 = Rd.get<int>(), n2 = Rd.get<int>();
        its[k] = Rd.get<int>(); sigma[k] = Rd.get<float>();
        const float* K = Rd.arr<float>(9);
        const float* k1 = Rd.arr<float>(2 * (size_t)n1);
        const float* k2 = Rd.arr<float>(2 * (size_t)n2);
        const int32_t* m = Rd.arr<int32_t>(n1);
        ref[k].mK.create(3, 3, CV_32F);
        for (int i = 0; i < 9; ++i) ref[k].mK.at<float>(i / 3, i % 3) = K[i];
        cur[k].mK = ref[k].mK;
        for (int i = 0; i < n1; ++i) ref[k].mvKeysUn.push_back(cv::KeyPoint(k1[2 * i], k1[2 * i + 1], 31.f));
        for (int i = 0; i < n2; ++i) cur[k].mvKeysUn.push_back(cv::KeyPoint(k2[2 * i], k2[2 * i + 1], 31.f));
        vm[k].assign(m, m + n1);
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    int status = 0;
    fwrite(&status, 4, 1, f);
    for (int pass = 0; pass < 2 && status == 0; ++pass) {
        g_script_pos = 0;
        std::vector<Init*> inits;
        std::vector<Init::Job> jobs;
        for (int k = 0; k < np; ++k) inits.push_back(new Init(ref[k], sigma[k], its[k]));
        for (int k = 0; k < np; ++k) jobs.push_back(Init::Job(inits[k], cur[k], vm[k]));
        if (pass == 0) {
            status = Init::InitializeAll(jobs);
        } else {
            for (int k = 0; k < np && status == 0; ++k) {
                jobs[k].ok = inits[k]->Initialize(cur[k], vm[k], jobs[k].R21, jobs[k].t21, jobs[k].vP3D, jobs[k].vbTriangulated);
                status = Init::LastStatus();
            }
        }
        if (status != 0) fprintf(stderr, "initializer failed: %s\n", slamit_last_error());
        for (int k = 0; k < np && status == 0; ++k) {
            const Init::Job& J = jobs[k];
            const int n1 = (int)ref[k].mvKeysUn.size();
            const int head[4] = {J.ok ? 1 : 0, inits[k]->Kind(), inits[k]->Motion(), (int)(inits[k]->Sets().size() / 8)};
            fwrite(head, 4, 4, f);
            float rt[12] = {0};
            if (!J.R21.empty()) for (int i = 0; i < 9; ++i) rt[i] = J.R21.at<float>(i / 3, i % 3);
            if (!J.t21.empty()) for (int i = 0; i < 3; ++i) rt[9 + i] = J.t21.at<float>(i, 0);
            fwrite(rt, 4, 12, f);
            std::vector<float> p(3 * (size_t)n1, 0.f);
            std::vector<unsigned char> vb(n1, 0);
            for (size_t i = 0; i < J.vP3D.size(); ++i) { p[3 * i] = J.vP3D[i].x; p[3 * i + 1] = J.vP3D[i].y; p[3 * i + 2] = J.vP3D[i].z; }
            for (size_t i = 0; i < J.vbTriangulated.size(); ++i) vb[i] = J.vbTriangulated[i] ? 1 : 0;
            fwrite(p.data(), 4, p.size(), f); fwrite(vb.data(), 1, vb.size(), f);
            fwrite(inits[k]->Sets().data(), 4, inits[k]->Sets().size(), f);
        }
        for (int k = 0; k < np; ++k) delete inits[k];
    }
    fseek(f, 0, SEEK_SET);
    fwrite(&status, 4, 1, f);
    fclose(f);
    return 0;
}

// ---- PnPsolver through the template: the candidates of one relocalisation, one EvaluateAll (two launches) -------------------------
// problem.bin: int32 nsolvers nrand ; uint32 rand[nrand] (one RandomInt stream for all solvers in order; the constructors draw
//   nothing) ; per solver: int32 n lead min_inliers max_its min_set ; float epsilon th2 K[4] p3d[3n] p2d[2n] sigma2[n]
//   (the frame holds `lead` keypoints without a map point in front of the n matched ones)
// out.bin: int32 status ; per solver: int32 set_status accepted n_inliers ncalls max_its min_inliers no_more ; float Tcw[16] (zeros
//   for an empty matrix) ; u8 vbInliers[lead + n] (zeros where iterate() left the vector empty)
struct MockPnpFrame {
    float fx, fy, cx, cy;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
};
static int run_pnpsolver(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int ns = Rd.get<int>(), nrand = Rd.get<int>();
    { const uint32_t* r = Rd.arr<uint32_t>(nrand); g_script.assign(r, r + nrand); g_script_pos = 0; }
    pnpsolver::RandomInt() = scripted_random_int;
    typedef PnPsolver<MockPnpFrame, MockFusePoint> Solver;
    std::vector<MockPnpFrame> frames(ns);
    std::vector<std::vector<MockFusePoint> > pts(ns);
    std::vector<Solver*> solvers;
    std::vector<int> total(ns), set_status(ns);
    for (int k = 0; k < ns; ++k) {
        const int n = Rd.get<int>(), ld = Rd.get<int>(), minInl = Rd.get<int>(), maxIts = Rd.get<int>(), minSet = Rd.get<int>();
        const float eps = Rd.get<float>(), th2 = Rd.get<float>();
        const float* K = Rd.arr<float>(4);
        const float* p3d = Rd.arr<float>(3 * (size_t)n);
        const float* p2d = Rd.arr<float>(2 * (size_t)n);
        const float* sg = Rd.arr<float>(n);
        total[k] = ld + n;
        MockPnpFrame& F = frames[k];
        F.fx = K[0]; F.fy = K[1]; F.cx = K[2]; F.cy = K[3];
        F.mvKeysUn.resize(ld + n); F.mvLevelSigma2.assign(sg, sg + n);
        pts[k].resize(n);
        std::vector<MockFusePoint*> vpMapPointMatches(ld + n, (MockFusePoint*)0);
        for (int i = 0; i < n; ++i) {
            MockFusePoint& p = pts[k][i];
            p.id = i; p.pos = mat_from(p3d + 3 * (size_t)i, 3);
            F.mvKeysUn[ld + i] = cv::KeyPoint(p2d[2 * i], p2d[2 * i + 1], 31.f, -1.f, 0, i);   // one sigma entry per keypoint keeps sigma2 exact
            vpMapPointMatches[ld + i] = &p;
        }
        Solver* s = new Solver(F, vpMapPointMatches);
        set_status[k] = s->SetRansacParameters(0.99, minInl, maxIts, minSet, eps, th2);   // Tracking.cc:1723
        solvers.push_back(s);
    }
    int status = Solver::EvaluateAll(solvers);   // every candidate: one hypothesis launch, one refine launch
    if (status != 0) fprintf(stderr, "pnpsolver failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f);
    for (int k = 0; k < ns && status == 0; ++k) {
        Solver* s = solvers[k];
        std::vector<bool> vbInliers;
        int nInliers = 0, ncalls = 0;
        bool bNoMore = false;
        cv::Mat T;
        while (T.empty() && !bNoMore && ncalls < 4) {   // Tracking.cc:1740-1760: iterate(5) until a pose or bNoMore
            T = s->iterate(5, bNoMore, vbInliers, nInliers);
            ++ncalls;
        }
        const int acc = s->AcceptedHypothesis(), its = s->GetRansacMaxIts(), mi = s->GetRansacMinInliers(), nm = bNoMore ? 1 : 0;
        fwrite(&set_status[k], 4, 1, f); fwrite(&acc, 4, 1, f); fwrite(&nInliers, 4, 1, f); fwrite(&ncalls, 4, 1, f);
        fwrite(&its, 4, 1, f); fwrite(&mi, 4, 1, f); fwrite(&nm, 4, 1, f);
        float t16[16] = {0};
        if (!T.empty()) for (int i = 0; i < 16; ++i) t16[i] = T.at<float>(i / 4, i % 4);
        fwrite(t16, 4, 16, f);
        for (int i = 0; i < total[k]; ++i) { const unsigned char b = i < (int)vbInliers.size() && vbInliers[i] ? 1 : 0; fwrite(&b, 1, 1, f); }
        printf("solver %d: %s hypothesis %d, %d inliers, %d call(s)\n", k, T.empty() ? "no pose," : "pose from", acc, nInliers, ncalls);
    }
    fclose(f);
    for (size_t k = 0; k < solvers.size(); ++k) delete solvers[k];
    return status;
}

// ---- the closest-point walks of a stereo / RGB-D frame through Tracking.h, and ComputeStereoFromRGBD through FrameOps.h -----------
static int g_unp_seq = 0;
struct MockDepthKF;
struct MockDepthPoint {
    int id, nobs, seq[5];   // seq: the order of AddObservation, KeyFrame::AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Map::AddMapPoint
    float pos[3], normal[3], maxd, mind;
    MockDepthPoint() : id(-1), nobs(0), maxd(0.f), mind(0.f) { for (int k = 0; k < 5; ++k) seq[k] = -1; }
    int Observations() { return nobs; }
    void AddObservation(MockDepthKF*, size_t) { ++nobs; seq[0] = g_unp_seq++; }
    void ComputeDistinctiveDescriptors() { seq[2] = g_unp_seq++; }
    void UpdateNormalAndDepth() { seq[3] = g_unp_seq++; }
};
struct MockDepthKF {
    std::vector<MockDepthPoint*> pts;
    void AddMapPoint(MockDepthPoint* p, size_t i) { pts[i] = p; p->seq[1] = g_unp_seq++; }
};
struct MockDepthMap {
    std::vector<MockDepthPoint*> pts;
    void AddMapPoint(MockDepthPoint* p) { pts.push_back(p); p->seq[4] = g_unp_seq++; }
};
struct MockDepthFrame {
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth, mvScaleFactors;
    std::vector<MockDepthPoint*> mvpMapPoints;
    cv::Mat mRwc, mOw;
    float fx, fy, cx, cy, invfx, invfy, mbf;
};
struct MockMonoFrame {   // no mbf, no mvDepth: FrameOps::ComputeStereoFromRGBD refuses it
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight;
};

// problem.bin: int32 variant ;
//   variant 0 UpdateLastFrame, 1 CreateNewKeyFramePoints, 2 StereoInitializationPoints: int32 n ; slamit_unproject_frame ;
//     cv::KeyPoint kps_un[n] ; float depth[n] ; u8 state[n] (0 no point, 1 a point with observations, 2 a point without)
//   out.bin: int32 status made close_ok nmap ntotal ; int32 counts[6] ; int32 ncreated ; per created point, in the order of creation:
//     int32 id keypoint seq[5], float pos[3] normal[3] maxd mind ; per keypoint int32 owner (-1 none, -2 / -3 the frame's own point
//     with / without observations, else the new point's id) ; int32 temporal size, keyframe points, map points
//   variant 3 ComputeStereoFromRGBD: int32 n w h type ; float factor mbf ; cv::KeyPoint kps[n] kps_un[n] ; float plane[w h]
//   out.bin: int32 status refused_status ; float mvuRight[n] mvDepth[n] ; u8 status[n]
static int run_unproject(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader R{raw.data()};
    const int variant = R.get<int>();
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    if (variant == 3) {
        const int n = R.get<int>(), w = R.get<int>(), h = R.get<int>(), type = R.get<int>();
        const float factor = R.get<float>();
        MockDepthFrame F;
        F.mbf = R.get<float>();
        const cv::KeyPoint* kps = R.arr<cv::KeyPoint>(n); const cv::KeyPoint* kun = R.arr<cv::KeyPoint>(n);
        if (type != 0) return 2;   // cvlite holds bytes and floats
        cv::Mat im(h, w, CV_32F, (void*)R.arr<float>((size_t)w * h));
        F.mvKeys.assign(kps, kps + n); F.mvKeysUn.assign(kun, kun + n);
        std::vector<uint8_t> st;
        FrameOps::ComputeStereoFromRGBD(F, im, factor, &st);
        const int status = FrameOps::LastStatus();
        if (status != 0) fprintf(stderr, "rgbd failed: %s\n", slamit_last_error());
        MockMonoFrame M;
        M.mvKeys = F.mvKeys; M.mvKeysUn = F.mvKeysUn;
        FrameOps::ComputeStereoFromRGBD(M, im);
        const int refused = FrameOps::LastStatus();
        fwrite(&status, 4, 1, f); fwrite(&refused, 4, 1, f);
        fwrite(F.mvuRight.data(), 4, n, f); fwrite(F.mvDepth.data(), 4, n, f); fwrite(st.data(), 1, n, f);
        fclose(f);
        return 0;
    }
    const int n = R.get<int>();
    const slamit_unproject_frame fr = R.get<slamit_unproject_frame>();
    const cv::KeyPoint* kun = R.arr<cv::KeyPoint>(n);
    const float* depth = R.arr<float>(n);
    const unsigned char* state = R.arr<unsigned char>(n);
    MockDepthFrame F;
    F.mvKeysUn.assign(kun, kun + n); F.mvDepth.assign(depth, depth + n);
    F.mvScaleFactors.assign(fr.scale_factors, fr.scale_factors + fr.n_levels);
    F.mRwc = cv::Mat(3, 3, CV_32F); F.mOw = mat_from(fr.Ow, 3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F.mRwc.at<float>(r, c) = fr.Rwc[3 * r + c];
    F.fx = fr.fx; F.fy = fr.fy; F.cx = fr.cx; F.cy = fr.cy; F.invfx = fr.invfx; F.invfy = fr.invfy; F.mbf = 0.f;
    MockDepthPoint own1, own2;
    own1.nobs = 3; own1.id = -2; own2.nobs = 0; own2.id = -3;
    F.mvpMapPoints.assign(n, (MockDepthPoint*)0);
    for (int i = 0; i < n; ++i) F.mvpMapPoints[i] = state[i] == 1 ? &own1 : state[i] == 2 ? &own2 : (MockDepthPoint*)0;
    std::vector<MockDepthPoint*> temporal, created;
    std::vector<int> created_at;
    MockDepthKF KF;
    KF.pts.assign(n, (MockDepthPoint*)0);
    MockDepthMap map;
    int next_id = 1000;
    auto make = [&](const cv::Mat& x3D, int i, const float* normal, float maxd, float mind) {
        MockDepthPoint* p = new MockDepthPoint();
        p->id = next_id++;   // MapPoint::nNextId: the order of creation
        for (int r = 0; r < 3; ++r) { p->pos[r] = x3D.at<float>(r, 0); p->normal[r] = normal[r]; }
        p->maxd = maxd; p->mind = mind;
        created.push_back(p); created_at.push_back(i);
        return p;
    };
    int made = 0;
    if (variant == 0) made = Tracking::UpdateLastFrame(F, fr.th_depth, temporal, make);
    else if (variant == 1) made = Tracking::CreateNewKeyFramePoints(F, &KF, &map, fr.th_depth, make);
    else made = Tracking::StereoInitializationPoints(F, &KF, &map, make);
    const int status = Tracking::LastStatus();
    if (status != 0) fprintf(stderr, "unproject failed: %s\n", slamit_last_error());
    const slamit_unproject_counts cn = Tracking::LastCounts();
    // NeedNewKeyFrame's counts on the frame as the walk found it
    MockDepthFrame G = F;
    for (int i = 0; i < n; ++i) G.mvpMapPoints[i] = state[i] == 1 ? &own1 : state[i] == 2 ? &own2 : (MockDepthPoint*)0;
    int nmap = -1, ntotal = -1;
    const int close_ok = Tracking::CloseRatio(G, fr.th_depth, nmap, ntotal) ? 1 : 0;
    const int head[5] = {status, made, close_ok, nmap, ntotal};
    fwrite(head, 4, 5, f); fwrite(&cn, 4, 6, f);
    const int nc = (int)created.size();
    fwrite(&nc, 4, 1, f);
    for (int k = 0; k < nc; ++k) {
        const MockDepthPoint& p = *created[k];
        fwrite(&p.id, 4, 1, f); fwrite(&created_at[k], 4, 1, f); fwrite(p.seq, 4, 5, f);
        fwrite(p.pos, 4, 3, f); fwrite(p.normal, 4, 3, f); fwrite(&p.maxd, 4, 1, f); fwrite(&p.mind, 4, 1, f);
    }
    for (int i = 0; i < n; ++i) { const int o = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->id : -1; fwrite(&o, 4, 1, f); }
    int nkf = 0;
    for (int i = 0; i < n; ++i) nkf += KF.pts[i] ? 1 : 0;
    const int tail[3] = {(int)temporal.size(), nkf, (int)map.pts.size()};
    fwrite(tail, 4, 3, f);
    fclose(f);
    for (size_t k = 0; k < created.size(); ++k) delete created[k];
    return 0;
}

// ---- local_map: Tracking::UpdateLocalMap over mock types whose addresses are NOT in creation order ------------------------------
struct MockLmKF;
struct MockLmPoint {
    bool bad;
    std::map<MockLmKF*, size_t> obs;
    long unsigned int mnTrackReferenceForFrame;
    MockLmPoint() : bad(false), mnTrackReferenceForFrame(0) {}
    bool isBad() const { return bad; }
    std::map<MockLmKF*, size_t> GetObservations() const { return obs; }
};
struct MockLmKF {
    bool bad;
    std::vector<MockLmPoint*> pts;
    std::vector<MockLmKF*> ordered;
    std::set<MockLmKF*> childs;
    MockLmKF* parent;
    long unsigned int mnTrackReferenceForFrame;
    MockLmKF() : bad(false), parent(NULL), mnTrackReferenceForFrame(0) {}
    bool isBad() const { return bad; }
    std::vector<MockLmPoint*> GetMapPointMatches() const { return pts; }
    std::vector<MockLmKF*> GetBestCovisibilityKeyFrames(int n) const {
        return (int)ordered.size() < n ? ordered : std::vector<MockLmKF*>(ordered.begin(), ordered.begin() + n);
    }
    std::set<MockLmKF*> GetChilds() const { return childs; }
    MockLmKF* GetParent() const { return parent; }
};
struct MockLmFrame {
    long unsigned int mnId;
    std::vector<MockLmPoint*> mvpMapPoints;
    MockLmKF* mpReferenceKF;
};

// The host loops the shim stands in for, over the same mock types: votes per observer in a std::map, the voted keyframes in the map's
// order, one neighbour, one child and the parent per visited keyframe, then the keyframes' points once each.
static void plain_update_local_map(MockLmFrame& F, std::vector<MockLmKF*>& localKFs, std::vector<MockLmPoint*>& localMPs, MockLmKF*& refKF) {
    std::map<MockLmKF*, int> counter;
    for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {
        MockLmPoint* p = F.mvpMapPoints[i];
        if (!p) continue;
        if (p->isBad()) { F.mvpMapPoints[i] = NULL; continue; }
        const std::map<MockLmKF*, size_t> obs = p->GetObservations();
        for (std::map<MockLmKF*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) counter[it->first]++;
    }
    if (!counter.empty()) {
        int best = 0;
        MockLmKF* bestKF = NULL;
        localKFs.clear();
        for (std::map<MockLmKF*, int>::const_iterator it = counter.begin(); it != counter.end(); ++it) {
            if (it->first->isBad()) continue;
            if (it->second > best) { best = it->second; bestKF = it->first; }
            localKFs.push_back(it->first);
            it->first->mnTrackReferenceForFrame = F.mnId;
        }
        const size_t voted = localKFs.size();
        for (size_t v = 0; v < voted; ++v) {
            if (localKFs.size() > 80) break;
            MockLmKF* kf = localKFs[v];
            const std::vector<MockLmKF*> neigh = kf->GetBestCovisibilityKeyFrames(10);
            for (size_t j = 0; j < neigh.size(); ++j)
                if (!neigh[j]->isBad() && neigh[j]->mnTrackReferenceForFrame != F.mnId) {
                    localKFs.push_back(neigh[j]);
                    neigh[j]->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            const std::set<MockLmKF*> childs = kf->GetChilds();
            for (std::set<MockLmKF*>::const_iterator c = childs.begin(); c != childs.end(); ++c)
                if (!(*c)->isBad() && (*c)->mnTrackReferenceForFrame != F.mnId) {
                    localKFs.push_back(*c);
                    (*c)->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            MockLmKF* parent = kf->GetParent();
            if (parent && parent->mnTrackReferenceForFrame != F.mnId) {
                localKFs.push_back(parent);
                parent->mnTrackReferenceForFrame = F.mnId;
                break;
            }
        }
        if (bestKF) { refKF = bestKF; F.mpReferenceKF = bestKF; }
    }
    localMPs.clear();
    for (size_t k = 0; k < localKFs.size(); ++k) {
        const std::vector<MockLmPoint*> pts = localKFs[k]->GetMapPointMatches();
        for (size_t i = 0; i < pts.size(); ++i) {
            MockLmPoint* p = pts[i];
            if (!p || p->mnTrackReferenceForFrame == F.mnId || p->isBad()) continue;
            localMPs.push_back(p);
            p->mnTrackReferenceForFrame = F.mnId;
        }
    }
}

//     shim_test local_map <seed> <keyframes> <points> <keypoints>
// Three scenarios on one generated map (a frame with observers, one whose points nobody observes, one whose observers are all bad);
// each runs the plain loops and Tracking::UpdateLocalMap from the same state and prints one line ending in MATCH or MISMATCH.
static int run_local_map(int argc, char** argv) {
    if (argc != 6) return 2;
    unsigned long long rng = 0x9e3779b97f4a7c15ULL ^ (unsigned long long)atoll(argv[2]);
    const int K = atoi(argv[3]), NP = atoi(argv[4]), NKP = atoi(argv[5]);
    if (K < 4 || NP < 2 * K || NKP < 1) return 2;
    struct Rand {
        unsigned long long& s;
        unsigned next(unsigned mod) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(s >> 33) % mod; }
    } R = {rng};
    std::vector<MockLmKF> kfPool(K);
    std::vector<MockLmPoint> mpPool(NP + 8);   // the last 8 are in no keyframe
    std::vector<int> perm(K);
    for (int i = 0; i < K; ++i) perm[i] = i;
    for (int i = K - 1; i > 0; --i) std::swap(perm[i], perm[R.next(i + 1)]);   // creation order i lives at address perm[i]
    std::vector<MockLmKF*> kf(K);
    for (int i = 0; i < K; ++i) kf[i] = &kfPool[perm[i]];
    const int width = 3 * NP / K + 4;
    for (int i = 0; i < K; ++i) {
        const int lo = (int)((long long)i * (NP - width) / (K - 1));
        kf[i]->bad = R.next(10) == 0;
        kf[i]->pts.assign(width + 10, (MockLmPoint*)NULL);
        for (int j = 0; j < width; ++j) {
            if (R.next(5) == 0) continue;
            MockLmPoint* p = &mpPool[lo + j];
            const size_t at = R.next(width + 10);
            if (kf[i]->pts[at]) continue;
            kf[i]->pts[at] = p;
            p->obs[kf[i]] = at;
        }
        if (i > 0) { kf[i]->parent = kf[R.next(3) == 0 && i > 1 ? i - 2 : i - 1]; kf[i]->parent->childs.insert(kf[i]); }
    }
    for (int p = 0; p < NP; ++p) mpPool[p].bad = R.next(20) == 0;
    for (int i = 0; i < K; ++i) {   // neighbours by shared points, the strongest first
        std::map<MockLmKF*, int> w;
        for (size_t j = 0; j < kf[i]->pts.size(); ++j)
            if (kf[i]->pts[j])
                for (std::map<MockLmKF*, size_t>::const_iterator it = kf[i]->pts[j]->obs.begin(); it != kf[i]->pts[j]->obs.end(); ++it)
                    if (it->first != kf[i]) w[it->first]++;
        std::vector<std::pair<int, MockLmKF*> > order;
        for (std::map<MockLmKF*, int>::const_iterator it = w.begin(); it != w.end(); ++it) order.push_back(std::make_pair(-it->second, it->first));
        std::sort(order.begin(), order.end());
        for (size_t j = 0; j < order.size(); ++j) kf[i]->ordered.push_back(order[j].second);
    }
    bool shuffled = false;
    for (int i = 1; i < K; ++i) shuffled = shuffled || kf[i] < kf[i - 1];
    printf("local_map keyframes=%d points=%d addresses_shuffled=%d\n", K, NP, shuffled ? 1 : 0);
    int failures = 0;
    for (int scenario = 0; scenario < 3; ++scenario) {
        std::vector<bool> wasBad(K);
        for (int i = 0; i < K; ++i) wasBad[i] = kf[i]->bad;
        std::vector<MockLmPoint*> tracked(NKP, (MockLmPoint*)NULL);
        const int lo = NP / 3;
        for (int i = 0; i < NKP; ++i) {
            if (R.next(3) == 0) continue;
            tracked[i] = scenario == 1 ? &mpPool[NP + R.next(8)] : &mpPool[lo + R.next(NP / 4)];
        }
        if (scenario == 2)
            for (int i = 0; i < NKP; ++i)
                if (tracked[i])
                    for (std::map<MockLmKF*, size_t>::const_iterator it = tracked[i]->obs.begin(); it != tracked[i]->obs.end(); ++it) it->first->bad = true;
        const std::vector<MockLmKF*> startKFs(1, kf[K / 2]);
        MockLmKF* const startRef = kf[K / 2];
        // the plain loops
        MockLmFrame FA = {100ul + 2 * scenario, tracked, NULL};
        std::vector<MockLmKF*> kfsA = startKFs;
        std::vector<MockLmPoint*> mpsA;
        MockLmKF* refA = startRef;
        plain_update_local_map(FA, kfsA, mpsA, refA);
        // the shim, from the same state under another frame id
        MockLmFrame FB = {101ul + 2 * scenario, tracked, NULL};
        std::vector<MockLmKF*> kfsB = startKFs;
        std::vector<MockLmPoint*> mpsB;
        MockLmKF* refB = startRef;
        const int nB = Tracking::UpdateLocalMap(FB, kfsB, mpsB, refB);
        const int status = Tracking::LastStatus();
        if (status != 0) fprintf(stderr, "local_map failed: %s\n", slamit_last_error());
        bool marks = true;
        for (int i = 0; i < K; ++i) marks = marks && ((kf[i]->mnTrackReferenceForFrame == FB.mnId) == (std::find(kfsB.begin(), kfsB.end(), kf[i]) != kfsB.end() && (scenario != 1)));
        for (int p = 0; p < NP + 8; ++p)
            marks = marks && ((mpPool[p].mnTrackReferenceForFrame == FB.mnId) == (std::find(mpsB.begin(), mpsB.end(), &mpPool[p]) != mpsB.end()));
        const bool same = status == 0 && kfsA == kfsB && mpsA == mpsB && refA == refB && FA.mvpMapPoints == FB.mvpMapPoints && FA.mpReferenceKF == FB.mpReferenceKF &&
                          nB == (int)mpsA.size() && marks;
        int refSlot = -1;
        for (int i = 0; i < K; ++i) refSlot = kf[i] == refB ? i : refSlot;
        printf("local_map scenario %d: status=%d kfs=%zu mps=%zu ref=%d frame_ref_set=%d %s\n", scenario, status, kfsB.size(), mpsB.size(), refSlot,
               FB.mpReferenceKF ? 1 : 0, same ? "MATCH" : "MISMATCH");
        failures += same ? 0 : 1;
        for (int i = 0; i < K; ++i) kf[i]->bad = wasBad[i];
    }
    return failures ? 1 : 0;
}

// ---- Optimizer::OptimizeEssentialGraph through the class surface ----
struct MockEgKF {
    long unsigned int mnId; bool bad; cv::Mat R, t, pose; bool poseSet;
    MockEgKF* parent; std::set<MockEgKF*> children, loopEdges; std::vector<MockEgKF*> ordered; std::vector<int> weights;
    bool isBad() { return bad; }
    cv::Mat GetRotation() { return R; }
    cv::Mat GetTranslation() { return t; }
    MockEgKF* GetParent() { return parent; }
    std::set<MockEgKF*> GetChilds() { return children; }
    std::set<MockEgKF*> GetLoopEdges() { return loopEdges; }
    std::vector<MockEgKF*> GetVectorCovisibleKeyFrames() { return ordered; }
    int GetWeight(MockEgKF* k) { for (size_t i = 0; i < ordered.size(); ++i) if (ordered[i] == k) return weights[i]; return 0; }
    void SetPose(const cv::Mat& T) { pose = T.clone(); poseSet = true; }
};
struct MockEgPoint {
    bool bad; cv::Mat pos; long unsigned int mnCorrectedByKF, mnCorrectedReference; MockEgKF* ref; int updated;
    bool isBad() { return bad; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    void SetWorldPos(const cv::Mat& X) { pos = X.clone(); }
    MockEgKF* GetReferenceKeyFrame() { return ref; }
    void UpdateNormalAndDepth() { ++updated; }
};
struct MockEgMap {
    std::vector<MockEgKF*> kfs; std::vector<MockEgPoint*> pts; std::mutex mMutexMapUpdate;
    std::vector<MockEgKF*> GetAllKeyFrames() { return std::vector<MockEgKF*>(kfs.rbegin(), kfs.rend()); }   // (no order promised)
    std::vector<MockEgPoint*> GetAllMapPoints() { return pts; }
};
// problem.bin: int32 n m loop cur fix row_cap ; int32 bad[n] id[n] parent[n] ; CSRs as int32 ptr[n + 1] + values: children, loop edges,
//   LoopConnections ; int32 ord_n[n] ord_kf[n row_cap] ord_w[n row_cap] ; double scw[13 n] snc[13 n] (R, t, s) ; int32 corrected[n] (the
//   keyframe is a key of CorrectedSim3 / NonCorrectedSim3) ; float pos[3 m] ; int32 pt_bad[m] pt_ref[m] pt_by_cur[m]
// out.bin: int32 status ; per keyframe int32 pose_set, float pose[12] (R row-major, t) ; per point float pos[3], int32 updated
static int run_essential(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> raw = slurp(argv[2]);
    Reader Rd{raw.data()};
    const int n = Rd.get<int>(), m = Rd.get<int>(), loop = Rd.get<int>(), cur = Rd.get<int>(), fix = Rd.get<int>(), cap = Rd.get<int>();
    const int* bad = Rd.arr<int>(n); const int* id = Rd.arr<int>(n); const int* par = Rd.arr<int>(n);
    const int* cp = Rd.arr<int>(n + 1); const int* ck = Rd.arr<int>(cp[n]);
    const int* lp = Rd.arr<int>(n + 1); const int* lk = Rd.arr<int>(lp[n]);
    const int* qp = Rd.arr<int>(n + 1); const int* qk = Rd.arr<int>(qp[n]);
    const int* on = Rd.arr<int>(n); const int* okf = Rd.arr<int>((size_t)n * cap); const int* ow = Rd.arr<int>((size_t)n * cap);
    const double* scw = Rd.arr<double>(13 * (size_t)n); const double* snc = Rd.arr<double>(13 * (size_t)n);
    const int* corrected = Rd.arr<int>(n);
    const float* pos = Rd.arr<float>(3 * (size_t)m); const int* pbad = Rd.arr<int>(m); const int* pref = Rd.arr<int>(m); const int* pcur = Rd.arr<int>(m);
    std::vector<MockEgKF> K(n);
    std::vector<MockEgPoint> Pt(m);
    MockEgMap map;
    std::map<MockEgKF*, MockSim3> NonCorrected, Corrected;
    std::map<MockEgKF*, std::set<MockEgKF*> > Conn;
    for (int i = 0; i < n; ++i) {
        MockEgKF& k = K[i];
        k.mnId = (long unsigned int)id[i]; k.bad = bad[i] != 0; k.poseSet = false; k.parent = par[i] >= 0 ? &K[par[i]] : (MockEgKF*)0;
        const double* map_pose = snc + 13 * (size_t)i;   // the map's own pose: the non-corrected Sim3 (scale 1)
        k.R = cv::Mat(3, 3, CV_32F); k.t = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) k.R.at<float>(r, c) = (float)map_pose[3 * r + c]; k.t.at<float>(r, 0) = (float)map_pose[9 + r]; }
        for (int j = cp[i]; j < cp[i + 1]; ++j) k.children.insert(&K[ck[j]]);
        for (int j = lp[i]; j < lp[i + 1]; ++j) k.loopEdges.insert(&K[lk[j]]);
        for (int j = 0; j < on[i]; ++j) { k.ordered.push_back(&K[okf[(size_t)i * cap + j]]); k.weights.push_back(ow[(size_t)i * cap + j]); }
        for (int j = qp[i]; j < qp[i + 1]; ++j) Conn[&k].insert(&K[qk[j]]);
        if (corrected[i]) {
            MockSim3 a, b;
            memcpy(a.R, scw + 13 * (size_t)i, 72); memcpy(a.t, scw + 13 * (size_t)i + 9, 24); a.s = scw[13 * (size_t)i + 12];
            memcpy(b.R, map_pose, 72); memcpy(b.t, map_pose + 9, 24); b.s = map_pose[12];
            Corrected[&k] = a; NonCorrected[&k] = b;
        }
        map.kfs.push_back(&k);
    }
    for (int p = 0; p < m; ++p) {
        MockEgPoint& q = Pt[p];
        q.bad = pbad[p] != 0; q.pos = mat_from(pos + 3 * (size_t)p, 3); q.updated = 0; q.ref = 0;
        q.mnCorrectedByKF = 0xFFFFFFFFul; q.mnCorrectedReference = 0;
        if (pcur[p]) { q.mnCorrectedByKF = K[cur].mnId; q.mnCorrectedReference = K[pref[p]].mnId; q.ref = &K[loop]; }   // (the reference keyframe is then not read)
        else q.ref = &K[pref[p]];
        map.pts.push_back(&q);
    }
    const bool bFix = fix != 0;
    Optimizer::OptimizeEssentialGraph(&map, &K[loop], &K[cur], NonCorrected, Corrected, Conn, bFix);
    const int status = Optimizer::LastStatus();
    if (status != 0) fprintf(stderr, "essential failed: %s\n", slamit_last_error());
    FILE* f = fopen(argv[3], "wb");
    fwrite(&status, 4, 1, f);
    for (int i = 0; i < n; ++i) {
        const int set = K[i].poseSet ? 1 : 0;
        float T[12] = {0};
        if (set) for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[3 * r + c] = K[i].pose.at<float>(r, c); T[9 + r] = K[i].pose.at<float>(r, 3); }
        fwrite(&set, 4, 1, f); fwrite(T, 4, 12, f);
    }
    for (int p = 0; p < m; ++p) {
        float X[3] = {Pt[p].pos.at<float>(0, 0), Pt[p].pos.at<float>(1, 0), Pt[p].pos.at<float>(2, 0)};
        fwrite(X, 4, 3, f); fwrite(&Pt[p].updated, 4, 1, f);
    }
    fclose(f);
    return 0;
}

// map_grow: LocalMapping::GrowMap over a world small enough to follow by hand.  Two keyframes of four keypoints, three points (point 2
// bad); a new keyframe whose frame tracked points 0, 2 and 1 at keypoints 0, 2 and 3; a stereo point at its keypoint 1, the association
// loop, a pair with keyframe 0's keypoint 3 at the same keypoint 1, and a rejected pair.  Prints what the objects hold afterwards.
namespace grow_case {
struct MPt;
struct KFr {
    int id;
    std::vector<MPt*> mvpMapPoints; std::vector<float> mvuRight; std::vector<cv::KeyPoint> mvKeysUn;
};
struct MapG {
    std::set<int> points, keyframes;
    void AddKeyFrame(KFr* k) { keyframes.insert(k->id); }
    void AddMapPoint(MPt* p);
    void EraseMapPoint(MPt* p);
};
struct MPt {
    int id; bool mbBad; int nObs;
    std::map<KFr*, size_t> mObservations; KFr* mpRefKF;
};
void MapG::AddMapPoint(MPt* p) { points.insert(p->id); }
void MapG::EraseMapPoint(MPt* p) { points.erase(p->id); }
struct Make {
    std::vector<MPt>* pool; int* next;
    MPt* operator()(const float*, KFr* ref) const {
        MPt* p = &(*pool)[(size_t)*next];
        p->id = (*next)++; p->mbBad = false; p->nObs = 0; p->mpRefKF = ref;
        return p;
    }
};
}  // namespace grow_case

static int run_map_grow(int, char**) {
    using namespace grow_case;
    typedef ORB_SLAM2::LocalMapping::GrowOp<KFr> Op;
    std::vector<KFr> K(3);
    std::vector<MPt> P(6);
    for (int k = 0; k < 3; ++k) { K[k].id = k; K[k].mvpMapPoints.assign(4, (MPt*)NULL); K[k].mvuRight.assign(4, -1.f); K[k].mvKeysUn.assign(4, cv::KeyPoint(0, 0, 1, -1, 0, k)); }
    K[0].mvuRight[3] = 5.f;                                               // a stereo keypoint: its observation weighs 2
    for (int p = 0; p < 3; ++p) { P[p].id = p; P[p].mbBad = p == 2; P[p].nObs = 0; P[p].mpRefKF = &K[0]; }
    const int obs[4][3] = {{0, 0, 0}, {0, 1, 0}, {1, 0, 1}, {2, 1, 2}};   // point, keyframe, keypoint
    for (int o = 0; o < 4; ++o) { P[obs[o][0]].mObservations[&K[obs[o][1]]] = (size_t)obs[o][2]; P[obs[o][0]].nObs++; K[obs[o][1]].mvpMapPoints[obs[o][2]] = &P[obs[o][0]]; }
    K[2].mvpMapPoints[0] = &P[0]; K[2].mvpMapPoints[2] = &P[2]; K[2].mvpMapPoints[3] = &P[1];
    MapG map;
    map.keyframes.insert(0); map.keyframes.insert(1);
    for (int p = 0; p < 3; ++p) map.points.insert(p);
    const Op proto = {0, &K[2], &K[2], 1, (KFr*)NULL, 0, true, false, {1.f, 2.f, 3.f}};
    std::vector<Op> ops(5, proto);
    ops[0].kind = SLAMIT_GROW_NEW_KF;
    ops[1].kind = SLAMIT_GROW_NEW_POINT;
    ops[2].kind = SLAMIT_GROW_ASSOCIATE;
    ops[3].kind = SLAMIT_GROW_NEW_POINT; ops[3].pKFb = &K[0]; ops[3].idxB = 3; ops[3].recent = true;
    ops[4] = ops[3]; ops[4].accepted = false;
    std::list<MPt*> recent;
    int next = 3;
    Make mk = {&P, &next};
    const int made = ORB_SLAM2::LocalMapping::GrowMap<MPt>(ops, &map, recent, mk);
    const int st = ORB_SLAM2::LocalMapping::LastStatus();
    if (st != 0) fprintf(stderr, "grow_map failed: %s\n", slamit_last_error());
    printf("map_grow: status=%d made=%d", st, made);
    for (int k = 0; k < 3; k += 2) {
        printf(" kf%d=", k);
        for (int i = 0; i < 4; ++i) printf("%s%d", i ? "," : "", K[k].mvpMapPoints[i] ? K[k].mvpMapPoints[i]->id : -1);
    }
    printf(" recent=");
    for (std::list<MPt*>::const_iterator it = recent.begin(); it != recent.end(); ++it) printf("%s%d", it == recent.begin() ? "" : ",", (*it)->id);
    printf(" nobs=");
    for (int p = 0; p < next; ++p) printf("%s%d", p ? "," : "", P[p].nObs);
    printf(" observers=");
    for (int p = 0; p < next; ++p) printf("%s%zu", p ? "," : "", P[p].mObservations.size());
    printf(" map_points=%zu map_kfs=%zu\n", map.points.size(), map.keyframes.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::string mode = argv[1];
    if (mode == "orb") return run_orb(argc, argv);
    if (mode == "match") return run_match(argc, argv);
    if (mode == "ba") return run_ba(argc, argv);
    if (mode == "pose") return run_pose(argc, argv);
    if (mode == "search") return run_search(argc, argv);
    if (mode == "frame") return run_frame(argc, argv);
    if (mode == "fuse") return run_fuse(argc, argv);
    if (mode == "fuse_targets") return run_fuse_targets(argc, argv);
    if (mode == "init") return run_init(argc, argv);
    if (mode == "bow") return run_bow(argc, argv);
    if (mode == "sim3") return run_sim3(argc, argv);
    if (mode == "osim3") return run_osim3(argc, argv);
    if (mode == "essential") return run_essential(argc, argv);
    if (mode == "sim3solver") return run_sim3solver(argc, argv);
    if (mode == "pnpsolver") return run_pnpsolver(argc, argv);
    if (mode == "initializer") return run_initializer(argc, argv);
    if (mode == "triangulate") return run_triangulate(argc, argv);
    if (mode == "triangulate_stereo") return run_triangulate_stereo(argc, argv);
    if (mode == "frustum") return run_frustum(argc, argv);
    if (mode == "stereo") return run_stereo(argc, argv);
    if (mode == "unproject") return run_unproject(argc, argv);
    if (mode == "local_map") return run_local_map(argc, argv);
    if (mode == "map_grow") return run_map_grow(argc, argv);
    return 2;
}
