// frustum.h — one local map point of Tracking::SearchLocalPoints (ORB_SLAM2/src/Tracking.cc:1409-1464): Frame::isInFrustum
// (src/Frame.cc:389-445) with MapPoint::PredictScale (src/MapPoint.cc:391-400), and the search window that
// ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) builds from what isInFrustum stored (src/ORBmatcher.cc:47-71,
// RadiusByViewingCos :134-140).  Plain C++ over IEEE +,-,*,/ and sqrt, float and double exactly where the reference has them; it
// must be compiled with -ffp-contract=off.  frustum.hip runs it one lane per point; the CPU test of the restatement, the shim's
// test driver and tools/bench_frustum.py build the same text with g++ for the host.  Monocular search only: mTrackProjXR is
// produced (one multiply), the stereo `er` gate of the search is not.
//
// The arithmetic, line by line (where the reference goes through OpenCV the order below is the statement of it,
// PARITY UNPINNED as for shim/ORBmatcher.h's slamit_gemm_row3, whose convention fru_gemm_row3 restates):
//   Pc = mRcw*P+mtcw  per row (r0 X + r1 Y) + r2 Z in float, then (float)((double)t0 + (double)t)      Frame.cc:398, cv::gemm, small-matrix branch
//   PcZ < 0.0f        rejects; -0 and +0 do not                                                         :404
//   invz              1.0f / PcZ in float: +-inf for PcZ == +-0                                         :408
//   u, v              ((fx * PcX) * invz) + cx in float, left to right                                   :409-410
//   uR                u - (bf * invz) in float                                                           :436
//   bounds            u < min_x || u > max_x, then v: a NaN (PcX == 0 with PcZ == 0) passes both         :412-415
//   PO = P - mOw      float; mOw as the frame holds it, not recomputed from Rcw and tcw                  :420
//   dist              (float)sqrt(double sum of double squares, in order)                                :421, cv::norm
//   distance gate     dist < 0.8f * min_dist || dist > 1.2f * max_dist, the products in float            :423, MapPoint.cc:379-389
//   viewCos           (float)(((double)PO0 Pn0 + (double)PO1 Pn1) + (double)PO2 Pn2) / (double)dist)     :429, Mat::dot returns double
//   viewing angle     viewCos < viewingCosLimit rejects: a NaN (dist == 0) passes                        :431
//   ratio             max_dist / dist in float (the RAW mfMaxDistance, not the 1.2f one)                 MapPoint.cc:396
//   level             (int)ceilf(fru_logf(ratio) / logScaleFactor), quotient in float                    MapPoint.cc:399
//   r                 viewCos > 0.998 (the float against a double literal) ? 2.5f : 4.0f;                ORBmatcher.cc:134-140
//                     if (th != 1.0) r *= th;  window radius r * scale_factors[level], levels level-1 .. level   :51, :65-71
//
// WHICH LOG.  MapPoint.cc:399 is `ceil(log(ratio)/logScaleFactor)` with `ratio` and `logScaleFactor` float.  The file writes
// `unique_lock<mutex>` without std::, so a using-directive for std is in force in that translation unit, and <cmath> arrives through
// opencv2/core; overload resolution on a float argument then takes std::log(float), i.e. logf.  (Without the directive the global
// ::log of the C++ library headers carries the same float overload.)  The quotient of two floats is a float and ceil(float) is
// ceilf.  So the level is a FLOAT computation, and near an integer value of log(ratio)/logScaleFactor it depends on the last bit
// of the platform's logf.  That one function is not an IEEE operation, and the C library's and the device library's differ, so
// neither is called: fru_logf below is this header's own, built from IEEE double operations in a fixed order, and gives the same
// bits under g++ and under hipcc.  It is correctly rounded except within about 1e-9 ulp of a tie; a 1-ulp logf (glibc's, bionic's,
// numpy's) can differ from it in the last bit, which moves the level only where |q - round(q)| is a few float ulps
// (tests/frustum_ref.py: a point is DECIDED when that distance exceeds 8 * 2^-20).
//
// ONE STATED DEPARTURE.  The reference's PredictScale does not clamp (this tree's MapPoint.cc:391-400), and with the 0.8 / 1.2 gates
// the level can be -1 or n_levels, n_levels + 1; mvScaleFactors[nPredictedLevel] (ORBmatcher.cc:66) is then read out of bounds:
// undefined.  Here a point that passes every gate but whose level lies outside [0, n_levels) gets a status of its own,
// FRU_LEVEL (7); so does a point whose ratio is not finite and positive (dist == 0 with min_dist <= 0, max_dist <= 0, NaN), which is
// tested BEFORE any float-to-int conversion and reports level INT32_MIN, as does a quotient outside the int range.  Such a point
// keeps its u, v, uR, viewCos and raw level, has r = 0, produces no search query and is not counted in view (mbTrackInView = false).
//
// Outputs of a rejected point: every field the walk did not reach is zero.  u, v, uR are written once the depth test has passed
// (codes 3..7 and 0), viewCos once the distance gate has (6, 7, 0), level for 7 and 0, r for 0 only.
// Documented corner cases: PcZ == +0 with PcX != 0 gives u = +-inf and code 3; dist == 0 with min_dist <= 0 gives viewCos = NaN,
// ratio = +inf (or NaN) and code 7.
#ifndef SLAMIT_FRUSTUM_H
#define SLAMIT_FRUSTUM_H
#include <math.h>

#if defined(__HIPCC__)
#define FRU_HD __host__ __device__ __forceinline__
#else
#define FRU_HD static inline
#endif

#define FRU_MAX_LEVELS 16          // = SLAMIT_MAX_LEVELS; a power of two: the table index is masked with FRU_MAX_LEVELS - 1
#define FRU_LEVEL_NONE (-2147483647 - 1)

enum { FRU_IN_VIEW = 0, FRU_SKIPPED = 1, FRU_DEPTH = 2, FRU_U = 3, FRU_V = 4, FRU_DISTANCE = 5, FRU_ANGLE = 6, FRU_LEVEL = 7 };

// What the frame contributes (Frame: mRcw, mtcw, mOw, fx, fy, cx, cy, mbf, mnMinX .. mnMaxY, mfLogScaleFactor, mvScaleFactors) and
// what the two callers pass (viewingCosLimit = 0.5, Tracking.cc:1440; th, :1452-1460).  Layout of slamit_frustum_frame.
struct FrustumFrame {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, bf;
    float min_x, max_x, min_y, max_y;
    float view_cos_limit, log_scale_factor, th;
    int n_levels;
    float scale_factors[FRU_MAX_LEVELS];
};

struct FrustumOut {
    float u, v, uR, viewCos, r;    // mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos, the search window's half size
    int level;                     // mnTrackScaleLevel
};

// shim/ORBmatcher.h's slamit_gemm_row3: the float dot left to right, the translation added in double
FRU_HD float fru_gemm_row3(const float* r, const float P[3], float t) {
    const float t0 = r[0] * P[0] + r[1] * P[1] + r[2] * P[2];
    return (float)((double)t0 + (double)t);
}

// log of a finite positive float, rounded to float.  x = m 2^e with m in (sqrt(1/2), sqrt(2)] (exact), s = (m - 1) / (m + 1),
// log m = 2 s (1 + s^2/3 + s^4/5 + ... + s^18/19): |s| < 0.1716, so the first term left out is below 3e-17 of the sum.  Horner in
// double, every product and sum rounded on its own (no contraction).
FRU_HD float fru_logf(float x) {
    const double d = (double)x;                      // a subnormal float is a normal double
    unsigned long long b;
    __builtin_memcpy(&b, &d, 8);
    int e = (int)(b >> 52) - 1023;
    b = (b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
    double m;
    __builtin_memcpy(&m, &b, 8);                     // [1, 2)
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    return (float)((double)e * 0.6931471805599453 + (2.0 * s) * p);
}

// MapPoint::PredictScale without the float-to-int conversion of a value no int holds: false = FRU_LEVEL with FRU_LEVEL_NONE
FRU_HD bool fru_predict_scale(float max_dist, float dist, float log_scale_factor, int& level) {
    const float ratio = max_dist / dist;
    level = FRU_LEVEL_NONE;
    if (!(ratio > 0.0f && ratio <= 3.402823466e+38f)) return false;
    const float q = ceilf(fru_logf(ratio) / log_scale_factor);
    if (!(q >= -2147483648.0f && q < 2147483648.0f)) return false;
    level = (int)q;
    return true;
}

// One point: the code of the first test that rejects it (0 = in view), and what the reference stores in the MapPoint.
FRU_HD int frustum_point(const FrustumFrame& F, const float P[3], const float Pn[3], float max_dist, float min_dist, bool skip, FrustumOut& o) {
    o.u = 0.f; o.v = 0.f; o.uR = 0.f; o.viewCos = 0.f; o.r = 0.f; o.level = 0;
    if (skip) return FRU_SKIPPED;
    const float PcX = fru_gemm_row3(&F.Rcw[0], P, F.tcw[0]);
    const float PcY = fru_gemm_row3(&F.Rcw[3], P, F.tcw[1]);
    const float PcZ = fru_gemm_row3(&F.Rcw[6], P, F.tcw[2]);
    if (PcZ < 0.0f) return FRU_DEPTH;
    const float invz = 1.0f / PcZ;
    const float u = F.fx * PcX * invz + F.cx;
    const float v = F.fy * PcY * invz + F.cy;
    o.u = u; o.v = v; o.uR = u - F.bf * invz;
    if (u < F.min_x || u > F.max_x) return FRU_U;
    if (v < F.min_y || v > F.max_y) return FRU_V;
    const float PO[3] = {P[0] - F.Ow[0], P[1] - F.Ow[1], P[2] - F.Ow[2]};
    const float dist = (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);
    if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) return FRU_DISTANCE;
    const float viewCos = (float)((((double)PO[0] * (double)Pn[0] + (double)PO[1] * (double)Pn[1]) + (double)PO[2] * (double)Pn[2]) / (double)dist);
    o.viewCos = viewCos;
    if (viewCos < F.view_cos_limit) return FRU_ANGLE;
    int level;
    const bool has = fru_predict_scale(max_dist, dist, F.log_scale_factor, level);
    o.level = level;
    if (!has || level < 0 || level >= F.n_levels || level >= FRU_MAX_LEVELS) return FRU_LEVEL;
    float r = viewCos > 0.998 ? 2.5f : 4.0f;
    if (F.th != 1.0) r *= F.th;
    o.r = r * F.scale_factors[level & (FRU_MAX_LEVELS - 1)];
    return FRU_IN_VIEW;
}

// The query ORBmatcher::SearchByProjection builds from a point (shim/ORBmatcher.h, the loop over vpMapPoints): window centre and
// half size, levels level - 1 .. level, valid = mbTrackInView.  A point that is not in view is a query with valid = 0 and zeros.
FRU_HD void frustum_query(int status, const FrustumOut& o, float uvr[3], int& level_min, int& level_max, unsigned char& valid) {
    const bool in = status == FRU_IN_VIEW;
    uvr[0] = in ? o.u : 0.f; uvr[1] = in ? o.v : 0.f; uvr[2] = in ? o.r : 0.f;
    level_min = in ? o.level - 1 : 0; level_max = in ? o.level : 0;
    valid = in ? 1 : 0;
}

#endif
