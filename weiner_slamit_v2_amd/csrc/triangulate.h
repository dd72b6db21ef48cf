// triangulate.h — one matched pair of LocalMapping::CreateNewMapPoints (ORB_SLAM2/src/LocalMapping.cc:348-483), monocular: the
// parallax test of the two rays, the 4x4 linear triangulation, both depth tests, both reprojection gates and the scale-consistency
// test.  Plain C++ over IEEE +,-,*,/ and sqrt, float and double exactly where the reference has them; it must be compiled with
// -ffp-contract=off.  triangulate.hip runs it one lane per pair; the CPU test of the restatement and tools/bench_triangulate.py
// build the same text with g++ for the host.  tri_pair is the monocular pair; tri_pair_stereo adds bStereo1/2, the stereo cosines,
// KeyFrame::UnprojectStereo and the 7.8 gates and returns what tri_pair returns when neither keypoint is stereo.
//
// Where the reference goes through OpenCV the evaluation order below is the statement of it (PARITY UNPINNED):
//   xn                ((pt.x - cx) * invfx, (pt.y - cy) * invfy, 1) in float                      :348-349, cv::Mat_<float> <<
//   ray = Rwc * xn    (r0 x0 + r1 x1) + r2 x2 in float over the transposed rotation                :351-352, cv::gemm on CV_32F
//   cosParallaxRays   double sum of double products / (sqrt(double sum) * sqrt(double sum)),        :353, Mat::dot and cv::norm
//                     the quotient rounded to float                                                      return double
//   cos < 0.9998      the float against a double literal                                             :369
//   rows of A         xn * Tcw.row(2)[j] - Tcw.row(r)[j] in float, two roundings                     :373-376, scaled MatExpr
//   x3D               right singular vector of the smallest singular value of the float A:           :379-381, cv::SVD on CV_32F
//                     one-sided (Hestenes) Jacobi in float, TRI_SVD_SWEEPS sweeps
//   x3D / w           v * (float)(1.0 / (double)w): Mat / float is a convertTo with scale 1./s       :387
//   z, x, y           (float)(double sum of double products + (double)t)                             :404-415, Mat::dot returns double
//   invz              (float)(1.0 / (double)z)                                                       :416, :443
//   u, v              ((f * x) * invz) + c in float                                                  :420-421
//   err > 5.991 s2    (double)(float ex ex + ey ey) > 5.991 * (double)s2                             :424, :452
//   Ow                -((r0 t0 + r1 t1) + r2 t2) in float over the transposed rotation               KeyFrame.cc:80-81
//   dist              (float)sqrt(double sum of squares of the float differences)                    :468-472, cv::norm
//   ratios            float                                                                          :477-482
// tri_pair_stereo:
//   bStereo           ur >= 0 (0.0f is stereo, NaN is not)                                           :337, :345
//   cosParallaxStereo cos 2t = (d d - h h) / (d d + h h) with h = mb / 2 in float, d = mvDepth,       :360, :362, cos(2*atan2(mb/2, d))
//                     evaluated in double and rounded once to float (PARITY UNPINNED)
//   min               b < a ? b : a                                                                  :364, std::min
//   UnprojectStereo   x = ((u - cx) * z) * invfx, y = ((v - cy) * z) * invfy on the RAW keypoint,    KeyFrame.cc:623-639
//                     ((r0 x + r1 y) + r2 z) + Ow in float over the transposed rotation               cv::gemm on CV_32F
//   u_r               u - bf * invz, two roundings                                                   :430, :458
//   err > 7.8 s2      (double)(float (ex ex + ey ey) + er er) > 7.8 * (double)s2                     :435, :463
#ifndef SLAMIT_TRIANGULATE_H
#define SLAMIT_TRIANGULATE_H
#include <math.h>

#if defined(__HIPCC__)
#define TRI_HD __host__ __device__ __forceinline__
#else
#define TRI_HD static inline
#endif

// Sweeps of the one-sided Jacobi.  A sweep is the six column pairs of the 4x4 once; the method converges quadratically once the
// columns are nearly orthogonal.  On the fixtures 4 sweeps give the statuses and points of 12 (3 do not); FIVE is what ships, one
// sweep of margin.  tests/test_triangulate_ref.py requires that 10 sweeps change no status and move no fixture point by more than
// the yardstick Y of DESIGN.md §14 (measured: 0.36 Y, the rounding of the extra rotations).
#ifndef TRI_SVD_SWEEPS
#define TRI_SVD_SWEEPS 5
#endif

enum {
    TRI_OK = 0, TRI_PARALLAX = 1, TRI_W_ZERO = 2, TRI_Z1 = 3, TRI_Z2 = 4, TRI_REPROJ1 = 5, TRI_REPROJ2 = 6, TRI_DIST_ZERO = 7, TRI_SCALE = 8,
    TRI_UNPROJECT_DEPTH = 9   // tri_pair_stereo only: the keypoint chosen for UnprojectStereo has depth <= 0 (the reference reads an empty Mat)
};
enum { TRI_SRC_NONE = 0, TRI_SRC_TRIANGULATED = 1, TRI_SRC_UNPROJECT1 = 2, TRI_SRC_UNPROJECT2 = 3 };

struct TriView {
    float T[12];                          // Tcw, row-major 3x4
    float fx, fy, cx, cy, invfx, invfy;
    float O[3];                           // camera centre, tri_centre()
};

TRI_HD void tri_centre(TriView& c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) c.O[i] = -((c.T[i] * c.T[3] + c.T[4 + i] * c.T[7]) + c.T[8 + i] * c.T[11]);
}

TRI_HD double tri_dot3d(const float a[3], const float b[3]) { return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2]; }

// :348-353
TRI_HD float tri_cos_parallax(const TriView& c1, const TriView& c2, const float p1[2], const float p2[2], float xn1[2], float xn2[2]) {
    xn1[0] = (p1[0] - c1.cx) * c1.invfx; xn1[1] = (p1[1] - c1.cy) * c1.invfy;
    xn2[0] = (p2[0] - c2.cx) * c2.invfx; xn2[1] = (p2[1] - c2.cy) * c2.invfy;
    float r1[3], r2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r1[i] = (c1.T[i] * xn1[0] + c1.T[4 + i] * xn1[1]) + c1.T[8 + i] * 1.0f;
        r2[i] = (c2.T[i] * xn2[0] + c2.T[4 + i] * xn2[1]) + c2.T[8 + i] * 1.0f;
    }
    return (float)(tri_dot3d(r1, r2) / (sqrt(tri_dot3d(r1, r1)) * sqrt(tri_dot3d(r2, r2))));
}

// :373-376
TRI_HD void tri_build_A(const TriView& c1, const TriView& c2, const float xn1[2], const float xn2[2], float (&A)[4][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        A[0][j] = xn1[0] * c1.T[8 + j] - c1.T[j];
        A[1][j] = xn1[1] * c1.T[8 + j] - c1.T[4 + j];
        A[2][j] = xn2[0] * c2.T[8 + j] - c2.T[j];
        A[3][j] = xn2[1] * c2.T[8 + j] - c2.T[4 + j];
    }
}

// One Hestenes rotation: columns P and Q of G (and of V) are turned so that the two columns of G become orthogonal.  P and Q are
// compile-time so that both matrices stay in registers.  A pair that is orthogonal already (or NaN) is turned by the identity.
template <int P, int Q>
TRI_HD void tri_rotate(float (&G)[4][4], float (&V)[4][4]) {
    const float a = ((G[0][P] * G[0][P] + G[1][P] * G[1][P]) + G[2][P] * G[2][P]) + G[3][P] * G[3][P];
    const float b = ((G[0][Q] * G[0][Q] + G[1][Q] * G[1][Q]) + G[2][Q] * G[2][Q]) + G[3][Q] * G[3][Q];
    const float g = ((G[0][P] * G[0][Q] + G[1][P] * G[1][Q]) + G[2][P] * G[2][Q]) + G[3][P] * G[3][Q];
    const bool turn = fabsf(g) > 0.f;
    const float zeta = (b - a) / (2.0f * (turn ? g : 1.0f));
    float t = 1.0f / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
    t = zeta < 0.f ? -t : t;
    float c = 1.0f / sqrtf(1.0f + t * t), s = c * t;
    c = turn ? c : 1.0f;
    s = turn ? s : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gp = G[r][P], gq = G[r][Q], vp = V[r][P], vq = V[r][Q];
        G[r][P] = c * gp - s * gq; G[r][Q] = s * gp + c * gq;
        V[r][P] = c * vp - s * vq; V[r][Q] = s * vp + c * vq;
    }
}

// right singular vector of the smallest singular value of A (the first such column on a tie); v and -v are the same point
TRI_HD void tri_null_vector(const float (&A)[4][4], float v[4]) {
    float G[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { G[r][c] = A[r][c]; V[r][c] = r == c ? 1.0f : 0.0f; }
#pragma unroll 1
    for (int sweep = 0; sweep < TRI_SVD_SWEEPS; ++sweep) {
        tri_rotate<0, 1>(G, V); tri_rotate<0, 2>(G, V); tri_rotate<0, 3>(G, V);
        tri_rotate<1, 2>(G, V); tri_rotate<1, 3>(G, V); tri_rotate<2, 3>(G, V);
    }
    float best = ((G[0][0] * G[0][0] + G[1][0] * G[1][0]) + G[2][0] * G[2][0]) + G[3][0] * G[3][0];
    v[0] = V[0][0]; v[1] = V[1][0]; v[2] = V[2][0]; v[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float n = ((G[0][k] * G[0][k] + G[1][k] * G[1][k]) + G[2][k] * G[2][k]) + G[3][k] * G[3][k];
        const bool lower = n < best;
        best = lower ? n : best;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = lower ? V[r][k] : v[r];
    }
}

// row r of Tcw applied to X (:404, :414-415)
TRI_HD float tri_row(const TriView& c, int r, const float X[3]) { return (float)(tri_dot3d(&c.T[4 * r], X) + (double)c.T[4 * r + 3]); }

// :412-425 / :439-453 for one keyframe whose depth z has passed its test: true = rejected
TRI_HD bool tri_reproj_rejects(const TriView& c, const float X[3], float z, const float p[2], float sigma2) {
    const float x = tri_row(c, 0, X), y = tri_row(c, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const float ex = u - p[0], ey = v - p[1];
    return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
}

TRI_HD float tri_dist(const float X[3], const float O[3]) {
    const float d[3] = {X[0] - O[0], X[1] - O[1], X[2] - O[2]};
    return (float)sqrt(tri_dot3d(d, d));
}

// :467-483: 0, TRI_DIST_ZERO or TRI_SCALE
TRI_HD int tri_scale_gate(const float X[3], const float O1[3], const float O2[3], float sf1, float sf2, float ratioFactor) {
    const float dist1 = tri_dist(X, O1), dist2 = tri_dist(X, O2);
    if (dist1 == 0 || dist2 == 0) return TRI_DIST_ZERO;
    const float ratioDist = dist2 / dist1, ratioOctave = sf1 / sf2;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return TRI_SCALE;
    return TRI_OK;
}

// :401-483 on a Euclidean point
TRI_HD int tri_gates(const TriView& c1, const TriView& c2, const float p1[2], const float p2[2], float sigma2_1, float sigma2_2, float sf1,
                     float sf2, float ratioFactor, const float X[3]) {
    const float z1 = tri_row(c1, 2, X);
    if (z1 <= 0) return TRI_Z1;
    const float z2 = tri_row(c2, 2, X);
    if (z2 <= 0) return TRI_Z2;
    if (tri_reproj_rejects(c1, X, z1, p1, sigma2_1)) return TRI_REPROJ1;
    if (tri_reproj_rejects(c2, X, z2, p2, sigma2_2)) return TRI_REPROJ2;
    return tri_scale_gate(X, c1.O, c2.O, sf1, sf2, ratioFactor);
}

// :381-387 on the homogeneous solution: false = w == 0
TRI_HD bool tri_dehomogenise(const float v[4], float X[3]) {
    if (v[3] == 0) return false;
    const float s = (float)(1.0 / (double)v[3]);
    X[0] = v[0] * s; X[1] = v[1] * s; X[2] = v[2] * s;
    return true;
}

// One pair: the code of the first gate that rejects it (0 = a new map point at X).  X is written whenever the pair got as far as
// a point (codes 0 and 3..8) and is left at zero otherwise.
TRI_HD int tri_pair(const TriView& c1, const TriView& c2, const float p1[2], const float p2[2], float sigma2_1, float sigma2_2, float sf1,
                    float sf2, float ratioFactor, float X[3]) {
    X[0] = 0.f; X[1] = 0.f; X[2] = 0.f;
    float xn1[2], xn2[2];
    const float cosParallaxRays = tri_cos_parallax(c1, c2, p1, p2, xn1, xn2);
    // monocular: cosParallaxStereo = cos + 1, so :369 is cos < cos + 1 && cos > 0 && cos < 0.9998
    if (!(cosParallaxRays < cosParallaxRays + 1 && cosParallaxRays > 0 && cosParallaxRays < 0.9998)) return TRI_PARALLAX;
    float A[4][4], v[4];
    tri_build_A(c1, c2, xn1, xn2, A);
    tri_null_vector(A, v);
    if (!tri_dehomogenise(v, X)) return TRI_W_ZERO;
    return tri_gates(c1, c2, p1, p2, sigma2_1, sigma2_2, sf1, sf2, ratioFactor, X);
}

// ---- stereo keypoints (LocalMapping.cc:335-465, KeyFrame.cc:623-639) ----

// the right-image side of one pair: mvuRight, mvDepth and the raw (distorted) keypoint mvKeys[idx].pt of each keyframe
struct TriStereoPair {
    float ur1, ur2, depth1, depth2;
    float raw1[2], raw2[2];
};

// :360 / :362, cos(2 * atan2(mb / 2, depth)) as the double-angle identity, one rounding
TRI_HD float tri_cos_stereo(float mb, float depth) {
    const float h = mb / 2;
    const double d2 = (double)depth * (double)depth, h2 = (double)h * (double)h;
    return (float)((d2 - h2) / (d2 + h2));
}

// KeyFrame::UnprojectStereo on a depth that is > 0
TRI_HD void tri_unproject_stereo(const TriView& c, const float raw[2], float z, float X[3]) {
    const float x = (raw[0] - c.cx) * z * c.invfx, y = (raw[1] - c.cy) * z * c.invfy;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = ((c.T[i] * x + c.T[4 + i] * y) + c.T[8 + i] * z) + c.O[i];
}

// :427-437 / :455-465 for a stereo keypoint: true = rejected
TRI_HD bool tri_reproj_rejects_stereo(const TriView& c, const float X[3], float z, const float p[2], float ur, float bf, float sigma2) {
    const float x = tri_row(c, 0, X), y = tri_row(c, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const float u_r = u - bf * invz;
    const float ex = u - p[0], ey = v - p[1], er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// One pair with its right-image side.  mb1 / mb2 are the two keyframes' baselines in metres, bf the CURRENT keyframe's mbf: the
// reference uses it for the neighbour's gate too (:458).  source says where X came from (TRI_SRC_*; 0 with codes 1, 2 and 9).
TRI_HD int tri_pair_stereo(const TriView& c1, const TriView& c2, const float p1[2], const float p2[2], const TriStereoPair& s, float mb1, float mb2,
                           float bf, float sigma2_1, float sigma2_2, float sf1, float sf2, float ratioFactor, float X[3], int& source) {
    X[0] = 0.f; X[1] = 0.f; X[2] = 0.f;
    source = TRI_SRC_NONE;
    const bool bStereo1 = s.ur1 >= 0, bStereo2 = s.ur2 >= 0;
    float xn1[2], xn2[2];
    const float cosParallaxRays = tri_cos_parallax(c1, c2, p1, p2, xn1, xn2);
    float cosParallaxStereo1 = cosParallaxRays + 1, cosParallaxStereo2 = cosParallaxRays + 1;
    if (bStereo1) cosParallaxStereo1 = tri_cos_stereo(mb1, s.depth1);
    else if (bStereo2) cosParallaxStereo2 = tri_cos_stereo(mb2, s.depth2);
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        float A[4][4], v[4];
        tri_build_A(c1, c2, xn1, xn2, A);
        tri_null_vector(A, v);
        if (!tri_dehomogenise(v, X)) return TRI_W_ZERO;
        source = TRI_SRC_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        if (s.depth1 <= 0) return TRI_UNPROJECT_DEPTH;
        tri_unproject_stereo(c1, s.raw1, s.depth1, X);
        source = TRI_SRC_UNPROJECT1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        if (s.depth2 <= 0) return TRI_UNPROJECT_DEPTH;
        tri_unproject_stereo(c2, s.raw2, s.depth2, X);
        source = TRI_SRC_UNPROJECT2;
    } else {
        return TRI_PARALLAX;
    }
    const float z1 = tri_row(c1, 2, X);
    if (z1 <= 0) return TRI_Z1;
    const float z2 = tri_row(c2, 2, X);
    if (z2 <= 0) return TRI_Z2;
    if (bStereo1 ? tri_reproj_rejects_stereo(c1, X, z1, p1, s.ur1, bf, sigma2_1) : tri_reproj_rejects(c1, X, z1, p1, sigma2_1)) return TRI_REPROJ1;
    if (bStereo2 ? tri_reproj_rejects_stereo(c2, X, z2, p2, s.ur2, bf, sigma2_2) : tri_reproj_rejects(c2, X, z2, p2, sigma2_2)) return TRI_REPROJ2;
    return tri_scale_gate(X, c1.O, c2.O, sf1, sf2, ratioFactor);
}

#endif
