// two_view.h — the monocular Initializer (ORB_SLAM2/src/Initializer.cc): Normalize, ComputeH21 / ComputeF21, CheckHomography /
// CheckFundamental, ReconstructH up to its eight motions, DecomposeE with the four motions of ReconstructF, CheckRT for one match,
// and the host scans over the results.  Plain C++ over IEEE +,-,*,/ and sqrt, float and double exactly where the reference has
// them; it must be compiled with -ffp-contract=off.  initializer.hip runs it on the device, the CPU tests and
// tools/bench_initializer.py build the same text with g++ for the host.
//
// A TEAM runs one 9-column decomposition: T threads that share one TvWork (LDS on the device) and meet at tv_sync().  On the host
// T = 1 and the same loops run in order; every rotation of a round touches its own two columns, so the result does not depend on T.
//
// Where the reference goes through OpenCV the evaluation order below is the statement of it (PARITY UNPINNED):
//   Normalize         sequential float sums over ALL keypoints, mean = sum / (float)N, s = (float)(1.0 / (double)meanDev),      :758-804
//                     point (x - mean) * s, T(0,2) = -mean * s in float
//   A of H / F        float products as written                                                                                    :248-266, :290-298
//   cv::SVDecomp      STATED DEPARTURE: one-sided (Hestenes) Jacobi in DOUBLE on the float matrix, a fixed number of sweeps;       :272, :303, :307,
//                     what the reference then uses (vt.row(8); u, w, vt of Fpre, A and E) is rounded to float once.               :597, :921
//                     SIGN RULE (a): a right singular vector's largest-magnitude component (the first on a tie) is positive,
//                     its left partner is A v / |A v|, w = |A v|, singular values descending (ties keep the column order).
//   3 x 3 products    (a0 b0 + a1 b1) + a2 b2 in float, left to right (T2inv*Hn*T1, T2t*Fn*T1, K.t()*F21*K, invK*H21*K,            cv::gemm on CV_32F
//                     u*diag(w)*vt, U*Rp*Vt, u*W*vt), matrix * vector likewise
//   3 x 3 inverses    cofactors and determinant in double from the float entries, each entry (float)(cof / det)    UNPINNED       :143, :170, :593
//   cv::determinant   m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20) + m02 (m10 m21 - m11 m20) in float        UNPINNED       :600, :932, :936
//   s*U*Rp*Vt         ((U Rp) scaled entry by entry by s in float) Vt                                              UNPINNED       :636, :674
//   t / cv::norm(t)   (float)((double)t_i * (1.0 / sqrt(double sum of squares)))                                                  :646, :684, :924
//   1.0/(...)         a double division of the float sum, rounded to float                                                        :361, :377, :877, :888
//   invSigmaSquare    (float)(1.0 / (double)(sigma * sigma))                                                                      :344, :420
//   chi > th          float against the float constants 5.991f / 3.841f; a NaN fails neither test and is added to the score        :369-388, :447-468
//   score             float, two conditional adds per match, in match order                                                       :372, :388
//   P2 = K*[R|t]      (k0 b0 + k1 b1) + k2 b2 in float; O2 = -((r0 t0 + r1 t1) + r2 t2) over the transposed rotation               :833, :835
//   Triangulate       rows pt.x * P.row(2) - P.row(0) in float, two roundings; null vector by tri_null_vector of triangulate.h;   :743-756
//                     x3D = v * (float)(1.0 / (double)v[3]), a zero v[3] gives a point that is not finite
//   dist              (float)sqrt(double sum of squares); cosParallax = (float)(double dot / (double)(dist1 * dist2))              :857-863
//   cos < 0.99998     the float against the double literal                                                                        :866, :872, :901
//   p3dC2             ((r0 x + r1 y) + r2 z) + t in float                                                                          :870
//   im1x              ((fx * x) * invZ) + cx in float; th2 = (float)(4.0 * (double)(sigma * sigma))                                :878, :503
//   parallax          the min(50, size - 1)-th smallest accepted cosine in the order of tv_cos_key (floats, -0 below +0, a NaN     :907-910
//                     at the end of its sign); the angle (float)((double)(acosf(c) * 180.f) / pi) on the host
#ifndef SLAMIT_TWO_VIEW_H
#define SLAMIT_TWO_VIEW_H
#include <math.h>
#include <stdint.h>

#include "triangulate.h"

#if defined(__HIPCC__)
#define TV_HD __host__ __device__ __forceinline__
#else
#define TV_HD static inline
#endif

// Sweeps of the two Jacobi decompositions; no loop exits on convergence (a collinear or degenerate sample is legal input and
// must return in bounded time).  Chosen on the host build as the count after which the largest gap to the float64 svd restatement
// (variant A of tests/initializer_ref.py) over the admitted hypotheses of four fixtures stops falling, plus two; the gaps are entry
// gaps relative to max(1, |entry|), tests/test_initializer_ref.py reproduces the tables:
//   9 columns, models H21i / F21i:    2 sweeps 438, 3: 75, 4: 3.5, 5: 4.0, 6: 1.0e-2, 7, 8, 10: 0           ->  TV_SVD9_SWEEPS = 9
//   3 x 3, models / motions R, t:     1 sweep 0.89 / 1.3, 2: 7.4e-2 / 0.17, 3: 9.5e-7 / 3.6e-7,
//                                     4, 5, 6, 8: 0 / 3.6e-7                                                  ->  TV_SVD3_SWEEPS = 6
#ifndef TV_SVD9_SWEEPS
#define TV_SVD9_SWEEPS 9
#endif
#ifndef TV_SVD3_SWEEPS
#define TV_SVD3_SWEEPS 6
#endif

enum { TV_MODEL_H = 0, TV_MODEL_F = 1 };
// CheckRT's verdict on one match: the first gate that rejected it
enum { TV_RT_OK = 0, TV_RT_NOT_INLIER = 1, TV_RT_NOT_FINITE = 2, TV_RT_Z1 = 3, TV_RT_Z2 = 4, TV_RT_REPROJ1 = 5, TV_RT_REPROJ2 = 6 };

struct TvTeam { int tid, size; };

TV_HD void tv_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

// shared by the team of one hypothesis
struct TvWork {
    double G[16][10];   // the columns being orthogonalised (column 9 is padding)
    double V[9][10];    // the accumulated rotations
    double cs[4][2];    // c, s of the four rotations of a round
};

// ---- small float matrices ----

TV_HD void tv_mul33(const float a[9], const float b[9], float c[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

TV_HD void tv_mul31(const float a[9], const float x[3], float y[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = (a[3 * i] * x[0] + a[3 * i + 1] * x[1]) + a[3 * i + 2] * x[2];
}

TV_HD void tv_transpose33(const float a[9], float t[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[3 * i + j] = a[3 * j + i];
}

TV_HD void tv_inv33(const float m[9], float inv[9]) {
    double a[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = (double)m[i];
    double c[9];   // c[3 * i + j] = cofactor of a[j][i]
    c[0] = a[4] * a[8] - a[5] * a[7]; c[1] = a[2] * a[7] - a[1] * a[8]; c[2] = a[1] * a[5] - a[2] * a[4];
    c[3] = a[5] * a[6] - a[3] * a[8]; c[4] = a[0] * a[8] - a[2] * a[6]; c[5] = a[2] * a[3] - a[0] * a[5];
    c[6] = a[3] * a[7] - a[4] * a[6]; c[7] = a[1] * a[6] - a[0] * a[7]; c[8] = a[0] * a[4] - a[1] * a[3];
    const double det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) inv[i] = (float)(c[i] / det);
}

TV_HD float tv_det33(const float m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// t / cv::norm(t)
TV_HD void tv_unit3(float t[3]) {
    const double s = 1.0 / sqrt(tri_dot3d(t, t));
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = (float)((double)t[i] * s);
}

// ---- Normalize (:758-804), host ----

struct TvNorm { float meanX, meanY, sX, sY; };

static inline TvNorm tv_normalize(const float* keys, int N) {
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; ++i) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; ++i) { meanDevX += fabsf(keys[2 * i] - meanX); meanDevY += fabsf(keys[2 * i + 1] - meanY); }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    TvNorm T;
    T.meanX = meanX; T.meanY = meanY;
    T.sX = (float)(1.0 / (double)meanDevX); T.sY = (float)(1.0 / (double)meanDevY);
    return T;
}

TV_HD void tv_norm_matrix(const TvNorm& n, float T[9]) {
    T[0] = n.sX; T[1] = 0.f; T[2] = -n.meanX * n.sX;
    T[3] = 0.f; T[4] = n.sY; T[5] = -n.meanY * n.sY;
    T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ---- the Jacobi rotation both decompositions use ----

// c, s that make two columns with squared norms a, b and inner product g orthogonal; the identity when g is 0 or NaN
TV_HD void tv_rotation(double a, double b, double g, double* c, double* s) {
    const bool turn = fabs(g) > 0.0;
    const double zeta = (b - a) / (2.0 * (turn ? g : 1.0));
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    t = zeta < 0.0 ? -t : t;
    const double cc = 1.0 / sqrt(1.0 + t * t);
    *c = turn ? cc : 1.0;
    *s = turn ? cc * t : 0.0;
}

// ---- ComputeH21 / ComputeF21: the right singular vector of the smallest singular value of an m x 9 float matrix ----

// W->G rows 0 .. m-1 hold the matrix.  Afterwards every thread holds the vector, sign-ruled and rounded to float.
TV_HD void tv_null9(const TvTeam& T, TvWork* W, int m, float h[9]) {
    for (int e = T.tid; e < 81; e += T.size) W->V[e / 9][e % 9] = e / 9 == e % 9 ? 1.0 : 0.0;
    tv_sync();
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SVD9_SWEEPS; ++sweep) {
        // round-robin over ten players, the tenth a bye: round r pairs (r + k) % 9 with (r - k) % 9, k = 1 .. 4
#pragma unroll 1
        for (int r = 0; r < 9; ++r) {
            for (int k = T.tid; k < 4; k += T.size) {
                const int p = (r + k + 1) % 9, q = (r + 8 - k) % 9;
                double a = 0.0, b = 0.0, g = 0.0;
                for (int i = 0; i < m; ++i) {
                    const double gp = W->G[i][p], gq = W->G[i][q];
                    a += gp * gp; b += gq * gq; g += gp * gq;
                }
                tv_rotation(a, b, g, &W->cs[k][0], &W->cs[k][1]);
            }
            tv_sync();
            const int rows = m + 9;
            for (int e = T.tid; e < 4 * rows; e += T.size) {
                const int k = e / rows, i = e % rows;
                const int p = (r + k + 1) % 9, q = (r + 8 - k) % 9;
                const double c = W->cs[k][0], s = W->cs[k][1];
                double* const row = i < m ? W->G[i] : W->V[i - m];
                const double xp = row[p], xq = row[q];
                row[p] = c * xp - s * xq; row[q] = s * xp + c * xq;
            }
            tv_sync();
        }
    }
    int best = 0;
    double least = 0.0;
    for (int k = 0; k < 9; ++k) {
        double nk = 0.0;
        for (int i = 0; i < m; ++i) nk += W->G[i][k] * W->G[i][k];
        if (k == 0 || nk < least) { least = nk; best = k; }
    }
    double v[9], big = 0.0;
    bool neg = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        v[i] = W->V[i][best];
        if (fabs(v[i]) > big) { big = fabs(v[i]); neg = v[i] < 0.0; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (float)(neg ? -v[i] : v[i]);
    tv_sync();   // W may be refilled
}

// ---- cv::SVD of a 3 x 3 float matrix: u, w, vt as floats ----

template <int P, int Q>
TV_HD void tv_rotate3(double (&G)[3][3], double (&V)[3][3]) {
    const double a = (G[0][P] * G[0][P] + G[1][P] * G[1][P]) + G[2][P] * G[2][P];
    const double b = (G[0][Q] * G[0][Q] + G[1][Q] * G[1][Q]) + G[2][Q] * G[2][Q];
    const double g = (G[0][P] * G[0][Q] + G[1][P] * G[1][Q]) + G[2][P] * G[2][Q];
    double c, s;
    tv_rotation(a, b, g, &c, &s);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[r][P], gq = G[r][Q], vp = V[r][P], vq = V[r][Q];
        G[r][P] = c * gp - s * gq; G[r][Q] = s * gp + c * gq;
        V[r][P] = c * vp - s * vq; V[r][Q] = s * vp + c * vq;
    }
}

// columns P < Q of V (with their squared norms) change places when the later one is strictly larger
template <int P, int Q>
TV_HD void tv_order3(double (&n2)[3], double (&V)[3][3]) {
    const bool sw = n2[Q] > n2[P];
    const double t = n2[P];
    n2[P] = sw ? n2[Q] : t; n2[Q] = sw ? t : n2[Q];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = V[r][P];
        V[r][P] = sw ? V[r][Q] : x; V[r][Q] = sw ? x : V[r][Q];
    }
}

TV_HD void tv_svd33(const float m[9], float u[9], float w[3], float vt[9]) {
    double A[3][3], G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { A[r][c] = (double)m[3 * r + c]; G[r][c] = A[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SVD3_SWEEPS; ++sweep) {
        tv_rotate3<0, 1>(G, V); tv_rotate3<0, 2>(G, V); tv_rotate3<1, 2>(G, V);
    }
    double n2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n2[k] = (G[0][k] * G[0][k] + G[1][k] * G[1][k]) + G[2][k] * G[2][k];
    tv_order3<0, 1>(n2, V); tv_order3<1, 2>(n2, V); tv_order3<0, 1>(n2, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double big = 0.0;
        bool neg = false;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (fabs(V[r][k]) > big) { big = fabs(V[r][k]); neg = V[r][k] < 0.0; }
        double v[3], y[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) v[r] = neg ? -V[r][k] : V[r][k];
#pragma unroll
        for (int r = 0; r < 3; ++r) y[r] = (A[r][0] * v[0] + A[r][1] * v[1]) + A[r][2] * v[2];
        const double wk = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        w[k] = (float)wk;
#pragma unroll
        for (int r = 0; r < 3; ++r) { u[3 * r + k] = (float)(y[r] / wk); vt[3 * k + r] = (float)v[r]; }
    }
}

// ---- one hypothesis: the model of eight normalised pairs ----

// row pair of ComputeH21's A (:248-266) / row of ComputeF21's (:290-298) for the normalised pair (u1, v1) <-> (u2, v2)
TV_HD void tv_fill_rows(TvWork* W, int model, int j, float u1, float v1, float u2, float v2) {
    if (model == TV_MODEL_H) {
        double* a = W->G[2 * j];
        double* b = W->G[2 * j + 1];
        a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = (double)-u1; a[4] = (double)-v1; a[5] = -1.0;
        a[6] = (double)(v2 * u1); a[7] = (double)(v2 * v1); a[8] = (double)v2;
        b[0] = (double)u1; b[1] = (double)v1; b[2] = 1.0; b[3] = 0.0; b[4] = 0.0; b[5] = 0.0;
        b[6] = (double)(-u2 * u1); b[7] = (double)(-u2 * v1); b[8] = (double)-u2;
    } else {
        double* a = W->G[j];
        a[0] = (double)(u2 * u1); a[1] = (double)(u2 * v1); a[2] = (double)u2;
        a[3] = (double)(v2 * u1); a[4] = (double)(v2 * v1); a[5] = (double)v2;
        a[6] = (double)u1; a[7] = (double)v1; a[8] = 1.0;
    }
}

// rows of pair j of a hypothesis from the raw match p = (u1, v1, u2, v2) and the two normalisations
TV_HD void tv_fill_pair(TvWork* W, int model, int j, const float p[4], const TvNorm& n1, const TvNorm& n2) {
    tv_fill_rows(W, model, j, (p[0] - n1.meanX) * n1.sX, (p[1] - n1.meanY) * n1.sY, (p[2] - n2.meanX) * n2.sX, (p[3] - n2.meanY) * n2.sY);
}

// H21i (and its inverse H12i) or F21i of the eight pairs the team has put into W with tv_fill_pair
TV_HD void tv_model(const TvTeam& T, TvWork* W, int model, const TvNorm& n1, const TvNorm& n2, float M[9], float Minv[9]) {
    tv_sync();
    float h[9], T1[9], T2[9], L[9], tmp[9];
    tv_null9(T, W, model == TV_MODEL_H ? 16 : 8, h);
    tv_norm_matrix(n1, T1);
    tv_norm_matrix(n2, T2);
    if (model == TV_MODEL_H) {
        tv_inv33(T2, L);
        tv_mul33(L, h, tmp);
        tv_mul33(tmp, T1, M);
        tv_inv33(M, Minv);
    } else {
        float u[9], w[3], vt[9], d[9], Fn[9];
        tv_svd33(h, u, w, vt);
        d[0] = w[0]; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = w[1]; d[5] = 0.f; d[6] = 0.f; d[7] = 0.f; d[8] = 0.f;
        tv_mul33(u, d, tmp);
        tv_mul33(tmp, vt, Fn);
        tv_transpose33(T2, L);
        tv_mul33(L, Fn, tmp);
        tv_mul33(tmp, T1, M);
#pragma unroll
        for (int i = 0; i < 9; ++i) Minv[i] = 0.f;
    }
}

// ---- CheckHomography / CheckFundamental for one match: the two score terms and whether each passed its test ----

struct TvTerms { float t1, t2; bool ok1, ok2; };

TV_HD float tv_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

TV_HD TvTerms tv_check_h(const float H[9], const float Hi[9], const float p[4], float invSigmaSquare) {
    const float th = 5.991f;
    const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
    TvTerms r;
    const float w2in1inv = (float)(1.0 / (double)(Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    r.ok1 = !(chiSquare1 > th);
    r.t1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H[6] * u1 + H[7] * v1 + H[8]));
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    r.ok2 = !(chiSquare2 > th);
    r.t2 = th - chiSquare2;
    return r;
}

TV_HD TvTerms tv_check_f(const float F[9], const float p[4], float invSigmaSquare) {
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
    TvTerms r;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    r.ok1 = !(chiSquare1 > th);
    r.t1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    r.ok2 = !(chiSquare2 > th);
    r.t2 = thScore - chiSquare2;
    return r;
}

TV_HD TvTerms tv_check(int model, const float M[9], const float Minv[9], const float p[4], float invSigmaSquare) {
    return model == TV_MODEL_H ? tv_check_h(M, Minv, p, invSigmaSquare) : tv_check_f(M, p, invSigmaSquare);
}

// ---- the motions ----

struct TvMotion { float R[9], t[3], n[3]; };

// ReconstructH (:593-695): motion mi of the eight of H21 under K.  false = the d1/d2, d2/d3 early return (:606).
TV_HD bool tv_motion_h(const float H21[9], const float K[9], int mi, TvMotion* out) {
    float invK[9], tmp[9], A[9], U[9], w[3], Vt[9], V[9];
    tv_inv33(K, invK);
    tv_mul33(invK, H21, tmp);
    tv_mul33(tmp, K, A);
    tv_svd33(A, U, w, Vt);
    tv_transpose33(Vt, V);
    const float s = (float)((double)tv_det33(U) * (double)tv_det33(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
#pragma unroll
    for (int i = 0; i < 9; ++i) out->R[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { out->t[i] = 0.f; out->n[i] = 0.f; }
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const int i = mi & 3;
    const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
    const bool plus = i == 0 || i == 3;   // the sign pattern {+, -, -, +} of stheta and sphi
    const float dd = mi < 4 ? d1 + d3 : d1 - d3;   // d' = d2 for the first four motions, d' = -d2 for the others
    const float aux_s = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / (dd * d2);             // aux_stheta / aux_sphi
    const float co = mi < 4 ? (d2 * d2 + d1 * d3) / (dd * d2) : (d1 * d3 - d2 * d2) / (dd * d2);   // ctheta / cphi
    const float si = plus ? aux_s : -aux_s;
    const float Rp[9] = {co, 0.f, mi < 4 ? -si : si, 0.f, mi < 4 ? 1.f : -1.f, 0.f, si, 0.f, mi < 4 ? co : -co};
    const float ts = mi < 4 ? d1 - d3 : d1 + d3;
    const float tp[3] = {x1 * ts, 0.f * ts, (mi < 4 ? -x3 : x3) * ts}, np[3] = {x1, 0.f, x3};
    tv_mul33(U, Rp, tmp);
#pragma unroll
    for (int k = 0; k < 9; ++k) tmp[k] = s * tmp[k];
    tv_mul33(tmp, Vt, out->R);
    tv_mul31(U, tp, out->t);
    tv_unit3(out->t);
    tv_mul31(V, np, out->n);
    if (out->n[2] < 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) out->n[k] = -out->n[k];
    return true;
}

// ReconstructF (:488-506) with DecomposeE (:918-938): motion mi of (R1, t), (R2, t), (R1, -t), (R2, -t)
TV_HD void tv_motion_f(const float F21[9], const float K[9], int mi, TvMotion* out) {
    float Kt[9], tmp[9], E[9], u[9], w[3], vt[9];
    tv_transpose33(K, Kt);
    tv_mul33(Kt, F21, tmp);
    tv_mul33(tmp, K, E);
    tv_svd33(E, u, w, vt);
    float t[3] = {u[2], u[5], u[8]};
    tv_unit3(t);
    const float w01 = (mi & 1) ? 1.f : -1.f;   // W for R1, its transpose for R2
    const float Wm[9] = {0.f, w01, 0.f, -w01, 0.f, 0.f, 0.f, 0.f, 1.f};
    tv_mul33(u, Wm, tmp);
    tv_mul33(tmp, vt, out->R);
    if (tv_det33(out->R) < 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) out->R[k] = -out->R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { out->t[k] = (mi & 2) ? -t[k] : t[k]; out->n[k] = 0.f; }
}

TV_HD int tv_motion_count(int model) { return model == TV_MODEL_H ? 8 : 4; }

TV_HD bool tv_motion(int model, const float M[9], const float K[9], int mi, TvMotion* out) {
    if (model == TV_MODEL_H) return tv_motion_h(M, K, mi, out);
    tv_motion_f(M, K, mi, out);
    return true;
}

// ---- CheckRT (:807-916) ----

struct TvCamera {
    float fx, fy, cx, cy;
    float P1[12], P2[12];   // K [I | 0], K [R | t]
    float R[9], t[3], O2[3];
    float th2;
};

TV_HD void tv_camera(const float K[9], const TvMotion& m, float sigma, TvCamera* c) {
    c->fx = K[0]; c->fy = K[4]; c->cx = K[2]; c->cy = K[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c->P1[4 * i + j] = K[3 * i + j];
            c->P2[4 * i + j] = (K[3 * i] * m.R[j] + K[3 * i + 1] * m.R[3 + j]) + K[3 * i + 2] * m.R[6 + j];
        }
        c->P1[4 * i + 3] = 0.f;
        c->P2[4 * i + 3] = (K[3 * i] * m.t[0] + K[3 * i + 1] * m.t[1]) + K[3 * i + 2] * m.t[2];
        c->O2[i] = -((m.R[i] * m.t[0] + m.R[3 + i] * m.t[1]) + m.R[6 + i] * m.t[2]);
        c->t[i] = m.t[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) c->R[i] = m.R[i];
    c->th2 = (float)(4.0 * (double)(sigma * sigma));
}

// One inlier match p = (u1, v1, u2, v2): the verdict, the point (written from TV_RT_Z1 on, zero before) and cosParallax.
// TV_RT_OK counts towards nGood; *good is vbGood (only below 0.99998).
TV_HD int tv_check_rt(const TvCamera& c, const float p[4], float X[3], float* cosParallax, bool* good) {
    X[0] = 0.f; X[1] = 0.f; X[2] = 0.f;
    *cosParallax = 0.f;
    *good = false;
    float A[4][4], v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        A[0][j] = p[0] * c.P1[8 + j] - c.P1[j];
        A[1][j] = p[1] * c.P1[8 + j] - c.P1[4 + j];
        A[2][j] = p[2] * c.P2[8 + j] - c.P2[j];
        A[3][j] = p[3] * c.P2[8 + j] - c.P2[4 + j];
    }
    tri_null_vector(A, v);
    const float sc = (float)(1.0 / (double)v[3]);
    const float x[3] = {v[0] * sc, v[1] * sc, v[2] * sc};
    if (!isfinite(x[0]) || !isfinite(x[1]) || !isfinite(x[2])) return TV_RT_NOT_FINITE;
    X[0] = x[0]; X[1] = x[1]; X[2] = x[2];
    const float n2[3] = {x[0] - c.O2[0], x[1] - c.O2[1], x[2] - c.O2[2]};
    const float dist1 = (float)sqrt(tri_dot3d(x, x)), dist2 = (float)sqrt(tri_dot3d(n2, n2));
    const float cosP = (float)(tri_dot3d(x, n2) / (double)(dist1 * dist2));
    *cosParallax = cosP;
    if (x[2] <= 0 && cosP < 0.99998) return TV_RT_Z1;
    float x2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) x2[i] = ((c.R[3 * i] * x[0] + c.R[3 * i + 1] * x[1]) + c.R[3 * i + 2] * x[2]) + c.t[i];
    if (x2[2] <= 0 && cosP < 0.99998) return TV_RT_Z2;
    const float invZ1 = (float)(1.0 / (double)x[2]);
    const float im1x = c.fx * x[0] * invZ1 + c.cx, im1y = c.fy * x[1] * invZ1 + c.cy;
    const float squareError1 = (im1x - p[0]) * (im1x - p[0]) + (im1y - p[1]) * (im1y - p[1]);
    if (squareError1 > c.th2) return TV_RT_REPROJ1;
    const float invZ2 = (float)(1.0 / (double)x2[2]);
    const float im2x = c.fx * x2[0] * invZ2 + c.cx, im2y = c.fy * x2[1] * invZ2 + c.cy;
    const float squareError2 = (im2x - p[2]) * (im2x - p[2]) + (im2y - p[3]) * (im2y - p[3]);
    if (squareError2 > c.th2) return TV_RT_REPROJ2;
    *good = cosP < 0.99998;
    return TV_RT_OK;
}

// floats in ascending order as unsigned keys: negative below positive, -0 below +0, NaN at the ends
TV_HD uint32_t tv_cos_key(uint32_t bits) { return (bits >> 31) ? ~bits : bits | 0x80000000u; }
TV_HD uint32_t tv_cos_unkey(uint32_t key) { return (key >> 31) ? key & 0x7fffffffu : ~key; }

// ---- the host scans (Initializer.cc:157-180, :121-127, :508-578, :698-740) ----

// the hypothesis FindHomography / FindFundamental keep: the first strict maximum above 0; -1 when no score is above 0
static inline int tv_best_hypothesis(int n_hyp, const float* score) {
    float best = 0.f;
    int at = -1;
    for (int h = 0; h < n_hyp; ++h)
        if (score[h] > best) { best = score[h]; at = h; }
    return at;
}

// RH = SH / (SH + SF) > 0.40: 1 = reconstruct from the homography
static inline int tv_choose_h(float SH, float SF) {
    const float RH = SH / (SH + SF);
    return RH > 0.40 ? 1 : 0;
}

// parallax of a motion: acos(c) * 180 / CV_PI, 0 when nothing was accepted
static inline float tv_parallax_deg(int nGood, float cos_sel) {
    if (nGood <= 0) return 0.f;
    return (float)((double)(acosf(cos_sel) * 180) / 3.1415926535897932384626433832795);
}

// ReconstructF's cascade: the winning motion 0 .. 3 or -1.  N = inliers of the chosen hypothesis.
static inline int tv_pick_f(const int32_t nGood[4], const float parallax[4], int N, float minParallax, int minTriangulated) {
    int maxGood = nGood[0];
    for (int k = 1; k < 4; ++k) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
    const int n09 = (int)(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
    for (int k = 0; k < 4; ++k)
        if (nGood[k] > 0.7 * maxGood) ++nsimilar;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int k = 0; k < 4; ++k)
        if (maxGood == nGood[k]) return parallax[k] > minParallax ? k : -1;
    return -1;
}

// ReconstructH's best / second-best rule: the winning motion 0 .. 7 or -1
static inline int tv_pick_h(const int32_t nGood[8], const float parallax[8], int N, float minParallax, int minTriangulated) {
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    for (int i = 0; i < 8; ++i) {
        if (nGood[i] > bestGood) {
            secondBestGood = bestGood; bestGood = nGood[i]; bestSolutionIdx = i; bestParallax = parallax[i];
        } else if (nGood[i] > secondBestGood) {
            secondBestGood = nGood[i];
        }
    }
    if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) return bestSolutionIdx;
    return -1;
}

#endif
