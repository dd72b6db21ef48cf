// sim3_horn.h — one Sim3Solver hypothesis: ComputeSim3 (ORB_SLAM2/src/Sim3Solver.cc:226-337, Horn 1987) on three
// correspondences and the two projections of CheckInliers (:340-364, :382-423) for one correspondence.
// Plain C++ over IEEE +,-,*,/ and sqrt / atan2 / sin / cos, float and double exactly where the reference has them; it must be
// compiled with -ffp-contract=off.  sim3_ransac.hip runs it wave-uniform on the device; the CPU test of the restatement and
// tools/bench_sim3_ransac.py build the same text with g++ for the host.
//
// Where the reference goes through OpenCV the evaluation order below is the statement of it ("Sim3Solver"):
//   centroid        ((p0 + p1) + p2) * (float)(1.0 / 3)                                   cv::reduce + Mat / int
//   3x3 products    (a0 b0 + a1 b1) + a2 b2 in float                                      cv::gemm on CV_32F
//   N               double sums of the float M entries, rounded to float                  :247-265
//   eigenvector     cyclic Jacobi in float on the 4x4 N; sign fixed to q0 >= 0            cv::eigen, CV_32F
//   ang             atan2(sqrt(double sum of squares), q0) in double                      :278
//   angle-axis      (float)((2 ang / norm) * v)                                           :280
//   Rodrigues       double: c I + (1 - c) r r^T + s [r]x with theta = |v|, stored float   cv::Rodrigues
//   scale           double sums of float products, nom / den                              :292-309
#ifndef SLAMIT_SIM3_HORN_H
#define SLAMIT_SIM3_HORN_H
#include <math.h>

#if defined(__HIPCC__)
#define SIM3H_HD __host__ __device__ __forceinline__
#else
#define SIM3H_HD static inline
#endif

struct Sim3Hyp {
    float R[9], t[3], s;      // mR12i (row-major), mt12i, ms12i
    float sR[9];              // rotation block of mT12i (its translation is t)
    float sRi[9], ti[3];      // mT21i
};

SIM3H_HD float sim3h_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// One Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into V (columns = eigenvectors).  P and Q are
// compile-time so that A and V stay in registers.
template <int P, int Q>
SIM3H_HD void sim3h_rotate(float (&A)[4][4], float (&V)[4][4], bool late) {
    const float apq = A[P][Q];
    const float g = 100.0f * fabsf(apq);
    if (late && fabsf(A[P][P]) + g == fabsf(A[P][P]) && fabsf(A[Q][Q]) + g == fabsf(A[Q][Q])) {
        A[P][Q] = 0.f; A[Q][P] = 0.f;
        return;
    }
    if (!(fabsf(apq) > 0.f)) return;   // zero, or NaN: nothing to rotate
    const float h = A[Q][Q] - A[P][P];
    float t;
    if (fabsf(h) + g == fabsf(h)) {
        t = apq / h;
    } else {
        const float theta = 0.5f * h / apq;
        t = 1.0f / (fabsf(theta) + sqrtf(1.0f + theta * theta));
        if (theta < 0.f) t = -t;
    }
    const float c = 1.0f / sqrtf(1.0f + t * t), s = t * c, tau = s / (1.0f + c);
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = 0.f; A[Q][P] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const float a = A[r][P], b = A[r][Q];
            const float na = a - s * (b + a * tau), nb = b + s * (a - b * tau);
            A[r][P] = na; A[P][r] = na; A[r][Q] = nb; A[Q][r] = nb;
        }
        const float va = V[r][P], vb = V[r][Q];
        V[r][P] = va - s * (vb + va * tau);
        V[r][Q] = vb + s * (va - vb * tau);
    }
}

// eigenvector of the largest eigenvalue of the symmetric 4x4 N (upper triangle n11 n12 n13 n14 n22 n23 n24 n33 n34 n44), q0 >= 0
SIM3H_HD void sim3h_top_eigenvector(const float n[10], float q[4]) {
    float A[4][4] = {{n[0], n[1], n[2], n[3]}, {n[1], n[4], n[5], n[6]}, {n[2], n[5], n[7], n[8]}, {n[3], n[6], n[8], n[9]}};
    float V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep) {
        const float off = ((fabsf(A[0][1]) + fabsf(A[0][2])) + (fabsf(A[0][3]) + fabsf(A[1][2]))) + (fabsf(A[1][3]) + fabsf(A[2][3]));
        if (!(off > 0.f)) break;   // converged (or NaN)
        const bool late = sweep > 3;
        sim3h_rotate<0, 1>(A, V, late); sim3h_rotate<0, 2>(A, V, late); sim3h_rotate<0, 3>(A, V, late);
        sim3h_rotate<1, 2>(A, V, late); sim3h_rotate<1, 3>(A, V, late); sim3h_rotate<2, 3>(A, V, late);
    }
    float best = A[0][0];
    q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = A[k][k] > best;
        best = up ? A[k][k] : best;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = up ? V[r][k] : q[r];
    }
    if (q[0] < 0.f) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
}

// P1[k], P2[k]: the k-th sampled point of mvX3Dc1 / mvX3Dc2 (the columns of P3Dc1i / P3Dc2i)
SIM3H_HD void sim3h_solve(const float P1[3][3], const float P2[3][3], int fix_scale, Sim3Hyp& H) {
    const float third = (float)(1.0 / 3.0);
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];   // Pr[row = axis][col = point]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        O1[a] = ((P1[0][a] + P1[1][a]) + P1[2][a]) * third;
        O2[a] = ((P2[0][a] + P2[1][a]) + P2[2][a]) * third;
#pragma unroll
        for (int k = 0; k < 3; ++k) { Pr1[a][k] = P1[k][a] - O1[a]; Pr2[a][k] = P2[k][a] - O2[a]; }
    }
    float M[3][3];   // M = Pr2 * Pr1^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = sim3h_dot3(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
    const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2], m20 = M[2][0], m21 = M[2][1], m22 = M[2][2];
    const float n[10] = {(float)(m00 + m11 + m22), (float)(m12 - m21), (float)(m20 - m02), (float)(m01 - m10), (float)(m00 - m11 - m22),
                         (float)(m01 + m10), (float)(m20 + m02), (float)(-m00 + m11 - m22), (float)(m12 + m21), (float)(-m00 - m11 + m22)};
    float q[4];
    sim3h_top_eigenvector(n, q);
    const double nrm = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
    const double ang = atan2(nrm, (double)q[0]);
    const double k = (2.0 * ang) / nrm;
    const float v[3] = {(float)(k * (double)q[1]), (float)(k * (double)q[2]), (float)(k * (double)q[3])};
    // cv::Rodrigues, vector to matrix, in double
    double rx = v[0], ry = v[1], rz = v[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < 2.2204460492503131e-16) {   // (a NaN vector, from norm == 0, fails this test and flows on as NaN: every pair an outlier)
#pragma unroll
        for (int i = 0; i < 9; ++i) H.R[i] = (i % 4 == 0) ? 1.f : 0.f;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
        rx *= it; ry *= it; rz *= it;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double rxm[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
        for (int i = 0; i < 9; ++i) H.R[i] = (float)((c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * rxm[i]);
    }
    float s12 = 1.0f;
    if (!fix_scale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float p3 = sim3h_dot3(H.R[3 * i], H.R[3 * i + 1], H.R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);   // P3 = R * Pr2
                nom += (double)(Pr1[i][j] * p3);
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    }
    H.s = s12;
    const double inv_s = 1.0 / (double)s12;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        H.t[i] = O1[i] - s12 * sim3h_dot3(H.R[3 * i], H.R[3 * i + 1], H.R[3 * i + 2], O2[0], O2[1], O2[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) { H.sR[3 * i + j] = s12 * H.R[3 * i + j]; H.sRi[3 * i + j] = (float)(inv_s * (double)H.R[3 * j + i]); }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) H.ti[i] = -sim3h_dot3(H.sRi[3 * i], H.sRi[3 * i + 1], H.sRi[3 * i + 2], H.t[0], H.t[1], H.t[2]);
}

// Project (:382-403) of X through [A | b] and K = (fx fy cx cy); FromCameraToImage (:405-423) is the same with no transform
SIM3H_HD void sim3h_image(const float X[3], const float K[4], float uv[2]) {
    const float invz = 1.0f / X[2];
    uv[0] = K[0] * (X[0] * invz) + K[2];
    uv[1] = K[1] * (X[1] * invz) + K[3];
}
SIM3H_HD void sim3h_project(const float A[9], const float b[3], const float X[3], const float K[4], float uv[2]) {
    const float Y[3] = {sim3h_dot3(A[0], A[1], A[2], X[0], X[1], X[2]) + b[0], sim3h_dot3(A[3], A[4], A[5], X[0], X[1], X[2]) + b[1],
                        sim3h_dot3(A[6], A[7], A[8], X[0], X[1], X[2]) + b[2]};
    sim3h_image(Y, K, uv);
}

// CheckInliers for one correspondence: err1 in image 1, err2 in image 2 (float squared distances)
SIM3H_HD void sim3h_errors(const Sim3Hyp& H, const float X1[3], const float X2[3], const float K1[4], const float K2[4], float* err1, float* err2) {
    float p1im1[2], p2im2[2], p2im1[2], p1im2[2];
    sim3h_image(X1, K1, p1im1);
    sim3h_image(X2, K2, p2im2);
    sim3h_project(H.sR, H.t, X2, K1, p2im1);
    sim3h_project(H.sRi, H.ti, X1, K2, p1im2);
    const float d1x = p1im1[0] - p2im1[0], d1y = p1im1[1] - p2im1[1], d2x = p1im2[0] - p2im2[0], d2y = p1im2[1] - p2im2[1];
    *err1 = d1x * d1x + d1y * d1y;
    *err2 = d2x * d2x + d2y * d2y;
}

#endif
