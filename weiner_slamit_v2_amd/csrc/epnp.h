// epnp.h — PnPsolver::compute_pose (ORB_SLAM2/src/PnPsolver.cc:383-670, :675-958) and CheckInliers (:316-347) as one text for the
// host and the device.  Plain C++ over IEEE +,-,*,/ and sqrt, double throughout as the reference has it (CheckInliers keeps its
// float / double split); it must be compiled with -ffp-contract=off.  pnp.hip runs it on the device; the CPU tests of the
// restatement (tests/pnp_ref.py) and tools/bench_pnp.py build the same text with g++ for the host.
//
// A TEAM runs one solve: T threads that share one EpnpWork (LDS on the device) and meet at epnp_sync().  On the host T = 1 and the
// same loops run in order.  Work is spread as tasks (`for (k = lane; k < count; k += T)`): the 72 + 72 element updates of a Jacobi
// round, the 144 entries of a projector, the three branches of the solve (one thread each), the correspondences of a pass.  Sums
// over the correspondences are team reductions (epnp_reduce): per-thread partial sums in index order, then the wave sum of
// wave_ops.h and a fixed-order sum over the waves.  Their order differs from the reference's sequential one; on the host (T = 1)
// it is the reference's.
//
// TWO PINNED CONVENTIONS.  The reference's pose depends on choices cvSVD makes that are no function of the
// input; both are fixed here, and in tests/pnp_ref.py alike:
//   (a) a PCA axis of choose_control_points is negated if its largest-magnitude component is negative
//   (b) for a four-point set the four null-space vectors of M^T M are replaced by the pivoted Cholesky factor of the projector
//       P = V V^T: four times, the column j of the largest remaining diagonal, q = P[:, j] / sqrt(P[j][j]), P -= q q^T.
// For five points and more the vectors are the eigenvectors of the four smallest eigenvalues in ascending order (ut rows 11 .. 8).
//
// EVERY LOOP HAS A FIXED TRIP COUNT.  A quadruple may repeat an index (the reference's sampler can): the PCA is then rank-deficient
// and the pose not finite.  That is legal input, so no Jacobi loop exits on convergence: EPNP_JACOBI_SWEEPS / EPNP_SVD3_SWEEPS
// sweeps are run, whatever the matrix.  A NaN pose gives NaN errors, and a NaN error is not below its bound (as in the reference).
//
// Where the reference goes through OpenCV: cvSVD of the symmetric 3 x 3 and 12 x 12 is a cyclic Jacobi eigen-decomposition,
// cvInvert(CV_SVD) of the 3 x 3 an inverse by cofactors, cvSolve(CV_SVD) of the 6 x 4 / 6 x 3 / 6 x 5 systems the least-squares
// solve by the reference's own qr_solve, and the cvSVD of ABt a one-sided Jacobi.
#ifndef SLAMIT_EPNP_H
#define SLAMIT_EPNP_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include "wave_ops.h"
#define EPNP_HD __host__ __device__ __forceinline__
#else
#define EPNP_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define EPNP_GLOBAL __attribute__((address_space(1)))
#else
#define EPNP_GLOBAL
#endif

#ifndef EPNP_JACOBI_SWEEPS
#define EPNP_JACOBI_SWEEPS 11   // 12 x 12; the gap to the restatement stops falling after 9, plus two
#endif
#ifndef EPNP_SVD3_SWEEPS
#define EPNP_SVD3_SWEEPS 6      // both 3 x 3 decompositions; the gap stops falling after 4, plus two
#endif
#define EPNP_MAX_WAVES 4        // a team is at most 256 threads
#define EPNP_MAX_SUMS 78        // the distinct entries of M^T M

struct EpnpBranch {             // one of the three find_betas_approx_* branches
    double a[30], b[6], x[5], a1[5], a2[5];   // the 6 x nc system of qr_solve
    double betas[4];
    double ccs[12];             // control points in the camera frame, after solve_for_sign
    double pc0[3], R[9], t[3];
};

struct EpnpWork {
    double A[144];              // M^T M and its Jacobi iterate; the projector of rule (b)
    double V[144];              // eigenvectors in columns: V[12 i + j] is component i of vector j
    double cs[12];              // c, s of the six rotations of a round
    double v[48];               // v[12 k + i]: component i of null-space vector k (k = 0: ut row 11)
    double L[60], rho[6];
    double c0[3], cws[12], ci[9];
    double sum[EPNP_MAX_SUMS];
    double red[EPNP_MAX_WAVES * EPNP_MAX_SUMS];
    EpnpBranch br[3];
    int idx4[4];
};

struct EpnpTeam { int lane, size; };

// the correspondences of one solve: a quadruple of indices (which may repeat) or the members of a bit mask over [0, n)
struct EpnpSet {
    const EPNP_GLOBAL float* p3d;        // n x 3
    const EPNP_GLOBAL float* p2d;        // n x 2
    const EPNP_GLOBAL int32_t* quad;     // four indices, or null
    const EPNP_GLOBAL uint32_t* mask;    // (n + 31) / 32 words, when quad is null
    int span;                            // loop bound: 4, or n
    int nc;                              // number of correspondences: 4, or the mask's population count
    int first;                           // position in [0, span) of the first correspondence
    double fu, fv, uc, vc;
};

EPNP_HD void epnp_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

// position k of the set -> its point; false if k is no member
EPNP_HD bool epnp_get(const EpnpSet& S, int k, double pw[3], double uv[2]) {
    int i = k;
    if (S.quad) i = S.quad[k];
    else if (!((S.mask[k >> 5] >> (k & 31)) & 1u)) return false;
    pw[0] = S.p3d[3 * i]; pw[1] = S.p3d[3 * i + 1]; pw[2] = S.p3d[3 * i + 2];
    uv[0] = S.p2d[2 * i]; uv[1] = S.p2d[2 * i + 1];
    return true;
}

// W->sum[k] = sum over the team of acc[k], k < K.  Every thread of the team calls it.
template <int K>
EPNP_HD void epnp_reduce(const EpnpTeam& T, EpnpWork* W, double (&acc)[K]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = T.lane >> 6, nw = T.size >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(acc[k]);
        if ((T.lane & 63) == 0) W->red[wave * EPNP_MAX_SUMS + k] = s;
    }
    __syncthreads();
    for (int k = T.lane; k < K; k += T.size) {
        double s = W->red[k];
        for (int w = 1; w < nw; ++w) s += W->red[w * EPNP_MAX_SUMS + k];
        W->sum[k] = s;
    }
    __syncthreads();
#else
    for (int k = 0; k < K; ++k) W->sum[k] = acc[k];
#endif
}

// c, s of the Jacobi rotation that annihilates a_pq (Numerical Recipes' form); the identity for a_pq == 0
EPNP_HD void epnp_rotation(double app, double aqq, double apq, double* c, double* s) {
    *c = 1.0; *s = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        *c = 1.0 / sqrt(t * t + 1.0);
        *s = t * *c;
    }
}

// symmetric 3 x 3 (a: 00 01 02 11 12 22) -> eigenvalues descending in d, eigenvectors in the ROWS of ut (cvSVD's D and U^T), rule (a) applied
EPNP_HD void epnp_eig3(const double a[6], double d[3], double ut[9]) {
    double A[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < EPNP_SVD3_SWEEPS; ++sweep) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
            double c, s;
            epnp_rotation(A[p][p], A[q][q], A[p][q], &c, &s);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double x = A[i][p], y = A[i][q];
                A[i][p] = c * x - s * y; A[i][q] = s * x + c * y;
                const double vx = V[i][p], vy = V[i][q];
                V[i][p] = c * vx - s * vy; V[i][q] = s * vx + c * vy;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double x = A[p][j], y = A[q][j];
                A[p][j] = c * x - s * y; A[q][j] = s * x + c * y;
            }
        }
    }
    double w[3] = {A[0][0], A[1][1], A[2][2]};
    double R[3][3];   // rows = vectors
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) R[j][i] = V[i][j];
#define EPNP_SWAP3(x, y)                                                                                  \
    if (w[x] < w[y]) {                                                                                    \
        const double tw = w[x]; w[x] = w[y]; w[y] = tw;                                                   \
        for (int i_ = 0; i_ < 3; ++i_) { const double tv = R[x][i_]; R[x][i_] = R[y][i_]; R[y][i_] = tv; } \
    }
    EPNP_SWAP3(0, 1) EPNP_SWAP3(1, 2) EPNP_SWAP3(0, 1)
#undef EPNP_SWAP3
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double big = R[j][0];
        if (fabs(R[j][1]) > fabs(big)) big = R[j][1];
        if (fabs(R[j][2]) > fabs(big)) big = R[j][2];
        const double sg = big < 0.0 ? -1.0 : 1.0;
        d[j] = w[j];
#pragma unroll
        for (int i = 0; i < 3; ++i) ut[3 * j + i] = sg * R[j][i];
    }
}

// the orthogonal factor U V^T of a 3 x 3 (row-major m) by one-sided Jacobi, as estimate_R_and_t takes it from cvSVD
EPNP_HD void epnp_polar3(const double m[9], double R[9]) {
    double A[3][3] = {{m[0], m[1], m[2]}, {m[3], m[4], m[5]}, {m[6], m[7], m[8]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < EPNP_SVD3_SWEEPS; ++sweep) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
            const double al = A[0][p] * A[0][p] + A[1][p] * A[1][p] + A[2][p] * A[2][p];
            const double be = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q];
            const double ga = A[0][p] * A[0][q] + A[1][p] * A[1][q] + A[2][p] * A[2][q];
            double c, s;
            epnp_rotation(al, be, ga, &c, &s);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double x = A[i][p], y = A[i][q];
                A[i][p] = c * x - s * y; A[i][q] = s * x + c * y;
                const double vx = V[i][p], vy = V[i][q];
                V[i][p] = c * vx - s * vy; V[i][q] = s * vx + c * vy;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double inv = 1.0 / sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) R[3 * i + k] += (A[i][j] * inv) * V[k][j];
    }
}

// qr_solve (:868-958) line by line on a row-major nr x nc system; false (X untouched) where the reference returns silently on eta == 0
EPNP_HD bool epnp_qr_solve(double* A, int nr, int nc, double* b, double* X, double* A1, double* A2) {
    for (int k = 0; k < nc; ++k) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; ++i) {
            const double elt = fabs(A[i * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return false;
        }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; ++i) {
            A[i * nc + k] *= inv_eta;
            sum += A[i * nc + k] * A[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s2 = 0;
            for (int i = k; i < nr; ++i) s2 += A[i * nc + k] * A[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; ++i) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {   // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau += A[i * nc + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; ++i) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];   // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) sum += A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

// find_betas_approx_1 / 2 / 3 (:675-766) for branch br = 0 / 1 / 2, then gauss_newton (:820-866)
EPNP_HD void epnp_betas(EpnpWork* W, int br) {
    EpnpBranch& B = W->br[br];
    const double* L = W->L;
    const int nc = br == 0 ? 4 : (br == 1 ? 3 : 5);
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < nc; ++j) {
            int col = j;                                  // approx_2 and _3 take columns 0 .. nc-1,
            if (br == 0) col = j == 2 ? 3 : (j == 3 ? 6 : j);   // approx_1 takes 0 1 3 6
            B.a[i * nc + j] = L[10 * i + col];
        }
        B.b[i] = W->rho[i];
    }
    for (int j = 0; j < 5; ++j) B.x[j] = 0.0;
    epnp_qr_solve(B.a, 6, nc, B.b, B.x, B.a1, B.a2);
    const double b0 = B.x[0], b1 = B.x[1], b2 = B.x[2], b3 = B.x[3];
    double* betas = B.betas;
    if (br == 0) {
        if (b0 < 0) {
            betas[0] = sqrt(-b0); betas[1] = -b1 / betas[0]; betas[2] = -b2 / betas[0]; betas[3] = -b3 / betas[0];
        } else {
            betas[0] = sqrt(b0); betas[1] = b1 / betas[0]; betas[2] = b2 / betas[0]; betas[3] = b3 / betas[0];
        }
    } else {
        if (b0 < 0) {
            betas[0] = sqrt(-b0); betas[1] = (b2 < 0) ? sqrt(-b2) : 0.0;
        } else {
            betas[0] = sqrt(b0); betas[1] = (b2 > 0) ? sqrt(b2) : 0.0;
        }
        if (b1 < 0) betas[0] = -betas[0];
        betas[2] = br == 2 ? b3 / betas[0] : 0.0;
        betas[3] = 0.0;
    }
    for (int j = 0; j < 4; ++j) B.x[j] = 0.0;
    for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < 6; ++i) {
            const double* rowL = L + i * 10;
            double* rowA = B.a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            B.b[i] = W->rho[i] -
                     (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                      rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                      rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                      rowL[9] * betas[3] * betas[3]);
        }
        epnp_qr_solve(B.a, 6, 4, B.b, B.x, B.a1, B.a2);
        for (int i = 0; i < 4; ++i) betas[i] += B.x[i];
    }
}

// alphas of one point (compute_barycentric_coordinates, :431-441)
EPNP_HD void epnp_alphas(const EpnpWork* W, const double pw[3], double a[4]) {
    const double* ci = W->ci;
    const double d0 = pw[0] - W->cws[0], d1 = pw[1] - W->cws[1], d2 = pw[2] - W->cws[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// compute_pose (:485-533): the pose of the set in pose[12] (R row-major, t), the same in every thread of the team
EPNP_HD void epnp_compute_pose(const EpnpTeam& T, EpnpWork* W, const EpnpSet& S, double pose[12]) {
    const double nc = (double)S.nc;
    // ---- choose_control_points (:383-417)
    {
        double acc[3] = {0, 0, 0};
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2];
            if (epnp_get(S, k, pw, uv)) { acc[0] += pw[0]; acc[1] += pw[1]; acc[2] += pw[2]; }
        }
        epnp_reduce<3>(T, W, acc);
    }
    const double c0[3] = {W->sum[0] / nc, W->sum[1] / nc, W->sum[2] / nc};
    epnp_sync();
    {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2];
            if (epnp_get(S, k, pw, uv)) {
                const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
                acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
            }
        }
        epnp_reduce<6>(T, W, acc);
    }
    if (T.lane == 0) {
        const double cov[6] = {W->sum[0], W->sum[1], W->sum[2], W->sum[3], W->sum[4], W->sum[5]};
        double dc[3], uct[9];
        epnp_eig3(cov, dc, uct);
        double cc[9];   // cc[3 i + j - 1] = cws[j][i] - cws[0][i]
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            W->c0[j] = c0[j];
            W->cws[j] = c0[j];
        }
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            const double k = sqrt(dc[i - 1] / nc);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                W->cws[3 * i + j] = c0[j] + k * uct[3 * (i - 1) + j];
                cc[3 * j + i - 1] = W->cws[3 * i + j] - c0[j];
            }
        }
        // compute_barycentric_coordinates: the inverse by cofactors
        const double det = cc[0] * (cc[4] * cc[8] - cc[5] * cc[7]) - cc[1] * (cc[3] * cc[8] - cc[5] * cc[6]) + cc[2] * (cc[3] * cc[7] - cc[4] * cc[6]);
        const double id = 1.0 / det;
        W->ci[0] = (cc[4] * cc[8] - cc[5] * cc[7]) * id; W->ci[1] = (cc[2] * cc[7] - cc[1] * cc[8]) * id; W->ci[2] = (cc[1] * cc[5] - cc[2] * cc[4]) * id;
        W->ci[3] = (cc[5] * cc[6] - cc[3] * cc[8]) * id; W->ci[4] = (cc[0] * cc[8] - cc[2] * cc[6]) * id; W->ci[5] = (cc[2] * cc[3] - cc[0] * cc[5]) * id;
        W->ci[6] = (cc[3] * cc[7] - cc[4] * cc[6]) * id; W->ci[7] = (cc[1] * cc[6] - cc[0] * cc[7]) * id; W->ci[8] = (cc[0] * cc[4] - cc[1] * cc[3]) * id;
        // compute_rho (:810-818)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int p = (0x211000 >> (4 * r)) & 15, q = (0x332321 >> (4 * r)) & 15;
            const double e0 = W->cws[3 * p] - W->cws[3 * q], e1 = W->cws[3 * p + 1] - W->cws[3 * q + 1], e2 = W->cws[3 * p + 2] - W->cws[3 * q + 2];
            W->rho[r] = e0 * e0 + e1 * e1 + e2 * e2;
        }
    }
    epnp_sync();
    // ---- fill_M (:444-459) and M^T M: 78 sums
    {
        double acc[78];
#pragma unroll
        for (int k = 0; k < 78; ++k) acc[k] = 0.0;
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2], a[4];
            if (!epnp_get(S, k, pw, uv)) continue;
            epnp_alphas(W, pw, a);
            double m1[12], m2[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                m1[3 * i] = a[i] * S.fu; m1[3 * i + 1] = 0.0; m1[3 * i + 2] = a[i] * (S.uc - uv[0]);
                m2[3 * i] = 0.0; m2[3 * i + 1] = a[i] * S.fv; m2[3 * i + 2] = a[i] * (S.vc - uv[1]);
            }
            int e = 0;
#pragma unroll
            for (int r = 0; r < 12; ++r)
#pragma unroll
                for (int c = r; c < 12; ++c, ++e) acc[e] += m1[r] * m1[c] + m2[r] * m2[c];
        }
        epnp_reduce<78>(T, W, acc);
    }
    for (int k = T.lane; k < 144; k += T.size) {
        const int i = k / 12, j = k - 12 * i;
        const int r = i < j ? i : j, c = i < j ? j : i;
        W->A[k] = W->sum[r * 12 - (r * (r - 1)) / 2 + (c - r)];
        W->V[k] = i == j ? 1.0 : 0.0;
    }
    epnp_sync();
    // ---- cvSVD of M^T M: cyclic Jacobi, the six disjoint rotations of a round-robin round at once
    for (int sweep = 0; sweep < EPNP_JACOBI_SWEEPS; ++sweep) {
        for (int round = 0; round < 11; ++round) {
            for (int k = T.lane; k < 6; k += T.size) {
                int p = k == 0 ? 11 : (round + k) % 11, q = k == 0 ? round : (round + 11 - k) % 11;
                double c, s;
                epnp_rotation(W->A[13 * p], W->A[13 * q], W->A[12 * p + q], &c, &s);
                W->cs[2 * k] = c; W->cs[2 * k + 1] = s;
            }
            epnp_sync();
            for (int task = T.lane; task < 72; task += T.size) {   // columns of A and of V
                const int k = task / 12, i = task - 12 * k;
                const int p = k == 0 ? 11 : (round + k) % 11, q = k == 0 ? round : (round + 11 - k) % 11;
                const double c = W->cs[2 * k], s = W->cs[2 * k + 1];
                const double x = W->A[12 * i + p], y = W->A[12 * i + q];
                W->A[12 * i + p] = c * x - s * y; W->A[12 * i + q] = s * x + c * y;
                const double vx = W->V[12 * i + p], vy = W->V[12 * i + q];
                W->V[12 * i + p] = c * vx - s * vy; W->V[12 * i + q] = s * vx + c * vy;
            }
            epnp_sync();
            for (int task = T.lane; task < 72; task += T.size) {   // rows of A
                const int k = task / 12, j = task - 12 * k;
                const int p = k == 0 ? 11 : (round + k) % 11, q = k == 0 ? round : (round + 11 - k) % 11;
                const double c = W->cs[2 * k], s = W->cs[2 * k + 1];
                const double x = W->A[12 * p + j], y = W->A[12 * q + j];
                W->A[12 * p + j] = c * x - s * y; W->A[12 * q + j] = s * x + c * y;
            }
            epnp_sync();
        }
    }
    // the four smallest eigenvalues in ascending order; the indices stay in [0, 12) whatever the values (NaN compares false)
    if (T.lane == 0) {
        unsigned taken = 0;
        for (int k = 0; k < 4; ++k) {
            int best = 0;
            while ((taken >> best) & 1u) ++best;
            for (int j = best + 1; j < 12; ++j)
                if (!((taken >> j) & 1u) && W->A[13 * j] < W->A[13 * best]) best = j;
            taken |= 1u << best;
            W->idx4[k] = best;
        }
    }
    epnp_sync();
    for (int task = T.lane; task < 48; task += T.size) {
        const int k = task / 12, i = task - 12 * k;
        W->v[task] = W->V[12 * i + W->idx4[k]];
    }
    epnp_sync();
    if (S.nc == 4) {   // rule (b)
        for (int task = T.lane; task < 144; task += T.size) {
            const int i = task / 12, j = task - 12 * i;
            W->A[task] = (W->v[i] * W->v[j] + W->v[12 + i] * W->v[12 + j]) + (W->v[24 + i] * W->v[24 + j] + W->v[36 + i] * W->v[36 + j]);
        }
        epnp_sync();
        for (int k = 0; k < 4; ++k) {
            int jb = 0;
            for (int j = 1; j < 12; ++j)
                if (W->A[13 * j] > W->A[13 * jb]) jb = j;
            const double inv = 1.0 / sqrt(W->A[13 * jb]);
            for (int i = T.lane; i < 12; i += T.size) W->v[12 * k + i] = W->A[12 * i + jb] * inv;
            epnp_sync();
            for (int task = T.lane; task < 144; task += T.size) {
                const int i = task / 12, j = task - 12 * i;
                W->A[task] -= W->v[12 * k + i] * W->v[12 * k + j];
            }
            epnp_sync();
        }
    }
    // ---- compute_L_6x10 (:768-808)
    for (int task = T.lane; task < 60; task += T.size) {
        const int r = task / 10, c = task - 10 * r;
        const int p = (0x211000 >> (4 * r)) & 15, q = (0x332321 >> (4 * r)) & 15;
        const int a = (int)((0x3210210100ULL >> (4 * c)) & 15), b = (int)((0x3333222110ULL >> (4 * c)) & 15);
        const double* va = W->v + 12 * a;
        const double* vb = W->v + 12 * b;
        const double d = (va[3 * p] - va[3 * q]) * (vb[3 * p] - vb[3 * q]) + (va[3 * p + 1] - va[3 * q + 1]) * (vb[3 * p + 1] - vb[3 * q + 1]) +
                         (va[3 * p + 2] - va[3 * q + 2]) * (vb[3 * p + 2] - vb[3 * q + 2]);
        W->L[task] = a == b ? d : 2.0 * d;
    }
    epnp_sync();
    // ---- the three branches, one thread each: betas, compute_ccs (:461-472), solve_for_sign (:644-657) on the first point
    for (int br = T.lane; br < 3; br += T.size) {
        epnp_betas(W, br);
        EpnpBranch& B = W->br[br];
        for (int j = 0; j < 12; ++j)
            B.ccs[j] = ((B.betas[0] * W->v[j] + B.betas[1] * W->v[12 + j]) + B.betas[2] * W->v[24 + j]) + B.betas[3] * W->v[36 + j];
        double pw[3], uv[2], a[4];
        epnp_get(S, S.first, pw, uv);
        epnp_alphas(W, pw, a);
        const double z = a[0] * B.ccs[2] + a[1] * B.ccs[5] + a[2] * B.ccs[8] + a[3] * B.ccs[11];
        if (z < 0.0)
            for (int j = 0; j < 12; ++j) B.ccs[j] = -B.ccs[j];
    }
    epnp_sync();
    // ---- estimate_R_and_t (:577-635): pc0 (pw0 is the centroid c0), ABt, its SVD
    {
        double acc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = 0.0;
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2], a[4];
            if (!epnp_get(S, k, pw, uv)) continue;
            epnp_alphas(W, pw, a);
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                const double* ccs = W->br[br].ccs;
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 * br + j] += a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
            }
        }
        epnp_reduce<9>(T, W, acc);
    }
    for (int k = T.lane; k < 9; k += T.size) W->br[k / 3].pc0[k % 3] = W->sum[k] / nc;
    epnp_sync();
    {
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2], a[4];
            if (!epnp_get(S, k, pw, uv)) continue;
            epnp_alphas(W, pw, a);
            const double w0 = pw[0] - W->c0[0], w1 = pw[1] - W->c0[1], w2 = pw[2] - W->c0[2];
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                const double* ccs = W->br[br].ccs;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double pc = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
                    const double e = pc - W->br[br].pc0[j];
                    acc[9 * br + 3 * j] += e * w0; acc[9 * br + 3 * j + 1] += e * w1; acc[9 * br + 3 * j + 2] += e * w2;
                }
            }
        }
        epnp_reduce<27>(T, W, acc);
    }
    for (int br = T.lane; br < 3; br += T.size) {
        EpnpBranch& B = W->br[br];
        double abt[9], R[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) abt[k] = W->sum[9 * br + k];
        epnp_polar3(abt, R);
        const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
        if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            B.t[i] = B.pc0[i] - (R[3 * i] * W->c0[0] + R[3 * i + 1] * W->c0[1] + R[3 * i + 2] * W->c0[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) B.R[3 * i + j] = R[3 * i + j];
        }
    }
    epnp_sync();
    // ---- reprojection_error (:558-575) of the three branches and the choice (:526-528)
    {
        double acc[3] = {0, 0, 0};
        for (int k = T.lane; k < S.span; k += T.size) {
            double pw[3], uv[2];
            if (!epnp_get(S, k, pw, uv)) continue;
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                const double* R = W->br[br].R;
                const double* t = W->br[br].t;
                const double Xc = (R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2]) + t[0];
                const double Yc = (R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2]) + t[1];
                const double inv_Zc = 1.0 / ((R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2]) + t[2]);
                const double ue = S.uc + S.fu * Xc * inv_Zc, ve = S.vc + S.fv * Yc * inv_Zc;
                acc[br] += sqrt((uv[0] - ue) * (uv[0] - ue) + (uv[1] - ve) * (uv[1] - ve));
            }
        }
        epnp_reduce<3>(T, W, acc);
    }
    const double e1 = W->sum[0] / nc, e2 = W->sum[1] / nc, e3 = W->sum[2] / nc;
    int N = 0;
    if (e2 < e1) N = 1;
    if (e3 < (N == 1 ? e2 : e1)) N = 2;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose[k] = W->br[N].R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose[9 + k] = W->br[N].t[k];
    epnp_sync();   // W may be reused by the caller
}

// CheckInliers (:316-347) for one correspondence, with the reference's float / double split
EPNP_HD bool epnp_inlier(const double pose[12], float X, float Y, float Z, float u, float v, double fu, double fv, double uc, double vc, float max_err) {
    const float Xc = (float)(pose[0] * X + pose[1] * Y + pose[2] * Z + pose[9]);
    const float Yc = (float)(pose[3] * X + pose[4] * Y + pose[5] * Z + pose[10]);
    const float invZc = (float)(1 / (pose[6] * X + pose[7] * Y + pose[8] * Z + pose[11]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float distX = (float)(u - ue);
    const float distY = (float)(v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;   // NaN: an outlier
}

#endif
