// ba_oracle.cc — CPU ORACLE for Optimizer::LocalBundleAdjustment.  TEST INFRASTRUCTURE ONLY.
//
// Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library
// (oracle/libba_oracle.so).  Nothing under weiner_slamit_v2_amd/ links or calls it.
//
// A from-scratch, single-threaded, fp64 restatement of what g2o does for the reference's local
// BA (reference paths: "S/" = ORB_SLAM2/src/, "G/" = Thirdparty/g2o/g2o/):
//   schedule, gates             S/Optimizer.cc:659-743
//   residual / Jacobians        G/types/types_six_dof_expmap.h:90-101, .cpp:103-147
//   Huber weighting             G/core/robust_kernel_impl.cpp:77-90, G/core/base_edge.h:96-102
//   normal equations            G/core/base_binary_edge.hpp:55-120, G/core/block_solver.hpp:502-560
//   Schur complement + solve    G/core/block_solver.hpp:367-486 (dense LDLt here instead of
//                               G/solvers/linear_solver_eigen.h's sparse SimplicialLDLT)
//   Levenberg-Marquardt control G/core/optimization_algorithm_levenberg.cpp:61-189
//   manifold updates            G/types/se3quat.h:218-253,103-109,276-281, types_sba.h:52-56
//
// PARITY STATUS: PINNED.  The reference's own g2o + Eigen compile in the authoring container
// (oracle/Makefile.ref -> oracle/_ref/libba_ref.so, driven by oracle/ba_ref_harness.cc); this
// restatement is checked against it there (tests/test_oracle_ba.py::test_vs_reference_g2o) and
// against the golden vectors it produced (tests/golden/ba_*.npz, tools/gen_ba_golden.py), which
// travel to the GPU box.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../include/slamit.h"

namespace {

struct Pose { double q[4]; double t[3]; };  // q = (x, y, z, w), world -> camera

inline void quat_to_R(const double q[4], double R[9]) {
    // Eigen::Quaterniond::toRotationMatrix
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

inline void R_to_quat(const double m[9], double q[4]) {
    // Eigen's rotation matrix -> quaternion (Shepperd, trace branch first)
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

inline void quat_normalize(double q[4]) {  // SE3Quat::normalizeRotation
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
    double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
}

inline void quat_mul(const double a[4], const double b[4], double r[4]) {
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

inline void quat_rot(const double q[4], const double v[3], double r[3]) {
    // Eigen: v + w*uv + u x uv, uv = 2 (u x v)
    double uv[3] = {2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])};
    r[0] = v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    r[1] = v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    r[2] = v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}

inline void mat3_mul(const double a[9], const double b[9], double c[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// T <- exp(update) * T, update = [omega, upsilon]     (SE3Quat::exp, VertexSE3Expmap::oplusImpl)
void pose_oplus(Pose& T, const double* u) {
    const double* w = u;
    const double* ups = u + 3;
    double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double O2[9];
    mat3_mul(O, O, O2);
    double R[9], V[9];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
        memcpy(V, R, sizeof(R));
    } else {
        double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / pow(theta, 3);
        for (int i = 0; i < 9; ++i) {
            double I = (i % 4 == 0 ? 1.0 : 0.0);
            R[i] = I + a * O[i] + b * O2[i];
            V[i] = I + b * O[i] + c * O2[i];
        }
    }
    double qe[4], te[3];
    R_to_quat(R, qe);
    quat_normalize(qe);  // SE3Quat(q, t) constructor normalises
    for (int i = 0; i < 3; ++i) te[i] = V[3 * i] * ups[0] + V[3 * i + 1] * ups[1] + V[3 * i + 2] * ups[2];
    // result = exp * T :  t = te + qe * T.t ; q = qe * T.q ; normalise
    double rt[3];
    quat_rot(qe, T.t, rt);
    double nq[4];
    quat_mul(qe, T.q, nq);
    for (int i = 0; i < 3; ++i) T.t[i] = te[i] + rt[i];
    memcpy(T.q, nq, sizeof(nq));
    quat_normalize(T.q);
}

struct Edge {
    int kf, pt;
    double u, v, w;
    double ur;       // right-image column of a stereo observation (EdgeStereoSE3ProjectXYZ); unused for a monocular edge
    bool stereo;
    bool active, robust;
    double err[3];   // err[2] = 0 for a monocular edge
    double chi2;
};

struct Problem {
    int K, P, E;
    std::vector<Pose> poses;
    std::vector<uint8_t> fixed;
    std::vector<double> intr, pts;
    std::vector<Edge> edges;
    double delta, gate;
    double delta_s, gate_s;        // stereo edges: S/Optimizer.cc:570 (thHuberStereo), :696 / :740 (7.815)
    std::vector<double> bf;        // per keyframe: KeyFrame::mbf (S/Optimizer.cc:641)
    const volatile uint8_t* stop;
    // index mapping of the current stage
    std::vector<int> pose_col;  // -1 = fixed, else block index among free poses
    int nfree;
};

inline bool stopped(const Problem& pb) { return pb.stop && *pb.stop; }

// computeActiveErrors + activeRobustChi2
double compute_errors(Problem& pb) {
    double total = 0;
    // RobustKernelHuber keeps delta^2 in a FLOAT member (G/core/robust_kernel_impl.h:84, set by setDelta :64-68)
    const double dsqr = (double)(float)(pb.delta * pb.delta);
    for (int e = 0; e < pb.E; ++e) {
        Edge& ed = pb.edges[e];
        if (!ed.active) continue;
        const Pose& T = pb.poses[ed.kf];
        double Xc[3];
        quat_rot(T.q, &pb.pts[3 * ed.pt], Xc);
        for (int i = 0; i < 3; ++i) Xc[i] += T.t[i];
        const double* in = &pb.intr[4 * ed.kf];
        double delta = pb.delta, dq = dsqr;
        if (!ed.stereo) {
            ed.err[0] = ed.u - (Xc[0] / Xc[2] * in[0] + in[2]);  // project2d then *fx + cx
            ed.err[1] = ed.v - (Xc[1] / Xc[2] * in[1] + in[3]);
            ed.err[2] = 0.0;
            ed.chi2 = ed.err[0] * ed.w * ed.err[0] + ed.err[1] * ed.w * ed.err[1];
        } else {
            // EdgeStereoSE3ProjectXYZ::cam_project (G/types/types_six_dof_expmap.cpp:150-157): the inverse depth is a FLOAT
            // (1.0f / z rounded to float), bf arrives through a `const float&`, and bf * invz is a float product
            const float invz = (float)(1.0 / Xc[2]);
            const double r0 = Xc[0] * (double)invz * in[0] + in[2];
            const double r1 = Xc[1] * (double)invz * in[1] + in[3];
            const float bfz = (float)pb.bf[ed.kf] * invz;
            const double r2 = r0 - (double)bfz;
            ed.err[0] = ed.u - r0; ed.err[1] = ed.v - r1; ed.err[2] = ed.ur - r2;
            ed.chi2 = ed.err[0] * ed.w * ed.err[0] + ed.err[1] * ed.w * ed.err[1] + ed.err[2] * ed.w * ed.err[2];
            delta = pb.delta_s; dq = (double)(float)(delta * delta);
        }
        if (ed.robust) {
            if (ed.chi2 <= dq) total += ed.chi2;
            else total += 2 * sqrt(ed.chi2) * delta - dq;
        } else total += ed.chi2;
    }
    return total;
}

struct System {
    int np, nl;
    std::vector<double> Hpp, Hll, Hpl, bp, bl;  // Hpp nfree*36 (row-major 6x6), Hll P*9, Hpl E*18 (6x3), b
};

void build_system(Problem& pb, System& S) {
    S.np = pb.nfree; S.nl = pb.P;
    S.Hpp.assign((size_t)S.np * 36, 0.0); S.Hll.assign((size_t)pb.P * 9, 0.0); S.Hpl.assign((size_t)pb.E * 18, 0.0);
    S.bp.assign((size_t)S.np * 6, 0.0); S.bl.assign((size_t)pb.P * 3, 0.0);
    const double dsqr = (double)(float)(pb.delta * pb.delta);   // (a float in the reference, see compute_errors)
    for (int e = 0; e < pb.E; ++e) {
        const Edge& ed = pb.edges[e];
        if (!ed.active) continue;
        const Pose& T = pb.poses[ed.kf];
        const double* in = &pb.intr[4 * ed.kf];
        const double fx = in[0], fy = in[1];
        double Xc[3], R[9];
        quat_rot(T.q, &pb.pts[3 * ed.pt], Xc);
        for (int i = 0; i < 3; ++i) Xc[i] += T.t[i];
        quat_to_R(T.q, R);
        const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
        double A[9], B[18];   // rows 0, 1 (and 2 for a stereo edge; zero otherwise)
        for (int i = 6; i < 9; ++i) A[i] = 0.0;
        for (int i = 12; i < 18; ++i) B[i] = 0.0;
        double delta = pb.delta, dq = dsqr;
        if (!ed.stereo) {
            // _jacobianOplusXi = -1/z * tmp * R
            double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 3; ++c)
                    A[3 * r + c] = -1. / z * (tmp[3 * r] * R[c] + tmp[3 * r + 1] * R[3 + c] + tmp[3 * r + 2] * R[6 + c]);
            B[0] = x * y / z_2 * fx; B[1] = -(1 + (x * x / z_2)) * fx; B[2] = y / z * fx;
            B[3] = -1. / z * fx; B[4] = 0; B[5] = x / z_2 * fx;
            B[6] = (1 + y * y / z_2) * fy; B[7] = -x * y / z_2 * fy; B[8] = -x / z * fy;
            B[9] = 0; B[10] = -1. / z * fy; B[11] = y / z_2 * fy;
        } else {
            // EdgeStereoSE3ProjectXYZ::linearizeOplus (G/types/types_six_dof_expmap.cpp:188-234), its expressions as written
            const double bf = pb.bf[ed.kf];
            for (int c = 0; c < 3; ++c) {
                A[c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
                A[3 + c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
                A[6 + c] = A[c] - bf * R[6 + c] / z_2;
            }
            B[0] = x * y / z_2 * fx; B[1] = -(1 + (x * x / z_2)) * fx; B[2] = y / z * fx;
            B[3] = -1. / z * fx; B[4] = 0; B[5] = x / z_2 * fx;
            B[6] = (1 + y * y / z_2) * fy; B[7] = -x * y / z_2 * fy; B[8] = -x / z * fy;
            B[9] = 0; B[10] = -1. / z * fy; B[11] = y / z_2 * fy;
            B[12] = B[0] - bf * y / z_2; B[13] = B[1] + bf * x / z_2; B[14] = B[2];
            B[15] = B[3]; B[16] = 0; B[17] = B[5] - bf / z_2;
            delta = pb.delta_s; dq = (double)(float)(delta * delta);
        }
        double rho1 = 1.0;
        if (ed.robust && ed.chi2 > dq) rho1 = delta / sqrt(ed.chi2);
        const double wO = rho1 * ed.w;                       // weightedOmega = rho[1] * information
        const double r0 = -ed.w * ed.err[0] * rho1, r1 = -ed.w * ed.err[1] * rho1, r2 = -ed.w * ed.err[2] * rho1;  // omega_r
        double* bl = &S.bl[3 * ed.pt];
        double* Hl = &S.Hll[9 * ed.pt];
        for (int i = 0; i < 3; ++i) {
            bl[i] += A[i] * r0 + A[3 + i] * r1 + A[6 + i] * r2;
            for (int j = 0; j < 3; ++j) Hl[3 * i + j] += (A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j]) * wO;
        }
        const int col = pb.pose_col[ed.kf];
        if (col >= 0) {
            double* bq = &S.bp[6 * col];
            double* Hp = &S.Hpp[36 * col];
            double* Hx = &S.Hpl[18 * (size_t)e];
            for (int i = 0; i < 6; ++i) {
                bq[i] += B[i] * r0 + B[6 + i] * r1 + B[12 + i] * r2;
                for (int j = 0; j < 6; ++j) Hp[6 * i + j] += (B[i] * B[j] + B[6 + i] * B[6 + j] + B[12 + i] * B[12 + j]) * wO;
                for (int j = 0; j < 3; ++j) Hx[3 * i + j] += (B[i] * A[j] + B[6 + i] * A[3 + j] + B[12 + i] * A[6 + j]) * wO;
            }
        }
    }
}

inline bool inv3(const double* m, double* o) {
    double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    double id = 1.0 / det;
    o[0] = c0 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c1 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c2 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    return true;
}

// dense LDLt without pivoting on the upper triangle; false if a pivot is exactly zero
// (what SimplicialLDLT reports as NumericalIssue)
bool ldlt_solve(std::vector<double>& A, int n, std::vector<double>& b) {
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k] * A[(size_t)k * n + k];
        if (d == 0.0 || !std::isfinite(d)) return false;
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k] * A[(size_t)k * n + k];
            A[(size_t)i * n + j] = s / d;
        }
    }
    for (int i = 0; i < n; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * b[k]; b[i] = s; }
    for (int i = 0; i < n; ++i) b[i] /= A[(size_t)i * n + i];
    for (int i = n - 1; i >= 0; --i) { double s = b[i]; for (int k = i + 1; k < n; ++k) s -= A[(size_t)k * n + i] * b[k]; b[i] = s; }
    return true;
}

// BlockSolver::solve with the diagonal already augmented by lambda. x = [poses | points]
bool solve_schur(const Problem& pb, const System& S, double lambda, const std::vector<std::vector<int> >& pt_edges,
                 std::vector<double>& x) {
    const int n = 6 * S.np;
    std::vector<double> Sm((size_t)n * n, 0.0), bs(S.bp), Dinv((size_t)pb.P * 9), coeff(n, 0.0);
    for (int k = 0; k < S.np; ++k)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) Sm[(size_t)(6 * k + i) * n + 6 * k + j] = S.Hpp[36 * k + 6 * i + j] + (i == j ? lambda : 0.0);
    for (int p = 0; p < pb.P; ++p) {
        double D[9];
        for (int i = 0; i < 9; ++i) D[i] = S.Hll[9 * p + i] + (i % 4 == 0 ? lambda : 0.0);
        double* Di = &Dinv[9 * (size_t)p];
        inv3(D, Di);
        double db[3];
        for (int i = 0; i < 3; ++i) db[i] = Di[3 * i] * S.bl[3 * p] + Di[3 * i + 1] * S.bl[3 * p + 1] + Di[3 * i + 2] * S.bl[3 * p + 2];
        const std::vector<int>& es = pt_edges[p];
        for (size_t a = 0; a < es.size(); ++a) {
            const int e1 = es[a], c1 = pb.pose_col[pb.edges[e1].kf];
            if (c1 < 0) continue;
            const double* B1 = &S.Hpl[18 * (size_t)e1];
            double BD[18];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 3; ++j) BD[3 * i + j] = B1[3 * i] * Di[j] + B1[3 * i + 1] * Di[3 + j] + B1[3 * i + 2] * Di[6 + j];
            for (int i = 0; i < 6; ++i) coeff[6 * c1 + i] += B1[3 * i] * db[0] + B1[3 * i + 1] * db[1] + B1[3 * i + 2] * db[2];
            for (size_t b2 = 0; b2 < es.size(); ++b2) {
                const int e2 = es[b2], c2 = pb.pose_col[pb.edges[e2].kf];
                if (c2 < 0) continue;
                const double* B2 = &S.Hpl[18 * (size_t)e2];
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j)
                        Sm[(size_t)(6 * c1 + i) * n + 6 * c2 + j] -= BD[3 * i] * B2[3 * j] + BD[3 * i + 1] * B2[3 * j + 1] + BD[3 * i + 2] * B2[3 * j + 2];
            }
        }
    }
    for (int i = 0; i < n; ++i) bs[i] -= coeff[i];
    x.assign((size_t)n + 3 * pb.P, 0.0);
    bool ok = true;
    if (n > 0) ok = ldlt_solve(Sm, n, bs);
    if (!ok) return false;
    for (int i = 0; i < n; ++i) x[i] = bs[i];
    // xl = Dinv * (bl - Bt * xp)
    for (int p = 0; p < pb.P; ++p) {
        double cl[3] = {S.bl[3 * p], S.bl[3 * p + 1], S.bl[3 * p + 2]};
        const std::vector<int>& es = pt_edges[p];
        for (size_t a = 0; a < es.size(); ++a) {
            const int e = es[a], c = pb.pose_col[pb.edges[e].kf];
            if (c < 0) continue;
            const double* B = &S.Hpl[18 * (size_t)e];
            for (int j = 0; j < 3; ++j)
                for (int i = 0; i < 6; ++i) cl[j] -= B[3 * i + j] * x[6 * c + i];
        }
        const double* Di = &Dinv[9 * (size_t)p];
        for (int i = 0; i < 3; ++i) x[n + 3 * p + i] = Di[3 * i] * cl[0] + Di[3 * i + 1] * cl[1] + Di[3 * i + 2] * cl[2];
    }
    return true;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg
int optimize(Problem& pb, int iterations, int stage, slamit_ba_stats* st) {
    // index mapping: free poses in id order (every free pose keeps a column even without active
    // edges: it then has a zero Hessian and a zero update; g2o leaves such a vertex out of the
    // optimisation, so its estimate is not even re-normalised: in_graph[k] = 0 skips its oplus)
    pb.pose_col.assign(pb.K, -1);
    pb.nfree = 0;
    for (int k = 0; k < pb.K; ++k) if (!pb.fixed[k]) pb.pose_col[k] = pb.nfree++;
    std::vector<std::vector<int> > pt_edges(pb.P);
    for (int e = 0; e < pb.E; ++e) if (pb.edges[e].active) pt_edges[pb.edges[e].pt].push_back(e);
    std::vector<char> in_graph(pb.K, 0);
    for (int e = 0; e < pb.E; ++e) if (pb.edges[e].active) in_graph[pb.edges[e].kf] = 1;
    bool any_active = false;
    for (int e = 0; e < pb.E; ++e) any_active |= pb.edges[e].active;
    if (!any_active) return 0;  // g2o: "0 vertices to optimize" -> optimize() returns without iterating
    const double tau = 1e-5, upper = 2. / 3., lower = 1. / 3.;
    const int maxTrials = 10;
    double lambda = -1, ni = 2;
    int nBad = 0, done = 0;
    System S;
    std::vector<double> x;
    bool ok = true;
    for (int it = 0; it < iterations && !stopped(pb) && ok; ++it) {
        double currentChi = compute_errors(pb);
        double tempChi = currentChi;
        const double iniChi = currentChi;
        build_system(pb, S);
        if (it == 0) {
            double maxDiag = 0;
            for (int k = 0; k < S.np; ++k) for (int j = 0; j < 6; ++j) maxDiag = std::max(fabs(S.Hpp[36 * k + 7 * j]), maxDiag);
            for (int p = 0; p < pb.P; ++p) for (int j = 0; j < 3; ++j) maxDiag = std::max(fabs(S.Hll[9 * p + 4 * j]), maxDiag);
            lambda = tau * maxDiag;
            ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            std::vector<Pose> backupPoses = pb.poses;  // push()
            std::vector<double> backupPts = pb.pts;
            bool ok2 = solve_schur(pb, S, lambda, pt_edges, x);
            if (ok2 || !x.empty()) {  // update(_solver->x())
                if (x.size() == (size_t)6 * S.np + 3 * pb.P) {
                    for (int k = 0; k < pb.K; ++k) if (pb.pose_col[k] >= 0 && in_graph[k]) pose_oplus(pb.poses[k], &x[6 * pb.pose_col[k]]);
                    for (int i = 0; i < 3 * pb.P; ++i) pb.pts[i] += x[6 * S.np + i];
                }
            }
            tempChi = compute_errors(pb);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;  // computeScale
            for (int k = 0; k < 6 * S.np; ++k) scale += x[k] * (lambda * x[k] + S.bp[k]);
            for (int k = 0; k < 3 * pb.P; ++k) scale += x[6 * S.np + k] * (lambda * x[6 * S.np + k] + S.bl[k]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - pow((2 * rho - 1), 3);
                alpha = std::min(alpha, upper);
                double scaleFactor = std::max(lower, alpha);
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                pb.poses = backupPoses;  // pop()
                pb.pts = backupPts;
            }
            ++qmax;
        } while (rho < 0 && qmax < maxTrials && !stopped(pb));
        ++done;
        if (st && it < SLAMIT_BA_MAX_ITS) {
            // robust cost of the last evaluated trial (what activeRobustChi2() returns afterwards)
            st->chi2[stage][it] = tempChi;
            st->lambda[stage][it] = lambda;
            st->trials[stage][it] = qmax;
        }
        if (qmax == maxTrials || rho == 0) { ok = false; continue; }  // Terminate
        if ((iniChi - currentChi) * 1e3 < iniChi) ++nBad; else nBad = 0;
        if (nBad >= 3) ok = false;
    }
    return done;
}

}  // namespace

extern "C" int ba_oracle_solve(const slamit_ba_problem* in, const slamit_ba_opts* op, slamit_ba_result* res) {
    Problem pb;
    pb.K = in->n_kf; pb.P = in->n_pt; pb.E = in->n_edge;
    pb.delta = op->huber_delta; pb.gate = op->chi2_gate; pb.stop = op->stop;
    pb.delta_s = op->huber_delta_stereo > 0 ? op->huber_delta_stereo : (double)(float)sqrt(7.815);
    pb.gate_s = op->chi2_gate_stereo > 0 ? op->chi2_gate_stereo : 7.815;
    if (in->edge_ur && !in->kf_bf) return -1;
    if (in->kf_bf) pb.bf.assign(in->kf_bf, in->kf_bf + pb.K);
    pb.poses.resize(pb.K);
    pb.fixed.assign(in->kf_fixed, in->kf_fixed + pb.K);
    pb.intr.assign(in->kf_intr, in->kf_intr + 4 * (size_t)pb.K);
    pb.pts.assign(in->pt_xyz, in->pt_xyz + 3 * (size_t)pb.P);
    for (int k = 0; k < pb.K; ++k) {  // Converter::toSE3Quat -> SE3Quat(R, t): Quaterniond(R), normalised
        R_to_quat(in->kf_pose + 12 * (size_t)k, pb.poses[k].q);
        quat_normalize(pb.poses[k].q);
        for (int i = 0; i < 3; ++i) pb.poses[k].t[i] = in->kf_pose[12 * (size_t)k + 9 + i];
    }
    pb.edges.resize(pb.E);
    for (int e = 0; e < pb.E; ++e) {
        Edge& ed = pb.edges[e];
        ed.kf = in->edge_kf[e]; ed.pt = in->edge_pt[e];
        if (ed.kf < 0 || ed.kf >= pb.K || ed.pt < 0 || ed.pt >= pb.P) return -1;
        ed.u = in->edge_uv[2 * (size_t)e]; ed.v = in->edge_uv[2 * (size_t)e + 1];
        ed.w = in->edge_inv_sigma2[e];
        ed.stereo = in->edge_ur && !(in->edge_ur[e] < 0);   // S/Optimizer.cc:596: mvuRight < 0 is a monocular observation
        ed.ur = ed.stereo ? in->edge_ur[e] : -1.0;
        ed.active = true; ed.robust = true;
        ed.err[0] = ed.err[1] = ed.err[2] = 0; ed.chi2 = 0;
    }
    slamit_ba_stats* st = res->stats;
    if (st) memset(st, 0, sizeof(*st));
    for (int stage = 0; stage < 2; ++stage) {
        if (stopped(pb)) break;  // S/Optimizer.cc:655-657, 664-666
        if (stage == 1) {
            for (int e = 0; e < pb.E; ++e) {
                Edge& ed = pb.edges[e];
                const Pose& T = pb.poses[ed.kf];
                double Xc[3];
                quat_rot(T.q, &pb.pts[3 * ed.pt], Xc);
                bool out = ed.chi2 > (ed.stereo ? pb.gate_s : pb.gate) || !(Xc[2] + T.t[2] > 0.0);
                if (out) ed.active = false;   // setLevel(1)
                ed.robust = false;            // setRobustKernel(0)
                if (res->edge_stage1_outlier) res->edge_stage1_outlier[e] = out;
            }
        }
        if (st) {
            // cost at the stage's starting point; per-edge errors are restored afterwards so the
            // stale values of de-activated edges stay what the reference would read
            std::vector<Edge> keep = pb.edges;
            st->chi2_init[stage] = compute_errors(pb);
            pb.edges = keep;
        }
        int n = optimize(pb, stage == 0 ? op->its_robust : op->its_final, stage, st);
        if (st) st->n_its[stage] = n;
    }
    for (int e = 0; e < pb.E; ++e) {
        const Edge& ed = pb.edges[e];
        const Pose& T = pb.poses[ed.kf];
        double Xc[3];
        quat_rot(T.q, &pb.pts[3 * ed.pt], Xc);
        if (res->edge_chi2) res->edge_chi2[e] = ed.chi2;
        if (res->edge_outlier) res->edge_outlier[e] = ed.chi2 > (ed.stereo ? pb.gate_s : pb.gate) || !(Xc[2] + T.t[2] > 0.0);
    }
    for (int k = 0; k < pb.K; ++k) {
        double R[9];
        quat_to_R(pb.poses[k].q, R);
        memcpy(res->kf_pose + 12 * (size_t)k, R, sizeof(R));
        for (int i = 0; i < 3; ++i) res->kf_pose[12 * (size_t)k + 9 + i] = pb.poses[k].t[i];
    }
    memcpy(res->pt_xyz, pb.pts.data(), sizeof(double) * 3 * (size_t)pb.P);
    return 0;
}


// =================================================================================================
// Optimizer::PoseOptimization (S/Optimizer.cc:239-451): one pose vertex, unary
// EdgeSE3ProjectXYZOnlyPose edges, BlockSolver_6_3 + LinearSolverDense + Levenberg; 4 rounds x 10
// iterations, every round restarted from the input pose; (float)chi2 > 5.991f relabels outliers;
// kernels dropped after round index 2.  Pinned to the reference's g2o the same way as the BA
// (oracle/ba_ref_harness.cc:pose_ref_solve, tests/golden/pose_*.npz).
// =================================================================================================
namespace {

struct PEdge { double X[3], u, v, w, ur; bool stereo, active, robust; double err[3], chi2; };

// the error of one edge at camera-frame point Xc: EdgeSE3ProjectXYZOnlyPose (project2d, then * f + c) or
// EdgeStereoSE3ProjectXYZOnlyPose::cam_project (G/types/types_six_dof_expmap.cpp:299-306: the inverse depth is a FLOAT, bf a double)
inline void pose_edge_error(PEdge& ed, const double* Xc, const double* in, double bf) {
    if (!ed.stereo) {
        ed.err[0] = ed.u - (Xc[0] / Xc[2] * in[0] + in[2]);
        ed.err[1] = ed.v - (Xc[1] / Xc[2] * in[1] + in[3]);
        ed.err[2] = 0.0;
        ed.chi2 = ed.err[0] * ed.w * ed.err[0] + ed.err[1] * ed.w * ed.err[1];
    } else {
        const float invz = (float)(1.0 / Xc[2]);
        const double r0 = Xc[0] * (double)invz * in[0] + in[2];
        const double r1 = Xc[1] * (double)invz * in[1] + in[3];
        const double r2 = r0 - bf * (double)invz;
        ed.err[0] = ed.u - r0; ed.err[1] = ed.v - r1; ed.err[2] = ed.ur - r2;
        ed.chi2 = ed.err[0] * ed.w * ed.err[0] + ed.err[1] * ed.w * ed.err[1] + ed.err[2] * ed.w * ed.err[2];
    }
}

double pose_errors(const Pose& T, const double* in, std::vector<PEdge>& E, double delta, double delta_s, double bf) {
    double total = 0;
    const double dsqr_m = (double)(float)(delta * delta);   // RobustKernelHuber::dsqr is a float (G/core/robust_kernel_impl.h:84)
    const double dsqr_s = (double)(float)(delta_s * delta_s);
    for (size_t e = 0; e < E.size(); ++e) {
        PEdge& ed = E[e];
        if (!ed.active) continue;
        double Xc[3];
        quat_rot(T.q, ed.X, Xc);
        for (int i = 0; i < 3; ++i) Xc[i] += T.t[i];
        pose_edge_error(ed, Xc, in, bf);
        const double d = ed.stereo ? delta_s : delta, dsqr = ed.stereo ? dsqr_s : dsqr_m;
        if (ed.robust && ed.chi2 > dsqr) total += 2 * sqrt(ed.chi2) * d - dsqr;
        else total += ed.chi2;
    }
    return total;
}

int pose_optimize_round(Pose& T, const double* in, std::vector<PEdge>& E, double delta, double delta_s, double bf, int iterations, double* lastChi) {
    bool any = false;
    for (size_t e = 0; e < E.size(); ++e) any |= E[e].active;
    if (!any) return 0;
    const double dsqr_m = (double)(float)(delta * delta), dsqr_s = (double)(float)(delta_s * delta_s);
    double lambda = -1, ni = 2;
    int nBad = 0, done = 0;
    bool ok = true;
    for (int it = 0; it < iterations && ok; ++it) {
        double currentChi = pose_errors(T, in, E, delta, delta_s, bf), tempChi = currentChi;
        const double iniChi = currentChi;
        double H[36], b[6];
        for (int i = 0; i < 36; ++i) H[i] = 0;
        for (int i = 0; i < 6; ++i) b[i] = 0;
        for (size_t e = 0; e < E.size(); ++e) {
            const PEdge& ed = E[e];
            if (!ed.active) continue;
            double Xc[3];
            quat_rot(T.q, ed.X, Xc);
            for (int i = 0; i < 3; ++i) Xc[i] += T.t[i];
            const double x = Xc[0], y = Xc[1], invz = 1.0 / Xc[2], invz_2 = invz * invz, fx = in[0], fy = in[1];
            double J[18];
            J[0] = x * y * invz_2 * fx; J[1] = -(1 + (x * x * invz_2)) * fx; J[2] = y * invz * fx;
            J[3] = -invz * fx; J[4] = 0; J[5] = x * invz_2 * fx;
            J[6] = (1 + y * y * invz_2) * fy; J[7] = -x * y * invz_2 * fy; J[8] = -x * invz * fy;
            J[9] = 0; J[10] = -invz * fy; J[11] = y * invz_2 * fy;
            if (ed.stereo) {   // EdgeStereoSE3ProjectXYZOnlyPose::linearizeOplus (G/types/types_six_dof_expmap.cpp:335-364)
                J[12] = J[0] - bf * y * invz_2; J[13] = J[1] + bf * x * invz_2; J[14] = J[2];
                J[15] = J[3]; J[16] = 0; J[17] = J[5] - bf * invz_2;
            } else {
                for (int i = 12; i < 18; ++i) J[i] = 0;
            }
            const double d = ed.stereo ? delta_s : delta, dsqr = ed.stereo ? dsqr_s : dsqr_m;
            double rho1 = 1.0;
            if (ed.robust && ed.chi2 > dsqr) rho1 = d / sqrt(ed.chi2);
            const double wO = rho1 * ed.w;
            for (int i = 0; i < 6; ++i) {
                if (ed.stereo) b[i] -= rho1 * (J[i] * ed.w * ed.err[0] + J[6 + i] * ed.w * ed.err[1] + J[12 + i] * ed.w * ed.err[2]);
                else b[i] -= rho1 * (J[i] * ed.w * ed.err[0] + J[6 + i] * ed.w * ed.err[1]);
                for (int j = 0; j < 6; ++j) {
                    if (ed.stereo) H[6 * i + j] += (J[i] * J[j] + J[6 + i] * J[6 + j] + J[12 + i] * J[12 + j]) * wO;
                    else H[6 * i + j] += (J[i] * J[j] + J[6 + i] * J[6 + j]) * wO;
                }
            }
        }
        if (it == 0) {
            double maxDiag = 0;
            for (int j = 0; j < 6; ++j) maxDiag = std::max(fabs(H[7 * j]), maxDiag);
            lambda = 1e-5 * maxDiag; ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            Pose backup = T;
            std::vector<double> A(36), x(b, b + 6);
            for (int i = 0; i < 36; ++i) A[i] = H[i] + (i % 7 == 0 ? lambda : 0.0);
            bool ok2 = ldlt_solve(A, 6, x);
            if (ok2) pose_oplus(T, x.data()); else x.assign(6, 0.0);
            tempChi = pose_errors(T, in, E, delta, delta_s, bf);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int k = 0; k < 6; ++k) scale += x[k] * (lambda * x[k] + b[k]);
            rho /= scale + 1e-3;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = std::min(1. - pow((2 * rho - 1), 3), 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2; currentChi = tempChi;
            } else {
                lambda *= ni; ni *= 2; T = backup;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++done;
        *lastChi = tempChi;
        if (qmax == 10 || rho == 0) { ok = false; continue; }
        if ((iniChi - currentChi) * 1e3 < iniChi) ++nBad; else nBad = 0;
        if (nBad >= 3) ok = false;
    }
    return done;
}

}  // namespace

// gate_margin (n entries, may be null): per edge the least |chi2 - gate| / gate over the four relabellings, i.e. how close the edge
// ever came to changing its flag (tests/test_ceiling_fixtures.py keeps the large fixtures clear of the gate with it)
static int pose_oracle_solve_impl(const slamit_pose_problem* pb, slamit_pose_result* res, double* gate_margin) {
    const int n = pb->n;
    if (gate_margin) for (int e = 0; e < n; ++e) gate_margin[e] = HUGE_VAL;
    Pose T0;
    R_to_quat(pb->pose, T0.q);
    quat_normalize(T0.q);
    for (int i = 0; i < 3; ++i) T0.t[i] = pb->pose[9 + i];
    for (int r = 0; r < 4; ++r) { res->n_its[r] = 0; res->chi2[r] = 0; }
    if (n < 3) {  // S/Optimizer.cc:364-365
        memcpy(res->pose, pb->pose, sizeof(double) * 12);
        res->n_inliers = 0;
        return 0;
    }
    const double delta = (double)(float)sqrt(5.991), delta_s = (double)(float)sqrt(7.815);   // deltaMono, deltaStereo (S/Optimizer.cc:264-265)
    const double bf = pb->ur ? pb->bf : 0.0;
    std::vector<PEdge> E(n);
    for (int e = 0; e < n; ++e) {
        for (int i = 0; i < 3; ++i) E[e].X[i] = pb->xw[3 * e + i];
        E[e].u = pb->uv[2 * e]; E[e].v = pb->uv[2 * e + 1]; E[e].w = pb->inv_sigma2[e];
        E[e].stereo = pb->ur && !(pb->ur[e] < 0);   // S/Optimizer.cc:281: mvuRight < 0 is a monocular observation
        E[e].ur = E[e].stereo ? pb->ur[e] : -1.0;
        E[e].active = true; E[e].robust = true; E[e].err[0] = E[e].err[1] = E[e].err[2] = 0; E[e].chi2 = 0;
        res->outlier[e] = 0;
    }
    Pose T = T0;
    int nBad = 0;
    for (int round = 0; round < 4; ++round) {
        T = T0;  // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) at the top of every round
        res->n_its[round] = pose_optimize_round(T, pb->intr, E, delta, delta_s, bf, 10, &res->chi2[round]);
        nBad = 0;
        for (int e = 0; e < n; ++e) {
            PEdge& ed = E[e];
            if (res->outlier[e]) {  // inactive edges are re-evaluated at the new pose (:379-382)
                double Xc[3];
                quat_rot(T.q, ed.X, Xc);
                for (int i = 0; i < 3; ++i) Xc[i] += T.t[i];
                pose_edge_error(ed, Xc, pb->intr, bf);
            }
            const float chi2 = (float)ed.chi2;
            if (gate_margin) { const double g = ed.stereo ? 7.815f : 5.991f; gate_margin[e] = std::min(gate_margin[e], fabs(ed.chi2 - g) / g); }
            if (chi2 > (ed.stereo ? 7.815f : 5.991f)) { res->outlier[e] = 1; ed.active = false; ++nBad; }   // chi2Mono / chi2Stereo (:369-370)
            else { res->outlier[e] = 0; ed.active = true; }
            if (round == 2) ed.robust = false;
        }
        if (n < 10) break;  // optimizer.edges().size() < 10
    }
    double R[9];
    quat_to_R(T.q, R);
    memcpy(res->pose, R, sizeof(R));
    for (int i = 0; i < 3; ++i) res->pose[9 + i] = T.t[i];
    res->n_inliers = n - nBad;
    return 0;
}

extern "C" int pose_oracle_solve(const slamit_pose_problem* pb, slamit_pose_result* res) { return pose_oracle_solve_impl(pb, res, nullptr); }
extern "C" int pose_oracle_solve_margin(const slamit_pose_problem* pb, slamit_pose_result* res, double* gate_margin) {
    return pose_oracle_solve_impl(pb, res, gate_margin);
}


// =================================================================================================
// Optimizer::OptimizeSim3 (S/Optimizer.cc:1046-1247): one VertexSim3Expmap, per correspondence a fixed point in each
// camera frame and the pair EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (G/types/types_seven_dof_expmap.h:118-152)
// with Huber kernels of width (float)sqrt(th2), BlockSolverX + LinearSolverDense + Levenberg.  The reference's analytic
// Jacobians are commented out, so g2o differentiates numerically (G/core/base_binary_edge.hpp:131-200: central
// differences, delta 1e-9, through the vertex's oplus = Sim3(update) * estimate, G/types/sim3.h:69-146).  Schedule:
// optimize(5), drop the pairs with chi2 > th2 on either edge, return 0 below 10 pairs, optimize(10 or 5), count.
// Pinned to the reference's g2o (oracle/ba_ref_harness.cc:sim3_ref_solve, tests/golden/sim3_*.npz).
// =================================================================================================
namespace {

struct Sim3 { double q[4], t[3], s; };   // q = (x, y, z, w)

// Sim3(const Vector7d& update): [omega, upsilon, sigma] (sim3.h:69-146)
Sim3 sim3_exp(const double u[7]) {
    const double omega[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]}, sigma = u[6];
    const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    const double O[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
    double O2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    Sim3 S;
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, R[9];
    double ca = 1.0, cb = 1.0;   // R = I + ca * Omega + cb * Omega2
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            ca = sin(theta) / theta; cb = (1 - cos(theta)) / (theta * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            ca = sin(theta) / theta; cb = (1 - cos(theta)) / (theta * theta);
            const double a = S.s * sin(theta), b = S.s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ca * O[i] + cb * O2[i];
    R_to_quat(R, S.q);   // Quaterniond(R): not normalised
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int j = 0; j < 3; ++j) acc += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * ups[j];
        S.t[i] = acc;
    }
    return S;
}
Sim3 sim3_mul(const Sim3& a, const Sim3& b) {   // sim3.h:258-264
    Sim3 r;
    quat_mul(a.q, b.q, r.q);
    double rt[3];
    quat_rot(a.q, b.t, rt);
    for (int i = 0; i < 3; ++i) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}
void sim3_map(const Sim3& S, const double x[3], double out[3]) {   // s * (r * xyz) + t
    double rx[3];
    quat_rot(S.q, x, rx);
    for (int i = 0; i < 3; ++i) out[i] = S.s * rx[i] + S.t[i];
}
Sim3 sim3_inverse(const Sim3& S) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    Sim3 r;
    r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
    const double k = -1. / S.s;
    const double kt[3] = {k * S.t[0], k * S.t[1], k * S.t[2]};
    quat_rot(r.q, kt, r.t);
    r.s = 1. / S.s;
    return r;
}

struct SPair { double p1[3], p2[3], o1[2], o2[2], w1, w2; bool active; double e12[2], e21[2], chi12, chi21; };

// the two edge errors of one pair at S (types_seven_dof_expmap.h:128-133, 146-151)
void sim3_pair_error(const Sim3& S, const Sim3& Sinv, const double* in1, const double* in2, const SPair& P, double e12[2], double e21[2]) {
    double v[3];
    sim3_map(S, P.p2, v);
    e12[0] = P.o1[0] - (v[0] / v[2] * in1[0] + in1[2]);
    e12[1] = P.o1[1] - (v[1] / v[2] * in1[1] + in1[3]);
    sim3_map(Sinv, P.p1, v);
    e21[0] = P.o2[0] - (v[0] / v[2] * in2[0] + in2[2]);
    e21[1] = P.o2[1] - (v[1] / v[2] * in2[1] + in2[3]);
}
inline double huber_rho(double chi2, double delta, double dsqr) { return chi2 > dsqr ? 2 * sqrt(chi2) * delta - dsqr : chi2; }

double sim3_errors(const Sim3& S, const double* in1, const double* in2, std::vector<SPair>& E, double delta) {
    const Sim3 Sinv = sim3_inverse(S);
    const double dsqr = (double)(float)(delta * delta);   // RobustKernelHuber::dsqr is a float (G/core/robust_kernel_impl.h:84)
    double total = 0;
    for (size_t k = 0; k < E.size(); ++k) {
        SPair& P = E[k];
        if (!P.active) continue;
        sim3_pair_error(S, Sinv, in1, in2, P, P.e12, P.e21);
        P.chi12 = P.e12[0] * P.w1 * P.e12[0] + P.e12[1] * P.w1 * P.e12[1];
        P.chi21 = P.e21[0] * P.w2 * P.e21[0] + P.e21[1] * P.w2 * P.e21[1];
        total += huber_rho(P.chi12, delta, dsqr) + huber_rho(P.chi21, delta, dsqr);
    }
    return total;
}

void sim3_oplus(Sim3& S, const double* x, bool fix_scale) {   // VertexSim3Expmap::oplusImpl
    double u[7];
    for (int i = 0; i < 7; ++i) u[i] = x[i];
    if (fix_scale) u[6] = 0;
    S = sim3_mul(sim3_exp(u), S);
}

int sim3_optimize_stage(Sim3& S, const double* in1, const double* in2, std::vector<SPair>& E, double delta, bool fix_scale, int iterations,
                        double* lastChi) {
    bool any = false;
    for (size_t k = 0; k < E.size(); ++k) any |= E[k].active;
    if (!any) return 0;
    const double dsqr = (double)(float)(delta * delta);   // RobustKernelHuber::dsqr is a float (G/core/robust_kernel_impl.h:84)
    double lambda = -1, ni = 2;
    int nBad = 0, done = 0;
    bool ok = true;
    for (int it = 0; it < iterations && ok; ++it) {
        double currentChi = sim3_errors(S, in1, in2, E, delta), tempChi = currentChi;
        const double iniChi = currentChi;
        double H[49], b[7];
        for (int i = 0; i < 49; ++i) H[i] = 0;
        for (int i = 0; i < 7; ++i) b[i] = 0;
        // numeric Jacobians of every active edge wrt the 7 increments (base_binary_edge.hpp:176-198)
        const double dl = 1e-9, scalar = 1.0 / (2 * dl);
        Sim3 Sp[7], Sm[7], Spi[7], Smi[7];
        for (int d = 0; d < 7; ++d) {
            double add[7] = {0, 0, 0, 0, 0, 0, 0};
            add[d] = dl;
            Sp[d] = S; sim3_oplus(Sp[d], add, fix_scale); Spi[d] = sim3_inverse(Sp[d]);
            add[d] = -dl;
            Sm[d] = S; sim3_oplus(Sm[d], add, fix_scale); Smi[d] = sim3_inverse(Sm[d]);
        }
        for (size_t k = 0; k < E.size(); ++k) {
            const SPair& P = E[k];
            if (!P.active) continue;
            double J12[14], J21[14];   // 2 x 7 each, row-major
            for (int d = 0; d < 7; ++d) {
                double a12[2], a21[2], c12[2], c21[2];
                sim3_pair_error(Sp[d], Spi[d], in1, in2, P, a12, a21);
                sim3_pair_error(Sm[d], Smi[d], in1, in2, P, c12, c21);
                J12[d] = scalar * (a12[0] - c12[0]); J12[7 + d] = scalar * (a12[1] - c12[1]);
                J21[d] = scalar * (a21[0] - c21[0]); J21[7 + d] = scalar * (a21[1] - c21[1]);
            }
            const double r12 = P.chi12 > dsqr ? delta / sqrt(P.chi12) : 1.0, r21 = P.chi21 > dsqr ? delta / sqrt(P.chi21) : 1.0;
            const double w12 = r12 * P.w1, w21 = r21 * P.w2;
            for (int i = 0; i < 7; ++i) {
                b[i] -= r12 * (J12[i] * P.w1 * P.e12[0] + J12[7 + i] * P.w1 * P.e12[1]);
                b[i] -= r21 * (J21[i] * P.w2 * P.e21[0] + J21[7 + i] * P.w2 * P.e21[1]);
                for (int j = 0; j < 7; ++j)
                    H[7 * i + j] += (J12[i] * J12[j] + J12[7 + i] * J12[7 + j]) * w12 + (J21[i] * J21[j] + J21[7 + i] * J21[7 + j]) * w21;
            }
        }
        if (it == 0) {
            double maxDiag = 0;
            for (int j = 0; j < 7; ++j) maxDiag = std::max(fabs(H[8 * j]), maxDiag);
            lambda = 1e-5 * maxDiag; ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Sim3 backup = S;
            std::vector<double> A(49), x(b, b + 7);
            for (int i = 0; i < 49; ++i) A[i] = H[i] + (i % 8 == 0 ? lambda : 0.0);
            const bool ok2 = ldlt_solve(A, 7, x);
            if (ok2) sim3_oplus(S, x.data(), fix_scale); else x.assign(7, 0.0);
            tempChi = sim3_errors(S, in1, in2, E, delta);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int k = 0; k < 7; ++k) scale += x[k] * (lambda * x[k] + b[k]);
            rho /= scale + 1e-3;
            if (rho > 0 && std::isfinite(tempChi)) {
                const double alpha = std::min(1. - pow((2 * rho - 1), 3), 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2; currentChi = tempChi;
            } else {
                lambda *= ni; ni *= 2; S = backup;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++done;
        *lastChi = tempChi;
        if (qmax == 10 || rho == 0) { ok = false; continue; }
        if ((iniChi - currentChi) * 1e3 < iniChi) ++nBad; else nBad = 0;
        if (nBad >= 3) ok = false;
    }
    return done;
}

}  // namespace

// gate_margin (n entries, may be null): per pair the least |chi2 - th2| / th2 over both edges and both tests (see pose_oracle_solve_impl)
static int sim3_oracle_solve_impl(const slamit_sim3_problem* pb, slamit_sim3_result* res, double* gate_margin) {
    const int n = pb->n;
    if (gate_margin) for (int k = 0; k < n; ++k) gate_margin[k] = HUGE_VAL;
    auto margin = [&](int k, const SPair& P) {
        if (gate_margin) gate_margin[k] = std::min(gate_margin[k], std::min(fabs(P.chi12 - (double)(float)pb->th2), fabs(P.chi21 - (double)(float)pb->th2)) / (double)(float)pb->th2);
    };
    Sim3 S;
    R_to_quat(pb->r12, S.q);   // Sim3(R, t, s): Quaterniond(R), not normalised
    for (int i = 0; i < 3; ++i) S.t[i] = pb->t12[i];
    S.s = pb->s12;
    const float th2 = (float)pb->th2;
    const double delta = (double)(float)sqrt(th2);   // const float deltaHuber = sqrt(th2)
    std::vector<SPair> E(n);
    for (int k = 0; k < n; ++k) {
        SPair& P = E[k];
        for (int i = 0; i < 3; ++i) { P.p1[i] = pb->p1[3 * k + i]; P.p2[i] = pb->p2[3 * k + i]; }
        for (int i = 0; i < 2; ++i) { P.o1[i] = pb->obs1[2 * k + i]; P.o2[i] = pb->obs2[2 * k + i]; }
        P.w1 = pb->inv_sigma2_1[k]; P.w2 = pb->inv_sigma2_2[k];
        P.active = true; P.e12[0] = P.e12[1] = P.e21[0] = P.e21[1] = 0; P.chi12 = P.chi21 = 0;
        res->inlier[k] = 1;
    }
    for (int k = 0; k < 2; ++k) { res->n_its[k] = 0; res->chi2[k] = 0; }
    memcpy(res->r12, pb->r12, sizeof(res->r12)); memcpy(res->t12, pb->t12, sizeof(res->t12)); res->s12 = pb->s12;
    res->n_its[0] = sim3_optimize_stage(S, pb->intr1, pb->intr2, E, delta, pb->fix_scale != 0, 5, &res->chi2[0]);
    int nBad = 0;
    for (int k = 0; k < n; ++k) {
        margin(k, E[k]);
        if (E[k].chi12 > th2 || E[k].chi21 > th2) { res->inlier[k] = 0; E[k].active = false; ++nBad; }
    }
    const int more = nBad > 0 ? 10 : 5;
    if (n - nBad < 10) { res->n_inliers = 0; return 0; }
    res->n_its[1] = sim3_optimize_stage(S, pb->intr1, pb->intr2, E, delta, pb->fix_scale != 0, more, &res->chi2[1]);
    int nIn = 0;
    for (int k = 0; k < n; ++k) {
        if (!E[k].active) continue;
        margin(k, E[k]);
        if (E[k].chi12 > th2 || E[k].chi21 > th2) res->inlier[k] = 0;
        else ++nIn;
    }
    double R[9];
    quat_to_R(S.q, R);   // rotation().toRotationMatrix()
    memcpy(res->r12, R, sizeof(R));
    for (int i = 0; i < 3; ++i) res->t12[i] = S.t[i];
    res->s12 = S.s;
    res->n_inliers = nIn;
    return 0;
}

extern "C" int sim3_oracle_solve(const slamit_sim3_problem* pb, slamit_sim3_result* res) { return sim3_oracle_solve_impl(pb, res, nullptr); }
extern "C" int sim3_oracle_solve_margin(const slamit_sim3_problem* pb, slamit_sim3_result* res, double* gate_margin) {
    return sim3_oracle_solve_impl(pb, res, gate_margin);
}
