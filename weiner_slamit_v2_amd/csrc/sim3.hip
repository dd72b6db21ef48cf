// sim3.hip — Optimizer::OptimizeSim3 on the GPU (include/slamit.h, slamit_sim3_*).
//
// Reference: ORB_SLAM2/src/Optimizer.cc:1046-1247 driving g2o (BlockSolverX + LinearSolverDense + Levenberg) over one
// VertexSim3Expmap and, per correspondence, the pair EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ
// (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:118-152, sim3.h:69-264).  The reference leaves the analytic
// Jacobians commented out, so g2o differentiates NUMERICALLY (core/base_binary_edge.hpp:131-200: central differences,
// delta 1e-9, through oplus = Sim3(update) * estimate); the same is done here: the 14 perturbed similarities and their
// inverses are built once per iteration, every lane evaluates its pairs at all of them.  The system is one 7x7 block, so
// the whole schedule — 5 iterations, the chi2 > th2 pruning of pairs, 10 (or 5) more iterations, the inlier count —
// runs inside ONE workgroup per problem with no host round trip; a batch is one launch.  This file holds the pairs (Sim3Model:
// errors, the perturbed similarities, normal-equation partials, oplus) and the two stages; the Levenberg iterations themselves are
// lm_block.h's lm_block_run<7, 8>, shared with pose.hip, over the rules of lm_step.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "lm_block.h"
#include "lm_layout.h"
#include "se3_device.h"
#include "slamit_internal.h"

// Device-side record of one problem (pointers into the batch slabs)
struct Sim3Prob {
    int32_t n, fix_scale;
    double intr1[4], intr2[4], S0[8], th2;   // S = q(x, y, z, w), t, s
    const SLAMIT_GLOBAL double* p1; const SLAMIT_GLOBAL double* p2; const SLAMIT_GLOBAL double* o1; const SLAMIT_GLOBAL double* o2;
    const SLAMIT_GLOBAL double* w1; const SLAMIT_GLOBAL double* w2;
    SLAMIT_GLOBAL double* chi12; SLAMIT_GLOBAL double* chi21;      // n each: chi2 of the last evaluated trial
    SLAMIT_GLOBAL uint8_t* inlier;                          // n out
    SLAMIT_GLOBAL double* out;                              // 16: R (9), t (3), s, chi2[2], pad
    SLAMIT_GLOBAL int32_t* ints;                            // 4: n_inliers, n_its[2], returned-at-the-10-pair-test flag
};

namespace {

__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* r) {   // Eigen quaternion product, (x, y, z, w)
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// Sim3(const Vector7d& update) (sim3.h:69-146) followed by (update) * S (sim3.h:258-264): S <- exp(u) * S
__device__ void sim3_oplus(double* S, const double* u_in, bool fix_scale) {
    double u[7];
    for (int i = 0; i < 7; ++i) u[i] = u_in[i];
    if (fix_scale) u[6] = 0;
    const double sigma = u[6];
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double O[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
    double O2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    const double es = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, ca = 1.0, cb = 1.0;   // R = I + ca Omega + cb Omega^2
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
        C = (es - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * es + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * es) / (sigma2 * sigma);
        } else {
            ca = sin(theta) / theta; cb = (1 - cos(theta)) / (theta * theta);
            const double a = es * sin(theta), b = es * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    double R[9], qe[4], te[3];
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ca * O[i] + cb * O2[i];
    R_to_quat(R, qe);   // Quaterniond(R): not normalised
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int j = 0; j < 3; ++j) acc += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * u[3 + j];
        te[i] = acc;
    }
    double nq[4], rt[3];
    quat_mul(qe, S, nq);
    quat_rot(qe, S + 4, rt);
    for (int i = 0; i < 4; ++i) S[i] = nq[i];
    for (int i = 0; i < 3; ++i) S[4 + i] = es * rt[i] + te[i];
    S[7] = es * S[7];
}

__device__ __forceinline__ void sim3_inverse(const double* S, double* I) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    I[0] = -S[0]; I[1] = -S[1]; I[2] = -S[2]; I[3] = S[3];
    const double k = -1. / S[7];
    const double kt[3] = {k * S[4], k * S[5], k * S[6]};
    quat_rot(I, kt, I + 4);
    I[7] = 1. / S[7];
}

// the two edge errors of one pair at (S, S^-1) (types_seven_dof_expmap.h:128-133, 146-151)
__device__ __forceinline__ void pair_error(const double* S, const double* Si, const double* in1, const double* in2, const double* p1,
                                           const double* p2, const double* o1, const double* o2, double* e12, double* e21) {
    double r[3];
    quat_rot(S, p2, r);
    const double x = S[7] * r[0] + S[4], y = S[7] * r[1] + S[5], z = S[7] * r[2] + S[6];
    e12[0] = o1[0] - (x / z * in1[0] + in1[2]);
    e12[1] = o1[1] - (y / z * in1[1] + in1[3]);
    quat_rot(Si, p1, r);
    const double xi = Si[7] * r[0] + Si[4], yi = Si[7] * r[1] + Si[5], zi = Si[7] * r[2] + Si[6];
    e21[0] = o2[0] - (xi / zi * in2[0] + in2[2]);
    e21[1] = o2[1] - (yi / zi * in2[1] + in2[3]);
}

__device__ __forceinline__ double huber(double c2, double delta, double dsqr) { return c2 > dsqr ? 2 * sqrt(c2) * delta - dsqr : c2; }

// errors + chi2 of every active pair at S; returns the robust cost
__device__ double sim3_errors(const Sim3Prob& P, const double* S, const uint8_t* active, double delta, double* sSi, double* sh) {
    if (threadIdx.x == 0) sim3_inverse(S, sSi);
    __syncthreads();
    const double dsqr = (double)(float)(delta * delta);   // RobustKernelHuber::dsqr is a float member (g2o/core/robust_kernel_impl.h:84)
    double part = 0;
    for (int k = threadIdx.x; k < P.n; k += 256) {
        if (!active[k]) continue;
        const double p1[3] = {P.p1[3 * k], P.p1[3 * k + 1], P.p1[3 * k + 2]}, p2[3] = {P.p2[3 * k], P.p2[3 * k + 1], P.p2[3 * k + 2]};
        const double o1[2] = {P.o1[2 * k], P.o1[2 * k + 1]}, o2[2] = {P.o2[2 * k], P.o2[2 * k + 1]};
        double e12[2], e21[2];
        pair_error(S, sSi, P.intr1, P.intr2, p1, p2, o1, o2, e12, e21);
        const double w1 = P.w1[k], w2 = P.w2[k];
        const double c12 = e12[0] * w1 * e12[0] + e12[1] * w1 * e12[1], c21 = e21[0] * w2 * e21[0] + e21[1] * w2 * e21[1];
        P.chi12[k] = c12; P.chi21[k] = c21;
        part += huber(c12, delta, dsqr) + huber(c21, delta, dsqr);
    }
    return lm_block_sum(part, sh);
}

// the pairs of one problem as lm_block_run sees them (lm_block.h); S = q(x, y, z, w), t, s
struct Sim3Model {
    const Sim3Prob& P;
    const uint8_t* active;     // LDS: the pair is still in the graph
    double delta;
    bool fix;
    double* sSi;               // LDS [8]: S^-1 of the last errors()
    double (*sPert)[8];        // LDS [28][8]: [2d] = S(+delta e_d), [2d+1] = S(-delta e_d), [14 + ..] their inverses
    double* sh;                // LDS [4]: the block sum's

    __device__ __forceinline__ double errors(const double* S) const { return sim3_errors(P, S, active, delta, sSi, sh); }
    __device__ __forceinline__ void oplus(double* S, const double* x) const { sim3_oplus(S, x, fix); }
    // the 14 perturbed similarities of g2o's numeric differentiation and their inverses
    __device__ __forceinline__ void prepare(const double* sS) const {
        const int tid = threadIdx.x;
        if (tid < 14) {
            double Sp[8], add[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 8; ++i) Sp[i] = sS[i];
            add[tid >> 1] = (tid & 1) ? -1e-9 : 1e-9;
            sim3_oplus(Sp, add, fix);
            double Ip[8];
            sim3_inverse(Sp, Ip);
            for (int i = 0; i < 8; ++i) { sPert[tid][i] = Sp[i]; sPert[14 + tid][i] = Ip[i]; }
        }
        __syncthreads();
    }
    // H (28 unique), b (7) over this thread's active pairs; chi2 and S^-1 are those errors() left at this very S
    __device__ __forceinline__ void accumulate(const double* sS, double* h, double* bb) const {
        const int tid = threadIdx.x, n = P.n;
        const double dsqr = (double)(float)(delta * delta), scalar = 1.0 / (2 * 1e-9);
        for (int k = tid; k < n; k += 256) {
            if (!active[k]) continue;
            const double p1[3] = {P.p1[3 * k], P.p1[3 * k + 1], P.p1[3 * k + 2]}, p2[3] = {P.p2[3 * k], P.p2[3 * k + 1], P.p2[3 * k + 2]};
            const double o1[2] = {P.o1[2 * k], P.o1[2 * k + 1]}, o2[2] = {P.o2[2 * k], P.o2[2 * k + 1]};
            double J12[14], J21[14];
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                double a12[2], a21[2], c12[2], c21[2];
                pair_error(sPert[2 * d], sPert[14 + 2 * d], P.intr1, P.intr2, p1, p2, o1, o2, a12, a21);
                pair_error(sPert[2 * d + 1], sPert[14 + 2 * d + 1], P.intr1, P.intr2, p1, p2, o1, o2, c12, c21);
                J12[d] = scalar * (a12[0] - c12[0]); J12[7 + d] = scalar * (a12[1] - c12[1]);
                J21[d] = scalar * (a21[0] - c21[0]); J21[7 + d] = scalar * (a21[1] - c21[1]);
            }
            double e12[2], e21[2];
            pair_error(sS, sSi, P.intr1, P.intr2, p1, p2, o1, o2, e12, e21);
            const double w1 = P.w1[k], w2 = P.w2[k], c12 = P.chi12[k], c21 = P.chi21[k];
            const double r12 = c12 > dsqr ? delta / sqrt(c12) : 1.0, r21 = c21 > dsqr ? delta / sqrt(c21) : 1.0;
            const double wa = r12 * w1, wb = r21 * w2;
            int q = 0;
#pragma unroll
            for (int a = 0; a < 7; ++a) {
                bb[a] -= r12 * (J12[a] * w1 * e12[0] + J12[7 + a] * w1 * e12[1]) + r21 * (J21[a] * w2 * e21[0] + J21[7 + a] * w2 * e21[1]);
#pragma unroll
                for (int c = a; c < 7; ++c)
                    h[q++] += (J12[a] * J12[c] + J12[7 + a] * J12[7 + c]) * wa + (J21[a] * J21[c] + J21[7 + a] * J21[7 + c]) * wb;
            }
        }
    }
};

}  // namespace

__global__ __launch_bounds__(256) void sim3_opt_kernel(const Sim3Prob* probs) {
    const Sim3Prob P = probs[blockIdx.x];
    const int tid = threadIdx.x, n = P.n;
    __shared__ LmBlock<7, 8> L;
    __shared__ double sSi[8], sPert[28][8];
    double* const sS = L.state;
    extern __shared__ uint8_t s_act[];   // n bytes: the pair is still in the graph
    const float th2f = (float)P.th2;
    const double th2 = (double)th2f;
    const double delta = (double)sqrtf(th2f);   // const float deltaHuber = sqrt(th2)
    const bool fix = P.fix_scale != 0;
    if (tid < 8) sS[tid] = P.S0[tid];
    for (int k = tid; k < n; k += 256) { s_act[k] = 1; P.inlier[k] = 1; P.chi12[k] = 0; P.chi21[k] = 0; }
    if (tid == 0) { P.ints[0] = 0; P.ints[1] = 0; P.ints[2] = 0; P.ints[3] = 0; P.out[13] = 0; P.out[14] = 0; }
    __syncthreads();
    int nBadPairs = 0;
    bool early = false;
    for (int stage = 0; stage < 2 && !early; ++stage) {
        const int iterations = stage == 0 ? 5 : (nBadPairs > 0 ? 10 : 5);
        int nact = 0;
        for (int k = tid; k < n; k += 256) nact += s_act[k];
        const bool any_active = lm_block_count(nact, &L.cnt) > 0;
        __syncthreads();
        int done = 0;
        double lastChi = 0;
        if (any_active) done = lm_block_run(L, Sim3Model{P, s_act, delta, fix, sSi, sPert, L.sum}, iterations, lastChi);
        if (tid == 0) { P.ints[1 + stage] = done; P.out[13 + stage] = lastChi; }
        // ---- the chi2 tests (:1184-1201, 1218-1234): the chi2 of the LAST EVALUATED trial, accepted or not ----
        int bad = 0;
        for (int k = tid; k < n; k += 256) {
            if (!s_act[k]) continue;
            if (P.chi12[k] > th2 || P.chi21[k] > th2) {
                P.inlier[k] = 0;
                if (stage == 0) s_act[k] = 0;
                ++bad;
            }
        }
        const int nbad = lm_block_count(bad, &L.cnt);
        __syncthreads();
        if (stage == 0) {
            nBadPairs = nbad;
            if (n - nBadPairs < 10) {   // :1212-1213: return 0, g2oS12 untouched
                early = true;
                if (tid == 0) {
                    double R[9];
                    quat_to_R(P.S0, R);
                    for (int i = 0; i < 9; ++i) P.out[i] = R[i];
                    for (int i = 0; i < 3; ++i) P.out[9 + i] = P.S0[4 + i];
                    P.out[12] = P.S0[7];
                    P.ints[0] = 0; P.ints[3] = 1;
                }
            }
        } else if (tid == 0) {
            double R[9];
            quat_to_R(sS, R);
            for (int i = 0; i < 9; ++i) P.out[i] = R[i];
            for (int i = 0; i < 3; ++i) P.out[9 + i] = sS[4 + i];
            P.out[12] = sS[7];
            P.ints[0] = n - nBadPairs - nbad;
        }
    }
}

extern "C" {

int slamit_sim3_optimize_batch(int device, int nprob, const slamit_sim3_problem* probs, slamit_sim3_result* results) {
    const char* const where = "slamit_sim3_optimize_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_optimize_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    for (int f = 0; f < nprob; ++f) {
        const slamit_sim3_problem& P = probs[f];
        if (P.n < 0 || (P.n && (!P.p1 || !P.p2 || !P.obs1 || !P.obs2 || !P.inv_sigma2_1 || !P.inv_sigma2_2 || !results[f].inlier)))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_optimize_batch: null array");
        if (P.n > SLAMIT_SIM3_MAX_N) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_sim3_optimize_batch: more than SLAMIT_SIM3_MAX_N correspondences");
        if (!(P.s12 > 0) || !(P.th2 > 0)) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_optimize_batch: scale and th2 must be positive");
    }
    SLAMIT_USE_DEVICE(device);
    // [doubles of every problem (lm_layout.h) | ints | Sim3Prob records | flags].  A problem's doubles mix what the kernel reads and
    // writes, so everything but the flags goes up and the whole block comes down.
    StageLayout L;
    std::vector<Sim3Spans> dbl(nprob);
    std::vector<StageSpan<uint8_t>> flags(nprob);
    int nmax = 1;
    for (int f = 0; f < nprob; ++f) { dbl[f] = sim3_take(L, probs[f].n); nmax = std::max(nmax, (int)probs[f].n); }
    const StageSpan<int32_t> ints = L.take<int32_t>(4 * (size_t)nprob, 4);   // per problem: Sim3Prob::ints
    const StageSpan<Sim3Prob> recs = L.take<Sim3Prob>(nprob, 16);
    L.end_inputs(1); L.out_off = 0;   // (the whole block comes down)
    for (int f = 0; f < nprob; ++f) flags[f] = lm_take_flags(L, probs[f].n);
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT(where, slamit_stage_reserve(S, device, L));
    for (int f = 0; f < nprob; ++f) {
        const slamit_sim3_problem& P = probs[f];
        const Sim3Spans& s = dbl[f];
        if (P.n) {
            memcpy(s.p1.at(S.host), P.p1, s.p1.bytes()); memcpy(s.p2.at(S.host), P.p2, s.p2.bytes());
            memcpy(s.o1.at(S.host), P.obs1, s.o1.bytes()); memcpy(s.o2.at(S.host), P.obs2, s.o2.bytes());
            memcpy(s.w1.at(S.host), P.inv_sigma2_1, s.w1.bytes()); memcpy(s.w2.at(S.host), P.inv_sigma2_2, s.w2.bytes());
        }
        Sim3Prob& Q = recs.at(S.host)[f];
        memset(&Q, 0, sizeof(Q));
        Q.n = P.n; Q.fix_scale = P.fix_scale; Q.th2 = P.th2;
        memcpy(Q.intr1, P.intr1, sizeof(Q.intr1)); memcpy(Q.intr2, P.intr2, sizeof(Q.intr2));
        R_to_quat(P.r12, Q.S0);   // Sim3(R, t, s): Quaterniond(R) by Eigen's rule, not normalised
        for (int i = 0; i < 3; ++i) Q.S0[4 + i] = P.t12[i];
        Q.S0[7] = P.s12;
        typedef SLAMIT_GLOBAL double gd;
        Q.p1 = (const gd*)s.p1.at(S.dev); Q.p2 = (const gd*)s.p2.at(S.dev); Q.o1 = (const gd*)s.o1.at(S.dev); Q.o2 = (const gd*)s.o2.at(S.dev);
        Q.w1 = (const gd*)s.w1.at(S.dev); Q.w2 = (const gd*)s.w2.at(S.dev); Q.chi12 = (gd*)s.chi12.at(S.dev); Q.chi21 = (gd*)s.chi21.at(S.dev);
        Q.out = (gd*)s.out.at(S.dev);
        Q.inlier = (SLAMIT_GLOBAL uint8_t*)flags[f].at(S.dev);
        Q.ints = (SLAMIT_GLOBAL int32_t*)(ints.at(S.dev) + 4 * f);
    }
    HIP_TRY_AT(where, slamit_stage_upload(S, L));
    if (nmax > 32 * 1024) HIP_TRY_AT(where, hipFuncSetAttribute(reinterpret_cast<const void*>(sim3_opt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, nmax + 16));
    hipLaunchKernelGGL(sim3_opt_kernel, dim3(nprob), dim3(256), (size_t)nmax + 16, S.st, recs.at(S.dev));
    HIP_TRY_AT(where, slamit_stage_download_and_wait(S, L));
    for (int f = 0; f < nprob; ++f) {
        const double* o = dbl[f].out.at(S.host);
        const int32_t* iv = ints.at(S.host) + 4 * f;
        memcpy(results[f].r12, o, 72); memcpy(results[f].t12, o + 9, 24);
        results[f].s12 = o[12];
        results[f].chi2[0] = o[13]; results[f].chi2[1] = o[14];
        results[f].n_inliers = iv[0]; results[f].n_its[0] = iv[1]; results[f].n_its[1] = iv[2];
        if (iv[3]) {   // the reference returned before touching g2oS12: hand the input back bit for bit
            memcpy(results[f].r12, probs[f].r12, 72); memcpy(results[f].t12, probs[f].t12, 24);
            results[f].s12 = probs[f].s12;
        }
        if (probs[f].n) memcpy(results[f].inlier, flags[f].at(S.host), flags[f].bytes());
    }
    return SLAMIT_OK;
}

int slamit_sim3_optimize(int device, const slamit_sim3_problem* prob, slamit_sim3_result* res) {
    return slamit_sim3_optimize_batch(device, 1, prob, res);
}

}  // extern "C"
