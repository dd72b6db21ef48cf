// pose.hip — Optimizer::PoseOptimization on the GPU (include/slamit.h, slamit_pose_*).
//
// Reference: ORB_SLAM2/src/Optimizer.cc:239-451 driving g2o (BlockSolver_6_3 + LinearSolverDense +
// Levenberg) over EdgeSE3ProjectXYZOnlyPose edges (Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h:143-170,
// cpp:266-288}) and, for the keypoints of a stereo / RGB-D frame that have a right-image column, EdgeStereoSE3ProjectXYZOnlyPose
// edges ({h:174-202, cpp:299-306, 335-364}; Optimizer.cc:319-356: three residual rows, Huber width sqrt(7.815), gate 7.815f).  The system is a single 6x6 block, so the whole schedule — 4 rounds x <= 10 LM
// iterations x <= 10 trials, the (float)chi2 > 5.991f relabelling between rounds, the kernel drop after
// the third round — runs inside ONE workgroup per frame with no host round trip; a batch of frames is
// one launch.  This file holds the edges (PoseModel: errors, normal-equation partials, oplus) and the rounds; the Levenberg
// iterations themselves are lm_block.h's lm_block_run<6, 7>, shared with sim3.hip, over the rules of lm_step.h.
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

struct PoseFrame {
    int32_t n;
    const SLAMIT_GLOBAL double* pose_in;   // 12
    const SLAMIT_GLOBAL double* intr;      // 4
    const SLAMIT_GLOBAL double* xw;        // n x 3
    const SLAMIT_GLOBAL double* uv;        // n x 2
    const SLAMIT_GLOBAL double* w;         // n
    SLAMIT_GLOBAL double* chi2;            // n scratch
    SLAMIT_GLOBAL uint8_t* outlier;        // n out
    SLAMIT_GLOBAL double* pose_out;        // 12
    SLAMIT_GLOBAL int32_t* n_inliers;      // 1
    SLAMIT_GLOBAL int32_t* n_its;          // 4
    SLAMIT_GLOBAL double* chi2_round;      // 4
    const SLAMIT_GLOBAL double* ur;        // n: right-image column, < 0 on a monocular correspondence; null when the frame has none (Optimizer.cc:281)
    double bf;               // Frame::mbf
};

namespace {

#define POSE_DELTA_STEREO ((double)(float)sqrt(7.815))   // deltaStereo, Optimizer.cc:265

__device__ __forceinline__ bool pose_is_stereo(const PoseFrame& F, int e) { return F.ur && !(F.ur[e] < 0.0); }

// error of a stereo edge at camera-frame point Xc: EdgeStereoSE3ProjectXYZOnlyPose::cam_project (types_six_dof_expmap.cpp:299-306),
// `const float invz = 1.0f / z` (the quotient rounded to float), bf a double member.  Returns chi2.
__device__ __forceinline__ double pose_stereo_error(const PoseFrame& F, int e, const double* Xc, double* err /*[3]*/) {
    const float invz = (float)(1.0 / Xc[2]);
    const double r0 = Xc[0] * (double)invz * F.intr[0] + F.intr[2];
    const double r1 = Xc[1] * (double)invz * F.intr[1] + F.intr[3];
    const double r2 = r0 - F.bf * (double)invz;
    err[0] = F.uv[2 * e] - r0; err[1] = F.uv[2 * e + 1] - r1; err[2] = F.ur[e] - r2;
    const double w = F.w[e];
    return err[0] * w * err[0] + err[1] * w * err[1] + err[2] * w * err[2];
}

// residual + chi2 of every active edge at pose T; returns the robust cost
__device__ double pose_errors(const PoseFrame& F, const double* T, const uint8_t* active, int robust, double delta, double* sh) {
    const double dsqr = (double)(float)(delta * delta);   // RobustKernelHuber::dsqr is a float member (g2o/core/robust_kernel_impl.h:84)
    const double delta_s = POSE_DELTA_STEREO, dsqr_s = (double)(float)(delta_s * delta_s);
    const double fx = F.intr[0], fy = F.intr[1], cx = F.intr[2], cy = F.intr[3];
    double part = 0;
    for (int e = threadIdx.x; e < F.n; e += 256) {
        if (!active[e]) continue;
        double Xc[3];
        quat_rot(T, F.xw + 3 * e, Xc);
        Xc[0] += T[4]; Xc[1] += T[5]; Xc[2] += T[6];
        if (pose_is_stereo(F, e)) {
            double err[3];
            const double c2 = pose_stereo_error(F, e, Xc, err);
            F.chi2[e] = c2;
            part += (robust && c2 > dsqr_s) ? 2 * sqrt(c2) * delta_s - dsqr_s : c2;
            continue;
        }
        const double e0 = F.uv[2 * e] - (Xc[0] / Xc[2] * fx + cx), e1 = F.uv[2 * e + 1] - (Xc[1] / Xc[2] * fy + cy);
        const double w = F.w[e];
        const double c2 = e0 * w * e0 + e1 * w * e1;
        F.chi2[e] = c2;
        part += (robust && c2 > dsqr) ? 2 * sqrt(c2) * delta - dsqr : c2;
    }
    return lm_block_sum(part, sh);
}

// the edges of one frame as lm_block_run sees them (lm_block.h); T = q(x, y, z, w), t
struct PoseModel {
    const PoseFrame& F;
    const uint8_t* active;   // LDS: the edge is at level 0
    int robust;
    double delta;
    double* sh;              // LDS [4]: the block sum's

    __device__ __forceinline__ double errors(const double* T) const { return pose_errors(F, T, active, robust, delta, sh); }
    __device__ __forceinline__ void prepare(const double*) const {}
    __device__ __forceinline__ void oplus(double* T, const double* x) const { pose_oplus(T, x); }
    // H (21 unique), b (6) over this thread's active edges; the chi2 are those errors() left at this very pose
    __device__ __forceinline__ void accumulate(const double* sT, double* h, double* bb) const {
        const int tid = threadIdx.x, n = F.n;
        const double dsqr = (double)(float)(delta * delta), fx = F.intr[0], fy = F.intr[1];
        for (int e = tid; e < n; e += 256) {
            if (!active[e]) continue;
            double Xc[3];
            quat_rot(sT, F.xw + 3 * e, Xc);
            Xc[0] += sT[4]; Xc[1] += sT[5]; Xc[2] += sT[6];
            const double x = Xc[0], y = Xc[1], invz = 1.0 / Xc[2], invz_2 = invz * invz;
            double J[12];
            J[0] = x * y * invz_2 * fx; J[1] = -(1 + (x * x * invz_2)) * fx; J[2] = y * invz * fx;
            J[3] = -invz * fx; J[4] = 0; J[5] = x * invz_2 * fx;
            J[6] = (1 + y * y * invz_2) * fy; J[7] = -x * y * invz_2 * fy; J[8] = -x * invz * fy;
            J[9] = 0; J[10] = -invz * fy; J[11] = y * invz_2 * fy;
            const double w = F.w[e], c2 = F.chi2[e];
            if (pose_is_stereo(F, e)) {   // third row: EdgeStereoSE3ProjectXYZOnlyPose::linearizeOplus (types_six_dof_expmap.cpp:335-364)
                const double bf = F.bf, delta_s = POSE_DELTA_STEREO, dsqr_s = (double)(float)(delta_s * delta_s);
                const double J2[6] = {J[0] - bf * y * invz_2, J[1] + bf * x * invz_2, J[2], J[3], 0.0, J[5] - bf * invz_2};
                double err[3];
                pose_stereo_error(F, e, Xc, err);
                const double hub1s = (robust && c2 > dsqr_s) ? delta_s / sqrt(c2) : 1.0;
                const double wOs = hub1s * w;
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    bb[a] -= hub1s * (J[a] * w * err[0] + J[6 + a] * w * err[1] + J2[a] * w * err[2]);
#pragma unroll
                    for (int c = a; c < 6; ++c) h[k++] += (J[a] * J[c] + J[6 + a] * J[6 + c] + J2[a] * J2[c]) * wOs;
                }
                continue;
            }
            const double e0 = F.uv[2 * e] - (x * invz * fx + F.intr[2]), e1 = F.uv[2 * e + 1] - (y * invz * fy + F.intr[3]);
            const double hub1 = (robust && c2 > dsqr) ? delta / sqrt(c2) : 1.0;
            const double wO = hub1 * w;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                bb[a] -= hub1 * (J[a] * w * e0 + J[6 + a] * w * e1);
#pragma unroll
                for (int c = a; c < 6; ++c) h[k++] += (J[a] * J[c] + J[6 + a] * J[6 + c]) * wO;
            }
        }
    }
};

}  // namespace

__global__ __launch_bounds__(256) void pose_opt_kernel(const PoseFrame* frames) {
    const PoseFrame F = frames[blockIdx.x];
    const int tid = threadIdx.x, n = F.n;
    __shared__ LmBlock<6, 7> S;
    __shared__ double sT0[7];
    double* const sT = S.state;
    extern __shared__ uint8_t s_act[];  // n bytes: edge is at level 0
    if (n < 3) {  // Optimizer.cc:364-365
        if (tid < 12) F.pose_out[tid] = F.pose_in[tid];
        if (tid < n) F.outlier[tid] = 0;
        if (tid == 0) { *F.n_inliers = 0; for (int r = 0; r < 4; ++r) { F.n_its[r] = 0; F.chi2_round[r] = 0; } }
        return;
    }
    if (tid == 0) {
        double R[9], q[4];
        for (int i = 0; i < 9; ++i) R[i] = F.pose_in[i];
        R_to_quat(R, q);
        quat_normalize(q);
        for (int i = 0; i < 4; ++i) sT0[i] = q[i];
        for (int i = 0; i < 3; ++i) sT0[4 + i] = F.pose_in[9 + i];
        for (int r = 0; r < 4; ++r) { F.n_its[r] = 0; F.chi2_round[r] = 0; }
    }
    for (int e = tid; e < n; e += 256) { s_act[e] = 1; F.outlier[e] = 0; F.chi2[e] = 0; }
    __syncthreads();
    const double delta = (double)(float)sqrt(5.991);
    int robust = 1, nBad = 0;
    for (int round = 0; round < 4; ++round) {
        if (tid < 7) sT[tid] = sT0[tid];  // every round restarts from the input pose (:373)
        int nact = 0;
        for (int e = tid; e < n; e += 256) nact += s_act[e];
        const bool any_active = lm_block_count(nact, &S.cnt) > 0;
        int done = 0;
        double lastChi = 0;
        if (any_active) done = lm_block_run(S, PoseModel{F, s_act, robust, delta, S.sum}, 10, lastChi);
        // ---- relabel (:374-404): outliers are re-evaluated at the new pose, (float)chi2 vs 5.991f ----
        const double fx = F.intr[0], fy = F.intr[1], cx = F.intr[2], cy = F.intr[3];
        int bad = 0;
        for (int e = tid; e < n; e += 256) {
            double c2 = F.chi2[e];
            if (F.outlier[e]) {
                double Xc[3];
                quat_rot(sT, F.xw + 3 * e, Xc);
                Xc[0] += sT[4]; Xc[1] += sT[5]; Xc[2] += sT[6];
                if (pose_is_stereo(F, e)) {
                    double err[3];
                    c2 = pose_stereo_error(F, e, Xc, err);
                } else {
                const double e0 = F.uv[2 * e] - (Xc[0] / Xc[2] * fx + cx), e1 = F.uv[2 * e + 1] - (Xc[1] / Xc[2] * fy + cy);
                const double w = F.w[e];
                c2 = e0 * w * e0 + e1 * w * e1;
                }
                F.chi2[e] = c2;
            }
            const bool out = (float)c2 > (pose_is_stereo(F, e) ? 7.815f : 5.991f);   // chi2Mono / chi2Stereo, Optimizer.cc:369-370
            F.outlier[e] = out;
            s_act[e] = !out;
            bad += out;
        }
        nBad = lm_block_count(bad, &S.cnt);
        if (round == 2) robust = 0;
        if (tid == 0) { F.n_its[round] = done; F.chi2_round[round] = lastChi; }
        __syncthreads();
        if (n < 10) break;  // optimizer.edges().size() < 10
    }
    if (tid == 0) {
        double R[9];
        quat_to_R(sT, R);
        for (int i = 0; i < 9; ++i) F.pose_out[i] = R[i];
        for (int i = 0; i < 3; ++i) F.pose_out[9 + i] = sT[4 + i];
        *F.n_inliers = n - nBad;
    }
}

extern "C" {

int slamit_pose_optimize_batch(int device, int nframes, const slamit_pose_problem* probs, slamit_pose_result* results) {
    const char* const where = "slamit_pose_optimize_batch";
    if (nframes < 0 || (nframes && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pose_optimize_batch: bad argument");
    if (nframes == 0) return SLAMIT_OK;
    for (int f = 0; f < nframes; ++f) {
        const slamit_pose_problem& P = probs[f];
        if (P.n < 0 || !P.pose || !P.intr || (P.n && (!P.xw || !P.uv || !P.inv_sigma2)) || !results[f].pose || (P.n && !results[f].outlier))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_pose_optimize_batch: null array");
        if (P.n > SLAMIT_POSE_MAX_N) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_pose_optimize_batch: more than SLAMIT_POSE_MAX_N correspondences");
    }
    SLAMIT_USE_DEVICE(device);
    // [doubles of every frame (lm_layout.h) | ints | PoseFrame records | flags].  A frame's doubles mix what the kernel reads and
    // writes, so everything but the flags goes up and the whole block comes down.
    StageLayout L;
    std::vector<PoseSpans> dbl(nframes);
    std::vector<StageSpan<uint8_t>> flags(nframes);
    int nmax = 1;
    for (int f = 0; f < nframes; ++f) { dbl[f] = pose_take(L, probs[f].n, probs[f].ur != nullptr); nmax = std::max(nmax, (int)probs[f].n); }
    const StageSpan<int32_t> ints = L.take<int32_t>(5 * (size_t)nframes, 4);   // per frame: n_inliers, n_its[4]
    const StageSpan<PoseFrame> frames = L.take<PoseFrame>(nframes, 16);
    L.end_inputs(1); L.out_off = 0;   // (the whole block comes down)
    for (int f = 0; f < nframes; ++f) flags[f] = lm_take_flags(L, probs[f].n);
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT(where, slamit_stage_reserve(S, device, L));
    for (int f = 0; f < nframes; ++f) {
        const slamit_pose_problem& P = probs[f];
        const PoseSpans& s = dbl[f];
        memcpy(s.pose_in.at(S.host), P.pose, s.pose_in.bytes()); memcpy(s.intr.at(S.host), P.intr, s.intr.bytes());
        if (P.n) { memcpy(s.xw.at(S.host), P.xw, s.xw.bytes()); memcpy(s.uv.at(S.host), P.uv, s.uv.bytes()); memcpy(s.w.at(S.host), P.inv_sigma2, s.w.bytes()); }
        PoseFrame& F = frames.at(S.host)[f];
        typedef SLAMIT_GLOBAL double gd;
        typedef SLAMIT_GLOBAL int32_t gi;
        F.n = P.n; F.pose_in = (const gd*)s.pose_in.at(S.dev); F.intr = (const gd*)s.intr.at(S.dev); F.xw = (const gd*)s.xw.at(S.dev);
        F.uv = (const gd*)s.uv.at(S.dev); F.w = (const gd*)s.w.at(S.dev);
        F.chi2 = (gd*)s.chi2.at(S.dev); F.pose_out = (gd*)s.pose_out.at(S.dev); F.chi2_round = (gd*)s.chi2_round.at(S.dev);
        F.ur = nullptr; F.bf = 0.0;
        if (P.ur && P.n) { memcpy(s.ur.at(S.host), P.ur, s.ur.bytes()); F.ur = (const gd*)s.ur.at(S.dev); F.bf = P.bf; }
        F.outlier = (SLAMIT_GLOBAL uint8_t*)flags[f].at(S.dev);
        F.n_inliers = (gi*)(ints.at(S.dev) + 5 * f); F.n_its = (gi*)(ints.at(S.dev) + 5 * f + 1);
    }
    HIP_TRY_AT(where, slamit_stage_upload(S, L));
    if (nmax > 32 * 1024) HIP_TRY_AT(where, hipFuncSetAttribute(reinterpret_cast<const void*>(pose_opt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, nmax + 16));
    hipLaunchKernelGGL(pose_opt_kernel, dim3(nframes), dim3(256), (size_t)nmax + 16, S.st, frames.at(S.dev));
    HIP_TRY_AT(where, slamit_stage_download_and_wait(S, L));
    for (int f = 0; f < nframes; ++f) {
        const PoseSpans& s = dbl[f];
        const int32_t* iv = ints.at(S.host) + 5 * f;
        memcpy(results[f].pose, s.pose_out.at(S.host), s.pose_out.bytes());
        for (int r = 0; r < 4; ++r) { results[f].chi2[r] = s.chi2_round.at(S.host)[r]; results[f].n_its[r] = iv[1 + r]; }
        results[f].n_inliers = iv[0];
        if (probs[f].n) memcpy(results[f].outlier, flags[f].at(S.host), flags[f].bytes());
    }
    return SLAMIT_OK;
}

int slamit_pose_optimize(int device, const slamit_pose_problem* prob, slamit_pose_result* res) {
    return slamit_pose_optimize_batch(device, 1, prob, res);
}

}  // extern "C"
