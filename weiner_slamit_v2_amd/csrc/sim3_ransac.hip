// sim3_ransac.hip — Sim3Solver's hypothesis evaluation on the GPU (include/slamit.h, slamit_sim3_ransac*).
//
// Reference: ORB_SLAM2/src/Sim3Solver.cc.  iterate() (:140-207) draws three correspondences, ComputeSim3 (:226-337) solves Horn's
// closed form on them, CheckInliers (:340-364) projects all N correspondences both ways and counts those under their chi-square
// bounds.  Every (candidate keyframe, hypothesis) pair is independent: ONE WAVEFRONT takes one pair.  The closed form (sim3_horn.h)
// runs wave-uniform -- all 64 lanes compute the same 13 numbers, which costs nothing a lane would otherwise use -- then the lanes
// stride over the correspondences, a ballot builds the inlier words and its popcount the count.  No LDS, no atomics, no
// cross-wave traffic; a batch of candidates is one launch.  The sampling and iterate()'s sequential acceptance scan stay on
// the host (shim/Sim3Solver.h, api.Sim3Solver).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/slamit.h"
#include "sim3_horn.h"
#include "slamit_internal.h"

struct Sim3RansacProb {
    int32_t n, n_hyp, fix_scale, words;   // words = (n + 31) / 32
    float intr1[4], intr2[4];
    const SLAMIT_GLOBAL float* x1; const SLAMIT_GLOBAL float* x2; const SLAMIT_GLOBAL float* e1; const SLAMIT_GLOBAL float* e2;
    const SLAMIT_GLOBAL int32_t* triples;
    SLAMIT_GLOBAL float* t12; SLAMIT_GLOBAL int32_t* counts; SLAMIT_GLOBAL uint32_t* bits;
};

// grid (ceil(max n_hyp / 4), problems), 256 threads: wave w of block b takes hypothesis 4 b + w of problem blockIdx.y.
// The host has checked every triple index against [0, n).
__global__ __launch_bounds__(256) void sim3_ransac_kernel(const Sim3RansacProb* __restrict__ probs) {
    const Sim3RansacProb P = probs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int h = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int n = P.n;
    if (h >= P.n_hyp) return;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int idx = P.triples[3 * h + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) { P1[k][a] = P.x1[3 * idx + a]; P2[k][a] = P.x2[3 * idx + a]; }
    }
    Sim3Hyp H;
    sim3h_solve(P1, P2, P.fix_scale, H);
    const float K1[4] = {P.intr1[0], P.intr1[1], P.intr1[2], P.intr1[3]}, K2[4] = {P.intr2[0], P.intr2[1], P.intr2[2], P.intr2[3]};
    int count = 0;
    SLAMIT_GLOBAL uint32_t* bits = P.bits + (size_t)h * P.words;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float X1[3] = {P.x1[3 * i], P.x1[3 * i + 1], P.x1[3 * i + 2]}, X2[3] = {P.x2[3 * i], P.x2[3 * i + 1], P.x2[3 * i + 2]};
            float err1, err2;
            sim3h_errors(H, X1, X2, K1, K2, &err1, &err2);
            in = err1 < P.e1[i] && err2 < P.e2[i];   // NaN: an outlier
        }
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        const int w = base >> 5;
        if (lane == 0) bits[w] = (uint32_t)m;
        if (lane == 1 && w + 1 < P.words) bits[w + 1] = (uint32_t)(m >> 32);
    }
    if (lane < 13) {
        float v = H.s;
#pragma unroll
        for (int k = 0; k < 9; ++k) v = lane == k ? H.R[k] : v;
#pragma unroll
        for (int k = 0; k < 3; ++k) v = lane == 9 + k ? H.t[k] : v;
        P.t12[13 * (size_t)h + lane] = v;
    }
    if (lane == 0) P.counts[h] = count;
}

extern "C" {

int slamit_sim3_ransac_batch(int device, int nprob, const slamit_sim3_ransac_problem* probs, slamit_sim3_ransac_result* results) {
    const char* const where = "slamit_sim3_ransac_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    int max_hyp = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_sim3_ransac_problem& P = probs[f];
        if (P.n < 0 || P.n_hyp < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: negative count");
        if (P.n > SLAMIT_SIM3_RANSAC_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: more than SLAMIT_SIM3_RANSAC_MAX_N correspondences");
        if (P.n_hyp > SLAMIT_SIM3_RANSAC_MAX_HYP) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: more than SLAMIT_SIM3_RANSAC_MAX_HYP hypotheses");
        if (P.n == 0 || P.n_hyp == 0) continue;   // nothing to evaluate, nothing written
        if (!P.x1 || !P.x2 || !P.max_err1 || !P.max_err2 || !P.triples || !results[f].t12 || !results[f].n_inliers)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: null array");
        for (int k = 0; k < 3 * P.n_hyp; ++k)
            if (P.triples[k] < 0 || P.triples[k] >= P.n) return slamit_fail(SLAMIT_ERR_ARG, "slamit_sim3_ransac_batch: triple index outside [0, n)");
        max_hyp = std::max(max_hyp, (int)P.n_hyp);
    }
    if (max_hyp == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: x1 x2 max_err1 max_err2 triples] go up; [per problem: t12 counts (bits when asked for)] come down; the bits
    // nobody asked for stay on the device
    static thread_local SlamitScratch S;
    return slamit_staged_batch<Sim3RansacProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, Sim3RansacProb& Q) {
            const slamit_sim3_ransac_problem& P = probs[f];
            const slamit_sim3_ransac_result& R = results[f];
            const size_t hyp = P.n == 0 ? 0 : (size_t)P.n_hyp, words = ((size_t)P.n + 31) / 32;
            const size_t n = hyp ? (size_t)P.n : 0;
            Q.n = P.n; Q.n_hyp = (int32_t)hyp; Q.fix_scale = P.fix_scale; Q.words = (int32_t)words;
            memcpy(Q.intr1, P.intr1, sizeof(Q.intr1)); memcpy(Q.intr2, P.intr2, sizeof(Q.intr2));
            Q.x1 = slamit_global(b.in(P.x1, 3 * n)); Q.x2 = slamit_global(b.in(P.x2, 3 * n));
            Q.e1 = slamit_global(b.in(P.max_err1, n)); Q.e2 = slamit_global(b.in(P.max_err2, n));
            Q.triples = slamit_global(b.in(P.triples, 3 * hyp));
            Q.t12 = slamit_global(b.out(R.t12, 13 * hyp)); Q.counts = slamit_global(b.out(R.n_inliers, hyp));
            Q.bits = slamit_global(R.inlier_bits ? b.out(R.inlier_bits, hyp * words) : b.scratch<uint32_t>(hyp * words));
        },
        [&](const Sim3RansacProb* d_recs) {
            hipLaunchKernelGGL(sim3_ransac_kernel, dim3((max_hyp + 3) / 4, nprob), dim3(256), 0, S.st, d_recs);
            return hipGetLastError();
        });
}

int slamit_sim3_ransac(int device, const slamit_sim3_ransac_problem* prob, slamit_sim3_ransac_result* res) {
    return slamit_sim3_ransac_batch(device, 1, prob, res);
}

}  // extern "C"
