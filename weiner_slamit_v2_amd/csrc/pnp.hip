// pnp.hip — PnPsolver's hypothesis evaluation and Refine() on the GPU (include/slamit.h, slamit_pnp_*).
//
// Reference: ORB_SLAM2/src/PnPsolver.cc.  iterate() (:173-266) draws four correspondences, compute_pose (:485-533) solves EPnP on them,
// CheckInliers (:316-347) reprojects all N correspondences and counts those under their chi-square bounds; Refine() (:268-313) does
// the same from the inliers of the best hypothesis.  The solve is csrc/epnp.h, the same text the host tests build: a TEAM of threads
// shares one EpnpWork in LDS.
//
//   pnp_hyp_kernel     one wavefront (a workgroup of 64) per (candidate keyframe, hypothesis).  The 12 x 12 Jacobi runs its six
//                      independent rotations of a round over the lanes (72 element pairs per half round), the three
//                      find_betas_approx branches run in three lanes, everything lives in 8.6 KB of LDS; then the lanes stride over
//                      the correspondences, a ballot builds the inlier words and its popcount the count.
//   pnp_refine_kernel  one workgroup of 256 per problem: the sums over the subset (centroid, PW0^T PW0, the 78 entries of M^T M, per
//                      branch the centroids, ABt and the reprojection error) are block reductions, the small dense part is the same
//                      code with more threads, CheckInliers over all n follows.
//
// Launches are small (35 hypotheses per candidate under Tracking's parameters): latency matters, not throughput.  The sampling,
// SetRansacParameters and iterate()'s scan stay on the host (shim/PnPsolver.h, api.PnPsolver).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "epnp.h"
#include "slamit_internal.h"

struct PnpProb {
    int32_t n, n_hyp, words, pad;   // words = (n + 31) / 32
    double intr[4];
    const SLAMIT_GLOBAL float* p3d; const SLAMIT_GLOBAL float* p2d; const SLAMIT_GLOBAL float* max_err;
    const SLAMIT_GLOBAL int32_t* quads;
    SLAMIT_GLOBAL double* pose; SLAMIT_GLOBAL int32_t* counts; SLAMIT_GLOBAL uint32_t* bits;
};

struct PnpRefineProb {
    int32_t n, nc, first, words;    // nc = members of the subset, first = the lowest of them; the host has counted
    double intr[4];
    const SLAMIT_GLOBAL float* p3d; const SLAMIT_GLOBAL float* p2d; const SLAMIT_GLOBAL float* max_err;
    const SLAMIT_GLOBAL uint32_t* subset;
    SLAMIT_GLOBAL double* pose; SLAMIT_GLOBAL int32_t* count; SLAMIT_GLOBAL uint32_t* bits;
};

// CheckInliers for the correspondences base + lane of one 64-chunk: the ballot of the inliers; lanes 0 and 1 store its two words
template <typename ProbT>
__device__ __forceinline__ unsigned long long pnp_check_chunk(const ProbT& P, const double pose[12], int base, int lane, SLAMIT_GLOBAL uint32_t* bits) {
    const int i = base + lane;
    bool in = false;
    if (i < P.n)
        in = epnp_inlier(pose, P.p3d[3 * i], P.p3d[3 * i + 1], P.p3d[3 * i + 2], P.p2d[2 * i], P.p2d[2 * i + 1], P.intr[0], P.intr[1], P.intr[2], P.intr[3],
                         P.max_err[i]);
    const unsigned long long m = __ballot(in);
    const int w = base >> 5;
    if (lane == 0) bits[w] = (uint32_t)m;
    if (lane == 1 && w + 1 < P.words) bits[w + 1] = (uint32_t)(m >> 32);
    return m;
}

// grid (max n_hyp, problems), 64 threads: the workgroup is hypothesis blockIdx.x of problem blockIdx.y.
// The host has checked every quadruple index against [0, n).
__global__ __launch_bounds__(64) void pnp_hyp_kernel(const PnpProb* __restrict__ probs) {
    __shared__ EpnpWork W;
    const PnpProb P = probs[blockIdx.y];
    const int lane = threadIdx.x, h = blockIdx.x;
    if (h >= P.n_hyp) return;   // uniform over the workgroup
    EpnpSet S;
    S.p3d = P.p3d; S.p2d = P.p2d; S.quad = P.quads + 4 * h; S.mask = nullptr;
    S.span = 4; S.nc = 4; S.first = 0;
    S.fu = P.intr[0]; S.fv = P.intr[1]; S.uc = P.intr[2]; S.vc = P.intr[3];
    const EpnpTeam T = {lane, 64};
    double pose[12];
    epnp_compute_pose(T, &W, S, pose);
    int count = 0;
    SLAMIT_GLOBAL uint32_t* bits = P.bits + (size_t)h * P.words;
    for (int base = 0; base < P.n; base += 64) count += __popcll(pnp_check_chunk(P, pose, base, lane, bits));
    if (lane < 12) {
        double v = pose[0];
#pragma unroll
        for (int k = 1; k < 12; ++k) v = lane == k ? pose[k] : v;
        P.pose[12 * (size_t)h + lane] = v;
    }
    if (lane == 0) P.counts[h] = count;
}

// grid (problems), 256 threads.  The host has checked 4 <= nc.
__global__ __launch_bounds__(256) void pnp_refine_kernel(const PnpRefineProb* __restrict__ probs) {
    __shared__ EpnpWork W;
    __shared__ int wave_count[4];
    const PnpRefineProb P = probs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    EpnpSet S;
    S.p3d = P.p3d; S.p2d = P.p2d; S.quad = nullptr; S.mask = P.subset;
    S.span = P.n; S.nc = P.nc; S.first = P.first;
    S.fu = P.intr[0]; S.fv = P.intr[1]; S.uc = P.intr[2]; S.vc = P.intr[3];
    const EpnpTeam T = {tid, 256};
    double pose[12];
    epnp_compute_pose(T, &W, S, pose);
    int count = 0;
    for (int base = 64 * wave; base < P.n; base += 256) count += __popcll(pnp_check_chunk(P, pose, base, lane, P.bits));
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid < 12) {
        double v = pose[0];
#pragma unroll
        for (int k = 1; k < 12; ++k) v = tid == k ? pose[k] : v;
        P.pose[tid] = v;
    }
    if (tid == 0) P.count[0] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

extern "C" {

int slamit_pnp_ransac_batch(int device, int nprob, const slamit_pnp_problem* probs, slamit_pnp_result* results) {
    const char* const where = "slamit_pnp_ransac_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    int max_hyp = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_pnp_problem& P = probs[f];
        if (P.n < 0 || P.n_hyp < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: negative count");
        if (P.n > SLAMIT_PNP_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: more than SLAMIT_PNP_MAX_N correspondences");
        if (P.n_hyp > SLAMIT_PNP_MAX_HYP) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: more than SLAMIT_PNP_MAX_HYP hypotheses");
        if (P.n == 0 || P.n_hyp == 0) continue;   // nothing to evaluate, nothing written
        if (!P.p3d || !P.p2d || !P.max_err || !P.quads || !results[f].pose || !results[f].n_inliers)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: null array");
        for (int k = 0; k < 4 * P.n_hyp; ++k)
            if (P.quads[k] < 0 || P.quads[k] >= P.n) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_ransac_batch: quadruple index outside [0, n)");
        max_hyp = std::max(max_hyp, (int)P.n_hyp);
    }
    if (max_hyp == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: p3d p2d max_err quads] go up; [per problem: pose counts (bits when asked for)] come down; the bits
    // nobody asked for stay on the device
    static thread_local SlamitScratch S;
    return slamit_staged_batch<PnpProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, PnpProb& Q) {
            const slamit_pnp_problem& P = probs[f];
            const slamit_pnp_result& R = results[f];
            const size_t hyp = P.n == 0 ? 0 : (size_t)P.n_hyp, words = ((size_t)P.n + 31) / 32;
            const size_t n = hyp ? (size_t)P.n : 0;
            Q.n = P.n; Q.n_hyp = (int32_t)hyp; Q.words = (int32_t)words;
            memcpy(Q.intr, P.intr, sizeof(Q.intr));
            Q.p3d = slamit_global(b.in(P.p3d, 3 * n)); Q.p2d = slamit_global(b.in(P.p2d, 2 * n)); Q.max_err = slamit_global(b.in(P.max_err, n));
            Q.quads = slamit_global(b.in(P.quads, 4 * hyp));
            Q.pose = slamit_global(b.out(R.pose, 12 * hyp)); Q.counts = slamit_global(b.out(R.n_inliers, hyp));
            Q.bits = slamit_global(R.inlier_bits ? b.out(R.inlier_bits, hyp * words) : b.scratch<uint32_t>(hyp * words));
        },
        [&](const PnpProb* d_recs) {
            hipLaunchKernelGGL(pnp_hyp_kernel, dim3(max_hyp, nprob), dim3(64), 0, S.st, d_recs);
            return hipGetLastError();
        });
}

int slamit_pnp_ransac(int device, const slamit_pnp_problem* prob, slamit_pnp_result* res) {
    return slamit_pnp_ransac_batch(device, 1, prob, res);
}

int slamit_pnp_refine_batch(int device, int nprob, const slamit_pnp_refine_problem* probs, slamit_pnp_refine_result* results) {
    const char* const where = "slamit_pnp_refine_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_refine_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    struct Live { int f, nc, first; };   // a problem with correspondences: the members of its subset and the lowest of them
    std::vector<Live> live;
    for (int f = 0; f < nprob; ++f) {
        const slamit_pnp_refine_problem& P = probs[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_refine_batch: negative count");
        if (P.n > SLAMIT_PNP_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_refine_batch: more than SLAMIT_PNP_MAX_N correspondences");
        if (P.n == 0) continue;   // nothing to solve, nothing written
        if (!P.p3d || !P.p2d || !P.max_err || !P.subset_bits) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_refine_batch: null array");
        Live l = {f, 0, -1};
        for (int i = 0; i < P.n; ++i)
            if ((P.subset_bits[i >> 5] >> (i & 31)) & 1u) {
                if (l.first < 0) l.first = i;
                ++l.nc;
            }
        if (l.nc < 4) return slamit_fail(SLAMIT_ERR_ARG, "slamit_pnp_refine_batch: a subset of fewer than four correspondences");
        live.push_back(l);
    }
    if (live.empty()) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per live problem: p3d p2d max_err subset] go up; [per live problem: pose count (bits when asked for)] come down
    static thread_local SlamitScratch S;
    return slamit_staged_batch<PnpRefineProb>(
        where, S, device, (int)live.size(),
        [&](StageBinder& b, int k, PnpRefineProb& Q) {
            const slamit_pnp_refine_problem& P = probs[live[k].f];
            slamit_pnp_refine_result& R = results[live[k].f];
            const size_t n = (size_t)P.n, words = (n + 31) / 32;
            Q.n = P.n; Q.nc = live[k].nc; Q.first = live[k].first; Q.words = (int32_t)words;
            memcpy(Q.intr, P.intr, sizeof(Q.intr));
            Q.p3d = slamit_global(b.in(P.p3d, 3 * n)); Q.p2d = slamit_global(b.in(P.p2d, 2 * n)); Q.max_err = slamit_global(b.in(P.max_err, n));
            Q.subset = slamit_global(b.in(P.subset_bits, words));
            Q.pose = slamit_global(b.out(R.pose, 12)); Q.count = slamit_global(b.out(&R.n_inliers, 1));
            Q.bits = slamit_global(R.inlier_bits ? b.out(R.inlier_bits, words) : b.scratch<uint32_t>(words));
        },
        [&](const PnpRefineProb* d_recs) {
            hipLaunchKernelGGL(pnp_refine_kernel, dim3((unsigned)live.size()), dim3(256), 0, S.st, d_recs);
            return hipGetLastError();
        });
}

}  // extern "C"
