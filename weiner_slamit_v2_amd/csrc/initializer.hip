// initializer.hip — the monocular Initializer on the GPU (include/slamit.h, slamit_init_*).
//
// Reference: ORB_SLAM2/src/Initializer.cc.  FindHomography / FindFundamental (:133-232) solve one model per eight-match set and score
// it over all matches; ReconstructH / ReconstructF (:479-741) turn the kept model into eight / four motions and run CheckRT
// (:807-916) for each over the inliers of the kept hypothesis.  All arithmetic is csrc/two_view.h, the text the host tests build.
//
//   init_hyp_kernel     one wavefront (a workgroup of 64) per (problem, hypothesis, model): grid (max n_hyp, 2, problems).  Lanes 0..7
//                       gather the eight pairs, the 9-column Jacobi runs its four rotations of a round over the lanes in 2.1 KB of LDS,
//                       then the lanes stride over the matches: a ballot builds the inlier words, and the two score terms of the 64
//                       matches of a chunk are added by ONE chain of dependent float adds in match order (v_readlane per term), which
//                       is the order of the reference's loop.  No tree: the float sum decides the kept hypothesis and RH.
//   init_motion_kernel  one workgroup of 256 per (problem, motion): grid (8, problems).  Every workgroup recomputes the 3 x 3
//                       decomposition (cheaper than a round trip), its lanes stride over the matches of the subset, write status and
//                       point per match, ballot the vbGood words and collect the keys of the accepted cosines in LDS; the
//                       min(50, nGood - 1)-th smallest is found bit by bit over the keys (32 counting passes), an exact selection.
//
// Sampling, the strict-> scan over the scores, RH and the ReconstructF / ReconstructH cascades stay on the host (two_view.h, exported
// below for the shim and the binding).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "two_view.h"

struct InitHypProb {
    int32_t n, n_hyp, words, pad;
    TvNorm n1, n2;
    float inv_sigma2, pad2[3];
    const SLAMIT_GLOBAL float* m12; const SLAMIT_GLOBAL int32_t* sets;
    SLAMIT_GLOBAL float* model; SLAMIT_GLOBAL float* score; SLAMIT_GLOBAL int32_t* counts; SLAMIT_GLOBAL uint32_t* bits;
};

struct InitMotionProb {
    int32_t n, kind, words, pad;
    float M[9], K[9], sigma, pad2;
    const SLAMIT_GLOBAL float* m12; const SLAMIT_GLOBAL uint32_t* subset;
    SLAMIT_GLOBAL int32_t* decomposable; SLAMIT_GLOBAL float* R; SLAMIT_GLOBAL float* t; SLAMIT_GLOBAL int32_t* n_good; SLAMIT_GLOBAL float* cos_sel;
    SLAMIT_GLOBAL uint8_t* status; SLAMIT_GLOBAL float* points; SLAMIT_GLOBAL uint32_t* good_bits;
};

// score += the accepted terms of one chunk in match order: lane l's two terms follow lane l-1's
__device__ __forceinline__ float init_chain(float score, float t1, float t2, unsigned long long ok1, unsigned long long ok2) {
#pragma unroll
    for (int l = 0; l < 64; ++l) {
        const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t1), l));
        const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t2), l));
        const float sa = score + a;
        score = ((ok1 >> l) & 1ull) ? sa : score;
        const float sb = score + b;
        score = ((ok2 >> l) & 1ull) ? sb : score;
    }
    return score;
}

// grid (max n_hyp, 2, problems), 64 threads.  The host has checked every set index against [0, n).
__global__ __launch_bounds__(64) void init_hyp_kernel(const InitHypProb* __restrict__ probs) {
    __shared__ TvWork W;
    const InitHypProb P = probs[blockIdx.z];
    const int lane = threadIdx.x, h = blockIdx.x, model = blockIdx.y;
    if (h >= P.n_hyp) return;   // uniform over the workgroup
    const TvTeam T = {lane, 64};
    if (lane < 8) {
        const SLAMIT_GLOBAL float* q = P.m12 + 4 * (size_t)P.sets[8 * (size_t)h + lane];
        const float p[4] = {q[0], q[1], q[2], q[3]};
        tv_fill_pair(&W, model, lane, p, P.n1, P.n2);
    }
    float M[9], Mi[9];
    tv_model(T, &W, model, P.n1, P.n2, M, Mi);
    const size_t slot = (size_t)model * P.n_hyp + h;
    SLAMIT_GLOBAL uint32_t* bits = P.bits + slot * P.words;
    float score = 0.f;
    int count = 0;
    for (int base = 0; base < P.n; base += 64) {
        const int i = base + lane;
        TvTerms r = {0.f, 0.f, false, false};
        if (i < P.n) {
            const SLAMIT_GLOBAL float* q = P.m12 + 4 * (size_t)i;
            const float p[4] = {q[0], q[1], q[2], q[3]};
            r = tv_check(model, M, Mi, p, P.inv_sigma2);
        }
        const unsigned long long ok1 = __ballot(r.ok1), ok2 = __ballot(r.ok2), in = ok1 & ok2;
        score = init_chain(score, r.t1, r.t2, ok1, ok2);
        const int w = base >> 5;
        if (lane == 0) bits[w] = (uint32_t)in;
        if (lane == 1 && w + 1 < P.words) bits[w + 1] = (uint32_t)(in >> 32);
        count += __popcll(in);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) P.model[9 * slot + k] = M[k];
        P.score[slot] = score; P.counts[slot] = count;
    }
}

#define INIT_MOTION_THREADS 256

// grid (8, problems), 256 threads.  Motion blockIdx.x of the problem's model; F has four.
__global__ __launch_bounds__(INIT_MOTION_THREADS) void init_motion_kernel(const InitMotionProb* __restrict__ probs) {
    __shared__ uint32_t keys[SLAMIT_INIT_MAX_N];
    __shared__ int n_keys;
    __shared__ int below[32];
    const InitMotionProb P = probs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mi = blockIdx.x;
    if (mi >= tv_motion_count(P.kind)) return;   // uniform over the workgroup
    if (tid == 0) n_keys = 0;
    if (tid < 32) below[tid] = 0;
    TvMotion mo;
    const bool ok = tv_motion(P.kind, P.M, P.K, mi, &mo);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) P.R[9 * mi + k] = mo.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) P.t[3 * mi + k] = mo.t[k];
        if (mi == 0) P.decomposable[0] = ok ? 1 : 0;
    }
    SLAMIT_GLOBAL uint8_t* status = P.status + (size_t)mi * P.n;
    SLAMIT_GLOBAL float* points = P.points + 3 * (size_t)mi * P.n;
    SLAMIT_GLOBAL uint32_t* good = P.good_bits + (size_t)mi * P.words;
    if (!ok) {   // uniform: ReconstructH returned before any CheckRT, so no match was looked at
        for (int i = tid; i < P.n; i += INIT_MOTION_THREADS) {
            status[i] = (uint8_t)TV_RT_NOT_INLIER;
            points[3 * (size_t)i] = 0.f; points[3 * (size_t)i + 1] = 0.f; points[3 * (size_t)i + 2] = 0.f;
        }
        for (int w = tid; w < P.words; w += INIT_MOTION_THREADS) good[w] = 0u;
        if (tid == 0) { P.n_good[mi] = 0; P.cos_sel[mi] = 1.f; }
        return;
    }
    TvCamera cam;
    tv_camera(P.K, mo, P.sigma, &cam);
    __syncthreads();
    for (int base = 64 * wave; base < P.n; base += INIT_MOTION_THREADS) {
        const int i = base + lane;
        bool is_good = false;
        if (i < P.n) {
            int st = TV_RT_NOT_INLIER;
            float X[3] = {0.f, 0.f, 0.f}, c = 0.f;
            if ((P.subset[i >> 5] >> (i & 31)) & 1u) {
                const SLAMIT_GLOBAL float* q = P.m12 + 4 * (size_t)i;
                const float p[4] = {q[0], q[1], q[2], q[3]};
                st = tv_check_rt(cam, p, X, &c, &is_good);
                if (st == TV_RT_OK) keys[atomicAdd(&n_keys, 1)] = tv_cos_key(__float_as_uint(c));   // at most n <= SLAMIT_INIT_MAX_N of them
            }
            status[i] = (uint8_t)st;
            points[3 * (size_t)i] = X[0]; points[3 * (size_t)i + 1] = X[1]; points[3 * (size_t)i + 2] = X[2];
        }
        const unsigned long long g = __ballot(is_good);
        const int w = base >> 5;
        if (lane == 0) good[w] = (uint32_t)g;
        if (lane == 1 && w + 1 < P.words) good[w + 1] = (uint32_t)(g >> 32);
    }
    __syncthreads();
    const int m = n_keys;
    if (m == 0) {
        if (tid == 0) { P.n_good[mi] = 0; P.cos_sel[mi] = 1.f; }
        return;
    }
    // the k-th smallest key, k = min(50, m - 1): the largest value v with fewer than k + 1 keys below it, built from the top bit down
    const int k = m - 1 < 50 ? m - 1 : 50;
    uint32_t v = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
        const uint32_t cand = v | (1u << b);
        int mine = 0;
        for (int j = tid; j < m; j += INIT_MOTION_THREADS) mine += keys[j] < cand ? 1 : 0;
        if (mine) atomicAdd(&below[b], mine);
        __syncthreads();
        if (below[b] <= k) v = cand;
    }
    if (tid == 0) { P.n_good[mi] = m; P.cos_sel[mi] = __uint_as_float(tv_cos_unkey(v)); }
}

// ---- C-ABI ----

// the matches of a problem as (u1, v1, u2, v2); the caller has checked the indices
static void init_gather(const float* keys1, const float* keys2, const int32_t* matches, int n, float* m12) {
    if (!m12) return;
    for (int i = 0; i < n; ++i) {
        const int a = matches[2 * i], b = matches[2 * i + 1];
        m12[4 * i] = keys1[2 * a]; m12[4 * i + 1] = keys1[2 * a + 1]; m12[4 * i + 2] = keys2[2 * b]; m12[4 * i + 3] = keys2[2 * b + 1];
    }
}

// n, the key tables and the match indices of a problem; null = fine
static const char* init_check_frames(int n1, const float* keys1, int n2, const float* keys2, int n, const int32_t* matches) {
    if (n1 < 0 || n2 < 0 || n < 0) return "negative count";
    if (n > SLAMIT_INIT_MAX_N) return "more than SLAMIT_INIT_MAX_N matches";
    if (n < 8) return "fewer than eight matches";
    if (!keys1 || !keys2 || !matches) return "null array";
    for (int i = 0; i < n; ++i)
        if (matches[2 * i] < 0 || matches[2 * i] >= n1 || matches[2 * i + 1] < 0 || matches[2 * i + 1] >= n2) return "match index outside its keypoint table";
    return nullptr;
}

extern "C" {

int slamit_init_hyp_batch(int device, int nprob, const slamit_init_problem* probs, slamit_init_result* results) {
    const char* const where = "slamit_init_hyp_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_refuse(where, "bad argument");
    if (nprob == 0) return SLAMIT_OK;
    int max_hyp = 0;
    std::vector<int> live;
    for (int f = 0; f < nprob; ++f) {
        const slamit_init_problem& P = probs[f];
        if (P.n_hyp < 0) return slamit_refuse(where, "negative count");
        if (P.n_hyp > SLAMIT_INIT_MAX_HYP) return slamit_refuse(where, "more than SLAMIT_INIT_MAX_HYP hypotheses");
        if (P.n_hyp == 0) continue;   // nothing to evaluate, nothing written
        if (const char* bad = init_check_frames(P.n1, P.keys1, P.n2, P.keys2, P.n, P.matches)) return slamit_refuse(where, bad);
        if (!P.sets || !results[f].model || !results[f].score || !results[f].n_inliers) return slamit_refuse(where, "null array");
        for (int h = 0; h < P.n_hyp; ++h)
            for (int j = 0; j < 8; ++j) {
                const int s = P.sets[8 * h + j];
                if (s < 0 || s >= P.n) return slamit_refuse(where, "set index outside [0, n)");
                for (int i = 0; i < j; ++i)
                    if (P.sets[8 * h + i] == s) return slamit_refuse(where, "a set repeats an index");
            }
        max_hyp = std::max(max_hyp, (int)P.n_hyp);
        live.push_back(f);
    }
    if (live.empty()) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per live problem: matches as coordinates, sets] go up; [model score counts (bits when asked for)] come down
    static thread_local SlamitScratch S;
    return slamit_staged_batch<InitHypProb>(
        where, S, device, (int)live.size(),
        [&](StageBinder& b, int k, InitHypProb& Q) {
            const slamit_init_problem& P = probs[live[k]];
            const slamit_init_result& R = results[live[k]];
            const size_t n = (size_t)P.n, hyp = (size_t)P.n_hyp, words = (n + 31) / 32;
            Q.n = P.n; Q.n_hyp = P.n_hyp; Q.words = (int32_t)words;
            float* m12 = nullptr;
            Q.m12 = slamit_global(b.in_fill<float>(4 * n, &m12));
            if (m12) {   // the bind pass: Normalize runs here, once per frame, over ALL keypoints
                init_gather(P.keys1, P.keys2, P.matches, P.n, m12);
                Q.n1 = tv_normalize(P.keys1, P.n1); Q.n2 = tv_normalize(P.keys2, P.n2);
                Q.inv_sigma2 = tv_inv_sigma2(P.sigma);
            }
            Q.sets = slamit_global(b.in(P.sets, 8 * hyp));
            Q.model = slamit_global(b.out(R.model, 2 * 9 * hyp)); Q.score = slamit_global(b.out(R.score, 2 * hyp));
            Q.counts = slamit_global(b.out(R.n_inliers, 2 * hyp));
            Q.bits = slamit_global(R.inlier_bits ? b.out(R.inlier_bits, 2 * hyp * words) : b.scratch<uint32_t>(2 * hyp * words));
        },
        [&](const InitHypProb* d_recs) {
            hipLaunchKernelGGL(init_hyp_kernel, dim3(max_hyp, 2, (unsigned)live.size()), dim3(64), 0, S.st, d_recs);
            return hipGetLastError();
        });
}

int slamit_init_hyp(int device, const slamit_init_problem* prob, slamit_init_result* res) { return slamit_init_hyp_batch(device, 1, prob, res); }

int slamit_init_reconstruct_batch(int device, int nprob, const slamit_init_reconstruct_problem* probs, slamit_init_reconstruct_result* results) {
    const char* const where = "slamit_init_reconstruct_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_refuse(where, "bad argument");
    if (nprob == 0) return SLAMIT_OK;
    for (int f = 0; f < nprob; ++f) {
        const slamit_init_reconstruct_problem& P = probs[f];
        if (const char* bad = init_check_frames(P.n1, P.keys1, P.n2, P.keys2, P.n, P.matches)) return slamit_refuse(where, bad);
        if (P.kind != SLAMIT_INIT_H && P.kind != SLAMIT_INIT_F) return slamit_refuse(where, "kind is neither SLAMIT_INIT_H nor SLAMIT_INIT_F");
        if (!P.subset_bits) return slamit_refuse(where, "null array");
    }
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: matches as coordinates, subset] go up; [per problem: R t nGood cosine (status points bits when asked for)] come down
    static thread_local SlamitScratch S;
    return slamit_staged_batch<InitMotionProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, InitMotionProb& Q) {
            const slamit_init_reconstruct_problem& P = probs[f];
            slamit_init_reconstruct_result& R = results[f];
            const size_t n = (size_t)P.n, words = (n + 31) / 32, nm = (size_t)tv_motion_count(P.kind);
            Q.n = P.n; Q.kind = P.kind; Q.words = (int32_t)words; Q.sigma = P.sigma;
            memcpy(Q.M, P.model, sizeof(Q.M)); memcpy(Q.K, P.K, sizeof(Q.K));
            float* m12 = nullptr;
            Q.m12 = slamit_global(b.in_fill<float>(4 * n, &m12));
            init_gather(P.keys1, P.keys2, P.matches, P.n, m12);
            Q.subset = slamit_global(b.in(P.subset_bits, words));
            Q.decomposable = slamit_global(b.out(&R.decomposable, 1));
            Q.R = slamit_global(b.out(R.R, 9 * nm)); Q.t = slamit_global(b.out(R.t, 3 * nm));
            Q.n_good = slamit_global(b.out(R.n_good, nm)); Q.cos_sel = slamit_global(b.out(R.cos_sel, nm));
            Q.status = slamit_global(R.status ? b.out(R.status, nm * n) : b.scratch<uint8_t>(nm * n));
            Q.points = slamit_global(R.points ? b.out(R.points, 3 * nm * n) : b.scratch<float>(3 * nm * n));
            Q.good_bits = slamit_global(R.good_bits ? b.out(R.good_bits, nm * words) : b.scratch<uint32_t>(nm * words));
            R.n_motions = (int32_t)nm;
        },
        [&](const InitMotionProb* d_recs) {
            hipLaunchKernelGGL(init_motion_kernel, dim3(8, (unsigned)nprob), dim3(INIT_MOTION_THREADS), 0, S.st, d_recs);
            return hipGetLastError();
        });
}

int slamit_init_reconstruct(int device, const slamit_init_reconstruct_problem* prob, slamit_init_reconstruct_result* res) {
    return slamit_init_reconstruct_batch(device, 1, prob, res);
}

int slamit_init_best_hypothesis(int n_hyp, const float* score) { return score && n_hyp > 0 ? tv_best_hypothesis(n_hyp, score) : -1; }
int slamit_init_choose_h(float SH, float SF) { return tv_choose_h(SH, SF); }
float slamit_init_parallax_deg(int n_good, float cos_sel) { return tv_parallax_deg(n_good, cos_sel); }
int slamit_init_pick_f(const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated) {
    return tv_pick_f(n_good, parallax, n_inliers, min_parallax, min_triangulated);
}
int slamit_init_pick_h(const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated) {
    return tv_pick_h(n_good, parallax, n_inliers, min_parallax, min_triangulated);
}

}  // extern "C"
