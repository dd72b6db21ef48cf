// lm_block.h — g2o's Levenberg over ONE dense D x D block, run by one 256-thread workgroup: the driver pose.hip (D = 6, SE3 state of
// 7 doubles) and sim3.hip (D = 7, similarity of 8) share.  The scalar rules are lm_step.h's; this file adds what is cooperative: the
// fixed-order reductions (lane-strided partials, DPP tree per wave, four waves in order), the LDS record, and the iteration /
// trial loop with its barriers.  What differs between the two problems comes in as a `model`, a small struct of force-inlined members:
//     double errors(const double* state)                       block-wide: writes the per-edge chi2, returns the robust cost
//     void   prepare(const double* state)                      block-wide, before the partials (Sim3: the perturbed similarities)
//     void   accumulate(const double* state, double* h, double* bb)   this thread's partials over its active edges: h = the
//                                                              D (D + 1) / 2 upper-triangle entries of H by rows, bb = b
//     void   oplus(double* state, const double* x)             thread 0 only, on a private copy of the state
// Everything around the loop (rounds, stages, relabelling, pruning) stays with the kernels.
#ifndef SLAMIT_LM_BLOCK_H
#define SLAMIT_LM_BLOCK_H
#include <hip/hip_runtime.h>

#include "lm_step.h"
#include "se3_device.h"

// LDS of one problem.  D: dimension of the increment, NS: doubles of the state.
template <int D, int NS>
struct LmBlock {
    double state[NS], bak[NS];
    double H[D * D], b[D], x[D];
    double red[4][D * (D + 1) / 2 + D];   // per-wave sums of h | bb
    double sum[4];                        // lm_block_sum's
    double lambda, ni, cur, rho;
    int ok2, cnt;
};

// sum over the 256 threads, the same value in every thread
__device__ __forceinline__ double lm_block_sum(double v, double* sh /*[4]*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// integer sum over the 256 threads through *cnt (LDS).  No barrier after the read: the caller places one before *cnt is used again.
__device__ __forceinline__ int lm_block_count(int mine, int* cnt) {
    if (threadIdx.x == 0) *cnt = 0;
    __syncthreads();
    if (mine) atomicAdd(cnt, mine);
    __syncthreads();
    return *cnt;
}

// Up to max_it iterations from S.state, which ends as the last accepted state.  Returns the iterations done; lastChi: the cost of
// the last evaluated trial, accepted or not (the per-edge chi2 the model wrote are that trial's too).
template <int D, int NS, class Model>
__device__ __forceinline__ int lm_block_run(LmBlock<D, NS>& S, const Model& model, int max_it, double& lastChi) {
    constexpr int NH = D * (D + 1) / 2;
    const int tid = threadIdx.x;
    int done = 0, nBad = 0;
    bool ok = true;
    for (int it = 0; it < max_it && ok; ++it) {
        // g2o re-evaluates the errors at the top of every iteration; after an accepted trial (the only way to get here with it > 0)
        // they are the ones that trial just computed at this very state: same bits, one pass saved
        const double currentChi0 = it == 0 ? model.errors(S.state) : S.cur;
        model.prepare(S.state);
        // ---- normal equations H (NH unique), b (D): per-thread partials, shuffle tree, 4 waves in order ----
        double h[NH], bb[D];
        for (int i = 0; i < NH; ++i) h[i] = 0;
        for (int i = 0; i < D; ++i) bb[i] = 0;
        model.accumulate(S.state, h, bb);
        for (int i = 0; i < NH; ++i) { const double v = wave_sum(h[i]); if ((tid & 63) == 0) S.red[tid >> 6][i] = v; }
        for (int i = 0; i < D; ++i) { const double v = wave_sum(bb[i]); if ((tid & 63) == 0) S.red[tid >> 6][NH + i] = v; }
        __syncthreads();
        if (tid == 0) {
            int k = 0;
            for (int a = 0; a < D; ++a)
                for (int c = a; c < D; ++c) { const double v = S.red[0][k] + S.red[1][k] + S.red[2][k] + S.red[3][k]; S.H[D * a + c] = v; S.H[D * c + a] = v; ++k; }
            for (int a = 0; a < D; ++a) S.b[a] = S.red[0][NH + a] + S.red[1][NH + a] + S.red[2][NH + a] + S.red[3][NH + a];
            if (it == 0) { S.lambda = lm_lambda_init<D>(S.H); S.ni = 2; }
            S.cur = currentChi0;
        }
        __syncthreads();
        const double iniChi = currentChi0;
        int qmax = 0;
        double rho = 0, tempChi = currentChi0;
        do {
            if (tid == 0) {
                for (int i = 0; i < NS; ++i) S.bak[i] = S.state[i];
                double x[D];
                const bool ok2 = lm_solve<D>(S.H, S.lambda, S.b, x);
                if (ok2) { double T[NS]; for (int i = 0; i < NS; ++i) T[i] = S.state[i]; model.oplus(T, x); for (int i = 0; i < NS; ++i) S.state[i] = T[i]; }
                else for (int i = 0; i < D; ++i) x[i] = 0;
                for (int i = 0; i < D; ++i) S.x[i] = x[i];
                S.ok2 = ok2;
            }
            __syncthreads();
            tempChi = model.errors(S.state);
            if (!S.ok2) tempChi = DBL_MAX;
            if (tid == 0) {
                double scale = 0;
                for (int k = 0; k < D; ++k) scale += S.x[k] * (S.lambda * S.x[k] + S.b[k]);
                bool accepted;
                const double r = lm_accept(S.cur, tempChi, scale, S.lambda, S.ni, accepted);
                if (!accepted) for (int i = 0; i < NS; ++i) S.state[i] = S.bak[i];
                S.rho = r;
            }
            __syncthreads();
            rho = S.rho;
            ++qmax;
        } while (lm_try_again(rho, qmax));
        ++done;
        lastChi = tempChi;
        ok = !lm_stop(qmax, rho, iniChi, S.cur, nBad);
    }
    return done;
}

#endif
