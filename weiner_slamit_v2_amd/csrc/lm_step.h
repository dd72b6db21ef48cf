// lm_step.h — the scalar rules of g2o's OptimizationAlgorithmLevenberg (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:
// 61-180), stated once: the damped solve of a single dense block, the lambda seed, the gain ratio with its accept / reject update of
// lambda, and the stop rules.  These pin the LM PATH (iteration counts, per-round chi2) to the reference's, so the single-block
// driver (lm_block.h: pose.hip, sim3.hip) and the local BA's k_decide (ba_kernels.hip) all call them.  Plain C++17, no HIP include:
// tests/test_lm_step.py builds it with g++.
#ifndef SLAMIT_LM_STEP_H
#define SLAMIT_LM_STEP_H
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define LM_FN __host__ __device__ __forceinline__
#else
#define LM_FN inline
#endif

#define LM_MAX_TRIALS 10   // _maxTrialsAfterFailure

// (H + lambda I) x = b for a symmetric D x D block (row-major, full): LDLt without pivoting; false on a zero or non-finite pivot
// (x is then unspecified).
template <int D>
LM_FN bool lm_solve(const double* H, double lambda, const double* b, double* x) {
    double A[D * D];
    for (int i = 0; i < D * D; ++i) A[i] = H[i] + (i % (D + 1) == 0 ? lambda : 0.0);
    for (int j = 0; j < D; ++j) {
        double d = A[(D + 1) * j];
        for (int k = 0; k < j; ++k) d -= A[D * j + k] * A[D * j + k] * A[(D + 1) * k];
        if (d == 0.0 || !(fabs(d) <= DBL_MAX)) return false;
        A[(D + 1) * j] = d;
        for (int i = j + 1; i < D; ++i) {
            double s = A[D * i + j];
            for (int k = 0; k < j; ++k) s -= A[D * i + k] * A[D * j + k] * A[(D + 1) * k];
            A[D * i + j] = s / d;
        }
    }
    for (int i = 0; i < D; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= A[D * i + k] * x[k]; x[i] = s; }
    for (int i = 0; i < D; ++i) x[i] /= A[(D + 1) * i];
    for (int i = D - 1; i >= 0; --i) { double s = x[i]; for (int k = i + 1; k < D; ++k) s -= A[D * k + i] * x[k]; x[i] = s; }
    return true;
}

// computeLambdaInit: tau (1e-5) times the largest |H_jj|; ni starts at 2 beside it
template <int D>
LM_FN double lm_lambda_init(const double* H) {
    double m = 0;
    for (int j = 0; j < D; ++j) m = fmax(m, fabs(H[(D + 1) * j]));
    return 1e-5 * m;
}

// One trial's verdict.  cur: the cost the iteration holds, temp: the cost at the tentative state (DBL_MAX when the solve failed),
// scale: sum of x (lambda x + b).  Returns the gain ratio rho; `accepted`: the step stands and cur takes temp, or it is undone (the
// caller restores its state).  lambda and ni are updated either way.
LM_FN double lm_accept(double& cur, double temp, double scale, double& lambda, double& ni, bool& accepted) {
    const double rho = (cur - temp) / (scale + 1e-3);
    accepted = rho > 0 && fabs(temp) <= DBL_MAX;
    if (accepted) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        lambda *= fmax(1. / 3., alpha);
        ni = 2;
        cur = temp;
    } else {
        lambda *= ni;
        ni *= 2;
    }
    return rho;
}

// another trial of the same iteration?  (qmax: trials made so far)
LM_FN bool lm_try_again(double rho, int qmax) { return rho < 0 && qmax < LM_MAX_TRIALS; }

// After an iteration's last trial: true when the optimisation stops.  g2o's own Terminate (the trials ran out, or the gain ratio is
// exactly 0), then ORB-SLAM2's g2o fork: the third iteration in a row that gained less than a thousandth of its initial cost
// (nBad counts the run, iniChi is the cost the iteration started from, cur the one it ends with).
LM_FN bool lm_stop(int qmax, double rho, double iniChi, double cur, int& nBad) {
    bool terminate = qmax == LM_MAX_TRIALS || rho == 0;
    if (!terminate) {
        if ((iniChi - cur) * 1e3 < iniChi) nBad += 1; else nBad = 0;
        if (nBad >= 3) terminate = true;
    }
    return terminate;
}

#endif
