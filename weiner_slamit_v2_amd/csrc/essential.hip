// essential.hip — Optimizer::OptimizeEssentialGraph on the GPU (include/slamit.h, slamit_essential_*).
//
// Reference: ORB_SLAM2/src/Optimizer.cc:781-1044 with g2o's VertexSim3Expmap / EdgeSim3 (types_seven_dof_expmap.h, sim3.h), the
// numeric Jacobians of core/base_binary_edge.hpp:131-200 and the Levenberg step of core/optimization_algorithm_levenberg.cpp, whose
// scalar rules are lm_step.h's.  Everything is double.  A Sim3 is 8 doubles: q (x, y, z, w as Eigen stores it, never normalised), t, s.
//
// Per LM trial the stream carries: eg_zero, eg_assemble (H + lambda I and b from the Jacobians, edge by edge in list order),
// per 32-column panel eg_diag / eg_rows / eg_update (dense LDLt without pivoting on the lower triangle, held as 32 x 32 tiles in
// HBM; the trailing update runs on v_mfma_f64_16x16x4_f64), eg_solve, eg_step, eg_errors, eg_decide.  The HOST reads eg_decide's
// verdict (8 bytes) after every trial and queues the next trial, the next iteration or the recovery.  The panel scheme is
// ba_kernels.hip's k_ldlt_tiled_*, restated here over packed tiles; sharing it is a follow-up.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "essential_plan.h"
#include "lm_step.h"
#include "se3_device.h"
#include "slamit_internal.h"

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef SLAMIT_GLOBAL double gdouble;

#define EG_NB 32                      // panel width = tile edge
#define EG_TILE (EG_NB * EG_NB)
#define EG_P (EG_NB + 1)              // LDS pitch of a tile
#define EG_MT 64                      // macro tile of the trailing update
#define EG_PITCH 34                   // LDS pitch of the update's operands (ba_kernels.hip: conflict-free reads)

struct EgState {
    double lambda, ni, cur, ini, scale, last;
    int32_t nbad, qmax, it, fail;
    int32_t verdict[2];               // again, stop: what the host reads after a trial
    int32_t n_free_dev, bad_tables;   // read together by the host before anything else runs
};

// everything the kernels see: counts and device pointers
struct EgDev {
    int32_t n_kf, n_edge, n_pt, n_free, fix_scale, n, T;   // n = 7 n_free unknowns, T = tiles per side
    const double *scw_r, *scw_t, *scw_s, *snc_r, *snc_t, *snc_s;
    const uint8_t *fixed, *bad, *pt_bad;
    const int32_t *v0, *v1, *kind, *inc_ptr, *inc_edge, *pt_ref;
    const float* pt_pos;
    double *o_r, *o_t, *o_s, *o_pose;
    float* o_pt;
    int32_t *touched, *n_touched;
    slamit_eg_stats* stats;
    // workspace
    EgState* st;
    double *scw_q, *snc_q, *est, *bak, *meas, *err, *chi, *J, *b, *x, *dvec, *H;
    int32_t *blk, *free_list;
};

// ---- Sim3 (sim3.h) ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void eg_quat_mul(const double* a, const double* b, double* r) {   // Eigen's product, (x, y, z, w)
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void eg_mul(const double* a, const double* b, double* r) {   // operator*: r, s (r other.t) + t, s other.s
    double rt[3];
    eg_quat_mul(a, b, r);
    quat_rot(a, b + 4, rt);
#pragma unroll
    for (int i = 0; i < 3; ++i) r[4 + i] = a[7] * rt[i] + a[4 + i];
    r[7] = a[7] * b[7];
}
__device__ __forceinline__ void eg_inverse(const double* S, double* I) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    I[0] = -S[0]; I[1] = -S[1]; I[2] = -S[2]; I[3] = S[3];
    const double k = -1. / S[7];
    const double kt[3] = {k * S[4], k * S[5], k * S[6]};
    quat_rot(I, kt, I + 4);
    I[7] = 1. / S[7];
}
__device__ __forceinline__ void eg_map(const double* S, const double* x, double* y) {   // s (r xyz) + t
    double r[3];
    quat_rot(S, x, r);
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = S[7] * r[i] + S[4 + i];
}
__device__ __forceinline__ void eg_from_rts(const double* r, const double* t, double s, double* S) {   // Sim3(R, t, s): Quaterniond(R)
    R_to_quat(r, S);
    S[4] = t[0]; S[5] = t[1]; S[6] = t[2]; S[7] = s;
}

// A, B, C of exp and log: the four branches of sim3.h:92-135 / :169-213
__device__ __forceinline__ void eg_abc(double sigma, double s, double theta, bool small_theta, double& A, double& B, double& C) {
    const double eps = 0.00001;
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
}
__device__ __forceinline__ void eg_skew2(const double* w, double* O, double* O2) {
    O[0] = 0; O[1] = -w[2]; O[2] = w[1]; O[3] = w[2]; O[4] = 0; O[5] = -w[0]; O[6] = -w[1]; O[7] = w[0]; O[8] = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
}

// Sim3(const Vector7d& update), sim3.h:70-142
static __device__ void eg_exp(const double* u, double* S) {
    const double sigma = u[6];
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double O[9], O2[9];
    eg_skew2(u, O, O2);
    const double es = exp(sigma);
    const bool small = theta < 0.00001;
    double A, B, C;
    eg_abc(sigma, es, theta, small, A, B, C);
    const double ca = small ? 1.0 : sin(theta) / theta, cb = small ? 1.0 : (1 - cos(theta)) / (theta * theta);
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ca * O[i] + cb * O2[i];
    R_to_quat(R, S);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * u[3 + j];
        S[4 + i] = acc;
    }
    S[7] = es;
}

// W x = t by LU with partial pivoting, as Matrix3d::lu().solve(): rows in named registers, swaps by value (no indexed array)
__device__ __forceinline__ void eg_swap4(double* a, double* b, bool doit) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double x = a[i], y = b[i]; a[i] = doit ? y : x; b[i] = doit ? x : y; }
}
__device__ __forceinline__ void eg_lu_solve3(const double* W, const double* t, double* x) {
    double r0[4] = {W[0], W[1], W[2], t[0]}, r1[4] = {W[3], W[4], W[5], t[1]}, r2[4] = {W[6], W[7], W[8], t[2]};
    eg_swap4(r0, r1, fabs(r1[0]) > fabs(r0[0]));   // the first largest of the column
    eg_swap4(r0, r2, fabs(r2[0]) > fabs(r0[0]));
    // (after the two conditional swaps r0 holds the largest; a tie keeps the earlier row, as maxCoeff does for row 0)
    const double l1 = r1[0] / r0[0], l2 = r2[0] / r0[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) { r1[i] -= l1 * r0[i]; r2[i] -= l2 * r0[i]; }
    eg_swap4(r1, r2, fabs(r2[1]) > fabs(r1[1]));
    const double l3 = r2[1] / r1[1];
    r2[2] -= l3 * r1[2]; r2[3] -= l3 * r1[3];
    x[2] = r2[3] / r2[2];
    x[1] = (r1[3] - r1[2] * x[2]) / r1[1];
    x[0] = (r0[3] - r0[1] * x[1] - r0[2] * x[2]) / r0[0];
}

// Sim3::log(), sim3.h:148-230
static __device__ void eg_log(const double* S, double* res) {
    const double s = S[7], sigma = log(s);
    double R[9];
    quat_to_R(S, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const bool small = d > 1 - 0.00001;
    double theta = 0, k = 0.5;
    if (!small) { theta = acos(d); k = theta / (2 * sqrt(1 - d * d)); }
    const double omega[3] = {k * dR[0], k * dR[1], k * dR[2]};
    double A, B, C;
    eg_abc(sigma, s, theta, small, A, B, C);
    double O[9], O2[9], W[9];
    eg_skew2(omega, O, O2);
#pragma unroll
    for (int i = 0; i < 9; ++i) W[i] = A * O[i] + B * O2[i] + (i % 4 == 0 ? C : 0.0);
    eg_lu_solve3(W, S + 4, res + 3);
    res[0] = omega[0]; res[1] = omega[1]; res[2] = omega[2];
    res[6] = sigma;
}

// EdgeSim3::computeError: log(C * v1->estimate() * v2->estimate().inverse())
static __device__ void eg_edge_error(const double* C, const double* Si, const double* Sj, double* e) {
    double a[8], inv[8], b[8];
    eg_mul(C, Si, a);
    eg_inverse(Sj, inv);
    eg_mul(a, inv, b);
    eg_log(b, e);
}
__device__ __forceinline__ void eg_load8(const double* p, double* S) {
#pragma unroll
    for (int i = 0; i < 8; ++i) S[i] = p[i];
}
__device__ __forceinline__ double eg_chi2(const double* e) {
    double c = 0;
#pragma unroll
    for (int m = 0; m < 7; ++m) c += e[m] * e[m];
    return c;
}

// index of element (r, c), c's tile <= r's tile, in the packed lower triangle of 32 x 32 tiles
__device__ __forceinline__ size_t eg_at(int r, int c) {
    const size_t tr = (size_t)(r >> 5), tc = (size_t)(c >> 5);
    return (tr * (tr + 1) / 2 + tc) * EG_TILE + (size_t)(r & 31) * EG_NB + (c & 31);
}

// fixed-order sum of v over the 256 threads of a workgroup (sh: 256 doubles); every thread gets it
__device__ __forceinline__ double eg_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

// ---- set-up --------------------------------------------------------------------------------------------------------------------------
// the LM record, cleared once the call has passed its checks (a refused call writes nothing of the result)
__global__ void eg_stats_init(EgDev D) {
    slamit_eg_stats& t = *D.stats;
    t.n_its = 0; t.n_trials = 0; t.n_free = D.st->n_free_dev; t.status = 0; t.chi2_init = 0;
    for (int k = 0; k < SLAMIT_EG_MAX_ITS; ++k) { t.chi2[k] = 0; t.lambda[k] = 0; t.trials[k] = 0; }
    for (int k = 0; k < SLAMIT_EG_MAX_TRIALS; ++k) { t.trial_chi2[k] = 0; t.trial_rho[k] = 0; }
}

__global__ __launch_bounds__(256) void eg_init(EgDev D, double lambda_init) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        EgState& s = *D.st;
        s.lambda = lambda_init; s.ni = 2; s.cur = 0; s.ini = 0; s.scale = 0; s.last = 0;
        s.nbad = 0; s.qmax = 0; s.it = 0; s.fail = 0; s.verdict[0] = 0; s.verdict[1] = 1; s.n_free_dev = 0; s.bad_tables = 0;
    }
    if (i >= D.n_kf) return;
    double S[8];
    eg_from_rts(D.scw_r + 9 * (size_t)i, D.scw_t + 3 * (size_t)i, D.scw_s[i], S);
#pragma unroll
    for (int k = 0; k < 8; ++k) { D.scw_q[8 * (size_t)i + k] = S[k]; D.est[8 * (size_t)i + k] = S[k]; }
    eg_from_rts(D.snc_r + 9 * (size_t)i, D.snc_t + 3 * (size_t)i, D.snc_s[i], S);
#pragma unroll
    for (int k = 0; k < 8; ++k) D.snc_q[8 * (size_t)i + k] = S[k];
}

// One workgroup: rank[i] = number of set flags before i (or -1 where the flag is clear), list = the set indices ascending, *count.
// mode 0: keyframes that are neither fixed nor bad (blk, free_list; the count must be D.n_free); mode 1: good points (touched).
__global__ __launch_bounds__(1024) void eg_compact(EgDev D, int mode) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = mode == 0 ? D.n_kf : D.n_pt;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const bool f = i < n && (mode == 0 ? (!D.fixed[i] && !D.bad[i]) : !D.pt_bad[i]);
        const unsigned long long m = __ballot(f);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wv; ++w) off += s_wave[w];
        const int rank = off + before;
        if (mode == 0) {
            if (i < n) D.blk[i] = f && rank < D.n_free ? rank : -1;
            if (f && rank < D.n_free) D.free_list[rank] = i;
        } else if (f) {
            D.touched[rank] = i;
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += s_wave[w]; s_base += t; }
        __syncthreads();
    }
    if (tid == 0) {
        if (mode == 0) D.st->n_free_dev = s_base;
        else *D.n_touched = s_base;
    }
}

// The device form's tables, which the host cannot look at: an edge outside [0, n_kf), on a bad keyframe, from a keyframe to itself or of an
// unknown kind, a good point whose reference keyframe is outside the table or bad, or an incidence pointer outside [0, 2 n_edge] or
// descending, sets bad_tables; the host then refuses the call before any
// kernel that indexes by them runs.  (grid over max(n_edge, n_kf + 1, n_pt); launched after eg_init on the same stream.)
__global__ __launch_bounds__(256) void eg_check_tables(EgDev D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < D.n_edge) {
        const int a = D.v0[i], b = D.v1[i], k = D.kind[i];
        bad = a < 0 || a >= D.n_kf || b < 0 || b >= D.n_kf || a == b || (k != SLAMIT_EG_NORMAL && k != SLAMIT_EG_LOOP_CONNECTION);
        if (!bad) bad = D.bad[a] || D.bad[b];
    }
    if (i < D.n_pt && !D.pt_bad[i]) {   // as the host form: a good point's reference keyframe is in the table and not bad
        const int r = D.pt_ref[i];
        bad = bad || r < 0 || r >= D.n_kf;
        if (!bad) bad = D.bad[r];
    }
    if (i <= D.n_kf) {
        const int p = D.inc_ptr[i];
        bad = bad || p < 0 || p > 2 * D.n_edge || (i == 0 && p != 0) || (i > 0 && p < D.inc_ptr[i - 1]);
    }
    if (bad) D.st->bad_tables = 1;
}

// :857-867 / :889-914 — Sji = Sjw * Swi from the corrected Sim3s (a LoopConnections edge) or the non-corrected ones
__global__ __launch_bounds__(256) void eg_measure(EgDev D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D.n_edge) return;
    const double* src = D.kind[e] == SLAMIT_EG_LOOP_CONNECTION ? D.scw_q : D.snc_q;
    double Siw[8], Sjw[8], Swi[8], Sji[8];
    eg_load8(src + 8 * (size_t)D.v0[e], Siw);
    eg_load8(src + 8 * (size_t)D.v1[e], Sjw);
    eg_inverse(Siw, Swi);
    eg_mul(Sjw, Swi, Sji);
#pragma unroll
    for (int k = 0; k < 8; ++k) D.meas[8 * (size_t)e + k] = Sji[k];
}

// ---- linearise: 32 lanes per edge, ONE evaluation of the error per lane --------------------------------------------------------------
// lane l < 28: vertex l / 14, coordinate (l % 14) / 2, +delta on even lanes and -delta on odd ones; lane 28: the unperturbed error
// and the edge's chi2.  Column d of a Jacobian is (1 / 2 delta) (e+ - e-): the odd lane's error reaches the even lane by a lane
// exchange, so no lane holds more than its own 7-vector.  A fixed vertex is not perturbed and its Jacobian is not written
// (base_binary_edge.hpp:152,176); eg_assemble never reads it.
__global__ __launch_bounds__(256) void eg_linearize(EgDev D) {
    const int g = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const int e = g < D.n_edge ? g : D.n_edge - 1;   // whole waves stay in the exchange; the surplus group repeats the last edge and writes nothing
    const int i0 = D.v0[e], i1 = D.v1[e];
    double C[8], Si[8], Sj[8], err[7];
    eg_load8(D.meas + 8 * (size_t)e, C);
    eg_load8(D.est + 8 * (size_t)i0, Si);
    eg_load8(D.est + 8 * (size_t)i1, Sj);
    const int side = l >= 14 ? 1 : 0, d = (l - 14 * side) >> 1;
    const bool is_free = D.blk[side ? i1 : i0] >= 0;
    if (l < 28 && is_free) {
        const double delta = (l & 1) ? -1e-9 : 1e-9;
        double u[7], X[8], N[8];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = k == d ? delta : 0.0;
        if (D.fix_scale) u[6] = 0;
        eg_exp(u, X);
        if (side) { eg_mul(X, Sj, N); eg_load8(N, Sj); }
        else { eg_mul(X, Si, N); eg_load8(N, Si); }
    }
    eg_edge_error(C, Si, Sj, err);
    const double scalar = 1.0 / (2 * 1e-9);
    const bool writer = g < D.n_edge && l < 28 && !(l & 1) && is_free;
    double* Jd = D.J + 98 * (size_t)e + 49 * side + d;
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        const double other = __shfl_xor(err[m], 1);
        if (writer) Jd[7 * m] = scalar * (err[m] - other);
    }
    if (g < D.n_edge && l == 28) {
#pragma unroll
        for (int m = 0; m < 7; ++m) D.err[7 * (size_t)e + m] = err[m];
        D.chi[e] = eg_chi2(err);
    }
}

// the errors at the tentative state: chi2 per edge (err keeps the linearisation point's: b is not rebuilt between trials)
__global__ __launch_bounds__(256) void eg_errors(EgDev D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D.n_edge) return;
    double C[8], Si[8], Sj[8], err[7];
    eg_load8(D.meas + 8 * (size_t)e, C);
    eg_load8(D.est + 8 * (size_t)D.v0[e], Si);
    eg_load8(D.est + 8 * (size_t)D.v1[e], Sj);
    eg_edge_error(C, Si, Sj, err);
    D.chi[e] = eg_chi2(err);
}

// start of an iteration: currentChi = iniChi = the cost at the linearisation point, no trial made yet
__global__ __launch_bounds__(256) void eg_iter_begin(EgDev D) {
    __shared__ double sh[256];
    double acc = 0;
    for (int e = threadIdx.x; e < D.n_edge; e += 256) acc += D.chi[e];
    const double c = eg_block_sum(acc, sh);
    if (threadIdx.x == 0) {
        D.st->cur = c; D.st->ini = c; D.st->qmax = 0;
        if (D.st->it == 0) D.stats->chi2_init = c;
    }
}

// ---- the system ------------------------------------------------------------------------------------------------------------------------
// grid (T, T): tile (blockIdx.y, blockIdx.x) of the lower triangle <- 0, the unit diagonal past n (the padding solves to x = 0)
__global__ __launch_bounds__(256) void eg_zero(EgDev D) {
    const int tr = blockIdx.y, tc = blockIdx.x;
    if (tc > tr) return;
    gdouble* H = (gdouble*)D.H + ((size_t)tr * (tr + 1) / 2 + tc) * EG_TILE;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u, r = i >> 5, c = i & 31;
        H[i] = (tr == tc && r == c && EG_NB * tr + r >= D.n) ? 1.0 : 0.0;
    }
    if (tr == tc && threadIdx.x < EG_NB && EG_NB * tr + (int)threadIdx.x >= D.n) { D.b[EG_NB * tr + threadIdx.x] = 0; D.x[EG_NB * tr + threadIdx.x] = 0; }
    if (tr == 0 && threadIdx.x == 0) D.st->fail = 0;
}

// One workgroup per free keyframe a, thread (r, c) of its 7 x 7 blocks: the keyframe's edges in list order (constructQuadraticForm,
// base_binary_edge.hpp:55-120 with omega = I): the diagonal block and b in registers, the block towards every free neighbour of a
// LOWER block index read-modify-written in place (this thread alone owns that element, so parallel edges add up in list order).
__global__ __launch_bounds__(64) void eg_assemble(EgDev D) {
    const int a = blockIdx.x, tid = threadIdx.x;
    if (tid >= 49) return;
    const int r = tid / 7, c = tid - 7 * r;
    const int slot = D.free_list[a];
    gdouble* H = (gdouble*)D.H;
    const gdouble* J = (const gdouble*)D.J;
    const gdouble* E = (const gdouble*)D.err;
    double diag = 0, bacc = 0;
    for (int k = D.inc_ptr[slot]; k < D.inc_ptr[slot + 1]; ++k) {   // (eg_check_tables: inside [0, 2 n_edge])
        const int ent = D.inc_edge[k], e = ent >> 1, side = ent & 1;
        if (ent < 0 || e >= D.n_edge) continue;   // (an entry of a device-form table is not checked before: skipped, never dereferenced)
        const int other = side ? D.v0[e] : D.v1[e];
        const gdouble* Ja = J + 98 * (size_t)e + 49 * side;
        double s = 0;
#pragma unroll
        for (int m = 0; m < 7; ++m) s += Ja[7 * m + r] * Ja[7 * m + c];
        diag += s;
        if (c == 0) {
            double t = 0;
#pragma unroll
            for (int m = 0; m < 7; ++m) t += Ja[7 * m + r] * -E[7 * (size_t)e + m];
            bacc += t;
        }
        const int ob = D.blk[other];
        if (ob >= 0 && ob < a) {
            const gdouble* Jo = J + 98 * (size_t)e + 49 * (1 - side);
            double o = 0;
#pragma unroll
            for (int m = 0; m < 7; ++m) o += Ja[7 * m + r] * Jo[7 * m + c];
            H[eg_at(7 * a + r, 7 * ob + c)] += o;
        }
    }
    if (c <= r) H[eg_at(7 * a + r, 7 * a + c)] = r == c ? diag + D.st->lambda : diag;
    if (c == 0) D.b[7 * a + r] = bacc;
}

// Panel step 1: the 32 x 32 diagonal tile in LDS, thread (r, c) owns element (r, c): a[r][c] -= a[r][j] a[c][j] / d_j for every j < c,
// one barrier per column; then unit L below the diagonal, D into dvec.  A pivot that is zero or not finite fails the trial.
__global__ __launch_bounds__(1024) void eg_diag(EgDev D, int panel) {
    if (D.st->fail) return;
    __shared__ double A[EG_NB * EG_P];
    const int tid = threadIdx.x, r = tid >> 5, c = tid & 31;
    gdouble* Hd = (gdouble*)D.H + ((size_t)panel * (panel + 1) / 2 + panel) * EG_TILE;
    A[r * EG_P + c] = c <= r ? Hd[r * EG_NB + c] : 0.0;
    for (int j = 0; j < EG_NB; ++j) {
        __syncthreads();
        const double d = A[j * EG_P + j];
        if (d == 0.0 || !(fabs(d) <= DBL_MAX)) {   // the same d in every thread
            if (tid == 0) D.st->fail = 1;
            return;
        }
        if (c > j && r >= c) A[r * EG_P + c] -= A[r * EG_P + j] * A[c * EG_P + j] / d;
    }
    __syncthreads();
    if (c < r) Hd[r * EG_NB + c] = A[r * EG_P + c] / A[c * EG_P + c];
    else Hd[r * EG_NB + c] = r == c ? 1.0 : 0.0;
    if (r == c) D.dvec[EG_NB * panel + r] = A[r * EG_P + r];
}

// Panel step 2: every row below the panel, one lane each: w = a L11^-T (right-looking, the row in registers), then L21 = w / d
__global__ __launch_bounds__(256) void eg_rows(EgDev D, int panel) {
    if (D.st->fail) return;
    __shared__ double L[EG_NB * EG_P];
    __shared__ double sd[EG_NB];
    const int tid = threadIdx.x;
    const gdouble* Hd = (const gdouble*)D.H + ((size_t)panel * (panel + 1) / 2 + panel) * EG_TILE;
    for (int i = tid; i < EG_TILE; i += 256) L[(i >> 5) * EG_P + (i & 31)] = Hd[i];
    if (tid < EG_NB) sd[tid] = D.dvec[EG_NB * panel + tid];
    __syncthreads();
    const int v = blockIdx.x * 256 + tid, ti = panel + 1 + (v >> 5);
    if (ti >= D.T) return;
    gdouble* row = (gdouble*)D.H + ((size_t)ti * (ti + 1) / 2 + panel) * EG_TILE + (size_t)(v & 31) * EG_NB;
    double w[EG_NB];
#pragma unroll
    for (int k = 0; k < EG_NB; ++k) w[k] = row[k];
#pragma unroll
    for (int k = 0; k < EG_NB - 1; ++k) {
#pragma unroll
        for (int m = k + 1; m < EG_NB; ++m) w[m] -= w[k] * L[m * EG_P + k];
    }
#pragma unroll
    for (int k = 0; k < EG_NB; ++k) row[k] = w[k] / sd[k];
}

// Panel step 3: A22 -= L21 D L21^T on one lower 64 x 64 macro tile of the trailing matrix (grid (RT, RT), the upper ones return):
// v_mfma_f64_16x16x4_f64, wave w owns rows 16 w .. 16 w + 15 and four 16-column tiles; -L21 (A operand) and L21 D (B operand) in LDS.
__global__ __launch_bounds__(256) void eg_update(EgDev D, int panel) {
    if (D.st->fail) return;
    const int rt = blockIdx.y, ct = blockIdx.x;
    if (ct > rt) return;
    const int base = EG_NB * (panel + 1), rows = EG_NB * D.T - base, jb = EG_NB * panel;
    __shared__ __attribute__((aligned(16))) double As[EG_MT * EG_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[EG_MT * EG_PITCH];
    __shared__ double s_d[EG_NB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    gdouble* H = (gdouble*)D.H;
    if (tid < EG_NB) s_d[tid] = D.dvec[jb + tid];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (EG_MT * EG_NB) / 256; ++u) {
        const int i = tid + 256 * u, r = i >> 5, c = i & 31;
        const int va = EG_MT * rt + r, vb = EG_MT * ct + r;
        As[r * EG_PITCH + c] = va < rows ? -H[eg_at(base + va, jb + c)] : 0.0;
        Bs[r * EG_PITCH + c] = vb < rows ? H[eg_at(base + vb, jb + c)] * s_d[c] : 0.0;
    }
    // C/D layout of v_mfma_f64_16x16x4: col = lane & 15, row = (lane >> 4) + 4 * reg
    double4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int vr = EG_MT * rt + 16 * wv + (lane >> 4) + 4 * g, vc = EG_MT * ct + 16 * j + (lane & 15);
            acc[j][g] = (vr < rows && vc <= vr) ? H[eg_at(base + vr, base + vc)] : 0.0;
        }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < EG_NB; ks += 4) {
        const double a = As[(16 * wv + (lane & 15)) * EG_PITCH + ks + (lane >> 4)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double b = Bs[(16 * j + (lane & 15)) * EG_PITCH + ks + (lane >> 4)];
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int vr = EG_MT * rt + 16 * wv + (lane >> 4) + 4 * g, vc = EG_MT * ct + 16 * j + (lane & 15);
            if (vr < rows && vc <= vr) H[eg_at(base + vr, base + vc)] = acc[j][g];
        }
}

// x = L^-T D^-1 L^-1 b in one workgroup of 32 x 32 threads (g, c), x in LDS (dynamic: 32 T doubles).  Forward, block row kb: thread
// (g, c) sums L(kb, jb)[g][c] y[32 jb + c] over the tiles left of the diagonal (rows of L: coalesced), thread g < 32 adds the 32
// partial sums of its row in a fixed order, wavefront 0 solves the unit triangle (lane r owns y_r, v_readlane broadcasts).
// Backward, block kb: thread (g, c) sums L(ib, kb)[g][c] x[32 ib + g] over the tiles below, and the triangle is solved from the bottom.
__global__ __launch_bounds__(1024) void eg_solve(EgDev D) {
    if (D.st->fail) return;
    extern __shared__ __attribute__((aligned(16))) double xs[];
    __shared__ double part[EG_NB * EG_P];
    const int tid = threadIdx.x, g = tid >> 5, c = tid & 31, T = D.T;
    const gdouble* H = (const gdouble*)D.H;
    for (int i = tid; i < EG_NB * T; i += 1024) xs[i] = D.b[i];
    __syncthreads();
    for (int kb = 0; kb < T; ++kb) {
        const gdouble* rowt = H + ((size_t)kb * (kb + 1) / 2) * EG_TILE;
        double p = 0;
        for (int jb = 0; jb < kb; ++jb) p += rowt[(size_t)jb * EG_TILE + g * EG_NB + c] * xs[EG_NB * jb + c];
        part[g * EG_P + c] = p;
        __syncthreads();
        if (tid < 64) {
            const int r = tid;
            double v = 0;
            if (r < EG_NB) {
                double s = 0;
                for (int k = 0; k < EG_NB; ++k) s += part[r * EG_P + k];
                v = xs[EG_NB * kb + r] - s;
            }
            const gdouble* Ld = rowt + (size_t)kb * EG_TILE + (size_t)(r & 31) * EG_NB;   // row r of the unit triangle
#pragma unroll
            for (int j = 0; j < EG_NB - 1; ++j) {
                const double xj = readlane_d(v, j);   // final once every lower index has been applied
                const double lrj = Ld[j];
                if (r < EG_NB && r > j) v -= lrj * xj;
            }
            if (r < EG_NB) xs[EG_NB * kb + r] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < EG_NB * T; i += 1024) xs[i] = xs[i] / D.dvec[i];
    __syncthreads();
    for (int kb = T - 1; kb >= 0; --kb) {
        double p = 0;
        for (int ib = kb + 1; ib < T; ++ib) p += H[((size_t)ib * (ib + 1) / 2 + kb) * EG_TILE + g * EG_NB + c] * xs[EG_NB * ib + g];
        part[g * EG_P + c] = p;
        __syncthreads();
        if (tid < 64) {
            const int k = tid;
            double v = 0;
            if (k < EG_NB) {
                double s = 0;
                for (int q = 0; q < EG_NB; ++q) s += part[q * EG_P + k];
                v = xs[EG_NB * kb + k] - s;
            }
            const gdouble* Ld = H + ((size_t)kb * (kb + 1) / 2 + kb) * EG_TILE + (k & 31);   // column k of the unit triangle
#pragma unroll
            for (int m = EG_NB - 1; m > 0; --m) {
                const double xm = readlane_d(v, m);   // final once every higher index has been applied
                const double lmk = Ld[m * EG_NB];
                if (k < m) v -= lmk * xm;
            }
            if (k < EG_NB) xs[EG_NB * kb + k] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < EG_NB * T; i += 1024) D.x[i] = xs[i];
}

// push() and oplus on every free vertex (the update's coordinate 6 zeroed in place under fix_scale, as oplusImpl does)
__global__ __launch_bounds__(256) void eg_step(EgDev D) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= D.n_free || D.st->fail) return;
    const int slot = D.free_list[a];
    double S[8], X[8], N[8], u[7];
    eg_load8(D.est + 8 * (size_t)slot, S);
#pragma unroll
    for (int k = 0; k < 8; ++k) D.bak[8 * (size_t)slot + k] = S[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = D.x[7 * (size_t)a + k];
    if (D.fix_scale) { u[6] = 0; D.x[7 * (size_t)a + 6] = 0; }
    eg_exp(u, X);
    eg_mul(X, S, N);
#pragma unroll
    for (int k = 0; k < 8; ++k) D.est[8 * (size_t)slot + k] = N[k];
}

// The trial's verdict (optimization_algorithm_levenberg.cpp:123-163 through lm_step.h): chi2 and the gain ratio's scale as fixed-order
// sums, lambda and ni updated, the state restored on a reject, the iteration's record when no further trial follows.
__global__ __launch_bounds__(256) void eg_decide(EgDev D) {
    __shared__ double sh[256];
    __shared__ int s_restore;
    const int tid = threadIdx.x;
    EgState& s = *D.st;
    const bool failed = s.fail != 0;
    const double lambda = s.lambda;
    double acc = 0;
    for (int e = tid; e < D.n_edge; e += 256) acc += D.chi[e];
    const double chi = eg_block_sum(acc, sh);
    acc = 0;
    if (!failed)
        for (int j = tid; j < D.n; j += 256) { const double x = D.x[j]; acc += x * (lambda * x + D.b[j]); }
    const double scale = eg_block_sum(acc, sh);
    if (tid == 0) {
        const double temp = failed ? DBL_MAX : chi;
        double cur = s.cur, lam = lambda, ni = s.ni;
        bool accepted;
        const double rho = lm_accept(cur, temp, scale, lam, ni, accepted);
        s.cur = cur; s.lambda = lam; s.ni = ni; s.last = temp;
        const int q = ++s.qmax;
        slamit_eg_stats& t = *D.stats;
        if (t.n_trials < SLAMIT_EG_MAX_TRIALS) { t.trial_chi2[t.n_trials] = temp; t.trial_rho[t.n_trials] = rho; }
        ++t.n_trials;
        const bool again = lm_try_again(rho, q);
        int stop = 0;
        if (!again) {
            const int it = s.it;
            if (it < SLAMIT_EG_MAX_ITS) { t.chi2[it] = temp; t.lambda[it] = lam; t.trials[it] = q; }
            int nbad = s.nbad;
            stop = lm_stop(q, rho, s.ini, cur, nbad) ? 1 : 0;
            s.nbad = nbad;
            s.it = it + 1;
            t.n_its = it + 1;
        }
        s.verdict[0] = again ? 1 : 0; s.verdict[1] = stop;
        s_restore = !accepted && !failed;
    }
    __syncthreads();
    if (s_restore)
        for (int i = tid; i < 8 * D.n_free; i += 256) {
            const size_t at = 8 * (size_t)D.free_list[i >> 3] + (i & 7);
            D.est[at] = D.bak[at];
        }
}

// ---- recovery, :991-1043 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eg_recover(EgDev D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D.n_kf) return;
    double S[8], R[9];
    eg_load8(D.est + 8 * (size_t)i, S);
    quat_to_R(S, R);
    const double inv = 1. / S[7];
#pragma unroll
    for (int k = 0; k < 9; ++k) { D.o_r[9 * (size_t)i + k] = R[k]; D.o_pose[12 * (size_t)i + k] = R[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { D.o_t[3 * (size_t)i + k] = S[4 + k]; D.o_pose[12 * (size_t)i + 9 + k] = S[4 + k] * inv; }
    D.o_s[i] = S[7];
}

// one lane per point: correctedSwr.map(Srw.map(Xw)) in double from the widened float position, narrowed to float; a bad point, or one
// whose reference is outside the table (device form), keeps its position
__global__ __launch_bounds__(256) void eg_points(EgDev D) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= D.n_pt) return;
    const float X[3] = {D.pt_pos[3 * (size_t)p], D.pt_pos[3 * (size_t)p + 1], D.pt_pos[3 * (size_t)p + 2]};
    float Y[3] = {X[0], X[1], X[2]};
    const int r = D.pt_ref[p];
    if (!D.pt_bad[p] && r >= 0 && r < D.n_kf) {
        double Srw[8], Siw[8], Swr[8], a[3], b[3];
        const double x[3] = {(double)X[0], (double)X[1], (double)X[2]};
        eg_load8(D.scw_q + 8 * (size_t)r, Srw);
        // the corrected Sim3 as the RESULT holds it (r, t, s), so that the map can be restated from the result alone
        eg_from_rts(D.o_r + 9 * (size_t)r, D.o_t + 3 * (size_t)r, D.o_s[r], Siw);
        eg_inverse(Siw, Swr);
        eg_map(Srw, x, a);
        eg_map(Swr, a, b);
        Y[0] = (float)b[0]; Y[1] = (float)b[1]; Y[2] = (float)b[2];
    }
    D.o_pt[3 * (size_t)p] = Y[0]; D.o_pt[3 * (size_t)p + 1] = Y[1]; D.o_pt[3 * (size_t)p + 2] = Y[2];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the workspace, every array on a 256-byte boundary; `base` null measures
struct EgWorkspace {
    size_t bytes = 0;
    template <typename T>
    T* take(unsigned char* base, size_t count) {
        const size_t off = bytes;
        bytes += rup(sizeof(T) * (count ? count : 1), 256);
        return base ? reinterpret_cast<T*>(base + off) : nullptr;
    }
};
static size_t eg_carve(EgDev& D, unsigned char* base) {
    EgWorkspace W;
    const size_t K = (size_t)D.n_kf, E = (size_t)D.n_edge, T = (size_t)D.T;
    D.st = W.take<EgState>(base, 1);
    D.scw_q = W.take<double>(base, 8 * K); D.snc_q = W.take<double>(base, 8 * K);
    D.est = W.take<double>(base, 8 * K); D.bak = W.take<double>(base, 8 * K);
    D.blk = W.take<int32_t>(base, K); D.free_list = W.take<int32_t>(base, (size_t)D.n_free);
    D.meas = W.take<double>(base, 8 * E); D.err = W.take<double>(base, 7 * E); D.chi = W.take<double>(base, E);
    D.J = W.take<double>(base, 98 * E);
    D.b = W.take<double>(base, EG_NB * T); D.x = W.take<double>(base, EG_NB * T); D.dvec = W.take<double>(base, EG_NB * T);
    D.H = W.take<double>(base, T * (T + 1) / 2 * EG_TILE);
    return W.bytes;
}
static void eg_dims(EgDev& D) {
    D.n = 7 * D.n_free;
    D.T = (D.n + EG_NB - 1) / EG_NB;
}

static int eg_check_counts(const char* where, int n_free, int n_kf, int n_edge, int n_pt, int max_its) {
    if (n_kf < 0 || n_edge < 0 || n_pt < 0 || n_free < 0 || n_free > n_kf || max_its < 0) return slamit_refuse(where, "negative count");
    if (n_free > SLAMIT_EG_MAX_KF) return slamit_refuse(where, "more than SLAMIT_EG_MAX_KF free keyframes", SLAMIT_ERR_CAPACITY);
    if (n_edge > SLAMIT_EG_MAX_EDGES) return slamit_refuse(where, "more than SLAMIT_EG_MAX_EDGES edges", SLAMIT_ERR_CAPACITY);
    if (max_its > SLAMIT_EG_MAX_ITS) return slamit_refuse(where, "more than SLAMIT_EG_MAX_ITS iterations", SLAMIT_ERR_CAPACITY);
    if (n_pt > SLAMIT_EG_MAX_POINTS) return slamit_refuse(where, "more than SLAMIT_EG_MAX_POINTS points", SLAMIT_ERR_CAPACITY);
    return SLAMIT_OK;
}

// the whole schedule on `st`; h_verdict: 4 pinned ints.  D is complete (workspace carved).
static int eg_run(const char* where, const EgDev& D, int max_its, double lambda_init, hipStream_t st, int32_t* h_verdict) {
    const int K = D.n_kf, E = D.n_edge, T = D.T;
    auto grid = [](int n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); };
    hipLaunchKernelGGL(eg_init, grid(K), dim3(256), 0, st, D, lambda_init);
    hipLaunchKernelGGL(eg_check_tables, grid(std::max(std::max(E, K + 1), D.n_pt)), dim3(256), 0, st, D);
    hipLaunchKernelGGL(eg_compact, dim3(1), dim3(1024), 0, st, D, 0);
    HIP_TRY_AT(where, hipGetLastError());
    HIP_TRY_AT(where, hipMemcpyAsync(h_verdict, &D.st->n_free_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY_AT(where, hipStreamSynchronize(st));
    if (h_verdict[1]) return slamit_refuse(where, "an edge, a point's reference keyframe or an incidence pointer is outside its table");
    if (h_verdict[0] != D.n_free) return slamit_refuse(where, "n_free is not the number of keyframes that are neither fixed nor bad");
    hipLaunchKernelGGL(eg_stats_init, dim3(1), dim3(1), 0, st, D);
    if (E > 0 && D.n_free > 0 && max_its > 0) {
        const size_t lds = sizeof(double) * EG_NB * (size_t)T;   // beside 8,448 B static: past 64 KiB from 7,168 unknowns on
        HIP_TRY_AT(where, hipFuncSetAttribute(reinterpret_cast<const void*>(eg_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(eg_measure, grid(E), dim3(256), 0, st, D);
        for (int it = 0; it < max_its; ++it) {
            hipLaunchKernelGGL(eg_linearize, dim3((unsigned)((E + 7) / 8)), dim3(256), 0, st, D);
            hipLaunchKernelGGL(eg_iter_begin, dim3(1), dim3(256), 0, st, D);
            for (;;) {
                hipLaunchKernelGGL(eg_zero, dim3(T, T), dim3(256), 0, st, D);
                hipLaunchKernelGGL(eg_assemble, dim3(D.n_free), dim3(64), 0, st, D);
                for (int p = 0; p < T; ++p) {
                    hipLaunchKernelGGL(eg_diag, dim3(1), dim3(1024), 0, st, D, p);
                    const int below = T - 1 - p;
                    if (below > 0) {
                        hipLaunchKernelGGL(eg_rows, dim3((unsigned)((below * EG_NB + 255) / 256)), dim3(256), 0, st, D, p);
                        const int RT = (below * EG_NB + EG_MT - 1) / EG_MT;
                        hipLaunchKernelGGL(eg_update, dim3(RT, RT), dim3(256), 0, st, D, p);
                    }
                }
                hipLaunchKernelGGL(eg_solve, dim3(1), dim3(1024), lds, st, D);
                hipLaunchKernelGGL(eg_step, grid(D.n_free), dim3(256), 0, st, D);
                hipLaunchKernelGGL(eg_errors, grid(E), dim3(256), 0, st, D);
                hipLaunchKernelGGL(eg_decide, dim3(1), dim3(256), 0, st, D);
                HIP_TRY_AT(where, hipGetLastError());
                HIP_TRY_AT(where, hipMemcpyAsync(h_verdict, D.st->verdict, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                HIP_TRY_AT(where, hipStreamSynchronize(st));
                if (!h_verdict[0]) break;
            }
            if (h_verdict[1]) break;
        }
    }
    hipLaunchKernelGGL(eg_recover, grid(K), dim3(256), 0, st, D);
    hipLaunchKernelGGL(eg_compact, dim3(1), dim3(1024), 0, st, D, 1);
    hipLaunchKernelGGL(eg_points, grid(D.n_pt), dim3(256), 0, st, D);
    HIP_TRY_AT(where, hipGetLastError());
    return SLAMIT_OK;
}

static void eg_fill(EgDev& D, const slamit_eg_problem& P, const slamit_eg_result& R) {
    D.n_kf = P.n_kf; D.n_edge = P.n_edge; D.n_pt = P.n_pt; D.fix_scale = P.fix_scale != 0;
    D.scw_r = P.scw_r; D.scw_t = P.scw_t; D.scw_s = P.scw_s; D.snc_r = P.snc_r; D.snc_t = P.snc_t; D.snc_s = P.snc_s;
    D.fixed = P.fixed; D.bad = P.bad; D.pt_bad = P.pt_bad;
    D.v0 = P.edge_v0; D.v1 = P.edge_v1; D.kind = P.edge_kind; D.inc_ptr = P.inc_ptr; D.inc_edge = P.inc_edge; D.pt_ref = P.pt_ref;
    D.pt_pos = P.pt_pos;
    D.o_r = R.sim3_r; D.o_t = R.sim3_t; D.o_s = R.sim3_s; D.o_pose = R.pose; D.o_pt = R.pt_pos;
    D.touched = R.touched; D.n_touched = R.n_touched; D.stats = R.stats;
}

extern "C" {

int slamit_essential_plan(const slamit_eg_graph* g, int32_t edge_cap, int32_t* edge_v0, int32_t* edge_v1, int32_t* edge_kind,
                          int32_t* n_edge, int32_t* inc_ptr, int32_t* inc_edge) {
    const char* const where = "slamit_essential_plan";
    if (!g || !n_edge || edge_cap < 0 || (edge_cap > 0 && (!edge_v0 || !edge_v1 || !edge_kind))) return slamit_refuse(where, "bad argument");
    const char* why = "";
    if (eg_check_graph(*g, &why) != SLAMIT_OK) return slamit_refuse(where, why);
    std::vector<EgEdge> edges;
    if (eg_plan_edges(*g, edges, &why) != SLAMIT_OK) return slamit_refuse(where, why);
    const int32_t n = (int32_t)edges.size();
    if (n > edge_cap) {
        *n_edge = n;
        return slamit_refuse(where, "more edges than edge_cap", SLAMIT_ERR_CAPACITY);
    }
    for (int e = 0; e < n; ++e) { edge_v0[e] = edges[e].v0; edge_v1[e] = edges[e].v1; edge_kind[e] = edges[e].kind; }
    *n_edge = n;
    if (inc_ptr && (inc_edge || n == 0)) eg_incidence(g->n_kf, n, edge_v0, edge_v1, inc_ptr, inc_edge);
    return SLAMIT_OK;
}

size_t slamit_essential_graph_workspace(int n_free, int n_kf, int n_edge, int n_pt) {
    if (n_free < 0 || n_kf < 0 || n_edge < 0 || n_pt < 0 || n_free > SLAMIT_EG_MAX_KF || n_edge > SLAMIT_EG_MAX_EDGES) return 0;
    EgDev D;
    memset(&D, 0, sizeof(D));
    D.n_free = n_free; D.n_kf = n_kf; D.n_edge = n_edge; D.n_pt = n_pt;
    eg_dims(D);
    return eg_carve(D, nullptr);
}

int slamit_essential_graph_dev(int device, const slamit_eg_problem* prob, const slamit_eg_result* res, void* d_workspace, size_t workspace_bytes,
                               void* stream) {
    const char* const where = "slamit_essential_graph_dev";
    if (!prob || !res) return slamit_refuse(where, "bad argument");
    const slamit_eg_problem& P = *prob;
    const int rc = eg_check_counts(where, P.n_free, P.n_kf, P.n_edge, P.n_pt, P.max_its);
    if (rc != SLAMIT_OK) return rc;
    if (!res->stats || !res->n_touched || (P.n_kf && (!P.scw_r || !P.scw_t || !P.scw_s || !P.snc_r || !P.snc_t || !P.snc_s || !P.fixed || !P.bad || !P.inc_ptr ||
                                                      !res->sim3_r || !res->sim3_t || !res->sim3_s || !res->pose)) ||
        (P.n_edge && (!P.edge_v0 || !P.edge_v1 || !P.edge_kind || !P.inc_edge)) || (P.n_pt && (!P.pt_pos || !P.pt_ref || !P.pt_bad || !res->pt_pos || !res->touched)))
        return slamit_refuse(where, "null array");
    EgDev D;
    memset(&D, 0, sizeof(D));
    eg_fill(D, P, *res);
    D.n_free = P.n_free;
    eg_dims(D);
    const size_t need = eg_carve(D, nullptr);
    if (!d_workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(d_workspace) & 255)) return slamit_refuse(where, "workspace missing, too small or not 256-byte aligned");
    eg_carve(D, static_cast<unsigned char*>(d_workspace));
    SLAMIT_USE_DEVICE(device);
    static thread_local SlamitScratch V;   // the pinned verdict
    HIP_TRY_AT(where, slamit_scratch_reserve(V, device, 64, 64));
    return eg_run(where, D, P.max_its, P.lambda_init, static_cast<hipStream_t>(stream), reinterpret_cast<int32_t*>(V.host));
}

int slamit_essential_graph(int device, const slamit_eg_problem* prob, slamit_eg_result* res) {
    const char* const where = "slamit_essential_graph";
    if (!prob || !res) return slamit_refuse(where, "bad argument");
    const slamit_eg_problem& P = *prob;
    if (P.n_kf < 0 || P.n_edge < 0 || P.n_pt < 0 || P.max_its < 0) return slamit_refuse(where, "negative count");
    if (!res->n_touched || (P.n_kf && (!P.scw_r || !P.scw_t || !P.scw_s || !P.snc_r || !P.snc_t || !P.snc_s || !P.fixed || !P.bad || !res->sim3_r || !res->sim3_t ||
                                       !res->sim3_s || !res->pose)) ||
        (P.n_edge && (!P.edge_v0 || !P.edge_v1 || !P.edge_kind)) || (P.n_pt && (!P.pt_pos || !P.pt_ref || !P.pt_bad || !res->pt_pos || !res->touched)))
        return slamit_refuse(where, "null array");
    int n_free = 0;
    for (int i = 0; i < P.n_kf; ++i) n_free += !P.fixed[i] && !P.bad[i];
    const int rc = eg_check_counts(where, n_free, P.n_kf, P.n_edge, P.n_pt, P.max_its);
    if (rc != SLAMIT_OK) return rc;
    const char* why = "";
    if (eg_check_edges(P.n_kf, P.bad, P.n_edge, P.edge_v0, P.edge_v1, P.edge_kind, &why) != SLAMIT_OK) return slamit_refuse(where, why);
    for (int p = 0; p < P.n_pt; ++p)
        if (!P.pt_bad[p] && (P.pt_ref[p] < 0 || P.pt_ref[p] >= P.n_kf || P.bad[P.pt_ref[p]])) return slamit_refuse(where, "a good point's reference keyframe is outside [0, n_kf) or bad");
    std::vector<int32_t> inc_ptr, inc_edge;
    if (P.inc_ptr && (P.inc_edge || P.n_edge == 0)) {
        if (!eg_incidence_matches(P.n_kf, P.n_edge, P.edge_v0, P.edge_v1, P.inc_ptr, P.inc_edge)) return slamit_refuse(where, "inc_ptr / inc_edge are not the incidence lists of the edges");
    }
    inc_ptr.resize((size_t)P.n_kf + 1);
    inc_edge.resize((size_t)2 * P.n_edge + 1);
    eg_incidence(P.n_kf, P.n_edge, P.edge_v0, P.edge_v1, inc_ptr.data(), inc_edge.data());

    SLAMIT_USE_DEVICE(device);
    struct Rec { EgDev D; };
    EgDev Dh;
    memset(&Dh, 0, sizeof(Dh));
    static thread_local SlamitScratch S, V;   // V: the pinned words the verdict comes down into
    HIP_TRY_AT(where, slamit_scratch_reserve(V, device, 64, 64));
    int run_rc = SLAMIT_OK;
    const size_t K = (size_t)P.n_kf, E = (size_t)P.n_edge, N = (size_t)P.n_pt;
    const int rc2 = slamit_staged_batch<Rec>(
        where, S, device, 1,
        [&](StageBinder& b, int, Rec& Q) {
            slamit_eg_problem Pd = P;
            slamit_eg_result Rd = *res;
            Pd.scw_r = b.in(P.scw_r, 9 * K); Pd.scw_t = b.in(P.scw_t, 3 * K); Pd.scw_s = b.in(P.scw_s, K);
            Pd.snc_r = b.in(P.snc_r, 9 * K); Pd.snc_t = b.in(P.snc_t, 3 * K); Pd.snc_s = b.in(P.snc_s, K);
            Pd.fixed = b.in(P.fixed, K); Pd.bad = b.in(P.bad, K);
            Pd.edge_v0 = b.in(P.edge_v0, E); Pd.edge_v1 = b.in(P.edge_v1, E); Pd.edge_kind = b.in(P.edge_kind, E);
            Pd.inc_ptr = b.in(inc_ptr.data(), K + 1); Pd.inc_edge = b.in(inc_edge.data(), 2 * E);
            Pd.pt_pos = b.in(P.pt_pos, 3 * N); Pd.pt_ref = b.in(P.pt_ref, N); Pd.pt_bad = b.in(P.pt_bad, N);
            Rd.sim3_r = b.out(res->sim3_r, 9 * K); Rd.sim3_t = b.out(res->sim3_t, 3 * K); Rd.sim3_s = b.out(res->sim3_s, K);
            Rd.pose = b.out(res->pose, 12 * K); Rd.pt_pos = b.out(res->pt_pos, 3 * N);
            Rd.touched = N ? b.out(res->touched, N) : nullptr; Rd.n_touched = b.out(res->n_touched, 1);
            Rd.stats = res->stats ? b.out(res->stats, 1) : b.scratch<slamit_eg_stats>(1);
            eg_fill(Q.D, Pd, Rd);
            Q.D.n_free = n_free;
            eg_dims(Q.D);
            const size_t ws = eg_carve(Q.D, nullptr);
            unsigned char* const w = b.scratch<unsigned char>(ws + 256);
            if (w) eg_carve(Q.D, reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(w) + 255) & ~(uintptr_t)255));
            Dh = Q.D;
        },
        [&](const Rec*) {
            // `touched` past the count stays as the caller gave it only if it goes up first: the staged block's output region is fresh
            if (N) { const hipError_t e = hipMemsetAsync(Dh.touched, 0xFF, sizeof(int32_t) * N, S.st); if (e != hipSuccess) return e; }
            run_rc = eg_run(where, Dh, P.max_its, P.lambda_init, S.st, reinterpret_cast<int32_t*>(V.host));
            return run_rc == SLAMIT_ERR_DEVICE ? hipErrorUnknown : hipSuccess;
        });
    if (run_rc != SLAMIT_OK) return run_rc;
    return rc2;
}

}  // extern "C"
