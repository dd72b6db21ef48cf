// frustum.hip — Tracking::SearchLocalPoints' visibility pass on the GPU (include/slamit.h, slamit_frustum*).
//
// Reference: ORB_SLAM2/src/Tracking.cc:1409-1464, Frame::isInFrustum (src/Frame.cc:389-445), MapPoint::PredictScale
// (src/MapPoint.cc:391-400) and the window of ORBmatcher::SearchByProjection (src/ORBmatcher.cc:47-71).  Every local map point is
// independent: ONE LANE takes one point and runs frustum.h on it -- projection, bounds, distance and viewing-angle gates, the
// predicted level, the search window -- and writes the point's query at its own index, in the layout the guided search reads
// (search.hip: a query with valid = 0 leaves search_candidates_kernel before its window is read and resolves to no keypoint).
// The frame record is the same for every lane (scalar loads of the record, indexed by blockIdx.y); the point arrays are planes,
// so the 64 loads of a wavefront are contiguous; the scale table sits in the record and is indexed by the masked level.  No LDS,
// no atomics.  Host form: the points in view of a wavefront are a ballot's popcount, written to one slot per wavefront and summed
// on the host.  Device form: a second launch of one wavefront per frame sums the valid flags.  A batch of frames is one launch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "frustum.h"

static_assert(FRU_MAX_LEVELS == SLAMIT_MAX_LEVELS && (FRU_MAX_LEVELS & (FRU_MAX_LEVELS - 1)) == 0, "frustum.h masks the level with FRU_MAX_LEVELS - 1");
static_assert(sizeof(FrustumFrame) == sizeof(slamit_frustum_frame) && offsetof(FrustumFrame, th) == offsetof(slamit_frustum_frame, th) &&
                  offsetof(FrustumFrame, scale_factors) == offsetof(slamit_frustum_frame, scale_factors) &&
                  offsetof(FrustumFrame, min_x) == offsetof(slamit_frustum_frame, min_x),
              "slamit_frustum_frame is FrustumFrame");

// The arrays of one frame's points; `plane` is the distance between the x, y and z planes of pos / normal.  The last five of the
// device form may be null.
struct FruArrays {
    const SLAMIT_GLOBAL float* pos; const SLAMIT_GLOBAL float* normal; const SLAMIT_GLOBAL float* max_dist; const SLAMIT_GLOBAL float* min_dist;
    const SLAMIT_GLOBAL uint8_t* skip;
    SLAMIT_GLOBAL float* uvr; SLAMIT_GLOBAL int32_t* level_min; SLAMIT_GLOBAL int32_t* level_max; SLAMIT_GLOBAL uint8_t* valid;
    SLAMIT_GLOBAL uint8_t* status; SLAMIT_GLOBAL float* proj; SLAMIT_GLOBAL float* view_cos; SLAMIT_GLOBAL int32_t* level;
};

struct FruProb {
    FrustumFrame F;
    int32_t n, plane;
    FruArrays A;
    SLAMIT_GLOBAL int32_t* wave_counts;   // (n + 63) / 64
};

// point i (< n, checked by the caller) of a frame: true = in view
__device__ __forceinline__ bool frustum_lane(const FrustumFrame& F, const FruArrays& A, size_t plane, size_t i) {
    const float P[3] = {A.pos[i], A.pos[plane + i], A.pos[2 * plane + i]};
    const float Pn[3] = {A.normal[i], A.normal[plane + i], A.normal[2 * plane + i]};
    FrustumOut o;
    const int st = frustum_point(F, P, Pn, A.max_dist[i], A.min_dist[i], A.skip[i] != 0, o);
    float uvr[3];
    int l0, l1;
    unsigned char valid;
    frustum_query(st, o, uvr, l0, l1, valid);
    A.uvr[3 * i] = uvr[0]; A.uvr[3 * i + 1] = uvr[1]; A.uvr[3 * i + 2] = uvr[2];
    A.level_min[i] = l0; A.level_max[i] = l1; A.valid[i] = valid;
    if (A.status) A.status[i] = (uint8_t)st;
    if (A.proj) { A.proj[3 * i] = o.u; A.proj[3 * i + 1] = o.v; A.proj[3 * i + 2] = o.uR; }
    if (A.view_cos) A.view_cos[i] = o.viewCos;
    if (A.level) A.level[i] = o.level;
    return st == FRU_IN_VIEW;
}

// grid (ceil(max n / 256), problems), 256 threads: lane t of block b takes point 256 b + t of problem blockIdx.y
__global__ __launch_bounds__(256) void frustum_kernel(const FruProb* __restrict__ probs) {
    const FruProb& P = probs[blockIdx.y];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P.n) return;
    const bool in = frustum_lane(P.F, P.A, (size_t)P.plane, (size_t)i);
    const unsigned long long m = __ballot(in);   // the lanes past n have left: they count as 0
    // the point index rises with the lane, so lane 0 of a wavefront that has any live lane is live itself: a remapping must keep that
    if ((threadIdx.x & 63) == 0) P.wave_counts[i >> 6] = __popcll(m);
}

// The device form's records stay where the caller keeps them; the batch itself travels as the kernel's argument.
struct FruDev {
    int32_t q_cap;
    const FrustumFrame* frames; const int32_t* m;
    FruArrays A;   // frame 0's; frame f's start f * q_cap entries (3 f * q_cap for the planes and the triplets) further on
};

__device__ __forceinline__ FruArrays fru_frame_arrays(const FruArrays& B, size_t f, size_t q_cap) {
    FruArrays A;
    const size_t o = f * q_cap;
    A.pos = B.pos + 3 * o; A.normal = B.normal + 3 * o; A.max_dist = B.max_dist + o; A.min_dist = B.min_dist + o; A.skip = B.skip + o;
    A.uvr = B.uvr + 3 * o; A.level_min = B.level_min + o; A.level_max = B.level_max + o; A.valid = B.valid + o;
    A.status = B.status ? B.status + o : nullptr; A.proj = B.proj ? B.proj + 3 * o : nullptr;
    A.view_cos = B.view_cos ? B.view_cos + o : nullptr; A.level = B.level ? B.level + o : nullptr;
    return A;
}

__global__ __launch_bounds__(256) void frustum_dev_kernel(FruDev D) {
    const int f = blockIdx.y;
    const int m = min(D.m[f], D.q_cap);
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= m) return;
    // n_levels is the caller's, unchecked: frustum_point accepts a level only below min(n_levels, FRU_MAX_LEVELS) and masks the index
    frustum_lane(D.frames[f], fru_frame_arrays(D.A, (size_t)f, (size_t)D.q_cap), (size_t)D.q_cap, (size_t)i);
}

// grid (frames), 64 threads: the frame's valid flags summed by one wavefront, 64 flags per ballot
__global__ __launch_bounds__(64) void frustum_count_kernel(const uint8_t* __restrict__ valid, const int32_t* __restrict__ m_arr, int q_cap,
                                                           int32_t* __restrict__ n_in_view) {
    const int f = blockIdx.x;
    const int m = min(m_arr[f], q_cap);
    const uint8_t* V = valid + (size_t)f * q_cap;
    int count = 0;
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + (int)threadIdx.x;
        count += __popcll(__ballot(i < m && V[i] != 0));
    }
    if (threadIdx.x == 0) n_in_view[f] = count;
}

hipError_t slamit_launch_valid_count(const uint8_t* d_valid, const int32_t* d_m, int q_cap, int nframes, int32_t* d_count, hipStream_t stream) {
    hipLaunchKernelGGL(frustum_count_kernel, dim3(nframes), dim3(64), 0, stream, d_valid, d_m, q_cap, d_count);
    return hipGetLastError();
}

extern "C" {

int slamit_frustum_batch(int device, int nprob, const slamit_frustum_problem* probs, slamit_frustum_result* results) {
    const char* const where = "slamit_frustum_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    if (nprob > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: more than 65535 problems");
    int max_n = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_frustum_problem& P = probs[f];
        const slamit_frustum_result& R = results[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: negative count");
        if (P.n > SLAMIT_FRUSTUM_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: more than SLAMIT_FRUSTUM_MAX_N points");
        if (P.n == 0) continue;   // nothing to test, nothing read
        if (P.frame.n_levels < 1 || P.frame.n_levels > SLAMIT_MAX_LEVELS)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: n_levels outside [1, SLAMIT_MAX_LEVELS]");
        if (!P.pos || !P.normal || !P.max_dist || !P.min_dist || !P.skip || !R.status || !R.proj || !R.view_cos || !R.level || !R.uvr ||
            !R.level_min || !R.level_max || !R.valid)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch: null array");
        max_n = std::max(max_n, (int)P.n);
    }
    for (int f = 0; f < nprob; ++f) results[f].n_in_view = 0;
    if (max_n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: pos normal (planes) max_dist min_dist skip] go up; [per problem: the eight outputs, wave counts] come down
    std::vector<StageView<int32_t>> waves(nprob);
    static thread_local SlamitScratch S;
    const int rc = slamit_staged_batch<FruProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, FruProb& Q) {
            const slamit_frustum_problem& P = probs[f];
            const slamit_frustum_result& R = results[f];
            const size_t n = (size_t)P.n;
            Q.n = P.n; Q.plane = P.n;
            if (n) memcpy(&Q.F, &P.frame, sizeof(Q.F));
            float *pp, *pn;
            Q.A.pos = slamit_global(b.in_fill<float>(3 * n, &pp)); Q.A.normal = slamit_global(b.in_fill<float>(3 * n, &pn));
            if (pp)   // the caller's n x 3 rows become three planes
                for (int c = 0; c < 3; ++c)
                    for (size_t i = 0; i < n; ++i) { pp[c * n + i] = P.pos[3 * i + c]; pn[c * n + i] = P.normal[3 * i + c]; }
            Q.A.max_dist = slamit_global(b.in(P.max_dist, n)); Q.A.min_dist = slamit_global(b.in(P.min_dist, n));
            Q.A.skip = slamit_global(b.in(P.skip, n));
            Q.A.status = slamit_global(b.out(R.status, n)); Q.A.proj = slamit_global(b.out(R.proj, 3 * n));
            Q.A.view_cos = slamit_global(b.out(R.view_cos, n)); Q.A.level = slamit_global(b.out(R.level, n));
            Q.A.uvr = slamit_global(b.out(R.uvr, 3 * n)); Q.A.level_min = slamit_global(b.out(R.level_min, n));
            Q.A.level_max = slamit_global(b.out(R.level_max, n)); Q.A.valid = slamit_global(b.out(R.valid, n));
            Q.wave_counts = slamit_global(b.out_view((n + 63) / 64, &waves[f]));
        },
        [&](const FruProb* d_recs) {
            hipLaunchKernelGGL(frustum_kernel, dim3((max_n + 255) / 256, nprob), dim3(256), 0, S.st, d_recs);
            return hipGetLastError();
        });
    if (rc != SLAMIT_OK) return rc;
    for (int f = 0; f < nprob; ++f) results[f].n_in_view = stage_sum(waves[f].data, waves[f].count);
    return SLAMIT_OK;
}

int slamit_frustum(int device, const slamit_frustum_problem* prob, slamit_frustum_result* res) {
    return slamit_frustum_batch(device, 1, prob, res);
}

int slamit_frustum_batch_dev(int device, const slamit_frustum_batch_rec* B, void* stream) {
    if (!B || B->nframes < 0 || B->q_cap < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch_dev: bad argument");
    if (B->q_cap > SLAMIT_FRUSTUM_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch_dev: q_cap above SLAMIT_FRUSTUM_MAX_N");
    if (B->nframes == 0 || B->q_cap == 0) return SLAMIT_OK;
    if (!B->d_frames || !B->d_m || !B->d_pos || !B->d_normal || !B->d_max_dist || !B->d_min_dist || !B->d_skip || !B->d_uvr || !B->d_level_min ||
        !B->d_level_max || !B->d_valid)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch_dev: null array");
    if (B->nframes > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_frustum_batch_dev: more than 65535 frames");
    SLAMIT_USE_DEVICE(device);
    FruDev D;
    D.q_cap = B->q_cap;
    D.frames = reinterpret_cast<const FrustumFrame*>(B->d_frames); D.m = B->d_m;
    D.A.pos = (const SLAMIT_GLOBAL float*)B->d_pos; D.A.normal = (const SLAMIT_GLOBAL float*)B->d_normal;
    D.A.max_dist = (const SLAMIT_GLOBAL float*)B->d_max_dist; D.A.min_dist = (const SLAMIT_GLOBAL float*)B->d_min_dist;
    D.A.skip = (const SLAMIT_GLOBAL uint8_t*)B->d_skip;
    D.A.uvr = (SLAMIT_GLOBAL float*)B->d_uvr; D.A.level_min = (SLAMIT_GLOBAL int32_t*)B->d_level_min;
    D.A.level_max = (SLAMIT_GLOBAL int32_t*)B->d_level_max; D.A.valid = (SLAMIT_GLOBAL uint8_t*)B->d_valid;
    D.A.status = (SLAMIT_GLOBAL uint8_t*)B->d_status; D.A.proj = (SLAMIT_GLOBAL float*)B->d_proj;
    D.A.view_cos = (SLAMIT_GLOBAL float*)B->d_view_cos; D.A.level = (SLAMIT_GLOBAL int32_t*)B->d_level;
    hipLaunchKernelGGL(frustum_dev_kernel, dim3((B->q_cap + 255) / 256, B->nframes), dim3(256), 0, (hipStream_t)stream, D);
    HIP_TRY_AT("slamit_frustum_batch_dev", hipGetLastError());
    if (B->d_n_in_view) {
        HIP_TRY_AT("slamit_frustum_batch_dev", slamit_launch_valid_count(B->d_valid, B->d_m, B->q_cap, B->nframes, B->d_n_in_view, (hipStream_t)stream));
    }
    return SLAMIT_OK;
}

}  // extern "C"
