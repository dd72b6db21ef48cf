// rotation.hip — the rotation-consistency check after a guided search, resident (include/slamit.h, slamit_rotation_check_batch_dev).
//
// Reference: ORB_SLAM2/src/ORBmatcher.cc:1430-1471 (the bookkeeping of SearchByProjection(CurrentFrame, LastFrame, ...)) and
// ComputeThreeMaxima (:1605-1646), as shim::RotationHistogram restates them.  ONE WAVEFRONT walks a frame's queries 64 at a time:
//   pass 1  a matched query q -> keypoint k claims owner[k] by atomicMax(q): the reference assigns in query order, so the
//           last query wins, and the maximum is the last whatever the order the lanes arrive in.  Its bin is counted by an
//           integer add in LDS: a sum does not depend on the order either.
//   maxima  lane 0 runs ThreeMaxima over the 30 counts (strict '>' keeps the first bin on ties; the 10 % rule in float).
//   pass 2  every entry of another bin stores owner[k] = -1; all such stores carry the same value, and an owner that a pass-2 store
//           clears is never written again.  nmatches loses one per ENTRY: the sum of the rejected bins' counts.
// A block is one wavefront, so the barrier between the passes is a wait for the wavefront's own memory operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slamit.h"
#include "slamit_internal.h"

#define ROT_BINS 30   // ORBmatcher::HISTO_LENGTH

// shim::RotationHistogram::add: the bin of a match, -1 for an entry the reference drops
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
    float rot = angle1 - angle2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / ROT_BINS));
    if (bin == ROT_BINS) bin = 0;
    return bin >= 0 && bin < ROT_BINS ? bin : -1;
}

__global__ __launch_bounds__(64) void rotation_check_kernel(slamit_rotation_batch B) {
    __shared__ int s_count[ROT_BINS];
    __shared__ int s_keep[3];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = max(0, min(B.d_n[f], B.kp_cap)), m = min(B.d_m[f], B.q_cap);
    const int32_t* match = B.d_match_kp + (size_t)f * B.q_cap;
    const float* qangle = B.d_qangle + (size_t)f * B.q_cap;
    const slamit_kp* kps = B.d_kps_un + (size_t)f * B.kp_cap;
    int32_t* owner = B.d_kp_query + (size_t)f * B.kp_cap;
    for (int k = lane; k < B.kp_cap; k += 64) owner[k] = -1;
    if (lane < ROT_BINS) s_count[lane] = 0;
    __syncthreads();
    for (int q = lane; q < m; q += 64) {
        const int k = match[q];
        if (k < 0 || k >= n) continue;
        atomicMax(&owner[k], q);
        const int bin = rot_bin(qangle[q], kps[k].angle);
        if (bin >= 0) atomicAdd(&s_count[bin], 1);
    }
    __syncthreads();
    if (lane == 0) {
        int top[3] = {0, 0, 0}, at[3] = {-1, -1, -1};
#pragma unroll 1   // unrolled, the thirty rounds of compares keep more lane masks alive than there are scalar registers
        for (int i = 0; i < ROT_BINS; ++i) {
            const int s = s_count[i];
            const int pos = s > top[0] ? 0 : s > top[1] ? 1 : s > top[2] ? 2 : 3;
            for (int k = 2; k > pos; --k) { top[k] = top[k - 1]; at[k] = at[k - 1]; }
            if (pos < 3) { top[pos] = s; at[pos] = i; }
        }
        if (top[1] < 0.1f * (float)top[0]) { at[1] = -1; at[2] = -1; }
        else if (top[2] < 0.1f * (float)top[0]) at[2] = -1;
        int dropped = 0;
        for (int i = 0; i < ROT_BINS; ++i)
            if (i != at[0] && i != at[1] && i != at[2]) dropped += s_count[i];
        for (int k = 0; k < 3; ++k) { s_keep[k] = at[k]; B.d_bins[3 * f + k] = at[k]; }
        B.d_nmatches[f] -= dropped;
    }
    __syncthreads();
    const int k0 = s_keep[0], k1 = s_keep[1], k2 = s_keep[2];
    for (int q = lane; q < m; q += 64) {
        const int k = match[q];
        if (k < 0 || k >= n) continue;
        const int bin = rot_bin(qangle[q], kps[k].angle);
        if (bin >= 0 && bin != k0 && bin != k1 && bin != k2) owner[k] = -1;
    }
}

extern "C" int slamit_rotation_check_batch_dev(int device, const slamit_rotation_batch* B, void* stream) {
    if (!B || B->nframes < 0 || B->kp_cap < 0 || B->q_cap < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rotation_check_batch_dev: bad argument");
    if (B->nframes == 0) return SLAMIT_OK;
    if (!B->d_n || !B->d_kps_un || !B->d_m || !B->d_match_kp || !B->d_qangle || !B->d_kp_query || !B->d_nmatches || !B->d_bins)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_rotation_check_batch_dev: null array");
    SLAMIT_USE_DEVICE(device);
    hipLaunchKernelGGL(rotation_check_kernel, dim3(B->nframes), dim3(64), 0, (hipStream_t)stream, *B);
    HIP_TRY_AT("slamit_rotation_check_batch_dev", hipGetLastError());
    return SLAMIT_OK;
}
