// unproject.hip — the two links between a stereo / RGB-D frame's depths and its pose on the GPU (include/slamit.h, slamit_rgbd_depth*,
// slamit_unproject_closest*).
//
// rgbd_depth_kernel: Frame::ComputeStereoFromRGBD (ORB_SLAM2/src/Frame.cc:766-787).  One lane per keypoint, blockIdx.y = frame, so a
// wavefront stays on one frame: its plane record is a scalar load and its 64 scattered depth reads fall into one image.
//
// closest_points_kernel: the closest-point walk of Tracking::UpdateLastFrame / CreateNewKeyFrame / StereoInitialization
// (src/Tracking.cc:1039-1091, :1334-1396, :712-727) with Frame::UnprojectStereo and the new point's constructor (csrc/unproject.h).
// ONE WORKGROUP per frame.  Each wavefront owns a contiguous range of keypoints.  Pass 1 counts (ballot + popcount): candidates,
// close ones, NeedNewKeyFrame's two numbers.  Pass 2 compacts the candidates' 64-bit keys (depth bits << 32 | index) into LDS in
// index order, at the wavefront's base plus the popcount of the ballot below the lane.  Mode CLOSEST then sorts the keys in LDS
// (bitonic, padded with ~0 to a power of two): the keys are unique, so the sorted order is the reference's pair order and a
// keypoint's position does not depend on scheduling.  The walk's length is the closed form of unproject.h.  Finally position j's
// lane writes order[j] and the keypoint's status, and unprojects it when it needs a point.  No atomics; every output entry has
// exactly one writer.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "unproject.h"

static_assert(UNP_MAX_LEVELS == SLAMIT_MAX_LEVELS && (UNP_MAX_LEVELS & (UNP_MAX_LEVELS - 1)) == 0, "unproject.h masks the octave with UNP_MAX_LEVELS - 1");
static_assert(sizeof(UnprojectFrame) == sizeof(slamit_unproject_frame) && offsetof(UnprojectFrame, th_depth) == offsetof(slamit_unproject_frame, th_depth) &&
                  offsetof(UnprojectFrame, scale_factors) == offsetof(slamit_unproject_frame, scale_factors) &&
                  offsetof(UnprojectFrame, ctor) == offsetof(slamit_unproject_frame, ctor),
              "slamit_unproject_frame is UnprojectFrame");
static_assert(UNP_MODE_CLOSEST == SLAMIT_UNPROJECT_CLOSEST && UNP_MODE_ALL == SLAMIT_UNPROJECT_ALL && UNP_CTOR_FRAME == SLAMIT_UNPROJECT_CTOR_FRAME &&
                  UNP_CTOR_KEYFRAME == SLAMIT_UNPROJECT_CTOR_KEYFRAME && UNP_DEPTH_F32 == SLAMIT_DEPTH_F32 && UNP_DEPTH_U16 == SLAMIT_DEPTH_U16,
              "the header's enumerators are unproject.h's");
static_assert(sizeof(slamit_unproject_counts) == 6 * sizeof(int32_t), "six counters");

// ---- ComputeStereoFromRGBD -------------------------------------------------------------------------------------------------------

struct RgbdFrame {
    const SLAMIT_GLOBAL unsigned char* data;
    size_t pitch;
    int32_t width, height, type;
    float factor, mbf;
    int32_t n;
    const SLAMIT_GLOBAL slamit_kp* kps; const SLAMIT_GLOBAL slamit_kp* kps_un;
    SLAMIT_GLOBAL float* u_right; SLAMIT_GLOBAL float* depth; SLAMIT_GLOBAL uint8_t* status;   // status may be null
};

struct RgbdDev {
    int32_t cap;
    const slamit_depth_plane* planes; const float* mbf; const int32_t* n;
    const slamit_kp* kps; const slamit_kp* kps_un;
    float* u_right; float* depth; uint8_t* status;
};

__device__ __forceinline__ void rgbd_lane(const RgbdFrame& R, int i) {
    float ur, d;
    // the plane is addressed only after unp_rgbd has found row and column inside it
    const int st = unp_rgbd((const void*)R.data, R.pitch, R.width, R.height, R.type, R.factor, R.mbf, R.kps[i].x, R.kps[i].y, R.kps_un[i].x, ur, d);
    R.u_right[i] = ur; R.depth[i] = d;
    if (R.status) R.status[i] = (uint8_t)st;
}

// grid (ceil(max n / 256), frames), 256 threads.  probs != null: the host form's records; else the resident batch D.
__global__ __launch_bounds__(256) void rgbd_depth_kernel(const RgbdFrame* __restrict__ probs, RgbdDev D) {
    const int f = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (probs) {
        const RgbdFrame& R = probs[f];
        if (i < R.n) rgbd_lane(R, i);
        return;
    }
    const int n = min(max(D.n[f], 0), D.cap);
    if (i >= n) return;
    const slamit_depth_plane& P = D.planes[f];
    const size_t o = (size_t)f * D.cap;
    RgbdFrame R;
    R.data = (const SLAMIT_GLOBAL unsigned char*)P.data; R.pitch = P.pitch; R.width = P.width; R.height = P.height; R.type = P.type; R.factor = P.factor;
    R.mbf = D.mbf[f]; R.n = n;
    R.kps = (const SLAMIT_GLOBAL slamit_kp*)(D.kps + o); R.kps_un = (const SLAMIT_GLOBAL slamit_kp*)(D.kps_un + o);
    R.u_right = (SLAMIT_GLOBAL float*)(D.u_right + o); R.depth = (SLAMIT_GLOBAL float*)(D.depth + o);
    R.status = D.status ? (SLAMIT_GLOBAL uint8_t*)(D.status + o) : nullptr;
    rgbd_lane(R, i);
}

// ---- the closest-point walk ------------------------------------------------------------------------------------------------------

// One frame's arrays.  pos / normal entry (c, i) is at [c * stride_c + i * stride_i]: rows of three in the host form (1, 3), planes
// in the resident form (cap, 1).  merge: the resident form writes only where a point is created, into slamit_project_batch_dev's arrays.
struct UnpArrays {
    const SLAMIT_GLOBAL slamit_kp* kps_un; const SLAMIT_GLOBAL float* depth; const SLAMIT_GLOBAL uint8_t* tracked;   // tracked may be null in mode ALL
    SLAMIT_GLOBAL uint8_t* status; SLAMIT_GLOBAL int32_t* order; SLAMIT_GLOBAL float* pos; SLAMIT_GLOBAL float* normal;
    SLAMIT_GLOBAL float* max_dist; SLAMIT_GLOBAL float* min_dist; SLAMIT_GLOBAL int32_t* octave; SLAMIT_GLOBAL uint8_t* skip;
    SLAMIT_GLOBAL int32_t* counts;   // six
    int32_t stride_c, stride_i, merge;
};

struct UnpProb {
    UnprojectFrame F;
    int32_t n;
    UnpArrays A;
};

struct UnpDev {
    int32_t cap;
    const UnprojectFrame* frames; const int32_t* n;
    const slamit_kp* kps_un; const float* depth; const uint8_t* tracked;
    float* pos; int32_t* octave; uint8_t* skip; float* normal; float* max_dist; float* min_dist;
    uint8_t* status; int32_t* order; int32_t* counts;
};

#define UNP_MAX_WAVES 16
#define UNP_LDS_TAIL (size_t)(UNP_MAX_WAVES * 4 * sizeof(int))   // per-wavefront counters behind the keys

__device__ __forceinline__ void unp_store3(SLAMIT_GLOBAL float* a, const UnpArrays& A, int i, float x, float y, float z) {
    const size_t b = (size_t)i * A.stride_i;
    a[b] = x; a[b + A.stride_c] = y; a[b + 2 * (size_t)A.stride_c] = z;
}

// grid (frames), 256 or 1024 threads, dynamic LDS: P keys of 8 bytes (P = the power of two the host chose, >= every frame's n) and
// UNP_LDS_TAIL bytes.  probs != null: the host form's records; else the resident batch D.
__global__ __launch_bounds__(1024) void closest_points_kernel(const UnpProb* __restrict__ probs, UnpDev D, int P) {
    extern __shared__ unsigned long long unp_keys[];
    int* const wave_cnt = (int*)(unp_keys + P);   // [wave][4]: candidates, close, total, map
    const int f = blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = (int)blockDim.x >> 6;

    // the record stays in memory (scalar loads; the scale table is indexed by the octave): a copy would live in scratch memory
    const UnprojectFrame& F = probs ? probs[f].F : D.frames[f];
    UnpArrays A;
    int n;
    if (probs) {
        A = probs[f].A; n = probs[f].n;
    } else {
        n = min(max(D.n[f], 0), D.cap);
        const size_t o = (size_t)f * D.cap;
        A.kps_un = (const SLAMIT_GLOBAL slamit_kp*)(D.kps_un + o); A.depth = (const SLAMIT_GLOBAL float*)(D.depth + o);
        A.tracked = D.tracked ? (const SLAMIT_GLOBAL uint8_t*)(D.tracked + o) : nullptr;
        A.status = D.status ? (SLAMIT_GLOBAL uint8_t*)(D.status + o) : nullptr; A.order = D.order ? (SLAMIT_GLOBAL int32_t*)(D.order + o) : nullptr;
        A.pos = (SLAMIT_GLOBAL float*)(D.pos + 3 * o); A.normal = D.normal ? (SLAMIT_GLOBAL float*)(D.normal + 3 * o) : nullptr;
        A.max_dist = D.max_dist ? (SLAMIT_GLOBAL float*)(D.max_dist + o) : nullptr; A.min_dist = D.min_dist ? (SLAMIT_GLOBAL float*)(D.min_dist + o) : nullptr;
        A.octave = (SLAMIT_GLOBAL int32_t*)(D.octave + o); A.skip = (SLAMIT_GLOBAL uint8_t*)(D.skip + o);
        A.counts = D.counts ? (SLAMIT_GLOBAL int32_t*)(D.counts + 6 * (size_t)f) : nullptr;
        A.stride_c = D.cap; A.stride_i = 1; A.merge = 1;
    }
    n = min(n, P);   // the host sized P for every n it could see; a resident count is clamped to cap <= P
    const bool all = F.mode == UNP_MODE_ALL;
    const bool use_tracked = !all && A.tracked != nullptr;

    // the wavefront's keypoints: [lo, hi), a multiple of 64 per wavefront
    const int per = ((n + nwaves - 1) / nwaves + 63) & ~63;
    const int lo = min(wave * per, n), hi = min(lo + per, n);

    // pass 1: the counts of this wavefront
    int c_cand = 0, c_close = 0, c_total = 0, c_map = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        bool cand = false, close = false, below = false, map = false;
        if (i < hi) {
            const float z = A.depth[i];
            cand = unp_candidate(z);
            close = cand && !unp_far(z, F.th_depth);
            below = cand && unp_below(z, F.th_depth);
            map = below && A.tracked != nullptr && A.tracked[i] != 0;
        }
        c_cand += __popcll(__ballot(cand)); c_close += __popcll(__ballot(close));
        c_total += __popcll(__ballot(below)); c_map += __popcll(__ballot(map));
    }
    if (lane == 0) { wave_cnt[4 * wave] = c_cand; wave_cnt[4 * wave + 1] = c_close; wave_cnt[4 * wave + 2] = c_total; wave_cnt[4 * wave + 3] = c_map; }
    __syncthreads();
    int base = 0, M = 0, c = 0, n_total = 0, n_map = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int v = wave_cnt[4 * w];
        base += w < wave ? v : 0;
        M += v; c += wave_cnt[4 * w + 1]; n_total += wave_cnt[4 * w + 2]; n_map += wave_cnt[4 * w + 3];
    }

    // pass 2: candidates' keys into LDS in index order; a keypoint without depth is settled here
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        bool cand = false;
        float z = 0.f;
        if (i < hi) { z = A.depth[i]; cand = unp_candidate(z); }
        const unsigned long long m = __ballot(cand);
        if (cand) unp_keys[base + __popcll(m & ((1ull << lane) - 1ull))] = unp_key(z, i);
        base += __popcll(m);
        if (i < hi && !cand && !A.merge) {
            A.status[i] = UNP_NO_DEPTH;
            unp_store3(A.pos, A, i, 0.f, 0.f, 0.f); unp_store3(A.normal, A, i, 0.f, 0.f, 0.f);
            A.max_dist[i] = 0.f; A.min_dist[i] = 0.f;
        } else if (i < hi && !cand && A.status) {
            A.status[i] = UNP_NO_DEPTH;
        }
    }
    // the sort's size: the least power of two that holds the candidates (>= 2 so that the network has a stage)
    int S = 2;
    while (S < M) S <<= 1;
    for (int j = M + tid; j < S; j += (int)blockDim.x) unp_keys[j] = ~0ull;
    __syncthreads();

    if (!all) {
        for (int k = 2; k <= S; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (S >> 1); t += (int)blockDim.x) {
                    const int a = 2 * t - (t & (j - 1)), b = a | j;
                    const unsigned long long ka = unp_keys[a], kb = unp_keys[b];
                    const bool up = (a & k) == 0;
                    if ((ka > kb) == up) { unp_keys[a] = kb; unp_keys[b] = ka; }
                }
                __syncthreads();
            }
        }
    }

    const int n_visit = unp_n_visited(M, c, F.min_points, F.mode);

    // position j: the keypoint there, its status, its point
    int created = 0;
    for (int j0 = 0; j0 < n; j0 += (int)blockDim.x) {
        const int j = j0 + tid;
        bool made = false;
        if (j < M) {
            const unsigned long long key = unp_keys[j];
            const int i = (int)(unsigned)(key & 0xffffffffull);
            int st = UNP_BEYOND;
            UnprojectPoint o;
            o.pos[0] = o.pos[1] = o.pos[2] = 0.f; o.normal[0] = o.normal[1] = o.normal[2] = 0.f; o.max_dist = 0.f; o.min_dist = 0.f;
            int octave = 0;
            if (j < n_visit) {
                if (use_tracked && A.tracked[i] != 0) st = UNP_TRACKED;
                else {
                    const float u = A.kps_un[i].x, v = A.kps_un[i].y;
                    octave = A.kps_un[i].octave;
                    float zf;
                    const unsigned zb = (unsigned)(key >> 32);
                    __builtin_memcpy(&zf, &zb, 4);
                    if (unp_point(F, u, v, zf, octave, o)) { st = UNP_CREATED; made = true; }
                    else {
                        st = UNP_OCTAVE;
                        o.pos[0] = o.pos[1] = o.pos[2] = 0.f; o.normal[0] = o.normal[1] = o.normal[2] = 0.f;
                    }
                }
            }
            if (A.status) A.status[i] = (uint8_t)st;
            if (!A.merge || made) {
                unp_store3(A.pos, A, i, o.pos[0], o.pos[1], o.pos[2]);
                if (A.normal) unp_store3(A.normal, A, i, o.normal[0], o.normal[1], o.normal[2]);
                if (A.max_dist) A.max_dist[i] = o.max_dist;
                if (A.min_dist) A.min_dist[i] = o.min_dist;
            }
            if (A.merge && made) { A.octave[i] = octave; A.skip[i] = 0; }
        }
        if (j < n && A.order) A.order[j] = j < n_visit ? (int)(unsigned)(unp_keys[j] & 0xffffffffull) : -1;
        created += __popcll(__ballot(made));
    }
    __syncthreads();   // wave_cnt is read above by every wavefront before it is written again
    if (lane == 0) wave_cnt[4 * wave] = created;
    __syncthreads();
    if (tid == 0 && A.counts) {
        int n_created = 0;
        for (int w = 0; w < nwaves; ++w) n_created += wave_cnt[4 * w];
        A.counts[0] = M; A.counts[1] = c; A.counts[2] = n_visit; A.counts[3] = n_created; A.counts[4] = n_total; A.counts[5] = n_map;
    }
}

static int unp_pow2(int n) {
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

static hipError_t unp_launch(const UnpProb* d_probs, const UnpDev& D, int nframes, int max_n, hipStream_t st) {
    const int P = unp_pow2(max_n);
    const size_t lds = (size_t)P * sizeof(unsigned long long) + UNP_LDS_TAIL;
    if (lds > 32 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(closest_points_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(closest_points_kernel, dim3(nframes), dim3(P > 2048 ? 1024 : 256), lds, st, d_probs, D, P);
    return hipGetLastError();
}

extern "C" {

int slamit_rgbd_depth_batch(int device, int nprob, const slamit_rgbd_problem* probs, slamit_rgbd_result* results) {
    const char* const where = "slamit_rgbd_depth_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    if (nprob > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: more than 65535 problems");
    int max_n = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_rgbd_problem& P = probs[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: negative count");
        if (P.n > SLAMIT_STEREO_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_rgbd_depth_batch: more than SLAMIT_STEREO_MAX_KP keypoints");
        if (P.n == 0) continue;
        if (P.plane.type != SLAMIT_DEPTH_F32 && P.plane.type != SLAMIT_DEPTH_U16) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: unknown element type");
        const size_t es = P.plane.type == SLAMIT_DEPTH_U16 ? 2 : 4;
        if (P.plane.width < 0 || P.plane.height < 0 || P.plane.pitch < es * (size_t)P.plane.width)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: plane geometry");
        if (!P.kps || !P.kps_un || !results[f].u_right || !results[f].depth || !results[f].status || (!P.plane.data && P.plane.width && P.plane.height))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch: null array");
        max_n = std::max(max_n, (int)P.n);
    }
    if (max_n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: the depth plane, kps kps_un] go up; [per problem: u_right depth status] come down
    static thread_local SlamitScratch S;
    return slamit_staged_batch<RgbdFrame>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, RgbdFrame& Q) {
            const slamit_rgbd_problem& P = probs[f];
            const size_t n = (size_t)P.n;
            const size_t used = n ? (P.plane.type == SLAMIT_DEPTH_U16 ? 2 : 4) * (size_t)P.plane.width : 0, rows = n ? (size_t)P.plane.height : 0;
            const size_t row_bytes = (used + 3) & ~(size_t)3;   // rows go up without their padding
            Q.n = P.n;
            unsigned char* dst;
            Q.data = slamit_global(b.in_fill<unsigned char>(row_bytes * rows, &dst)); Q.pitch = row_bytes;
            if (dst)
                for (size_t r = 0; r < rows; ++r) memcpy(dst + r * row_bytes, (const unsigned char*)P.plane.data + r * P.plane.pitch, used);
            Q.width = P.plane.width; Q.height = P.plane.height; Q.type = P.plane.type; Q.factor = P.plane.factor; Q.mbf = P.mbf;
            Q.kps = slamit_global(b.in(P.kps, n)); Q.kps_un = slamit_global(b.in(P.kps_un, n));
            Q.u_right = slamit_global(b.out(results[f].u_right, n)); Q.depth = slamit_global(b.out(results[f].depth, n));
            Q.status = slamit_global(b.out(results[f].status, n));
        },
        [&](const RgbdFrame* d_recs) {
            RgbdDev none;
            memset(&none, 0, sizeof(none));
            hipLaunchKernelGGL(rgbd_depth_kernel, dim3((max_n + 255) / 256, nprob), dim3(256), 0, S.st, d_recs, none);
            return hipGetLastError();
        });
}

int slamit_rgbd_depth(int device, const slamit_rgbd_problem* prob, slamit_rgbd_result* res) { return slamit_rgbd_depth_batch(device, 1, prob, res); }

int slamit_rgbd_depth_batch_dev(int device, const slamit_rgbd_batch_rec* B, void* stream) {
    if (!B || B->nframes < 0 || B->cap < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch_dev: bad argument");
    if (B->cap > SLAMIT_STEREO_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_rgbd_depth_batch_dev: cap above SLAMIT_STEREO_MAX_KP");
    if (B->nframes == 0 || B->cap == 0) return SLAMIT_OK;
    if (B->nframes > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch_dev: more than 65535 frames");
    if (!B->d_planes || !B->d_mbf || !B->d_kps || !B->d_kps_un || !B->d_n || !B->d_u_right || !B->d_depth)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_rgbd_depth_batch_dev: null array");
    SLAMIT_USE_DEVICE(device);
    RgbdDev D;
    D.cap = B->cap; D.planes = B->d_planes; D.mbf = B->d_mbf; D.n = B->d_n; D.kps = B->d_kps; D.kps_un = B->d_kps_un;
    D.u_right = B->d_u_right; D.depth = B->d_depth; D.status = B->d_status;
    hipLaunchKernelGGL(rgbd_depth_kernel, dim3((B->cap + 255) / 256, B->nframes), dim3(256), 0, (hipStream_t)stream, (const RgbdFrame*)nullptr, D);
    HIP_TRY_AT("slamit_rgbd_depth_batch_dev", hipGetLastError());
    return SLAMIT_OK;
}

// the frame record's own checks, for both forms of the walk that can see it
static const char* unp_frame_error(const slamit_unproject_frame& F) {
    if (F.n_levels < 1 || F.n_levels > SLAMIT_MAX_LEVELS) return "n_levels outside [1, SLAMIT_MAX_LEVELS]";
    if (F.mode != SLAMIT_UNPROJECT_CLOSEST && F.mode != SLAMIT_UNPROJECT_ALL) return "unknown mode";
    if (F.ctor != SLAMIT_UNPROJECT_CTOR_FRAME && F.ctor != SLAMIT_UNPROJECT_CTOR_KEYFRAME) return "unknown ctor";
    if (F.min_points < 0) return "min_points below zero";
    return nullptr;
}

int slamit_unproject_closest_batch(int device, int nprob, const slamit_unproject_problem* probs, slamit_unproject_result* results) {
    const char* const where = "slamit_unproject_closest_batch";
    static thread_local char msg[160];
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    if (nprob > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch: more than 65535 problems");
    int max_n = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_unproject_problem& P = probs[f];
        const slamit_unproject_result& R = results[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch: negative count");
        if (P.n > SLAMIT_STEREO_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_unproject_closest_batch: more than SLAMIT_STEREO_MAX_KP keypoints");
        if (const char* e = unp_frame_error(P.frame)) {
            snprintf(msg, sizeof(msg), "slamit_unproject_closest_batch: %s", e);
            return slamit_fail(SLAMIT_ERR_ARG, msg);
        }
        if (P.n == 0) continue;
        if (!P.kps_un || !P.depth || (!P.tracked && P.frame.mode != SLAMIT_UNPROJECT_ALL) || !R.status || !R.order || !R.pos || !R.normal || !R.max_dist || !R.min_dist)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch: null array");
        max_n = std::max(max_n, (int)P.n);
    }
    for (int f = 0; f < nprob; ++f) memset(&results[f].counts, 0, sizeof(results[f].counts));
    if (max_n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: kps_un depth, tracked where given] go up; [per problem: the six outputs, the six counters] come down
    std::vector<StageView<int32_t>> counts(nprob);
    static thread_local SlamitScratch S;
    const int rc = slamit_staged_batch<UnpProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, UnpProb& Q) {
            const slamit_unproject_problem& P = probs[f];
            const slamit_unproject_result& R = results[f];
            const size_t n = (size_t)P.n;
            memcpy(&Q.F, &P.frame, sizeof(Q.F));
            Q.n = P.n;
            Q.A.kps_un = slamit_global(b.in(P.kps_un, n)); Q.A.depth = slamit_global(b.in(P.depth, n));
            Q.A.tracked = n ? slamit_global(b.in(P.tracked, n)) : nullptr;   // null without the caller's: mode ALL
            Q.A.status = slamit_global(b.out(R.status, n)); Q.A.order = slamit_global(b.out(R.order, n));
            Q.A.pos = slamit_global(b.out(R.pos, 3 * n)); Q.A.normal = slamit_global(b.out(R.normal, 3 * n));
            Q.A.max_dist = slamit_global(b.out(R.max_dist, n)); Q.A.min_dist = slamit_global(b.out(R.min_dist, n));
            Q.A.counts = slamit_global(b.out_view(6, &counts[f]));   // written for an empty problem too
            Q.A.stride_c = 1; Q.A.stride_i = 3; Q.A.merge = 0;
        },
        [&](const UnpProb* d_recs) {
            UnpDev none;
            memset(&none, 0, sizeof(none));
            return unp_launch(d_recs, none, nprob, max_n, S.st);
        });
    if (rc != SLAMIT_OK) return rc;
    for (int f = 0; f < nprob; ++f)
        if (probs[f].n) memcpy(&results[f].counts, counts[f].data, sizeof(results[f].counts));
    return SLAMIT_OK;
}

int slamit_unproject_closest(int device, const slamit_unproject_problem* prob, slamit_unproject_result* res) {
    return slamit_unproject_closest_batch(device, 1, prob, res);
}

int slamit_unproject_closest_batch_dev(int device, const slamit_unproject_batch_rec* B, void* stream) {
    if (!B || B->nframes < 0 || B->cap < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch_dev: bad argument");
    if (B->cap > SLAMIT_STEREO_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_unproject_closest_batch_dev: cap above SLAMIT_STEREO_MAX_KP");
    if (B->nframes == 0 || B->cap == 0) return SLAMIT_OK;
    if (!B->d_frames || !B->d_n || !B->d_kps_un || !B->d_depth || !B->d_tracked || !B->d_pos || !B->d_octave || !B->d_skip)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_unproject_closest_batch_dev: null array");
    SLAMIT_USE_DEVICE(device);
    UnpDev D;
    D.cap = B->cap; D.frames = reinterpret_cast<const UnprojectFrame*>(B->d_frames); D.n = B->d_n; D.kps_un = B->d_kps_un; D.depth = B->d_depth;
    D.tracked = B->d_tracked; D.pos = B->d_pos; D.octave = B->d_octave; D.skip = B->d_skip; D.normal = B->d_normal; D.max_dist = B->d_max_dist;
    D.min_dist = B->d_min_dist; D.status = B->d_status; D.order = B->d_order; D.counts = reinterpret_cast<int32_t*>(B->d_counts);
    HIP_TRY_AT("slamit_unproject_closest_batch_dev", unp_launch(nullptr, D, B->nframes, B->cap, (hipStream_t)stream));
    return SLAMIT_OK;
}

}  // extern "C"
