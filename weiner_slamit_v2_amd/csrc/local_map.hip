// local_map.hip — Tracking::UpdateLocalMap on the GPU (include/slamit.h, slamit_local_*; the walk is stated in local_map.h).
//
// Three passes, every one a grid over (something, frame), so a batch of frames is one launch per kernel:
//   (a) lm_votes_kernel     one lane per keypoint: range and bad test of its point (a bad one becomes -1 in frame_mp), then the lane
//                           walks the point's observers and adds 1 per observer with an integer atomicAdd -- into a histogram in
//                           LDS that the workgroup flushes when the map has at most LM_LDS_KF keyframes, into HBM otherwise.
//                           Integer sums do not depend on arrival order.  (Observer lists are a handful of entries; a wavefront
//                           striding one list at a time would idle most of its lanes, so the lanes take a point each.)
//   (b) lm_keyframes_kernel one wavefront per frame: the votes row 64 slots at a time, the voted non-bad ones compacted in ascending
//                           slot order with a ballot and wave_inclusive_scan_i32, the ballot itself being two words of the mark
//                           bitset in LDS; the maximum as a wave minimum of (inverted count, slot); then lane 0 runs lm_expand,
//                           at most 81 visits of ten neighbours, the children and the parent.
//   (c) lm_mark_kernel      seen[p] = 1 for the frame's own points and frame_seen
//       lm_keys_kernel      one wavefront per (frame, local keyframe): atomicMin of (list position << 16 | keypoint) per point
//       lm_count_kernel     the same walk: an occurrence is kept when its key is the point's minimum; kept per (frame, keyframe)
//       lm_write_kernel     the same walk again: offset = kept of the keyframes in front, rank by ballot and scan, so a
//                           wavefront's kept points go to consecutive entries of local_mp and of the planes the frustum pass reads
// keys / seen / counts are the caller's workspace, cleared on the stream by every call.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"
#include "map_check.h"
#include "local_map.h"

static_assert(sizeof(LmMap) == sizeof(slamit_map_index) && offsetof(LmMap, kf_mp_ptr) == offsetof(slamit_map_index, kf_mp_ptr) &&
                  offsetof(LmMap, kf_parent) == offsetof(slamit_map_index, kf_parent) && offsetof(LmMap, mp_min_dist) == offsetof(slamit_map_index, mp_min_dist),
              "slamit_map_index is LmMap");
static_assert(LM_BAD_SLOT == SLAMIT_LOCAL_MAP_BAD_SLOT && LM_KF_OVERFLOW == SLAMIT_LOCAL_MAP_KF_OVERFLOW && LM_MP_OVERFLOW == SLAMIT_LOCAL_MAP_MP_OVERFLOW &&
                  LM_ROW_CUT == SLAMIT_LOCAL_MAP_ROW_CUT && LM_MAX_KF == SLAMIT_LOCAL_MAP_MAX_KF && LM_MAX_ROW == SLAMIT_LOCAL_MAP_MAX_ROW &&
                  LM_MIN_KF_CAP == SLAMIT_LOCAL_MAP_MIN_KF_CAP && LM_BEST == SLAMIT_LOCAL_MAP_BEST,
              "local_map.h restates the C-ABI's constants");

#define LM_LDS_KF 4096                                   // keyframes whose votes fit the workgroup's LDS histogram (16 KiB)
#define LM_MARK_WORDS ((LM_MAX_KF + 1 + 63) / 64 * 2)    // the mark bitset, whole 64-slot chunks (8 KiB)

// The batch as the kernels' argument: the maps' records travel with it, the arrays stay where the caller keeps them.
struct LmBatch {
    int32_t nframes, n_maps, kp_cap, seen_cap, kf_cap, q_cap, vote_cap, mp_cap;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* frame_map; const int32_t* n; int32_t* frame_mp; const int32_t* n_seen; const int32_t* frame_seen;
    int32_t* votes; int32_t* local_kf; int32_t* n_local_kf; int32_t* ref_kf;
    int32_t* local_mp; int32_t* n_local_mp; float* pos; float* normal; float* max_dist; float* min_dist; uint8_t* skip; int32_t* m;
    int32_t* status;
    uint32_t* keys; uint8_t* seen; int32_t* counts;   // [nframes][mp_cap], [nframes][mp_cap], [nframes][kf_cap]
};

__device__ __forceinline__ int lm_clamp(int v, int cap) { return min(max(v, 0), cap); }
__device__ __forceinline__ int lm_wave_total(int v) { return __builtin_amdgcn_readlane(wave_inclusive_scan_i32(v), 63); }   // every lane active

// the map of frame f, or false for a map index outside the batch's
__device__ __forceinline__ bool lm_frame_map(const LmBatch& B, int f, LmMap& M) {
    const int fm = __builtin_amdgcn_readfirstlane(B.frame_map[f]);
    if ((unsigned)fm >= (unsigned)B.n_maps) return false;
    M = B.maps[fm];
    // the capacities bound every index into a per-frame row, whatever the record says
    M.n_kf = min(M.n_kf, B.vote_cap); M.n_mp = min(M.n_mp, B.mp_cap);
    return true;
}

// grid (ceil(kp_cap / 256), frames), 256 threads
__global__ __launch_bounds__(256) void lm_votes_kernel(LmBatch B) {
    __shared__ int hist[LM_LDS_KF];
    const int f = blockIdx.y;
    LmMap M;
    if (!lm_frame_map(B, f, M)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&B.status[f], LM_BAD_SLOT);
        return;
    }
    const int n = lm_clamp(B.n[f], B.kp_cap);
    if ((int)(blockIdx.x * 256) >= n) return;   // the whole workgroup
    const bool lds = M.n_kf <= LM_LDS_KF;
    if (lds) {
        for (int k = threadIdx.x; k < M.n_kf; k += 256) hist[k] = 0;
        __syncthreads();
    }
    int32_t* const votes = B.votes + (size_t)f * B.vote_cap;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    int st = 0;
    if (i < n) {
        int32_t* const slot = B.frame_mp + (size_t)f * B.kp_cap + i;
        const int p = *slot;
        if (p != -1) {
            if (!lm_mp_ok(M, p)) st = LM_BAD_SLOT;
            else if (M.mp_bad[p]) *slot = -1;
            else {
                const int e1 = M.obs_ptr[p + 1];
                for (int e = M.obs_ptr[p]; e < e1; ++e) {
                    const int k = M.obs_kf[e];
                    if (!lm_kf_ok(M, k)) { st = LM_BAD_SLOT; continue; }
                    if (lds) atomicAdd(&hist[k], 1); else atomicAdd(&votes[k], 1);
                }
            }
        }
    }
    if (st) atomicOr(&B.status[f], st);
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < M.n_kf; k += 256) {
            const int v = hist[k];
            if (v) atomicAdd(&votes[k], v);
        }
    }
}

// grid (frames), 64 threads
__global__ __launch_bounds__(64) void lm_keyframes_kernel(LmBatch B) {
    __shared__ uint32_t marks[LM_MARK_WORDS];
    const int f = blockIdx.x, lane = threadIdx.x;
    LmMap M;
    if (!lm_frame_map(B, f, M)) return;
    M.n_kf = min(M.n_kf, LM_MAX_KF);
    const int32_t* const votes = B.votes + (size_t)f * B.vote_cap;
    unsigned long long any = 0;
    for (int k0 = 0; k0 < M.n_kf; k0 += 64) {
        const int k = k0 + lane;
        any |= __ballot(k < M.n_kf && votes[k] > 0);
    }
    if (!any) return;   // :1540: before clear()
    int32_t* const local_kf = B.local_kf + (size_t)f * B.kf_cap;
    int base = 0, st = 0;
    unsigned long long best = ~0ull;   // (0x7fffffff - count, slot): the minimum is the largest count at its lowest slot
    for (int k0 = 0; k0 < M.n_kf; k0 += 64) {
        const int k = k0 + lane;
        const int v = k < M.n_kf ? votes[k] : 0;
        const bool take = v > 0 && !M.kf_bad[k];
        const unsigned long long mask = __ballot(take);
        const int rank = base + wave_inclusive_scan_i32(take ? 1 : 0) - 1;
        if (take) {
            if (rank < B.kf_cap) local_kf[rank] = k; else st = LM_KF_OVERFLOW;
            const unsigned long long key = ((unsigned long long)(unsigned)(0x7fffffff - v) << 32) | (unsigned)k;
            best = key < best ? key : best;
        }
        if (lane == 0) { marks[k0 >> 5] = (uint32_t)mask; marks[(k0 >> 5) + 1] = (uint32_t)(mask >> 32); }
        base += __popcll(mask);
    }
    best = wave_min_u64(best);
    if (st) atomicOr(&B.status[f], st);
    __syncthreads();   // the list and the marks, written by 64 lanes, are read by lane 0
    if (lane == 0) {
        int st0 = 0;
        B.n_local_kf[f] = lm_expand(M, local_kf, base, B.kf_cap, marks, st0);
        if (best != ~0ull) B.ref_kf[f] = (int)(unsigned)best;
        if (st0) atomicOr(&B.status[f], st0);
    }
}

// grid (ceil((kp_cap + seen_cap) / 256), frames), 256 threads
__global__ __launch_bounds__(256) void lm_mark_kernel(LmBatch B) {
    const int f = blockIdx.y;
    LmMap M;
    if (!lm_frame_map(B, f, M)) return;
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int p = -1;
    bool own = false;
    if (t < B.kp_cap) {
        if (t < lm_clamp(B.n[f], B.kp_cap)) { p = B.frame_mp[(size_t)f * B.kp_cap + t]; own = true; }
    } else if (B.frame_seen && B.n_seen) {
        const int s = t - B.kp_cap;
        if (s < lm_clamp(B.n_seen[f], B.seen_cap)) p = B.frame_seen[(size_t)f * B.seen_cap + s];
    }
    if (p == -1) return;
    if (!lm_mp_ok(M, p)) { atomicOr(&B.status[f], LM_BAD_SLOT); return; }
    if (own && M.mp_bad[p]) return;
    B.seen[(size_t)f * B.mp_cap + p] = 1;
}

// The row of local keyframe j of frame f: false when there is none.  `st` collects status bits.
struct LmRow { int begin, len; };
__device__ __forceinline__ bool lm_row(const LmBatch& B, const LmMap& M, int f, int j, LmRow& R, int& st) {
    if (j >= lm_clamp(B.n_local_kf[f], B.kf_cap)) return false;
    const int k = B.local_kf[(size_t)f * B.kf_cap + j];
    if (!lm_kf_ok(M, k)) { st |= LM_BAD_SLOT; return false; }
    R.begin = M.kf_mp_ptr[k];
    R.len = M.kf_mp_ptr[k + 1] - R.begin;
    if (R.len > LM_MAX_ROW) { R.len = LM_MAX_ROW; st |= LM_ROW_CUT; }
    return true;
}
// entry i of the row: the point, or -1 for none / bad / out of range
__device__ __forceinline__ int lm_row_point(const LmMap& M, const LmRow& R, int i, int& st) {
    if (i >= R.len) return -1;
    const int p = M.kf_mp[R.begin + i];
    if (p == -1) return -1;
    if (!lm_mp_ok(M, p)) { st |= LM_BAD_SLOT; return -1; }
    return M.mp_bad[p] ? -1 : p;
}

// grid (kf_cap, frames), 64 threads
__global__ __launch_bounds__(64) void lm_keys_kernel(LmBatch B) {
    const int j = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    LmMap M;
    if (!lm_frame_map(B, f, M)) return;
    LmRow R;
    int st = 0;
    if (lm_row(B, M, f, j, R, st)) {
        uint32_t* const keys = B.keys + (size_t)f * B.mp_cap;
        for (int i = lane; i < R.len; i += 64) {
            const int p = lm_row_point(M, R, i, st);
            if (p >= 0) atomicMin(&keys[p], lm_key(j, i));
        }
    }
    if (st) atomicOr(&B.status[f], st);   // the two walks below see the same slots: they do not report them again
}

__global__ __launch_bounds__(64) void lm_count_kernel(LmBatch B) {
    const int j = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    LmMap M;
    if (!lm_frame_map(B, f, M)) return;
    LmRow R;
    int st = 0, count = 0;
    if (lm_row(B, M, f, j, R, st)) {
        const uint32_t* const keys = B.keys + (size_t)f * B.mp_cap;
        for (int i0 = 0; i0 < R.len; i0 += 64) {
            const int i = i0 + lane;
            const int p = lm_row_point(M, R, i, st);
            count += __popcll(__ballot(p >= 0 && keys[p] == lm_key(j, i)));
        }
    }
    if (lane == 0) B.counts[(size_t)f * B.kf_cap + j] = count;
}

__global__ __launch_bounds__(64) void lm_write_kernel(LmBatch B) {
    const int j = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    LmMap M;
    if (!lm_frame_map(B, f, M)) {
        if (j == 0 && lane == 0) { B.n_local_mp[f] = 0; if (B.m) B.m[f] = 0; }
        return;
    }
    const int nl = lm_clamp(B.n_local_kf[f], B.kf_cap);
    const int32_t* const counts = B.counts + (size_t)f * B.kf_cap;
    if (j == 0) {   // the frame's totals
        int part = 0;
        for (int q = lane; q < nl; q += 64) part += counts[q];
        const int total = lm_wave_total(part);
        if (lane == 0) {
            B.n_local_mp[f] = total;
            if (B.m) B.m[f] = min(total, B.q_cap);
            if (total > B.q_cap) atomicOr(&B.status[f], LM_MP_OVERFLOW);
        }
    }
    LmRow R;
    int st = 0;
    if (!lm_row(B, M, f, j, R, st)) return;
    int part = 0;
    for (int q = lane; q < j; q += 64) part += counts[q];
    int base = lm_wave_total(part);
    const uint32_t* const keys = B.keys + (size_t)f * B.mp_cap;
    const uint8_t* const seen = B.seen + (size_t)f * B.mp_cap;
    const size_t q_cap = (size_t)B.q_cap, row = (size_t)f * q_cap;
    for (int i0 = 0; i0 < R.len && base < B.q_cap; i0 += 64) {
        const int i = i0 + lane;
        const int p = lm_row_point(M, R, i, st);
        const bool kept = p >= 0 && keys[p] == lm_key(j, i);
        const unsigned long long mask = __ballot(kept);
        const int r = base + wave_inclusive_scan_i32(kept ? 1 : 0) - 1;
        if (kept && r < B.q_cap) {
            B.local_mp[row + r] = p;
            B.skip[row + r] = seen[p];
            if (B.pos) {
                for (int c = 0; c < 3; ++c) {
                    B.pos[(3 * (size_t)f + c) * q_cap + r] = M.mp_pos[3 * (size_t)p + c];
                    B.normal[(3 * (size_t)f + c) * q_cap + r] = M.mp_normal[3 * (size_t)p + c];
                }
                B.max_dist[row + r] = M.mp_max_dist[p];
                B.min_dist[row + r] = M.mp_min_dist[p];
            }
        }
        base += __popcll(mask);
    }
}

static size_t lm_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the launches of (a) + (b); votes and status are the caller's to clear
static hipError_t lm_launch_keyframes(const LmBatch& B, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.votes, 0, sizeof(int32_t) * (size_t)B.nframes * B.vote_cap, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lm_votes_kernel, dim3(std::max(1, (B.kp_cap + 255) / 256), B.nframes), dim3(256), 0, st, B);
    hipLaunchKernelGGL(lm_keyframes_kernel, dim3(B.nframes), dim3(64), 0, st, B);
    return hipGetLastError();
}

// the launches of (c)
static hipError_t lm_launch_points(const LmBatch& B, hipStream_t st) {
    const size_t per = (size_t)B.nframes * B.mp_cap;
    hipError_t e = hipSuccess;
    if (per) {
        e = hipMemsetAsync(B.keys, 0xff, sizeof(uint32_t) * per, st);
        if (e == hipSuccess) e = hipMemsetAsync(B.seen, 0, per, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lm_mark_kernel, dim3(std::max(1, (B.kp_cap + B.seen_cap + 255) / 256), B.nframes), dim3(256), 0, st, B);
    hipLaunchKernelGGL(lm_keys_kernel, dim3(B.kf_cap, B.nframes), dim3(64), 0, st, B);
    hipLaunchKernelGGL(lm_count_kernel, dim3(B.kf_cap, B.nframes), dim3(64), 0, st, B);
    hipLaunchKernelGGL(lm_write_kernel, dim3(B.kf_cap, B.nframes), dim3(64), 0, st, B);
    return hipGetLastError();
}

extern "C" {   // what the host forms check before anything is launched: map_check.h and their own arguments

size_t slamit_local_map_workspace(int nframes, int mp_cap, int kf_cap) {
    if (nframes <= 0 || mp_cap < 0 || kf_cap < 0) return 0;
    const size_t per = (size_t)nframes * (size_t)mp_cap;
    return lm_align(sizeof(uint32_t) * per) + lm_align(per) + lm_align(sizeof(int32_t) * (size_t)nframes * (size_t)kf_cap);
}

int slamit_local_keyframes(int device, const slamit_map_index* map, int32_t n, int32_t* frame_mp, int32_t* votes, int32_t kf_cap,
                           int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf, int32_t* status) {
    const char* const where = "slamit_local_keyframes";
    if (!map || n < 0 || !votes || !local_kf || !n_local_kf || !ref_kf || !status || (n && !frame_mp))
        return slamit_refuse(where, "null array or negative count");
    if (n > SLAMIT_FRAME_MAX_KP) return slamit_refuse(where, "more than SLAMIT_FRAME_MAX_KP keypoints");
    if (const char* bad = map_sizes_error(map)) return slamit_refuse(where, bad);
    if (kf_cap < SLAMIT_LOCAL_MAP_MIN_KF_CAP || kf_cap > SLAMIT_LOCAL_MAP_MAX_KF)
        return slamit_refuse(where, "kf_cap outside [SLAMIT_LOCAL_MAP_MIN_KF_CAP, SLAMIT_LOCAL_MAP_MAX_KF]");
    if (!map->obs_ptr || !map->kf_child_ptr || (map->n_mp && !map->mp_bad) || (map->n_kf && (!map->kf_bad || !map->kf_best || !map->kf_parent)))
        return slamit_refuse(where, "null table");
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (!map_csr_ok(map->obs_ptr, n_mp) || !map_csr_ok(map->kf_child_ptr, n_kf))
        return slamit_refuse(where, "a CSR pointer array does not ascend from 0");
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_child = (size_t)map->kf_child_ptr[n_kf];
    if ((n_obs && !map->obs_kf) || (n_child && !map->kf_child)) return slamit_refuse(where, "null table");
    if (!map_slots_ok(frame_mp, (size_t)n, -1, n_mp)) return slamit_refuse(where, "frame_mp holds a slot outside [-1, n_mp)");
    if (!map_slots_ok(map->obs_kf, n_obs, 0, n_kf) || !map_slots_ok(map->kf_child, n_child, 0, n_kf) ||
        !map_slots_ok(map->kf_best, (size_t)n_kf * LM_BEST, -1, n_kf) || !map_slots_ok(map->kf_parent, (size_t)n_kf, -1, n_kf))
        return slamit_refuse(where, "a table holds a keyframe slot outside [0, n_kf)");
    SLAMIT_USE_DEVICE(device);
    LmBatch H;   // the bound record, for the launches
    const int32_t *in_mp = nullptr, *in_kf = nullptr, *in_nkf = nullptr, *in_ref = nullptr;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<LmBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, LmBatch& Q) {
            Q.nframes = 1; Q.n_maps = 1; Q.kp_cap = n; Q.kf_cap = kf_cap; Q.vote_cap = n_kf; Q.mp_cap = n_mp;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.obs_ptr = b.in(map->obs_ptr, (size_t)n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs);
            M.mp_bad = b.in(map->mp_bad, (size_t)n_mp); M.kf_bad = b.in(map->kf_bad, (size_t)n_kf);
            M.kf_best = b.in(map->kf_best, (size_t)n_kf * LM_BEST);
            M.kf_child_ptr = b.in(map->kf_child_ptr, (size_t)n_kf + 1); M.kf_child = b.in(map->kf_child, n_child);
            M.kf_parent = b.in(map->kf_parent, (size_t)n_kf);
            int32_t *h_map, *h_n;
            Q.frame_map = b.in_fill<int32_t>(1, &h_map); Q.n = b.in_fill<int32_t>(1, &h_n);
            if (h_map) { *h_map = 0; *h_n = n; }
            in_mp = b.in(frame_mp, (size_t)n); in_kf = b.in(local_kf, (size_t)kf_cap); in_nkf = b.in(n_local_kf, 1); in_ref = b.in(ref_kf, 1);
            Q.frame_mp = b.out(frame_mp, (size_t)n); Q.votes = b.out(votes, (size_t)n_kf);
            Q.local_kf = b.out(local_kf, (size_t)kf_cap); Q.n_local_kf = b.out(n_local_kf, 1); Q.ref_kf = b.out(ref_kf, 1);
            Q.status = b.out(status, 1);
            H = Q;
        },
        [&](const LmBatch*) {
            // the in / out arrays start as the caller's
            hipError_t e = hipSuccess;
            if (n) e = hipMemcpyAsync(H.frame_mp, in_mp, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, S.st);
            if (e == hipSuccess) e = hipMemcpyAsync(H.local_kf, in_kf, sizeof(int32_t) * (size_t)kf_cap, hipMemcpyDeviceToDevice, S.st);
            if (e == hipSuccess) e = hipMemcpyAsync(H.n_local_kf, in_nkf, sizeof(int32_t), hipMemcpyDeviceToDevice, S.st);
            if (e == hipSuccess) e = hipMemcpyAsync(H.ref_kf, in_ref, sizeof(int32_t), hipMemcpyDeviceToDevice, S.st);
            if (e == hipSuccess) e = hipMemsetAsync(H.status, 0, sizeof(int32_t), S.st);
            if (e != hipSuccess || n_kf == 0) return e;
            return lm_launch_keyframes(H, S.st);
        });
}

int slamit_local_points(int device, const slamit_map_index* map, int32_t n, const int32_t* frame_mp, int32_t n_seen,
                        const int32_t* frame_seen, int32_t n_local_kf, const int32_t* local_kf, int32_t q_cap, int32_t* local_mp,
                        uint8_t* skip, int32_t* n_local_mp, int32_t* status) {
    const char* const where = "slamit_local_points";
    if (!map || n < 0 || n_seen < 0 || n_local_kf < 0 || q_cap < 0 || !n_local_mp || !status || (n && !frame_mp) || (n_seen && !frame_seen) ||
        (n_local_kf && !local_kf) || (q_cap && (!local_mp || !skip)))
        return slamit_refuse(where, "null array or negative count");
    if (n > SLAMIT_FRAME_MAX_KP) return slamit_refuse(where, "more than SLAMIT_FRAME_MAX_KP keypoints");
    if (q_cap > SLAMIT_FRUSTUM_MAX_N) return slamit_refuse(where, "q_cap above SLAMIT_FRUSTUM_MAX_N");
    if (n_local_kf > SLAMIT_LOCAL_MAP_MAX_KF) return slamit_refuse(where, "more than SLAMIT_LOCAL_MAP_MAX_KF local keyframes");
    if (const char* bad = map_sizes_error(map)) return slamit_refuse(where, bad);
    if (!map->kf_mp_ptr || (map->n_mp && !map->mp_bad)) return slamit_refuse(where, "null table");
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (!map_csr_ok(map->kf_mp_ptr, n_kf)) return slamit_refuse(where, "kf_mp_ptr does not ascend from 0");
    const size_t n_kfmp = (size_t)map->kf_mp_ptr[n_kf];
    if (n_kfmp && !map->kf_mp) return slamit_refuse(where, "null table");
    for (int k = 0; k < n_kf; ++k)
        if (map->kf_mp_ptr[k + 1] - map->kf_mp_ptr[k] > SLAMIT_LOCAL_MAP_MAX_ROW)
            return slamit_refuse(where, "a keyframe with more than SLAMIT_LOCAL_MAP_MAX_ROW keypoints");
    if (!map_slots_ok(frame_mp, (size_t)n, -1, n_mp) || !map_slots_ok(frame_seen, (size_t)n_seen, -1, n_mp) || !map_slots_ok(map->kf_mp, n_kfmp, -1, n_mp))
        return slamit_refuse(where, "a point slot outside [-1, n_mp)");
    if (!map_slots_ok(local_kf, (size_t)n_local_kf, 0, n_kf)) return slamit_refuse(where, "local_kf holds a slot outside [0, n_kf)");
    SLAMIT_USE_DEVICE(device);
    LmBatch H;
    const int32_t* in_mp = nullptr;
    const uint8_t* in_skip = nullptr;
    const int kf_cap = std::max(n_local_kf, 1);
    static thread_local SlamitScratch S;
    return slamit_staged_batch<LmBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, LmBatch& Q) {
            Q.nframes = 1; Q.n_maps = 1; Q.kp_cap = n; Q.seen_cap = n_seen; Q.kf_cap = kf_cap; Q.q_cap = q_cap; Q.vote_cap = n_kf; Q.mp_cap = n_mp;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.mp_bad = b.in(map->mp_bad, (size_t)n_mp);
            M.kf_mp_ptr = b.in(map->kf_mp_ptr, (size_t)n_kf + 1); M.kf_mp = b.in(map->kf_mp, n_kfmp);
            int32_t* h3;
            const int32_t* const d3 = b.in_fill<int32_t>(4, &h3);   // frame_map, n, n_seen, n_local_kf
            if (h3) { h3[0] = 0; h3[1] = n; h3[2] = n_seen; h3[3] = n_local_kf; }
            Q.frame_map = d3; Q.n = d3 ? d3 + 1 : nullptr; Q.n_seen = d3 ? d3 + 2 : nullptr; Q.n_local_kf = d3 ? const_cast<int32_t*>(d3) + 3 : nullptr;
            Q.frame_mp = const_cast<int32_t*>(b.in(frame_mp, (size_t)n));
            Q.frame_seen = n_seen ? b.in(frame_seen, (size_t)n_seen) : nullptr;
            Q.local_kf = const_cast<int32_t*>(b.in(local_kf, (size_t)n_local_kf));
            in_mp = b.in(local_mp, (size_t)q_cap); in_skip = b.in(skip, (size_t)q_cap);
            Q.local_mp = b.out(local_mp, (size_t)q_cap); Q.skip = b.out(skip, (size_t)q_cap);
            Q.n_local_mp = b.out(n_local_mp, 1); Q.status = b.out(status, 1);
            Q.keys = b.scratch<uint32_t>((size_t)n_mp); Q.seen = b.scratch<uint8_t>((size_t)n_mp); Q.counts = b.scratch<int32_t>((size_t)kf_cap);
            H = Q;
        },
        [&](const LmBatch*) {
            hipError_t e = hipMemsetAsync(H.status, 0, sizeof(int32_t), S.st);
            if (e == hipSuccess && q_cap) e = hipMemcpyAsync(H.local_mp, in_mp, sizeof(int32_t) * (size_t)q_cap, hipMemcpyDeviceToDevice, S.st);
            if (e == hipSuccess && q_cap) e = hipMemcpyAsync(H.skip, in_skip, (size_t)q_cap, hipMemcpyDeviceToDevice, S.st);
            if (e != hipSuccess) return e;
            return lm_launch_points(H, S.st);
        });
}

int slamit_local_map_batch_dev(int device, const slamit_local_map_batch_rec* R, void* stream) {
    const char* const where = "slamit_local_map_batch_dev";
    if (!R || R->nframes < 0 || R->n_maps < 0 || R->kp_cap < 0 || R->seen_cap < 0 || R->q_cap < 0 || R->vote_cap < 0 || R->mp_cap < 0)
        return slamit_refuse(where, "bad argument");
    if (R->nframes == 0) return SLAMIT_OK;
    if (R->nframes > 65535) return slamit_refuse(where, "more than 65535 frames");
    if (R->n_maps < 1 || R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps)
        return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->kp_cap > SLAMIT_FRAME_MAX_KP) return slamit_refuse(where, "kp_cap above SLAMIT_FRAME_MAX_KP");
    if (R->q_cap > SLAMIT_FRUSTUM_MAX_N) return slamit_refuse(where, "q_cap above SLAMIT_FRUSTUM_MAX_N");
    if (R->kf_cap < SLAMIT_LOCAL_MAP_MIN_KF_CAP || R->kf_cap > SLAMIT_LOCAL_MAP_MAX_KF)
        return slamit_refuse(where, "kf_cap outside [SLAMIT_LOCAL_MAP_MIN_KF_CAP, SLAMIT_LOCAL_MAP_MAX_KF]");
    if (R->vote_cap > SLAMIT_LOCAL_MAP_MAX_KF) return slamit_refuse(where, "vote_cap above SLAMIT_LOCAL_MAP_MAX_KF");
    for (int i = 0; i < R->n_maps; ++i) {
        const slamit_map_index& M = R->maps[i];
        if (M.n_kf < 0 || M.n_mp < 0 || M.n_kf > R->vote_cap || M.n_mp > R->mp_cap)
            return slamit_refuse(where, "a map with n_kf above vote_cap or n_mp above mp_cap");
        if (!M.obs_ptr || !M.obs_kf || !M.mp_bad || !M.kf_bad || !M.kf_mp_ptr || !M.kf_mp || !M.kf_best || !M.kf_child_ptr || !M.kf_child ||
            !M.kf_parent || !M.mp_pos || !M.mp_normal || !M.mp_max_dist || !M.mp_min_dist)
            return slamit_refuse(where, "null table");
    }
    if (!R->d_frame_map || !R->d_n || !R->d_frame_mp || !R->d_votes || !R->d_local_kf || !R->d_n_local_kf || !R->d_ref_kf || !R->d_local_mp ||
        !R->d_n_local_mp || !R->d_pos || !R->d_normal || !R->d_max_dist || !R->d_min_dist || !R->d_skip || !R->d_m || !R->d_status ||
        (!R->d_n_seen) != (!R->d_frame_seen))
        return slamit_refuse(where, "null array");
    const size_t need = slamit_local_map_workspace(R->nframes, R->mp_cap, R->kf_cap);
    if (!R->d_workspace || R->workspace_bytes < need)
        return slamit_refuse(where, "workspace smaller than slamit_local_map_workspace()", SLAMIT_ERR_CAPACITY);
    SLAMIT_USE_DEVICE(device);
    LmBatch B;
    memset(&B, 0, sizeof(B));
    B.nframes = R->nframes; B.n_maps = R->n_maps; B.kp_cap = R->kp_cap; B.seen_cap = R->d_frame_seen ? R->seen_cap : 0; B.kf_cap = R->kf_cap;
    B.q_cap = R->q_cap; B.vote_cap = R->vote_cap; B.mp_cap = R->mp_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    B.frame_map = R->d_frame_map; B.n = R->d_n; B.frame_mp = R->d_frame_mp; B.n_seen = R->d_n_seen; B.frame_seen = R->d_frame_seen;
    B.votes = R->d_votes; B.local_kf = R->d_local_kf; B.n_local_kf = R->d_n_local_kf; B.ref_kf = R->d_ref_kf;
    B.local_mp = R->d_local_mp; B.n_local_mp = R->d_n_local_mp; B.pos = R->d_pos; B.normal = R->d_normal; B.max_dist = R->d_max_dist;
    B.min_dist = R->d_min_dist; B.skip = R->d_skip; B.m = R->d_m; B.status = R->d_status;
    const size_t per = (size_t)R->nframes * (size_t)R->mp_cap;
    unsigned char* const w = (unsigned char*)R->d_workspace;
    B.keys = (uint32_t*)w; B.seen = w + lm_align(sizeof(uint32_t) * per); B.counts = (int32_t*)(w + lm_align(sizeof(uint32_t) * per) + lm_align(per));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY_AT(where, hipMemsetAsync(B.status, 0, sizeof(int32_t) * (size_t)B.nframes, st));
    HIP_TRY_AT(where, lm_launch_keyframes(B, st));
    HIP_TRY_AT(where, lm_launch_points(B, st));
    return SLAMIT_OK;
}

}  // extern "C"
