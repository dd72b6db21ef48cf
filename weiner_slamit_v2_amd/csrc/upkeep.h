// upkeep.h — what local mapping does to a map point after every step that touches it: MapPoint::UpdateNormalAndDepth
// (ORB_SLAM2/src/MapPoint.cc:336-377), MapPoint::ComputeDistinctiveDescriptors (:248-313) and LocalMapping::MapPointCulling
// (src/LocalMapping.cc:184-219), over the slot tables of local_map.h plus the columns of UpIndex (the layout of slamit_point_index).
// One header for host and device: upkeep.hip runs the walks one wavefront per point / one workgroup per list and calls the per-point
// functions below; the CPU test of the restatement, the shim's test driver and tools/bench_upkeep.py build the *_seq functions with g++.
// Plain C++ over IEEE +, -, *, / and sqrt; it must be compiled with -ffp-contract=off.
//
// UpdateNormalAndDepth, line by line.  The float and double readings are unproject.h's (its table, rows PC .. min_dist), through
// unp_norm3 and unp_mat_div; PARITY UNPINNED as there: where the reference goes through OpenCV the order is read, not run.
//   a bad point, no observation   return: nothing changes                                                            :344, :351
//   normali                       mWorldPos - Owi in float, for EVERY observer: the reference does not ask isBad()   :360
//   normal                        normal + normali * unp_mat_div(unp_norm3(normali)) in float, from zeros,            :361
//                                 ONE OBSERVER AFTER THE OTHER IN ASCENDING SLOT (the order of std::map<KeyFrame*, size_t> for a
//                                 caller that numbers keyframes by address): float addition is not associative, so the sum is
//                                 never a tree.  obs_kf rows come in any order; up_sorted_seq / the kernel order them first
//   dist                          (float)unp_norm3(Pos - Ow_ref)                                                     :365-366
//   level                         the octave of observations[pRefKF]                                                 :367
//   max_dist, min_dist            dist * scale_factors[level]; max_dist / scale_factors[n_levels - 1]                 :373-374
//   mNormalVector                 normal * unp_mat_div((double)n)                                                    :375
// THE REFERENCE'S ODD PLACE, kept: a reference keyframe that is NOT among the observers.  observations[pRefKF] default-inserts
// index 0, so the level is the octave of keypoint 0 of that keyframe (kf_octave[kf_mp_ptr[ref]]); UP_REF_NOT_OBSERVER says so.
// STATED DEPARTURES, where the reference reads out of bounds: a reference slot of -1 (UP_NO_REF), a reference keyframe without
// keypoints in that odd place (UP_REF_NO_KP) and a level outside [0, n_levels) (UP_OCTAVE) leave the normal and both distances
// as they were.  A row above UP_MAX_OBS (UP_OBS_OVERFLOW) leaves the whole point as it was.
//
// ComputeDistinctiveDescriptors.  The rows are the descriptors kf_desc[kf_mp_ptr[k] + idx] of the observers that are NOT bad, in
// ascending slot; Distances are integers; the median of row i is vDists[(int)(0.5 * (N - 1))] of the sorted row and the first row
// with the least median wins (`median < BestMedian`).  The descriptor is COPIED into mp_desc[p].  A bad point, no observation or
// no good observer: nothing changes.  More than UP_MAX_DESC good observers: UP_DESC_OVERFLOW, the descriptor stays.
//
// MapPointCulling.  One verdict per entry of the recent list, the first matching row deciding: 1 already bad; 2
// (float)found / (float)visible < 0.25f as written (visible == 0 gives inf or NaN, which is not below); 3
// (int)cur - (int)first_kf >= 2 && nobs <= th (2 monocular, 3 otherwise); 4 (int)cur - (int)first_kf >= 3; 0 kept.  The kept
// entries are compacted in list order.  Nothing is applied and no verdict depends on another's.
#ifndef SLAMIT_UPKEEP_H
#define SLAMIT_UPKEEP_H
#include <stddef.h>
#include <stdint.h>

#include "local_map.h"
#include "unproject.h"

#define UP_MAX_OBS 512        // observers per point: a row is ordered in LDS (20 bytes per observer, upkeep.hip)
#define UP_MAX_DESC 128       // good observers per point in the descriptor pass = SLAMIT_DISTINCTIVE_MAX
#define UP_MAX_POINTS 65536   // listed points per call / per item
#define UP_MAX_RECENT 65536   // entries of a recent list
#define UP_KEY_SHIFT 10       // the order key of an observation: slot << 10 | position in the row (UP_MAX_OBS <= 1 << 10)

enum { UP_NORMAL = 1, UP_DESC = 2 };                                       // `what`
enum { UP_REF_NOT_OBSERVER = 1, UP_NO_REF = 2, UP_REF_NO_KP = 4, UP_OCTAVE = 8, UP_DESC_OVERFLOW = 16, UP_OBS_OVERFLOW = 32, UP_BAD_SLOT = 64 };
enum { UP_KEPT = 0, UP_WAS_BAD = 1, UP_LOW_RATIO = 2, UP_FEW_OBS = 3, UP_AGED = 4 };   // verdicts

struct UpIndex {
    int32_t n_levels, reserved;
    float scale_factors[UNP_MAX_LEVELS];
    const int32_t* obs_idx; const uint8_t* obs_octave; const uint8_t* kf_octave;
    const float* kf_center; const uint8_t* kf_desc;
    const int32_t* mp_ref_kf; const int32_t* mp_nobs; const int32_t* mp_found; const int32_t* mp_visible; const int32_t* mp_first_kf;
    float* mp_normal; float* mp_max_dist; float* mp_min_dist; uint8_t* mp_desc;
};

LM_HD uint32_t up_key(int slot, int pos) { return ((uint32_t)slot << UP_KEY_SHIFT) | (uint32_t)pos; }
LM_HD int up_key_slot(uint32_t key) { return (int)(key >> UP_KEY_SHIFT); }
LM_HD int up_key_pos(uint32_t key) { return (int)(key & ((1u << UP_KEY_SHIFT) - 1)); }

// :360-361 for one observer with camera centre Ow: what is added to the normal
LM_HD void up_contribution(const float* pos, const float* Ow, float c[3]) {
    const float d[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};
    const float inv = unp_mat_div(unp_norm3(d));
    c[0] = d[0] * inv; c[1] = d[1] * inv; c[2] = d[2] * inv;
}

// :365-369: the level of point p under reference keyframe mp_ref_kf[p], whose observation is entry o_ref of obs_kf (-1: it is not among
// the observers).  Returns the status bits; the level is usable when none of UP_NO_REF | UP_REF_NO_KP | UP_OCTAVE | UP_BAD_SLOT is set.
LM_HD int up_ref_level(const LmMap& M, const UpIndex& X, int ref, int o_ref, int& level) {
    level = 0;
    if (ref == -1) return UP_NO_REF;
    if (!lm_kf_ok(M, ref)) return UP_BAD_SLOT;
    int st = 0;
    if (o_ref >= 0) level = X.obs_octave[o_ref];
    else {
        st = UP_REF_NOT_OBSERVER;
        if (M.kf_mp_ptr[ref + 1] <= M.kf_mp_ptr[ref]) return st | UP_REF_NO_KP;
        level = X.kf_octave[M.kf_mp_ptr[ref]];
    }
    if (level >= X.n_levels || level >= UNP_MAX_LEVELS) st |= UP_OCTAVE;
    return st;
}

// :365-375 with the sum of :356-363 in `sum` over n observers: the three stores
LM_HD void up_store_normal(const LmMap& M, const UpIndex& X, int p, int ref, int level, const float sum[3], int n) {
    const float PC[3] = {M.mp_pos[3 * p] - X.kf_center[3 * ref], M.mp_pos[3 * p + 1] - X.kf_center[3 * ref + 1], M.mp_pos[3 * p + 2] - X.kf_center[3 * ref + 2]};
    const float dist = (float)unp_norm3(PC);
    const float max_dist = dist * X.scale_factors[level & (UNP_MAX_LEVELS - 1)];
    X.mp_max_dist[p] = max_dist;
    X.mp_min_dist[p] = max_dist / X.scale_factors[(X.n_levels - 1) & (UNP_MAX_LEVELS - 1)];
    const float inv_n = unp_mat_div((double)n);
    X.mp_normal[3 * p] = sum[0] * inv_n; X.mp_normal[3 * p + 1] = sum[1] * inv_n; X.mp_normal[3 * p + 2] = sum[2] * inv_n;
}

// is observation o of keyframe k a row of the descriptor pass?  (not bad, and its keypoint index inside the keyframe's row)
LM_HD bool up_desc_row(const LmMap& M, const UpIndex& X, int k, int o, int& status) {
    if (M.kf_bad[k]) return false;
    const int idx = X.obs_idx[o];
    if (idx < 0 || idx >= M.kf_mp_ptr[k + 1] - M.kf_mp_ptr[k]) { status |= UP_BAD_SLOT; return false; }
    return true;
}
LM_HD const uint8_t* up_desc_of(const LmMap& M, const UpIndex& X, int k, int o) { return X.kf_desc + 32 * ((size_t)M.kf_mp_ptr[k] + (size_t)X.obs_idx[o]); }

LM_HD int up_cull_verdict(const LmMap& M, const UpIndex& X, int p, int cur_id, bool monocular) {
    if (M.mp_bad[p]) return UP_WAS_BAD;
    if ((float)X.mp_found[p] / (float)X.mp_visible[p] < 0.25f) return UP_LOW_RATIO;
    const int age = (int)((uint32_t)cur_id - (uint32_t)X.mp_first_kf[p]);
    if (age >= 2 && X.mp_nobs[p] <= (monocular ? 2 : 3)) return UP_FEW_OBS;
    if (age >= 3) return UP_AGED;
    return UP_KEPT;
}

// ---- the sequential statement (host builds; the kernels do the same in parallel) ----------------------------------------------

// the valid observations of point p as keys in ascending (slot, position); keys holds UP_MAX_OBS.  -> their number
LM_HD int up_sorted_seq(const LmMap& M, int p, uint32_t* keys, int& status) {
    const int o0 = M.obs_ptr[p], n = M.obs_ptr[p + 1] - o0;
    int m = 0;
    for (int e = 0; e < n; ++e) {
        const int k = M.obs_kf[o0 + e];
        if (!lm_kf_ok(M, k)) { status |= UP_BAD_SLOT; continue; }
        const uint32_t key = up_key(k, e);
        int at = m++;
        for (; at > 0 && keys[at - 1] > key; --at) keys[at] = keys[at - 1];
        keys[at] = key;
    }
    return m;
}

LM_HD int up_hamming_seq(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 8; ++i) {   // a word at a time, as ORBmatcher::DescriptorDistance does
        uint32_t x, y;
        __builtin_memcpy(&x, a + 4 * i, 4); __builtin_memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

// ComputeDistinctiveDescriptors over rows[N] (pointers to 32 bytes): the index of the first row with the least median
LM_HD int up_select_seq(const uint8_t* const* rows, int N) {
    int best = 0, best_median = 0x7fffffff;
    const int at = (int)(0.5 * (N - 1));
    for (int i = 0; i < N; ++i) {
        int vDists[UP_MAX_DESC];   // the row, sorted as it is filled
        for (int j = 0; j < N; ++j) {
            const int d = i == j ? 0 : up_hamming_seq(rows[i], rows[j]);
            int e = j;
            for (; e > 0 && vDists[e - 1] > d; --e) vDists[e] = vDists[e - 1];
            vDists[e] = d;
        }
        const int median = vDists[at];
        if (median < best_median) { best_median = median; best = i; }
    }
    return best;
}

// one listed point.  keys[UP_MAX_OBS] and rows[UP_MAX_DESC] are scratch.  -> the status
LM_HD int up_point_seq(const LmMap& M, const UpIndex& X, int p, int what, uint32_t* keys, const uint8_t** rows) {
    if (!lm_mp_ok(M, p)) return UP_BAD_SLOT;
    const int o0 = M.obs_ptr[p], n_all = M.obs_ptr[p + 1] - o0;
    if (M.mp_bad[p] || n_all <= 0) return 0;
    if (n_all > UP_MAX_OBS) return UP_OBS_OVERFLOW;
    int status = 0;
    const int n = up_sorted_seq(M, p, keys, status);
    if (n == 0) return status;
    if (what & UP_NORMAL) {
        const int ref = X.mp_ref_kf[p];
        int o_ref = -1, level;
        for (int i = 0; i < n && o_ref < 0; ++i)
            if (up_key_slot(keys[i]) == ref) o_ref = o0 + up_key_pos(keys[i]);
        const int st = up_ref_level(M, X, ref, o_ref, level);
        status |= st;
        if (!(st & (UP_NO_REF | UP_REF_NO_KP | UP_OCTAVE | UP_BAD_SLOT))) {
            float sum[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < n; ++i) {
                float c[3];
                up_contribution(M.mp_pos + 3 * p, X.kf_center + 3 * up_key_slot(keys[i]), c);
                sum[0] = sum[0] + c[0]; sum[1] = sum[1] + c[1]; sum[2] = sum[2] + c[2];
            }
            up_store_normal(M, X, p, ref, level, sum, n);
        }
    }
    if (what & UP_DESC) {
        int N = 0;
        for (int i = 0; i < n; ++i) {
            const int k = up_key_slot(keys[i]), o = o0 + up_key_pos(keys[i]);
            if (!up_desc_row(M, X, k, o, status)) continue;
            if (N < UP_MAX_DESC) rows[N] = up_desc_of(M, X, k, o);
            ++N;
        }
        if (N > UP_MAX_DESC) status |= UP_DESC_OVERFLOW;
        else if (N > 0) {
            const uint8_t* const src = rows[up_select_seq(rows, N)];
            for (int b = 0; b < 32; ++b) X.mp_desc[32 * (size_t)p + b] = src[b];
        }
    }
    return status;
}

// the listed points one after the other; status[n] is written in full
LM_HD void up_points_seq(const LmMap& M, const UpIndex& X, int n, const int32_t* points, int what, int32_t* status, uint32_t* keys, const uint8_t** rows) {
    for (int j = 0; j < n; ++j) status[j] = up_point_seq(M, X, points[j], what, keys, rows);
}

// MapPointCulling over recent[n]: verdict[n] (an entry outside the table keeps its byte and is dropped, UP_BAD_SLOT), kept[*n_kept]
LM_HD void up_culling_seq(const LmMap& M, const UpIndex& X, int cur_id, bool monocular, int n, const int32_t* recent, uint8_t* verdict, int32_t* kept,
                          int32_t* n_kept, int& status) {
    int m = 0;
    for (int j = 0; j < n; ++j) {
        const int p = recent[j];
        if (!lm_mp_ok(M, p)) { status |= UP_BAD_SLOT; continue; }
        const int v = up_cull_verdict(M, X, p, cur_id, monocular);
        verdict[j] = (uint8_t)v;
        if (v == UP_KEPT) kept[m++] = p;
    }
    *n_kept = m;
}

#endif
