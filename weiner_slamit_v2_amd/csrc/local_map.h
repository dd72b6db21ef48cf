// local_map.h — Tracking::UpdateLocalMap (ORB_SLAM2/src/Tracking.cc:1467-1626) over slot-numbered tables: UpdateLocalKeyFrames
// (:1512-1626), UpdateLocalPoints (:1477-1509) and the skip flags of SearchLocalPoints' first loop (:1412-1428, :1436).  Everything
// here is integer work or a copy of a stored float, so there is no tolerance anywhere: the device equals this text exactly.
// One header for host and device: local_map.hip runs the votes, the compaction and the point passes in parallel and calls
// lm_expand (the sequential neighbour walk) from lane 0; the CPU test of the restatement, the shim's test driver and
// tools/bench_local_map.py build the *_seq functions with g++.
//
// TABLES (LmMap, the layout of slamit_map_index).  Every id is a slot, -1 = none.  obs_ptr / obs_kf: the keyframes observing point
// p (MapPoint::GetObservations, order free: votes are integer sums).  kf_mp_ptr / kf_mp: KeyFrame::GetMapPointMatches by keypoint
// index, -1 for NULL.  kf_best: the first ten of mvpOrderedConnectedKeyFrames, padded with -1.  kf_child_ptr / kf_child: the
// children in the order given.  kf_parent.  The CSR pointer arrays are trusted to ascend; every SLOT read from a table or a frame
// is range-checked before it indexes anything: one outside its table is skipped and sets LM_BAD_SLOT in the frame's status.
//
// ORDER.  The reference iterates std::map<KeyFrame*, int> and std::set<KeyFrame*>, i.e. in ADDRESS order, which differs from run to
// run.  Here: voted keyframes in ASCENDING SLOT order, children AS GIVEN.  A caller that numbers the keyframes it passes by
// std::less<KeyFrame*> and lists children in set order (shim/Tracking.h does) gets the reference's own order on that run.
//
// THE REFERENCE'S ODD PLACES, all kept:
//   no keyframe got a vote     :1540 returns BEFORE clear(): the list, its size and the reference keyframe stay as they were
//   every voted keyframe bad   the list is cleared and stays empty; pKFmax is NULL, so the reference keyframe is unchanged
//   the maximum                `it->second > max`, strictly: the first keyframe in the order above with the largest count
//   the expansion loop         its end iterator is taken before the pushes: it visits the voted, non-bad entries only, and
//                              leaves at the first visit that finds more than 80 in the list (so 81..83 are possible)
//   per visited entry          the first non-bad unmarked of the best ten, the first non-bad unmarked child, then the parent when
//                              it is unmarked -- WITHOUT a bad test -- and that `break` (:1615) leaves the OUTER loop
//   local points               keyframes in list order, keypoints in index order, NULL and bad points dropped, first occurrence
//                              kept: SearchByProjection is greedy in this order
//   skip                       a local point is skipped by SearchLocalPoints when its mnLastFrameSeen is the frame's id: it is one of
//                              the frame's own non-null, non-bad points (:1424) or was marked earlier (frame_seen: the outliers of
//                              :1015 and :1146)
//
// THE KEY.  The parallel form finds "first occurrence" as the minimum of (position in the keyframe list << 16) | keypoint index
// over every occurrence of a point, so both fields are 16 bits: at most LM_MAX_KF keyframes in a list (LM_KEY_NONE stays free)
// and 65536 keypoints per keyframe (a longer row is cut there and sets LM_ROW_CUT).
#ifndef SLAMIT_LOCAL_MAP_H
#define SLAMIT_LOCAL_MAP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_HD __host__ __device__ __forceinline__
#else
#define LM_HD static inline
#endif

#define LM_BEST 10            // GetBestCovisibilityKeyFrames(10)
#define LM_LIMIT 80           // mvpLocalKeyFrames.size() > 80
#define LM_MIN_KF_CAP 83      // a list the expansion touches holds at most 80 + 3: with this much room the walk never overflows
#define LM_MAX_KF 65535       // keyframes per map and per list: the key's upper field
#define LM_MAX_ROW 65536      // keypoints per keyframe: the key's lower field
#define LM_KEY_NONE 0xffffffffu

enum { LM_BAD_SLOT = 1, LM_KF_OVERFLOW = 2, LM_MP_OVERFLOW = 4, LM_ROW_CUT = 8 };

struct LmMap {
    int32_t n_kf, n_mp;
    const int32_t* obs_ptr; const int32_t* obs_kf;
    const uint8_t* mp_bad; const uint8_t* kf_bad;
    const int32_t* kf_mp_ptr; const int32_t* kf_mp;
    const int32_t* kf_best;
    const int32_t* kf_child_ptr; const int32_t* kf_child;
    const int32_t* kf_parent;
    const float* mp_pos; const float* mp_normal; const float* mp_max_dist; const float* mp_min_dist;
};

LM_HD bool lm_kf_ok(const LmMap& M, int k) { return (unsigned)k < (unsigned)M.n_kf; }
LM_HD bool lm_mp_ok(const LmMap& M, int p) { return (unsigned)p < (unsigned)M.n_mp; }
LM_HD int lm_list_n(int n, int cap) { n = n > 0 ? n : 0; return n < cap ? n : cap; }   // a list's length as the device reads it: n clamped to [0, cap]
LM_HD uint32_t lm_key(int list_pos, int kp) { return ((uint32_t)list_pos << 16) | (uint32_t)kp; }

// mnTrackReferenceForFrame == mCurrentFrame.mnId of the keyframes, as a bit per slot
LM_HD bool lm_marked(const uint32_t* marks, int k) { return (marks[k >> 5] >> (k & 31)) & 1u; }
LM_HD void lm_mark(uint32_t* marks, int k) { marks[k >> 5] |= 1u << (k & 31); }

LM_HD void lm_push_kf(int32_t* local_kf, int& n, int kf_cap, uint32_t* marks, int k, int& status) {
    if (n < kf_cap) local_kf[n] = k; else status |= LM_KF_OVERFLOW;
    ++n;
    lm_mark(marks, k);
}

// :1569-1619.  local_kf[0 .. n_voted) are the voted, non-bad keyframes, all marked; returns the size of the list afterwards.
LM_HD int lm_expand(const LmMap& M, int32_t* local_kf, int n_voted, int kf_cap, uint32_t* marks, int& status) {
    int n = n_voted;
    for (int it = 0; it < n_voted && it < kf_cap; ++it) {
        if (n > LM_LIMIT) break;
        const int k = local_kf[it];
        for (int b = 0; b < LM_BEST; ++b) {
            const int nb = M.kf_best[k * LM_BEST + b];
            if (nb == -1) continue;
            if (!lm_kf_ok(M, nb)) { status |= LM_BAD_SLOT; continue; }
            if (!M.kf_bad[nb] && !lm_marked(marks, nb)) { lm_push_kf(local_kf, n, kf_cap, marks, nb, status); break; }
        }
        for (int e = M.kf_child_ptr[k]; e < M.kf_child_ptr[k + 1]; ++e) {
            const int c = M.kf_child[e];
            if (!lm_kf_ok(M, c)) { status |= LM_BAD_SLOT; continue; }
            if (!M.kf_bad[c] && !lm_marked(marks, c)) { lm_push_kf(local_kf, n, kf_cap, marks, c, status); break; }
        }
        const int par = M.kf_parent[k];
        if (par != -1) {
            if (!lm_kf_ok(M, par)) status |= LM_BAD_SLOT;
            else if (!lm_marked(marks, par)) { lm_push_kf(local_kf, n, kf_cap, marks, par, status); break; }
        }
    }
    return n;
}

// ---- the sequential statement of the three passes (host builds; the kernels do the same in parallel) ---------------------------

// (a) :1518-1538.  votes[n_kf] is written in full; a bad point's entry of frame_mp becomes -1.
LM_HD void lm_votes_seq(const LmMap& M, int n, int32_t* frame_mp, int32_t* votes, int& status) {
    for (int k = 0; k < M.n_kf; ++k) votes[k] = 0;
    for (int i = 0; i < n; ++i) {
        const int p = frame_mp[i];
        if (p == -1) continue;
        if (!lm_mp_ok(M, p)) { status |= LM_BAD_SLOT; continue; }
        if (M.mp_bad[p]) { frame_mp[i] = -1; continue; }
        for (int e = M.obs_ptr[p]; e < M.obs_ptr[p + 1]; ++e) {
            const int k = M.obs_kf[e];
            if (!lm_kf_ok(M, k)) { status |= LM_BAD_SLOT; continue; }
            ++votes[k];
        }
    }
}

// (b) :1540-1625.  local_kf[kf_cap], n_local_kf and ref_kf are in / out; marks holds (n_kf + 31) / 32 words.  n_local_kf reports
// the size the list needs; beyond kf_cap (>= LM_MIN_KF_CAP) nothing is written and the status says LM_KF_OVERFLOW.
LM_HD void lm_keyframes_seq(const LmMap& M, const int32_t* votes, int kf_cap, int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf,
                            uint32_t* marks, int& status) {
    bool any = false;
    for (int k = 0; k < M.n_kf; ++k) any = any || votes[k] > 0;
    if (!any) return;
    for (int w = 0; w < (M.n_kf + 31) / 32; ++w) marks[w] = 0;
    int n = 0, max = 0, kmax = -1;
    for (int k = 0; k < M.n_kf; ++k) {
        if (votes[k] <= 0 || M.kf_bad[k]) continue;
        if (votes[k] > max) { max = votes[k]; kmax = k; }
        lm_push_kf(local_kf, n, kf_cap, marks, k, status);
    }
    *n_local_kf = lm_expand(M, local_kf, n, kf_cap, marks, status);
    if (kmax >= 0) *ref_kf = kmax;
}

// (c) :1477-1509 and the skip flags.  keys[n_mp] and seen[n_mp] are scratch.  Outputs are written for the first min(needed, q_cap)
// points only; *n_local_mp is the number needed.  The planes (coordinate c of point r at pos[c * q_cap + r]) may be null together.
LM_HD void lm_points_seq(const LmMap& M, int n, const int32_t* frame_mp, int n_seen, const int32_t* frame_seen, int n_local_kf,
                         const int32_t* local_kf, int q_cap, uint32_t* keys, uint8_t* seen, int32_t* local_mp, uint8_t* skip,
                         float* pos, float* normal, float* max_dist, float* min_dist, int32_t* n_local_mp, int& status) {
    for (int p = 0; p < M.n_mp; ++p) { keys[p] = LM_KEY_NONE; seen[p] = 0; }
    for (int i = 0; i < n; ++i) {
        const int p = frame_mp[i];
        if (p == -1) continue;
        if (!lm_mp_ok(M, p)) { status |= LM_BAD_SLOT; continue; }
        if (!M.mp_bad[p]) seen[p] = 1;
    }
    for (int i = 0; i < n_seen; ++i) {
        const int p = frame_seen[i];
        if (p == -1) continue;
        if (!lm_mp_ok(M, p)) { status |= LM_BAD_SLOT; continue; }
        seen[p] = 1;
    }
    int m = 0;
    for (int j = 0; j < n_local_kf; ++j) {
        const int k = local_kf[j];
        if (!lm_kf_ok(M, k)) { status |= LM_BAD_SLOT; continue; }
        int len = M.kf_mp_ptr[k + 1] - M.kf_mp_ptr[k];
        if (len > LM_MAX_ROW) { len = LM_MAX_ROW; status |= LM_ROW_CUT; }
        for (int i = 0; i < len; ++i) {
            const int p = M.kf_mp[M.kf_mp_ptr[k] + i];
            if (p == -1) continue;
            if (!lm_mp_ok(M, p)) { status |= LM_BAD_SLOT; continue; }
            if (keys[p] != LM_KEY_NONE || M.mp_bad[p]) continue;
            keys[p] = lm_key(j, i);
            if (m < q_cap) {
                local_mp[m] = p; skip[m] = seen[p];
                if (pos) {
                    for (int c = 0; c < 3; ++c) { pos[c * q_cap + m] = M.mp_pos[3 * p + c]; normal[c * q_cap + m] = M.mp_normal[3 * p + c]; }
                    max_dist[m] = M.mp_max_dist[p]; min_dist[m] = M.mp_min_dist[p];
                }
            }
            ++m;
        }
    }
    if (m > q_cap) status |= LM_MP_OVERFLOW;
    *n_local_mp = m;
}

#endif
