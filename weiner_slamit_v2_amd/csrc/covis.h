// covis.h — KeyFrame::UpdateConnections (ORB_SLAM2/src/KeyFrame.cc:296-386, with AddConnection / UpdateBestCovisibles :127-161) and
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:686-752) over the slot tables of local_map.h plus the columns of CvIndex (the
// layout of slamit_covis_index).  Integer work and float compares as the reference writes them: no tolerance anywhere, the device
// equals this text exactly.  One header for host and device: covis.hip runs the walks in parallel and calls the per-element
// functions below; the CPU tests, the shim's test driver and tools/bench_covis.py build the *_seq functions with g++.
//
// THE GRAPH.  Keyframe j's mConnectedKeyFrameWeights is row j of cw_kf / cw_w (cw_n[j] entries, ASCENDING SLOT: the order of a
// std::map<KeyFrame*, int> when slots are numbered by address); mvpOrderedConnectedKeyFrames / mvOrderedWeights are row j of ord_kf /
// ord_w (ord_n[j] entries).  Rows hold row_cap entries; what lies past a row's count is never read and never written.
//
// THE ORDER of an ordered row is the reference's sort of (weight, pointer) pushed to the front: DESCENDING weight, and within equal
// weight DESCENDING slot.  As one key, cv_key = weight << 32 | slot, descending.  Keys of one row are distinct (slots are), so the
// position of an entry is the number of keys above its own: cv_rank.  The sequential and the parallel form place every entry by that
// count, so they cannot differ.
//
// UpdateConnections, THE REFERENCE'S ODD PLACES, all kept:
//   a bad observer is counted       :322-327 test the point, never the observing keyframe
//   no observer at all              :331 returns: every row, kf_best and the parent stay; CV_NO_OBSERVER
//   nobody reaches 15               the single keyframe with the strictly largest count (`>`), first in ascending slot order
//   the neighbour's ordered row     AddConnection -> UpdateBestCovisibles lists j's WHOLE cw row, below-threshold entries included,
//                                   while k's own ordered row holds the thresholded list only
//   the neighbour that holds (k, w) returns before UpdateBestCovisibles: nothing of j changes
//   the parent                      the front of k's list when first_connection is set and k is not the origin, else -1; the
//                                   parent and children TABLES stay the caller's (a CSR cannot take an insert)
//
// KeyFrameCulling.  The candidates are the current keyframe's ordered row, in row order.  SetBadFlag on a culled keyframe erases its
// observations before the next candidate is looked at; here that is a function of the set S of keyframes culled so far in the call
// (a bit per slot) and of the tables, which are not modified:
//   an observer in S                is not there
//   Observations()                  mp_nobs[p] - sum of obs_weight over p's observers in S
//   a point that lost an observer and is left with <= 2 is bad (MapPoint::EraseObservation -> SetBadFlag)
//   a candidate with kf_not_erase   verdict CV_TO_BE_ERASED: SetBadFlag returns before it erases anything, it does not enter S
// The test itself is float and double compares as written: depth > th || depth < 0 (so a NaN depth passes), nRedundant > 0.9 * nMPs.
#ifndef SLAMIT_COVIS_H
#define SLAMIT_COVIS_H
#include <stddef.h>
#include <stdint.h>

#include "local_map.h"

#define CV_TH 15              // UpdateConnections' th
#define CV_OBS 3              // KeyFrameCulling's thObs
#define CV_MAX_ROW 1024       // entries per graph row: the rows are sorted in LDS

enum { CV_NO_OBSERVER = 1, CV_ROW_OVERFLOW = 2, CV_BAD_SLOT = 4 };
enum { CV_KEPT = 0, CV_CULLED = 1, CV_TO_BE_ERASED = 2, CV_ORIGIN = 3 };   // verdicts
enum { CV_COUNTS = 1, CV_REDUNDANT = 2 };                                   // cv_eval_point

struct CvIndex {
    int32_t row_cap, origin_kf;
    const uint8_t* obs_octave; const uint8_t* obs_weight; const int32_t* mp_nobs;
    const uint8_t* kf_octave; const float* kf_depth; const float* kf_th_depth; const uint8_t* kf_not_erase;
    int32_t* cw_kf; int32_t* cw_w; int32_t* cw_n;
    int32_t* ord_kf; int32_t* ord_w; int32_t* ord_n;
    int32_t* kf_best;
};

LM_HD int cv_clamp(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }
LM_HD unsigned long long cv_key(int w, int slot) { return ((unsigned long long)(uint32_t)w << 32) | (uint32_t)slot; }
LM_HD int cv_rank(const unsigned long long* keys, int n, unsigned long long key) {
    int r = 0;
    for (int e = 0; e < n; ++e) r += keys[e] > key;
    return r;
}
// entry i of keys[n] goes to its place in the ordered row of keyframe j and, among the first ten, in j's kf_best row
LM_HD void cv_place(const CvIndex& X, int j, const unsigned long long* keys, int n, int i) {
    const int r = cv_rank(keys, n, keys[i]);
    X.ord_kf[(size_t)j * X.row_cap + r] = (int32_t)(uint32_t)keys[i];
    X.ord_w[(size_t)j * X.row_cap + r] = (int32_t)(keys[i] >> 32);
    if (X.kf_best && r < LM_BEST) X.kf_best[(size_t)j * LM_BEST + r] = (int32_t)(uint32_t)keys[i];
}
// the padding of j's kf_best row behind a list of n: entry b of the ten
LM_HD void cv_pad_best(const CvIndex& X, int j, int n, int b) {
    if (X.kf_best && b >= n) X.kf_best[(size_t)j * LM_BEST + b] = -1;
}

// ---- KeyFrameCulling: one keypoint of candidate `cand` -- entry e of kf_mp -- against the culled set S (null = empty) --------
// -> 0, CV_COUNTS (in nMPs) or CV_COUNTS | CV_REDUNDANT
LM_HD int cv_eval_point(const LmMap& M, const CvIndex& X, int cand, int e, bool monocular, const uint32_t* S, int& status) {
    const int p = M.kf_mp[e];
    if (p == -1) return 0;
    if (!lm_mp_ok(M, p)) { status |= CV_BAD_SLOT; return 0; }
    if (M.mp_bad[p]) return 0;
    const int o0 = M.obs_ptr[p], o1 = M.obs_ptr[p + 1];
    int nobs = X.mp_nobs[p];
    if (S) {
        bool lost = false;
        for (int o = o0; o < o1; ++o) {
            const int kf = M.obs_kf[o];
            if (lm_kf_ok(M, kf) && lm_marked(S, kf)) { nobs -= X.obs_weight[o]; lost = true; }
        }
        if (lost && nobs <= 2) return 0;   // EraseObservation made it bad
    }
    if (!monocular) {
        const float d = X.kf_depth[e];
        if (d > X.kf_th_depth[cand] || d < 0) return 0;
    }
    if (!(nobs > CV_OBS)) return CV_COUNTS;
    const int level = X.kf_octave[e];
    int n = 0;
    for (int o = o0; o < o1; ++o) {
        const int kf = M.obs_kf[o];
        if (!lm_kf_ok(M, kf)) { status |= CV_BAD_SLOT; continue; }
        if (kf == cand || (S && lm_marked(S, kf))) continue;
        if ((int)X.obs_octave[o] <= level + 1 && ++n >= CV_OBS) break;
    }
    return n >= CV_OBS ? (CV_COUNTS | CV_REDUNDANT) : CV_COUNTS;
}
LM_HD int cv_verdict(const CvIndex& X, int cand, int n_mps, int n_redundant) {
    if (!((double)n_redundant > 0.9 * (double)n_mps)) return CV_KEPT;
    return X.kf_not_erase[cand] ? CV_TO_BE_ERASED : CV_CULLED;
}
// after the walk: did the culled set S turn point p bad?
LM_HD bool cv_turned_bad(const LmMap& M, const CvIndex& X, int p, const uint32_t* S) {
    if (M.mp_bad[p]) return false;
    int nobs = X.mp_nobs[p];
    bool lost = false;
    for (int o = M.obs_ptr[p]; o < M.obs_ptr[p + 1]; ++o) {
        const int kf = M.obs_kf[o];
        if (lm_kf_ok(M, kf) && lm_marked(S, kf)) { nobs -= X.obs_weight[o]; lost = true; }
    }
    return lost && nobs <= 2;
}

// ---- the sequential statement (host builds; the kernels do the same in parallel) ----------------------------------------------

// (a) :307-328.  counts[n_kf] is written in full.
LM_HD void cv_counts_seq(const LmMap& M, int k, int32_t* counts, int& status) {
    for (int j = 0; j < M.n_kf; ++j) counts[j] = 0;
    if (!lm_kf_ok(M, k)) { status |= CV_BAD_SLOT; return; }
    for (int e = M.kf_mp_ptr[k]; e < M.kf_mp_ptr[k + 1]; ++e) {
        const int p = M.kf_mp[e];
        if (p == -1) continue;
        if (!lm_mp_ok(M, p)) { status |= CV_BAD_SLOT; continue; }
        if (M.mp_bad[p]) continue;
        for (int o = M.obs_ptr[p]; o < M.obs_ptr[p + 1]; ++o) {
            const int j = M.obs_kf[o];
            if (!lm_kf_ok(M, j)) { status |= CV_BAD_SLOT; continue; }
            if (j != k) ++counts[j];
        }
    }
}

// AddConnection(k, w) on keyframe j, :127-161.  keys[row_cap] is scratch.
LM_HD void cv_add_connection_seq(const CvIndex& X, int j, int k, int w, unsigned long long* keys, int& status) {
    int32_t* const ckf = X.cw_kf + (size_t)j * X.row_cap;
    int32_t* const cw = X.cw_w + (size_t)j * X.row_cap;
    int n = cv_clamp(X.cw_n[j], X.row_cap), pos = 0;
    while (pos < n && ckf[pos] < k) ++pos;
    if (pos < n && ckf[pos] == k) {
        if (cw[pos] == w) return;
        cw[pos] = w;
    } else {
        if (n == X.row_cap) { status |= CV_ROW_OVERFLOW; return; }
        for (int e = n; e > pos; --e) { ckf[e] = ckf[e - 1]; cw[e] = cw[e - 1]; }
        ckf[pos] = k; cw[pos] = w;
        X.cw_n[j] = ++n;
    }
    for (int e = 0; e < n; ++e) keys[e] = cv_key(cw[e], ckf[e]);
    for (int e = 0; e < n; ++e) cv_place(X, j, keys, n, e);
    for (int b = 0; b < LM_BEST; ++b) cv_pad_best(X, j, n, b);
    X.ord_n[j] = n;
}

// (b)-(f) :330-385 from the counts of (a).  *n_counted is the size of the counter (0 with CV_NO_OBSERVER; above row_cap with
// CV_ROW_OVERFLOW, and then nothing else is written); *n_listed the length of k's new list, 0 when nothing was done; *parent is
// written when the list is.
LM_HD void cv_connections_seq(const LmMap& M, const CvIndex& X, int k, bool first_connection, const int32_t* counts, int32_t* n_counted,
                              int32_t* n_listed, int32_t* parent, unsigned long long* keys, unsigned long long* keys_j, int& status) {
    *n_listed = 0; *n_counted = 0;
    if (!lm_kf_ok(M, k)) { status |= CV_BAD_SLOT; return; }
    int nc = 0, nl = 0, nmax = 0, kmax = -1;
    for (int j = 0; j < M.n_kf; ++j) {
        if (counts[j] <= 0) continue;
        ++nc;
        if (counts[j] > nmax) { nmax = counts[j]; kmax = j; }
        if (counts[j] >= CV_TH) ++nl;
    }
    *n_counted = nc;
    if (nc == 0) { status |= CV_NO_OBSERVER; return; }
    if (nc > X.row_cap) { status |= CV_ROW_OVERFLOW; return; }
    int c = 0;
    nl = 0;
    for (int j = 0; j < M.n_kf; ++j) {
        if (counts[j] <= 0) continue;
        X.cw_kf[(size_t)k * X.row_cap + c] = j; X.cw_w[(size_t)k * X.row_cap + c] = counts[j];
        ++c;
        if (counts[j] >= CV_TH) keys[nl++] = cv_key(counts[j], j);
    }
    X.cw_n[k] = nc;
    if (nl == 0) keys[nl++] = cv_key(nmax, kmax);
    for (int e = 0; e < nl; ++e) cv_add_connection_seq(X, (int)(uint32_t)keys[e], k, (int)(keys[e] >> 32), keys_j, status);
    for (int e = 0; e < nl; ++e) cv_place(X, k, keys, nl, e);
    for (int b = 0; b < LM_BEST; ++b) cv_pad_best(X, k, nl, b);
    X.ord_n[k] = nl;
    *n_listed = nl;
    *parent = first_connection && k != X.origin_kf ? X.ord_kf[(size_t)k * X.row_cap] : -1;
}

// KeyFrameCulling for current keyframe c.  verdict / n_mps / n_redundant hold cand_cap >= row_cap entries, the first *n_cand are
// written; mp_turned_bad[n_mp]: bytes set to 1, the others left alone; S holds (n_kf + 31) / 32 words of scratch.
LM_HD void cv_culling_seq(const LmMap& M, const CvIndex& X, int c, bool monocular, uint8_t* verdict, int32_t* n_mps, int32_t* n_redundant,
                          int32_t* n_cand, uint8_t* mp_turned_bad, uint32_t* S, int& status) {
    *n_cand = 0;
    if (!lm_kf_ok(M, c)) { status |= CV_BAD_SLOT; return; }
    const int n = cv_clamp(X.ord_n[c], X.row_cap);
    *n_cand = n;
    for (int w = 0; w < (M.n_kf + 31) / 32; ++w) S[w] = 0;
    bool any = false;
    for (int t = 0; t < n; ++t) {
        const int cand = X.ord_kf[(size_t)c * X.row_cap + t];
        int v = CV_KEPT, nm = 0, nr = 0;
        if (!lm_kf_ok(M, cand)) status |= CV_BAD_SLOT;
        else if (cand == X.origin_kf) v = CV_ORIGIN;
        else {
            for (int e = M.kf_mp_ptr[cand]; e < M.kf_mp_ptr[cand + 1]; ++e) {
                const int r = cv_eval_point(M, X, cand, e, monocular, any ? S : (const uint32_t*)0, status);
                nm += r & CV_COUNTS; nr += (r & CV_REDUNDANT) != 0;
            }
            v = cv_verdict(X, cand, nm, nr);
            if (v == CV_CULLED) { lm_mark(S, cand); any = true; }
        }
        verdict[t] = (uint8_t)v; n_mps[t] = nm; n_redundant[t] = nr;
    }
    if (any)
        for (int p = 0; p < M.n_mp; ++p)
            if (cv_turned_bad(M, X, p, S)) mp_turned_bad[p] = 1;
}

#endif
