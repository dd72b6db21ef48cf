// map_edit.h — the point-side writers of the map over the slot tables of local_map.h: MapPoint::AddObservation, ::EraseObservation and
// ::SetBadFlag (ORB_SLAM2/src/MapPoint.cc:104-174) with KeyFrame::AddMapPoint / ::EraseMapPointMatch (src/KeyFrame.cc:215-243) as their
// callers pair them (Optimizer.cc:750-757, LocalMapping.cc ProcessNewKeyFrame / MapPointCulling / CreateNewMapPoints, ORBmatcher.cc
// Fuse).  An edit list is applied AS IF SEQUENTIALLY IN LIST ORDER; everything is integer work, so the device equals this text exactly.
// One header for host and device: me_walk is the walk of one point's edits, stated once over a row policy (MeRowSeq below: plain
// loops; map_edit.hip: the row in LDS, membership by wave ballot) and an emitter of kf_mp writes.  The CPU test of the restatement
// and tools/bench_map_edit.py build me_apply_seq with g++.
//
// THE EDITS, line by line.
//   ADD_OBS    :107 an observer that is present changes nothing of the point.  Else (kf, idx, octave, weight) is appended to the row
//              and nobs += weight (:111-114: 2 where mvuRight[idx] >= 0).  No bad test, as in the reference.  With MATCH also
//              KeyFrame::AddMapPoint: kf_mp[kf][idx] = mp, UNCONDITIONAL (Fuse and CreateNewMapPoints call both whatever the first did).
//   ERASE_OBS  with MATCH first KeyFrame::EraseMapPointMatch(MapPoint*): when the point holds kf at index i, kf_mp[kf][i] = -1.  Then
//              :122-138: when kf is an observer nobs -= its weight, the entry goes; mpRefKF == kf becomes mObservations.begin(), the
//              remaining observer with the SMALLEST SLOT (std::map<KeyFrame*, size_t> order for a caller that numbers keyframes by
//              address); nobs <= 2 runs SetBadFlag.  Not an observer: nothing.
//   SET_BAD    :157-174 bad = 1, kf_mp[k][i] = -1 for every observation (k, i) BY INDEX whatever is stored there, the row is emptied.
//              nobs stays, as in the reference.  Map::EraseMapPoint is the caller's (the set of points is not a table).
// STATED DEPARTURE, where the reference reads end(): erasing the reference keyframe as the last observer sets mp_ref_kf = -1 and ME_REF_END.
//
// WHY IT IS PARALLEL.  (1) A point's row, nobs, bad and ref_kf after the list depend only on that point's own edits in list order.
// (2) Every write to kf_mp is unconditional and determined by the issuing point's state at that edit (a cascaded SetBadFlag carries the
// list index of its ERASE_OBS), so kf_mp[kf][idx] after the list is the value of the write with the LARGEST LIST INDEX.  MapPoint::Replace
// reads a second point's observers (breaks 1) and KeyFrame::SetBadFlag walks the spanning tree sequentially: neither is here.
//
// THE NEW ROW is the old row's order with erased entries closed up and added ones appended in list order.  The walk keeps erased
// entries in place as dead ones (a physical row of at most ME_MAX_OBS + ME_MAX_PER_POINT entries) and closes up when it writes.
// LIMITS: more than ME_MAX_PER_POINT edits of one point in a list: NONE of them is applied, ME_EDIT_OVERFLOW.  A row above ME_MAX_OBS on
// input, or an add onto a row of ME_MAX_OBS live entries: none applied, ME_OBS_OVERFLOW (and only that bit).  TOUCHED: a point of which
// at least one edit appended or removed an entry.
#ifndef SLAMIT_MAP_EDIT_H
#define SLAMIT_MAP_EDIT_H
#include <stddef.h>
#include <stdint.h>

#include "local_map.h"

#define ME_MAX_PER_POINT 64    // edits of one point in one list: a bucket is ordered by one wavefront
#define ME_MAX_OBS 512         // observers per point = UP_MAX_OBS
#define ME_MAX_EDITS (1 << 20) // edits per list
#define ME_ROW (ME_MAX_OBS + ME_MAX_PER_POINT)   // the physical row of the walk
#define ME_SCAN_BLOCK 256      // entries per workgroup of the device scan

enum { ME_ADD_OBS = 1, ME_ERASE_OBS = 2, ME_SET_BAD = 3 };   // kind
enum { ME_MATCH = 1 };                                       // flags
enum { ME_REF_END = 1, ME_EDIT_OVERFLOW = 2, ME_OBS_OVERFLOW = 4, ME_BAD_SLOT = 8, ME_TABLE_OVERFLOW = 16 };

struct MeEdit {
    int32_t kind, flags, mp, kf, idx;
    uint8_t octave, weight, pad[2];
};

struct MeIndex {   // the layout of slamit_edit_index
    const int32_t* obs_idx; const uint8_t* obs_octave; const uint8_t* obs_weight;
    uint8_t* mp_bad; int32_t* mp_nobs; int32_t* mp_ref_kf; int32_t* kf_mp;
    int32_t* obs_ptr_out; int32_t* obs_kf_out; int32_t* obs_idx_out; uint8_t* obs_octave_out; uint8_t* obs_weight_out;
    int32_t obs_cap_out, reserved;
};

struct MeState { int32_t live, nobs, bad, ref, status, changed; };

// is the edit one the walk can apply?  (kind; for an add the keyframe, the keypoint index inside its row and the weight; for an erase
// the keyframe.  SET_BAD reads neither.)
LM_HD bool me_edit_ok(const LmMap& M, const MeEdit& e) {
    if (e.kind == ME_SET_BAD) return true;
    if (e.kind != ME_ADD_OBS && e.kind != ME_ERASE_OBS) return false;
    if (!lm_kf_ok(M, e.kf)) return false;
    if (e.kind == ME_ERASE_OBS) return true;
    return e.idx >= 0 && e.idx < M.kf_mp_ptr[e.kf + 1] - M.kf_mp_ptr[e.kf] && (e.weight == 1 || e.weight == 2);
}

// where (k, i) lies in kf_mp, -1 for a pair outside the table (an observation the caller's table holds wrongly: skipped, ME_BAD_SLOT)
LM_HD long long me_kfmp_at(const LmMap& M, int k, int i) {
    if (!lm_kf_ok(M, k)) return -1;
    if (i < 0 || i >= M.kf_mp_ptr[k + 1] - M.kf_mp_ptr[k]) return -1;
    return (long long)M.kf_mp_ptr[k] + i;
}

// SetBadFlag with the list index of the edit that runs it
template <class Row, class Emit>
LM_HD void me_set_bad(Row& r, MeState& s, Emit& emit, int li) {
    s.bad = 1;
    r.emit_live(emit, li);        // kf_mp[k][i] = -1 for every live (k, i)
    if (s.live > 0) s.changed = 1;
    r.clear();
    s.live = 0;
}

// The ne edits of point p, edits[order[0]], edits[order[1]], ... with order ascending (list order), over the row r and the state s.
// Row: find(kf) -> the physical position of the live entry of kf or -1, idx_at / weight_at(pos), push(kf, idx, octave, weight),
// kill(pos), min_slot() -> the smallest slot among the live entries or -1, emit_live(emit, li), clear(), uniform(v) -> v (the device
// policy says there that v is the same in every lane).  Emit: one(kf, idx, value, li).
// Leaves at once with ME_OBS_OVERFLOW when an add meets ME_MAX_OBS live entries: the caller then discards r and s.
template <class Row, class Emit>
LM_HD void me_walk(const LmMap& M, int p, Row& r, MeState& s, const MeEdit* edits, const int32_t* order, int ne, Emit& emit) {
    for (int j = 0; j < ne; ++j) {
        const int li = r.uniform(order[j]);
        const MeEdit e = edits[li];
        if (!me_edit_ok(M, e)) { s.status |= ME_BAD_SLOT; continue; }
        if (e.kind == ME_ADD_OBS) {
            if (r.find(e.kf) < 0) {
                if (s.live >= ME_MAX_OBS) { s.status = ME_OBS_OVERFLOW; return; }
                r.push(e.kf, e.idx, e.octave, e.weight);
                ++s.live; s.nobs += e.weight; s.changed = 1;
            }
            if (e.flags & ME_MATCH) emit.one(e.kf, e.idx, p, li);
        } else if (e.kind == ME_ERASE_OBS) {
            const int pos = r.find(e.kf);
            if (pos < 0) continue;
            if (e.flags & ME_MATCH) emit.one(e.kf, r.idx_at(pos), -1, li);
            s.nobs -= r.weight_at(pos);
            r.kill(pos);
            --s.live; s.changed = 1;
            if (s.ref == e.kf) {
                s.ref = r.min_slot();
                if (s.ref < 0) s.status |= ME_REF_END;
            }
            if (s.nobs <= 2) me_set_bad(r, s, emit, li);
        } else me_set_bad(r, s, emit, li);
    }
}

// ---- the sequential statement (host builds; the kernels do the same in parallel) ----------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)

struct MeRowSeq {
    int32_t kf[ME_ROW], idx[ME_ROW];
    uint8_t octave[ME_ROW], weight[ME_ROW], alive[ME_ROW];
    int n;
    void load(const LmMap& M, const MeIndex& X, int p) {
        const int o0 = M.obs_ptr[p];
        n = M.obs_ptr[p + 1] - o0;
        for (int e = 0; e < n; ++e) { kf[e] = M.obs_kf[o0 + e]; idx[e] = X.obs_idx[o0 + e]; octave[e] = X.obs_octave[o0 + e]; weight[e] = X.obs_weight[o0 + e]; alive[e] = 1; }
    }
    int find(int k) const {
        for (int e = 0; e < n; ++e)
            if (alive[e] && kf[e] == k) return e;
        return -1;
    }
    int uniform(int v) const { return v; }
    int idx_at(int pos) const { return idx[pos]; }
    int weight_at(int pos) const { return weight[pos]; }
    void push(int k, int i, uint8_t o, uint8_t w) { kf[n] = k; idx[n] = i; octave[n] = o; weight[n] = w; alive[n] = 1; ++n; }
    void kill(int pos) { alive[pos] = 0; }
    int min_slot() const {
        uint32_t best = 0xffffffffu;
        for (int e = 0; e < n; ++e)
            if (alive[e] && (uint32_t)kf[e] < best) best = (uint32_t)kf[e];
        return best == 0xffffffffu ? -1 : (int)best;
    }
    template <class Emit>
    void emit_live(Emit& emit, int li) const {
        for (int e = 0; e < n; ++e)
            if (alive[e]) emit.one(kf[e], idx[e], -1, li);
    }
    void clear() { for (int e = 0; e < n; ++e) alive[e] = 0; }
};

struct MeEmitNone { void one(int, int, int, int) {} };
// the winner per (kf, idx) is the write with the largest list index: stamp[kf_mp_ptr[n_kf]] holds list index + 1 of what kf_mp holds
struct MeEmitSeq {
    const LmMap* M; int32_t* kf_mp; int32_t* stamp; int bad;
    void one(int k, int i, int value, int li) {
        const long long at = me_kfmp_at(*M, k, i);
        if (at < 0) { bad = 1; return; }
        if (li + 1 >= stamp[at]) { stamp[at] = li + 1; kf_mp[at] = value; }
    }
};

// The list over one map.  Outputs as slamit_map_edit_apply documents them; bucket[n], start[n_mp + 1], stamp[kf_mp_ptr[n_kf]] are
// scratch.  The tables of X are rewritten in place and the new observation table is written, unless it needs more than obs_cap_out
// entries: then only *n_obs_out (the number needed) and *status (ME_TABLE_OVERFLOW) are written.
static inline void me_apply_seq(const LmMap& M, const MeIndex& X, int n, const MeEdit* edits, int32_t* status_mp, int32_t* touched, int32_t* n_touched,
                                int32_t* n_obs_out, int32_t* status, int32_t* bucket, int32_t* start, int32_t* stamp) {
    int call = 0;
    // bucket by point, list order inside a bucket (a counting sort is stable)
    for (int p = 0; p <= M.n_mp; ++p) start[p] = 0;
    for (int i = 0; i < n; ++i)
        if (lm_mp_ok(M, edits[i].mp)) ++start[edits[i].mp + 1]; else call |= ME_BAD_SLOT;
    for (int p = 0; p < M.n_mp; ++p) start[p + 1] += start[p];
    const int n_bucketed = start[M.n_mp];
    for (int i = n - 1; i >= 0; --i)     // from the back through start[p + 1], the bucket's end, which ends as its first entry
        if (lm_mp_ok(M, edits[i].mp)) bucket[--start[edits[i].mp + 1]] = i;
    for (int p = 0; p < M.n_mp; ++p) start[p] = start[p + 1];
    start[M.n_mp] = n_bucketed;
    // the count pass: the new lengths and what each point's walk says
    static thread_local MeRowSeq row;
    long long need = 0;
    for (int p = 0; p < M.n_mp; ++p) {
        const int ne = start[p + 1] - start[p], len0 = M.obs_ptr[p + 1] - M.obs_ptr[p];
        int len = len0;
        if (ne > 0 && ne <= ME_MAX_PER_POINT && len0 <= ME_MAX_OBS) {
            MeState s = {len0, X.mp_nobs[p], X.mp_bad[p], X.mp_ref_kf[p], 0, 0};
            MeEmitNone none;
            row.load(M, X, p);
            me_walk(M, p, row, s, edits, bucket + start[p], ne, none);
            if (!(s.status & ME_OBS_OVERFLOW)) len = s.live;
        }
        need += len;
    }
    *n_obs_out = (int32_t)need;
    if (need > X.obs_cap_out) { *status = call | ME_TABLE_OVERFLOW; return; }
    // the write pass
    const long long n_kfmp = M.kf_mp_ptr[M.n_kf];
    for (long long i = 0; i < n_kfmp; ++i) stamp[i] = 0;
    MeEmitSeq emit = {&M, X.kf_mp, stamp, 0};
    int at = 0, nt = 0;
    for (int p = 0; p < M.n_mp; ++p) {
        const int ne = start[p + 1] - start[p], o0 = M.obs_ptr[p], len0 = M.obs_ptr[p + 1] - o0;
        int st = 0;
        bool walked = false;
        X.obs_ptr_out[p] = at;
        if (ne > ME_MAX_PER_POINT) st = ME_EDIT_OVERFLOW;
        else if (len0 > ME_MAX_OBS && ne > 0) st = ME_OBS_OVERFLOW;
        else if (ne > 0) {
            MeState s = {len0, X.mp_nobs[p], X.mp_bad[p], X.mp_ref_kf[p], 0, 0};
            MeEmitNone none;
            row.load(M, X, p);
            me_walk(M, p, row, s, edits, bucket + start[p], ne, none);   // does it overflow?  then not one write of it may be seen
            if (s.status & ME_OBS_OVERFLOW) st = ME_OBS_OVERFLOW;
            else {
                s = MeState{len0, X.mp_nobs[p], X.mp_bad[p], X.mp_ref_kf[p], 0, 0};
                row.load(M, X, p);
                const int before = emit.bad;
                emit.bad = 0;
                me_walk(M, p, row, s, edits, bucket + start[p], ne, emit);
                st = s.status | (emit.bad ? ME_BAD_SLOT : 0);
                emit.bad |= before;
                for (int e = 0; e < row.n; ++e)
                    if (row.alive[e]) {
                        X.obs_kf_out[at] = row.kf[e]; X.obs_idx_out[at] = row.idx[e]; X.obs_octave_out[at] = row.octave[e]; X.obs_weight_out[at] = row.weight[e];
                        ++at;
                    }
                X.mp_bad[p] = (uint8_t)s.bad; X.mp_nobs[p] = s.nobs; X.mp_ref_kf[p] = s.ref;
                if (s.changed) touched[nt++] = p;
                walked = true;
            }
        }
        if (!walked)
            for (int e = 0; e < len0; ++e) {
                X.obs_kf_out[at] = M.obs_kf[o0 + e]; X.obs_idx_out[at] = X.obs_idx[o0 + e]; X.obs_octave_out[at] = X.obs_octave[o0 + e]; X.obs_weight_out[at] = X.obs_weight[o0 + e];
                ++at;
            }
        status_mp[p] = st;
    }
    X.obs_ptr_out[M.n_mp] = at;
    *n_touched = nt;
    *status = call;
}
#endif

#endif
