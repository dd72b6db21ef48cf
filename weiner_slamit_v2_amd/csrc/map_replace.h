// map_replace.h — MapPoint::Replace (ORB_SLAM2/src/MapPoint.cc:183-221) over the slot tables of local_map.h, as its callers use it:
// ORBmatcher::Fuse's tail (ORBmatcher.cc:956-973), LoopClosing::SearchAndFuse (:614-625) and ::CorrectLoop (:532-547).  Fuse interleaves
// Replace with the pair AddObservation + AddMapPoint on the same points, so a list carries both kinds and is applied AS IF SEQUENTIALLY
// IN LIST ORDER; everything is integer work, so the device equals this text exactly.  One header for host and device, built by g++
// without include/slamit.h: mr_walk_op is the effect of one op, stated once over a world policy (MrWorldSeq below: plain loops;
// map_replace.hip: the rows in the workspace, one wavefront per op, membership by wave ballot) and an emitter of kf_mp writes.
//
// THE OPS, line by line.
//   REPLACE  a = S, b = D.  :185 equal ids return at once.  :193-197 S's observations are taken, its map cleared, mbBad = true,
//            mpReplaced = D.  :199-214 for every observation (k, idx) of S in std::map order -- ASCENDING KEYFRAME SLOT for a caller that
//            numbers keyframes by address -- D not observing k: kf_mp[k][idx] = D (ReplaceMapPointMatch), the entry is appended to D's row
//            and mp_nobs[D] += weight (AddObservation); D observing k: kf_mp[k][idx] = -1 (EraseMapPointMatch).  :215-216 D's found and
//            visible counters take S's on top, int32 two's-complement wrap.  No bad test on D; S's nobs, found, visible are not touched;
//            a second Replace of a replaced S moves nothing but adds the counters again and overwrites mp_replaced.  All as written.
//            (:217 ComputeDistinctiveDescriptors of D is the caller's next call, over `touched`.)
//   ADD_OBS  a = the point, b = the keyframe: MapPoint::AddObservation (:104-115) and KeyFrame::AddMapPoint, exactly
//            ME_ADD_OBS | ME_MATCH of map_edit.h: an observer that is present changes nothing of the point, kf_mp[b][idx] = a either way.
// A row that holds one keyframe twice (no std::map does): the first entry in row order decides, the others are dropped.
//
// WHY IT IS NOT map_edit.h.  Replace reads D's observers and writes D's row from S's: a point's row depends on OTHER points' ops, so
// fact (1) of map_edit.h is gone.  What stays: op i must follow every earlier op that names either of its points, and nothing else --
// a DAG in list order.  Ops whose predecessors are done name disjoint points and may run at once.  Fact (2) stays as it is: every
// kf_mp write is unconditional given the state its op meets, so kf_mp[k][idx] after the list is the write with the LARGEST LIST INDEX.
//
// THE NEW ROW is the old order with the moved-out entries gone (S's row is emptied whole) and the received ones appended in the order
// they were received.  Nothing kills a single entry, so a row never holds more than MR_MAX_OBS physical entries.
// LIMITS, all-or-nothing for the call because points are coupled: a point named by more than MR_MAX_PER_POINT ops (either side):
// MR_OP_OVERFLOW.  An involved row above MR_MAX_OBS on input, or an append onto MR_MAX_OBS entries: MR_OBS_OVERFLOW.  The new table
// above obs_cap_out: MR_TABLE_OVERFLOW, with the need in n_obs_out.  In each case nothing else is written.  The first that holds in
// this order is the one reported, with MR_BAD_SLOT beside it where an OP was skipped.
// CAPACITY: Replace never creates an observation (an entry moves or dies), so obs_cap_out = the old table + the number of ADD_OBS
// ops always suffices.
// BAD SLOTS (the device form; the host form refuses them): an op whose point, keyframe, index or weight lies outside its range is
// skipped whole, counts towards no ceiling, and sets MR_BAD_SLOT.  An observation whose (k, idx) lies outside kf_mp is carried
// along, its kf_mp write is skipped, MR_BAD_SLOT is set when the call commits.
// TOUCHED: the points that received at least one observation, ascending.  moved[i] / erased[i]: the entries op i appended to its
// target and the ones it dropped (ADD_OBS: 1 or 0, and 0; a skipped op: 0 and 0).
#ifndef SLAMIT_MAP_REPLACE_H
#define SLAMIT_MAP_REPLACE_H
#include <stddef.h>
#include <stdint.h>

#include "local_map.h"

#define MR_MAX_OPS 16384       // ops per list: the round loop of one workgroup walks them
#define MR_MAX_PER_POINT 64    // ops naming one point, as either side: a bucket is ordered by one wavefront
#define MR_MAX_OBS 512         // observers per point = UP_MAX_OBS: a working row
#define MR_SCAN_BLOCK 256      // entries per workgroup of the device scan

enum { MR_REPLACE = 1, MR_ADD_OBS = 2 };   // kind
enum { MR_OP_OVERFLOW = 1, MR_OBS_OVERFLOW = 2, MR_TABLE_OVERFLOW = 4, MR_BAD_SLOT = 8 };

struct MrOp {   // the layout of slamit_map_replace
    int32_t kind, a, b, idx;
    uint8_t octave, weight, pad[2];
};

struct MrIndex {   // the layout of slamit_replace_index
    const int32_t* obs_idx; const uint8_t* obs_octave; const uint8_t* obs_weight;
    uint8_t* mp_bad; int32_t* mp_nobs; int32_t* mp_found; int32_t* mp_visible; int32_t* mp_replaced; int32_t* kf_mp;
    int32_t* obs_ptr_out; int32_t* obs_kf_out; int32_t* obs_idx_out; uint8_t* obs_octave_out; uint8_t* obs_weight_out;
    int32_t obs_cap_out, reserved;
};

// is the op one the walk can apply?
LM_HD bool mr_op_ok(const LmMap& M, const MrOp& e) {
    if (e.kind == MR_REPLACE) return lm_mp_ok(M, e.a) && lm_mp_ok(M, e.b);
    if (e.kind != MR_ADD_OBS) return false;
    if (!lm_mp_ok(M, e.a) || !lm_kf_ok(M, e.b)) return false;
    return e.idx >= 0 && e.idx < M.kf_mp_ptr[e.b + 1] - M.kf_mp_ptr[e.b] && (e.weight == 1 || e.weight == 2);
}
// does it do anything?  (:185: Replace of a point by itself returns at once)
LM_HD bool mr_op_acts(const MrOp& e) { return !(e.kind == MR_REPLACE && e.a == e.b); }

// where (k, i) lies in kf_mp, -1 for a pair outside the table
LM_HD long long mr_kfmp_at(const LmMap& M, int k, int i) {
    if (!lm_kf_ok(M, k)) return -1;
    if (i < 0 || i >= M.kf_mp_ptr[k + 1] - M.kf_mp_ptr[k]) return -1;
    return (long long)M.kf_mp_ptr[k] + i;
}

// the call's status from what was found.  committed: nothing stands against writing.
LM_HD int mr_call_status(bool op_over, bool obs_over, bool table_over, bool op_bad, bool obs_bad, bool& committed) {
    const int bad = op_bad ? MR_BAD_SLOT : 0;
    committed = false;
    if (op_over) return MR_OP_OVERFLOW | bad;
    if (obs_over) return MR_OBS_OVERFLOW | bad;
    if (table_over) return MR_TABLE_OVERFLOW | bad;
    committed = true;
    return bad | (obs_bad ? MR_BAD_SLOT : 0);
}

// Tracking::CheckReplacedInLastFrame (Tracking.cc:959-974) for one entry of a frame's point list: a point that was replaced gives way
// to its replacement, ONE hop as the reference follows one.  -> MR_BAD_SLOT for an entry outside the table, which is left alone.
LM_HD int mr_check_replaced_entry(int n_mp, const int32_t* mp_replaced, int32_t* entry) {
    const int p = *entry;
    if (p == -1) return 0;
    if ((unsigned)p >= (unsigned)n_mp) return MR_BAD_SLOT;
    const int r = mp_replaced[p];
    if (r >= 0) *entry = r;
    return 0;
}

// Op e with list index li over the world w.  World: holds(p, k) -> does p's row hold keyframe k; push(p, k, idx, octave, weight) -> 1
// after appending to p's row with nobs += weight and p marked as having received, 0 with the overflow noted where the row is full;
// fuse(S, D, emit, li, moved, erased): S's entries in ascending slot, each pushed onto D or dropped, with its kf_mp write;
// retire(S, D): S's row emptied, bad, replaced by D; D's counters take S's.  Emit: one(kf, idx, value, li).
template <class World, class Emit>
LM_HD void mr_walk_op(World& w, const MrOp& e, int li, Emit& emit, int& moved, int& erased) {
    moved = 0; erased = 0;
    if (e.kind == MR_ADD_OBS) {
        if (!w.holds(e.a, e.b)) moved = w.push(e.a, e.b, e.idx, e.octave, e.weight);
        emit.one(e.b, e.idx, e.a, li);            // KeyFrame::AddMapPoint, whatever AddObservation did
        return;
    }
    if (e.a == e.b) return;
    w.fuse(e.a, e.b, emit, li, moved, erased);
    w.retire(e.a, e.b);
}

// ---- the sequential statement (host builds; the kernels do the same in parallel) ----------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC__)
#include <algorithm>
#include <vector>

struct MrRowSeq {
    std::vector<int32_t> kf, idx;
    std::vector<uint8_t> octave, weight;
    int32_t bad, nobs, found, visible, replaced, received;
};
struct MrWrite { long long at; int32_t value; };

struct MrEmitSeq {   // sequential: a later write simply comes later
    const LmMap* M; std::vector<MrWrite>* writes; int bad;
    void one(int k, int i, int value, int) {
        const long long at = mr_kfmp_at(*M, k, i);
        if (at < 0) { bad = 1; return; }
        writes->push_back(MrWrite{at, value});
    }
};

struct MrWorldSeq {
    std::vector<MrRowSeq>* rows; const int32_t* cid; int obs_over;
    MrRowSeq& row(int p) { return (*rows)[(size_t)cid[p]]; }
    bool holds(int p, int k) {
        const MrRowSeq& r = row(p);
        for (size_t e = 0; e < r.kf.size(); ++e)
            if (r.kf[e] == k) return true;
        return false;
    }
    int push(int p, int k, int i, uint8_t o, uint8_t wt) {
        MrRowSeq& r = row(p);
        if (r.kf.size() >= MR_MAX_OBS) { obs_over = 1; return 0; }
        r.kf.push_back(k); r.idx.push_back(i); r.octave.push_back(o); r.weight.push_back(wt);
        r.nobs += wt; r.received = 1;
        return 1;
    }
    template <class Emit>
    void fuse(int S, int D, Emit& emit, int li, int& moved, int& erased) {
        MrRowSeq& s = row(S);
        std::vector<int> order(s.kf.size());
        for (size_t e = 0; e < order.size(); ++e) order[e] = (int)e;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return (uint32_t)s.kf[x] < (uint32_t)s.kf[y]; });
        for (size_t j = 0; j < order.size(); ++j) {
            const int e = order[j], k = s.kf[e];
            if (holds(D, k)) { emit.one(k, s.idx[e], -1, li); ++erased; }
            else {
                moved += push(D, k, s.idx[e], s.octave[e], s.weight[e]);
                emit.one(k, s.idx[e], D, li);
            }
        }
    }
    void retire(int S, int D) {
        MrRowSeq& s = row(S);
        MrRowSeq& d = row(D);
        s.kf.clear(); s.idx.clear(); s.octave.clear(); s.weight.clear();
        s.bad = 1; s.replaced = D;
        d.found = (int32_t)((uint32_t)d.found + (uint32_t)s.found);
        d.visible = (int32_t)((uint32_t)d.visible + (uint32_t)s.visible);
    }
};

// The list over one map.  Outputs as slamit_map_replace_apply documents them: with an overflow only *status (and *n_obs_out for
// MR_TABLE_OVERFLOW) is written.
static inline void mr_apply_seq(const LmMap& M, const MrIndex& X, int n, const MrOp* ops, int32_t* moved, int32_t* erased, int32_t* touched, int32_t* n_touched,
                                int32_t* n_obs_out, int32_t* status) {
    bool op_bad = false, committed;
    std::vector<int32_t> cnt((size_t)M.n_mp + 1, 0), cid((size_t)M.n_mp + 1, -1);
    for (int i = 0; i < n; ++i) {
        if (!mr_op_ok(M, ops[i])) { op_bad = true; continue; }
        if (!mr_op_acts(ops[i])) continue;
        ++cnt[ops[i].a];
        if (ops[i].kind == MR_REPLACE) ++cnt[ops[i].b];
    }
    for (int p = 0; p < M.n_mp; ++p)
        if (cnt[p] > MR_MAX_PER_POINT) { *status = mr_call_status(true, false, false, op_bad, false, committed); return; }
    // the involved points: a compact number in ascending slot, a working row
    std::vector<MrRowSeq> rows;
    std::vector<int32_t> inv;
    bool obs_over = false;
    for (int p = 0; p < M.n_mp; ++p) {
        if (!cnt[p]) continue;
        cid[p] = (int32_t)rows.size();
        inv.push_back(p);
        rows.push_back(MrRowSeq());
        MrRowSeq& r = rows.back();
        const int o0 = M.obs_ptr[p], len0 = M.obs_ptr[p + 1] - o0;
        if (len0 > MR_MAX_OBS) obs_over = true;
        else {
            r.kf.assign(M.obs_kf + o0, M.obs_kf + o0 + len0); r.idx.assign(X.obs_idx + o0, X.obs_idx + o0 + len0);
            r.octave.assign(X.obs_octave + o0, X.obs_octave + o0 + len0); r.weight.assign(X.obs_weight + o0, X.obs_weight + o0 + len0);
        }
        r.bad = X.mp_bad[p]; r.nobs = X.mp_nobs[p]; r.found = X.mp_found[p]; r.visible = X.mp_visible[p]; r.replaced = X.mp_replaced[p]; r.received = 0;
    }
    std::vector<MrWrite> writes;
    std::vector<int32_t> mv((size_t)n + 1, 0), er((size_t)n + 1, 0);
    MrWorldSeq w = {&rows, cid.data(), 0};
    MrEmitSeq emit = {&M, &writes, 0};
    for (int i = 0; i < n; ++i) {
        if (!mr_op_ok(M, ops[i])) continue;
        int a, b;
        mr_walk_op(w, ops[i], i, emit, a, b);
        mv[i] = a; er[i] = b;
    }
    obs_over = obs_over || w.obs_over;
    long long need = 0;
    for (int p = 0; p < M.n_mp; ++p) need += cid[p] < 0 ? M.obs_ptr[p + 1] - M.obs_ptr[p] : (int)rows[(size_t)cid[p]].kf.size();
    const bool table_over = !obs_over && need > X.obs_cap_out;
    *status = mr_call_status(false, obs_over, table_over, op_bad, emit.bad != 0, committed);
    if (table_over) *n_obs_out = (int32_t)need;
    if (!committed) return;
    *n_obs_out = (int32_t)need;
    int at = 0, nt = 0;
    for (int p = 0; p < M.n_mp; ++p) {
        X.obs_ptr_out[p] = at;
        if (cid[p] < 0) {
            for (int e = M.obs_ptr[p]; e < M.obs_ptr[p + 1]; ++e, ++at) {
                X.obs_kf_out[at] = M.obs_kf[e]; X.obs_idx_out[at] = X.obs_idx[e]; X.obs_octave_out[at] = X.obs_octave[e]; X.obs_weight_out[at] = X.obs_weight[e];
            }
            continue;
        }
        const MrRowSeq& r = rows[(size_t)cid[p]];
        for (size_t e = 0; e < r.kf.size(); ++e, ++at) {
            X.obs_kf_out[at] = r.kf[e]; X.obs_idx_out[at] = r.idx[e]; X.obs_octave_out[at] = r.octave[e]; X.obs_weight_out[at] = r.weight[e];
        }
        X.mp_bad[p] = (uint8_t)r.bad; X.mp_nobs[p] = r.nobs; X.mp_found[p] = r.found; X.mp_visible[p] = r.visible; X.mp_replaced[p] = r.replaced;
        if (r.received) touched[nt++] = p;
    }
    X.obs_ptr_out[M.n_mp] = at;
    for (size_t j = 0; j < writes.size(); ++j) X.kf_mp[writes[j].at] = writes[j].value;
    for (int i = 0; i < n; ++i) { moved[i] = mv[i]; erased[i] = er[i]; }
    *n_touched = nt;
}
#endif

#endif
