// map_fuse.h — the tail of ORBmatcher::Fuse (ORB_SLAM2/src/ORBmatcher.cc:853 and :955-975) as ONE op over the slot tables: it looks at
// kf_mp[k][idx] and at both points' mp_nobs AS THE EARLIER OPS OF THE LIST LEFT THEM and picks Replace in one direction, Replace in the
// other, or the pair AddObservation + AddMapPoint.  A list may hold it beside the two kinds of map_replace.h, and is applied AS IF
// SEQUENTIALLY IN LIST ORDER.  One header for host and device, built by g++ without include/slamit.h.  Every outcome resolves into
// mr_walk_op, so map_replace.h stays the only text of Replace and of the add pair; what this header adds is the choice.
//
// THE OP.  MF_FUSE  a = P (the projected point), b = k (the target keyframe), idx = the matched keypoint, octave and weight what goes
// beside a new observation (weight 2 where mvuRight[idx] >= 0).  In this order:
//   1. idx < 0                         MF_OUT_NOMATCH      nothing else is read (the list builder writes such ops: no compaction)
//   2. mp_bad[P]                       MF_OUT_SKIP_BAD     :853
//   3. P's row holds k                 MF_OUT_SKIP_IN_KF   :853
//   4. Q = kf_mp[k][idx];  Q == -1     MF_OUT_ADDED        exactly MR_ADD_OBS of (P, k, idx, octave, weight), :971-972
//   5. mp_bad[Q]                       MF_OUT_OCCUPANT_BAD nothing; the reference still counts it in nFused (:961, :974)
//   6. mp_nobs[Q] > mp_nobs[P]         MF_OUT_P_REPLACED   MR_REPLACE(P -> Q), :963-964
//      otherwise                       MF_OUT_Q_REPLACED   MR_REPLACE(Q -> P), :966.  P == Q (only on tables that hold one (k, idx) under two
//                                                          points) lands here and is Replace's own a == b: nothing.
// n_fused counts outcomes 4 to 6, the reference's return value.  A plain op (or an op skipped for a bad slot) has outcome MF_OUT_PLAIN.
//
// THE INVOLVED POINTS are known before the walk: {P_i} with {the INITIAL kf_mp[k_i][idx_i]} and {S, D of plain ops}.  Every value an
// entry of kf_mp can take during the walk is -1, its initial value, a D of a Replace or the point of an add; a D is P or Q of its op,
// and Q was read from kf_mp -- so by induction over the list every point the walk reads or writes lies in that set, on tables that
// hold one (k, idx) under two points too.  At most 2 per op.  What is NOT known before the walk is which ops touch which points, so
// the predecessor DAG of map_replace.h is gone and the list is walked in order; and kf_mp is READ mid-walk, so the walk keeps a
// working image of it instead of the largest-list-index rule.
//
// LIMITS, all-or-nothing as map_replace.h: an involved row above MR_MAX_OBS on input, or an append onto MR_MAX_OBS entries:
// MF_OBS_OVERFLOW.  The new table above obs_cap_out: MF_TABLE_OVERFLOW with the need in n_obs_out.  The first that holds is reported
// and nothing else is written.  There is no per-point ceiling.  An observation is created by ADD_OBS and by FUSE only, so obs_cap_out =
// the old table + the number of those ops always suffices.
// BAD SLOTS (the device form; the host form refuses them): an op with idx >= 0 whose point, keyframe, index or weight lies outside
// its range is skipped whole; so is a FUSE op that meets an occupant outside [-1, n_mp); both set MF_BAD_SLOT.  Observations outside
// kf_mp: as map_replace.h.
#ifndef SLAMIT_MAP_FUSE_H
#define SLAMIT_MAP_FUSE_H
#include "map_replace.h"

#define MF_MAX_OPS MR_MAX_OPS   // ops per list: one workgroup walks them

enum { MF_FUSE = 3 };   // kind, beside MR_REPLACE and MR_ADD_OBS
enum { MF_OUT_PLAIN = 0, MF_OUT_NOMATCH = 1, MF_OUT_SKIP_BAD = 2, MF_OUT_SKIP_IN_KF = 3, MF_OUT_ADDED = 4, MF_OUT_OCCUPANT_BAD = 5, MF_OUT_P_REPLACED = 6, MF_OUT_Q_REPLACED = 7 };
enum { MF_OBS_OVERFLOW = 2, MF_TABLE_OVERFLOW = 4, MF_BAD_SLOT = 8 };   // the values of MR_*: one reader of a status serves both

// is the op one the walk can apply?
LM_HD bool mf_op_ok(const LmMap& M, const MrOp& e) {
    if (e.kind != MF_FUSE) return mr_op_ok(M, e);
    if (e.idx < 0) return true;                                          // step 1 reads nothing else
    if (!lm_mp_ok(M, e.a) || !lm_kf_ok(M, e.b)) return false;
    return e.idx < M.kf_mp_ptr[e.b + 1] - M.kf_mp_ptr[e.b] && (e.weight == 1 || e.weight == 2);
}
// does it read or write a point?
LM_HD bool mf_op_acts(const MrOp& e) { return e.kind == MF_FUSE ? e.idx >= 0 : mr_op_acts(e); }
// the reference's nFused++
LM_HD bool mf_counts(int outcome) { return outcome >= MF_OUT_ADDED; }

// Op e with list index li over the world w -> its outcome.  World: what mr_walk_op asks for, and bad(p), nobs(p) -> mp_bad / mp_nobs
// now; occupant(k, idx) -> kf_mp[k][idx] now; point_ok(q) -> is q a slot of the table; skipped() notes an op left out.
template <class World, class Emit>
LM_HD int mf_walk_op(World& w, const MrOp& e, int li, Emit& emit, int& moved, int& erased) {
    moved = 0; erased = 0;
    if (e.kind != MF_FUSE) { mr_walk_op(w, e, li, emit, moved, erased); return MF_OUT_PLAIN; }
    if (e.idx < 0) return MF_OUT_NOMATCH;
    if (w.bad(e.a)) return MF_OUT_SKIP_BAD;
    if (w.holds(e.a, e.b)) return MF_OUT_SKIP_IN_KF;
    const int q = w.occupant(e.b, e.idx);
    MrOp r = e;
    if (q == -1) {
        r.kind = MR_ADD_OBS;
        mr_walk_op(w, r, li, emit, moved, erased);
        return MF_OUT_ADDED;
    }
    if (!w.point_ok(q)) { w.skipped(); return MF_OUT_PLAIN; }
    if (w.bad(q)) return MF_OUT_OCCUPANT_BAD;
    const bool p_goes = w.nobs(q) > w.nobs(e.a);
    r.kind = MR_REPLACE; r.a = p_goes ? e.a : q; r.b = p_goes ? q : e.a;
    mr_walk_op(w, r, li, emit, moved, erased);
    return p_goes ? MF_OUT_P_REPLACED : MF_OUT_Q_REPLACED;
}

// ---- the sequential statement (host builds; the kernel walks the same list with a wavefront inside each op) -------------------
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC__)

struct MfEmitSeq {   // the working image of kf_mp: a later write simply comes later, and a later FUSE reads it
    const LmMap* M; int32_t* image; int bad;
    void one(int k, int i, int value, int) {
        const long long at = mr_kfmp_at(*M, k, i);
        if (at < 0) { bad = 1; return; }
        image[at] = value;
    }
};

struct MfWorldSeq : MrWorldSeq {
    const LmMap* M; const int32_t* image; int op_bad;
    bool bad(int p) { return row(p).bad != 0; }
    int nobs(int p) { return row(p).nobs; }
    int occupant(int k, int i) { return image[mr_kfmp_at(*M, k, i)]; }   // an op that is ok: inside the table
    bool point_ok(int q) const { return lm_mp_ok(*M, q); }
    void skipped() { op_bad = 1; }
};

// The list over one map.  Outputs as slamit_map_fuse_apply documents them: with an overflow only *status (and *n_obs_out for
// MF_TABLE_OVERFLOW) is written.
static inline void mf_apply_seq(const LmMap& M, const MrIndex& X, int n, const MrOp* ops, int32_t* outcome, int32_t* moved, int32_t* erased, int32_t* touched,
                                int32_t* n_touched, int32_t* n_fused, int32_t* n_obs_out, int32_t* status) {
    bool op_bad = false, committed;
    const size_t n_kfmp = (size_t)M.kf_mp_ptr[M.n_kf];
    std::vector<int32_t> image(X.kf_mp, X.kf_mp + n_kfmp), cid((size_t)M.n_mp + 1, -1);
    std::vector<uint8_t> named((size_t)M.n_mp + 1, 0);
    for (int i = 0; i < n; ++i) {
        const MrOp& e = ops[i];
        if (!mf_op_ok(M, e)) { op_bad = true; continue; }
        if (!mf_op_acts(e)) continue;
        named[e.a] = 1;
        if (e.kind == MR_REPLACE) named[e.b] = 1;
        if (e.kind == MF_FUSE) {
            const int q = X.kf_mp[mr_kfmp_at(M, e.b, e.idx)];            // the INITIAL occupant
            if (lm_mp_ok(M, q)) named[q] = 1;
        }
    }
    std::vector<MrRowSeq> rows;
    bool obs_over = false;
    for (int p = 0; p < M.n_mp; ++p) {
        if (!named[p]) continue;
        cid[p] = (int32_t)rows.size();
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
    std::vector<int32_t> oc((size_t)n + 1, 0), mv((size_t)n + 1, 0), er((size_t)n + 1, 0);
    MfWorldSeq w;
    w.rows = &rows; w.cid = cid.data(); w.obs_over = 0; w.M = &M; w.image = image.data(); w.op_bad = 0;
    MfEmitSeq emit = {&M, image.data(), 0};
    int fused = 0;
    for (int i = 0; i < n && !obs_over; ++i) {                           // an input row above the ceiling: its working row was not made
        if (!mf_op_ok(M, ops[i])) continue;
        int a, b;
        oc[i] = mf_walk_op(w, ops[i], i, emit, a, b);
        mv[i] = a; er[i] = b;
        fused += mf_counts(oc[i]);
    }
    obs_over = obs_over || w.obs_over;
    op_bad = op_bad || w.op_bad;
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
    for (size_t j = 0; j < n_kfmp; ++j) X.kf_mp[j] = image[j];
    for (int i = 0; i < n; ++i) { outcome[i] = oc[i]; moved[i] = mv[i]; erased[i] = er[i]; }
    *n_touched = nt; *n_fused = fused;
}
#endif

#endif
