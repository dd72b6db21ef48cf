// kf_erase.h — KeyFrame::SetBadFlag (ORB_SLAM2/src/KeyFrame.cc:460-552) over the slot tables of local_map.h and the graph rows of
// covis.h, with EraseConnection / UpdateBestCovisibles (:560-574, :142-161) and ChangeParent / AddChild / EraseChild (:388-405).
// A list of keyframe ops is applied AS IF SEQUENTIALLY IN LIST ORDER; everything is integer work, so the device equals this text
// exactly.  One header for host and device: the per-element functions below are what kf_erase.hip calls from its one workgroup per
// map; ke_apply_seq is the same walk in plain loops, built by g++ for the CPU tests, the shim's test driver and tools/bench_kf_erase.py.
//
// THE OPS, line by line.
//   SET_PARENT(c, p)  mpParent = p; p->AddChild(c): kf_parent[c] = p, and c enters p's children row unless it is there.  No bad test,
//                     no erase from an old parent, as in the reference (:378-383 runs it on a first connection; ChangeParent is the same body).
//   SET_BAD(k)        1  :464-470  k == origin_kf: nothing, KE_ORIGIN.  kf_not_erase[k]: kf_to_be_erased[k] = 1, nothing else,
//                        KE_NOT_ERASE.  No bad test on k: a second SET_BAD runs the walk again over what k's rows then hold.
//                     2  STATED DEPARTURE: kf_parent[k] == -1 on a keyframe that is not the origin, where the reference dereferences a
//                        null parent (:544): the op is skipped as a whole, nothing changes, KE_NO_PARENT.
//                     3  :473-474  for every j of k's cw row, ascending slot: EraseConnection(k) on j.  j's cw row holding k: the entry
//                        goes, the row closes up, j's ord row becomes the sort of its WHOLE remaining cw row (cv_key / cv_rank / cv_place
//                        of covis.h) and kf_best[j] its first ten padded with -1.  j's row lacking k: j stays byte for byte, a
//                        thresholded ord row included.  A row that holds k while k's row lacks it keeps that stale entry, as in the reference.
//                     4  :476-478  for every keypoint i of k with kf_mp[k][i] != -1 one ERASE_OBS edit (no MATCH) of point kf_mp[k][i]
//                        and keyframe k is EMITTED, in map_edit.h's layout, by op and then by keypoint index.  The point side of
//                        SetBadFlag is map_edit.h's walk over that list: the caller's next call.  k's own kf_mp row is not cleared.
//                        STATED DEPARTURE: the list is emitted from the kf_mp THE CALL WAS GIVEN.  A later keyframe of the same list
//                        may name a point that an earlier op's cascade turned bad (whose kf_mp entries SetBadFlag nulled); ERASE_OBS of an
//                        absent observer is a no-op, so applying the list equals the sequential walk.
//                     5  :483-484  cw_n[k] = ord_n[k] = 0, kf_best[k] all -1.
//                     6  :487-546  candidates = {kf_parent[k]}.  Repeat: over k's children in row order, bad ones skipped, for each entry
//                        of the child's ord row in row order that is a candidate, w = GetWeight (the child's CW row, 0 when absent; ord_w
//                        is not read); strict w > max from -1 picks (child, candidate).  The picked child gets SET_PARENT(child,
//                        candidate), joins the candidates and leaves k's row; nothing picked ends the loop.  Every child still in
//                        k's row then gets SET_PARENT(child, kf_parent[k]), bad ones included, and STAYS in k's row.  k leaves its
//                        parent's row, kf_bad[k] = 1, kf_parent[k] stays.
//   Staying the caller's: mTcp (the library holds no poses: the caller reads kf_parent[k]), Map::EraseKeyFrame, KeyFrameDatabase::erase
//   (slamit_kfdb_erase), SetErase() and the loop edges.
//
// THE PICK as one key, smallest wins: (0x7fffffff - w) << 32 | child position << 16 | ord position.  The first strict maximum in the
// reference's loop order is the largest weight, then the first child, then the first entry of its row.
// CHILDREN ROWS are std::set<KeyFrame*>: ascending slot for a caller that numbers keyframes by address.  An insert goes before the first
// entry with a larger slot.  The new table is a packed CSR written out of place; a row no op touched is copied.
// IN PLACE: kf_bad, kf_parent, kf_to_be_erased and the seven graph arrays.  A graph row that changed is rewritten up to its new count;
// what lies past it keeps the caller's bytes.
// GATES: the new children table above child_cap_out entries, or more edits than edit_cap: NOTHING is written but the two needs and the
// call's status (KE_CHILD_OVERFLOW, KE_EDIT_OVERFLOW).
// LIMITS: KE_MAX_OPS ops per list.  A SET_BAD whose keyframe has more than KE_MAX_CHILD children is skipped whole, KE_ROW_OVERFLOW.
// BAD SLOTS (the device form; the host form refuses them): an op whose keyframe or parent lies outside the table, or whose keyframe's
// stored parent does, is skipped whole with KE_BAD_SLOT.  A neighbour or child slot outside the table (or a neighbour equal to k) is
// skipped, never dereferenced, and sets KE_BAD_SLOT in the call's status; an ord entry outside the table is no candidate.  A keyframe
// listed twice in k's cw row is visited once.
#ifndef SLAMIT_KF_ERASE_H
#define SLAMIT_KF_ERASE_H
#include <stddef.h>
#include <stdint.h>

#include "covis.h"
#include "map_edit.h"

#define KE_MAX_OPS 1024        // ops per list: one workgroup walks them one after the other
#define KE_MAX_CHILD 1024      // children of one SET_BAD: the row, and with the parent the candidates, live in LDS

enum { KE_SET_PARENT = 1, KE_SET_BAD = 2 };   // kind
// per op: the first five.  Per call: KE_BAD_SLOT, KE_ROW_OVERFLOW (some op met it) and the two gates.
enum { KE_ORIGIN = 1, KE_NOT_ERASE = 2, KE_NO_PARENT = 4, KE_BAD_SLOT = 8, KE_ROW_OVERFLOW = 16, KE_CHILD_OVERFLOW = 32, KE_EDIT_OVERFLOW = 64 };

struct KeOp { int32_t kind, kf, parent, reserved; };   // the layout of slamit_kf_op

struct KeIndex {   // the layout of slamit_tree_index
    int32_t row_cap, origin_kf;
    const uint8_t* kf_not_erase;
    uint8_t* kf_bad; int32_t* kf_parent; uint8_t* kf_to_be_erased;
    int32_t* cw_kf; int32_t* cw_w; int32_t* cw_n;
    int32_t* ord_kf; int32_t* ord_w; int32_t* ord_n;
    int32_t* kf_best;
    int32_t* child_ptr_out; int32_t* child_out;
    int32_t child_cap_out, reserved;
};

// is the op one the walk can apply?
LM_HD bool ke_op_ok(const LmMap& M, const KeOp& e) {
    if (e.kind == KE_SET_BAD) return lm_kf_ok(M, e.kf);
    return e.kind == KE_SET_PARENT && lm_kf_ok(M, e.kf) && lm_kf_ok(M, e.parent);
}
// the graph arrays as covis.h's functions take them
LM_HD CvIndex ke_graph(int row_cap, int32_t* cw_kf, int32_t* cw_w, int32_t* cw_n, int32_t* ord_kf, int32_t* ord_w, int32_t* ord_n, int32_t* kf_best) {
    CvIndex G = CvIndex();
    G.row_cap = row_cap; G.origin_kf = -1;
    G.cw_kf = cw_kf; G.cw_w = cw_w; G.cw_n = cw_n; G.ord_kf = ord_kf; G.ord_w = ord_w; G.ord_n = ord_n; G.kf_best = kf_best;
    return G;
}
// KeyFrame::GetWeight(kf) of keyframe c: the first entry of c's cw row that names kf, 0 when none does
LM_HD int ke_weight(const CvIndex& G, int c, int kf) {
    const int n = cv_clamp(G.cw_n[c], G.row_cap);
    for (int e = 0; e < n; ++e)
        if (G.cw_kf[(size_t)c * G.row_cap + e] == kf) return G.cw_w[(size_t)c * G.row_cap + e];
    return 0;
}
#define KE_PICK_NONE 0xffffffffffffffffull
LM_HD unsigned long long ke_pick_key(int w, int child_pos, int row_pos) {   // w >= 0, both positions below 65536
    return ((unsigned long long)(uint32_t)(0x7fffffff - w) << 32) | ((uint32_t)child_pos << 16) | (uint32_t)row_pos;
}
LM_HD int ke_pick_child(unsigned long long key) { return (int)((uint32_t)key >> 16); }
LM_HD int ke_pick_row(unsigned long long key) { return (int)((uint32_t)key & 0xffffu); }
// the edit step 4 emits; the fields ERASE_OBS does not read are written as map_edit.h's validation takes them
LM_HD MeEdit ke_edit(int mp, int k) {
    MeEdit e;
    e.kind = ME_ERASE_OBS; e.flags = 0; e.mp = mp; e.kf = k; e.idx = 0; e.octave = 0; e.weight = 0; e.pad[0] = 0; e.pad[1] = 0;
    return e;
}
// the call's status from what was found.  committed: nothing stands against writing.
LM_HD int ke_call_status(bool child_over, bool edit_over, int bits, bool& committed) {
    committed = !child_over && !edit_over;
    return (bits & (KE_BAD_SLOT | KE_ROW_OVERFLOW)) | (child_over ? KE_CHILD_OVERFLOW : 0) | (edit_over ? KE_EDIT_OVERFLOW : 0);
}

// ---- the sequential statement (host builds; the kernel does the same with the parallelism inside an op) ------------------------
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC__)
#include <vector>

// EraseConnection(k) on keyframe j, :560-574 with UpdateBestCovisibles.  keys[row_cap] is scratch.  -> did j change?
static inline bool ke_erase_connection_seq(const CvIndex& G, int j, int k, unsigned long long* keys) {
    int32_t* const ckf = G.cw_kf + (size_t)j * G.row_cap;
    int32_t* const cw = G.cw_w + (size_t)j * G.row_cap;
    const int n = cv_clamp(G.cw_n[j], G.row_cap);
    int pos = 0;
    while (pos < n && ckf[pos] != k) ++pos;
    if (pos == n) return false;
    for (int e = pos; e + 1 < n; ++e) { ckf[e] = ckf[e + 1]; cw[e] = cw[e + 1]; }
    const int n1 = n - 1;
    for (int e = 0; e < n1; ++e) keys[e] = cv_key(cw[e], ckf[e]);
    for (int e = 0; e < n1; ++e) cv_place(G, j, keys, n1, e);
    for (int b = 0; b < LM_BEST; ++b) cv_pad_best(G, j, n1, b);
    G.cw_n[j] = n1; G.ord_n[j] = n1;
    return true;
}

struct KeWorldSeq {
    const LmMap* M; CvIndex G;
    std::vector<int32_t> cw_kf, cw_w, cw_n, ord_kf, ord_w, ord_n, best, parent;
    std::vector<uint8_t> bad, tbe, dirty;
    std::vector<std::vector<int32_t> > child;
    std::vector<unsigned long long> keys;
    int call;
    void set_parent(int c, int p) {   // ChangeParent / the tail of UpdateConnections
        parent[(size_t)c] = p;
        std::vector<int32_t>& row = child[(size_t)p];
        size_t at = 0;
        while (at < row.size() && row[at] < c) ++at;
        if (at < row.size() && row[at] == c) return;
        row.insert(row.begin() + (long)at, c);
    }
    void erase_child(int p, int c) {
        std::vector<int32_t>& row = child[(size_t)p];
        for (size_t at = 0; at < row.size(); ++at)
            if (row[at] == c) { row.erase(row.begin() + (long)at); return; }
    }
};

// one op -> its status; *emits: does step 4 emit k's row?
static inline int ke_walk_op_seq(KeWorldSeq& W, const KeIndex& X, const KeOp& e, bool* emits) {
    const LmMap& M = *W.M;
    *emits = false;
    if (!ke_op_ok(M, e)) { W.call |= KE_BAD_SLOT; return KE_BAD_SLOT; }
    if (e.kind == KE_SET_PARENT) { W.set_parent(e.kf, e.parent); return 0; }
    const int k = e.kf, rc = X.row_cap;
    if (k == X.origin_kf) return KE_ORIGIN;
    if (X.kf_not_erase[k]) { W.tbe[(size_t)k] = 1; return KE_NOT_ERASE; }
    const int P = W.parent[(size_t)k];
    if (P == -1) return KE_NO_PARENT;
    if (!lm_kf_ok(M, P)) { W.call |= KE_BAD_SLOT; return KE_BAD_SLOT; }
    const std::vector<int32_t> ch = W.child[(size_t)k];   // the row as the op meets it
    if (ch.size() > KE_MAX_CHILD) { W.call |= KE_ROW_OVERFLOW; return KE_ROW_OVERFLOW; }
    // 3
    const int nk = cv_clamp(W.cw_n[(size_t)k], rc);
    std::vector<uint8_t> seen((size_t)M.n_kf, 0);
    for (int t = 0; t < nk; ++t) {
        const int j = W.cw_kf[(size_t)k * rc + t];
        if (!lm_kf_ok(M, j) || j == k) { W.call |= KE_BAD_SLOT; continue; }
        if (seen[(size_t)j]) continue;
        seen[(size_t)j] = 1;
        if (ke_erase_connection_seq(W.G, j, k, W.keys.data())) W.dirty[(size_t)j] = 1;
    }
    // 4
    *emits = true;
    // 5
    W.cw_n[(size_t)k] = 0; W.ord_n[(size_t)k] = 0; W.dirty[(size_t)k] = 1;
    for (int b = 0; b < LM_BEST; ++b) W.best[(size_t)k * LM_BEST + b] = -1;
    // 6
    std::vector<uint8_t> cand((size_t)M.n_kf, 0), alive(ch.size(), 1);
    cand[(size_t)P] = 1;
    for (;;) {
        unsigned long long pick = KE_PICK_NONE;
        for (size_t i = 0; i < ch.size(); ++i) {
            if (!alive[i]) continue;
            const int c = ch[i];
            if (!lm_kf_ok(M, c)) { W.call |= KE_BAD_SLOT; continue; }
            if (W.bad[(size_t)c]) continue;
            const int no = cv_clamp(W.ord_n[(size_t)c], rc);
            for (int t = 0; t < no; ++t) {
                const int kf = W.ord_kf[(size_t)c * rc + t];
                if (!lm_kf_ok(M, kf) || !cand[(size_t)kf]) continue;
                const int w = ke_weight(W.G, c, kf);
                if (w < 0) continue;   // never above -1
                const unsigned long long key = ke_pick_key(w, (int)i, t);
                if (key < pick) pick = key;
            }
        }
        if (pick == KE_PICK_NONE) break;
        const int i = ke_pick_child(pick), c = ch[(size_t)i], p = W.ord_kf[(size_t)c * rc + ke_pick_row(pick)];
        W.set_parent(c, p);
        cand[(size_t)c] = 1;
        W.erase_child(k, c);
        alive[(size_t)i] = 0;
    }
    for (size_t i = 0; i < ch.size(); ++i)
        if (alive[i] && lm_kf_ok(M, ch[i])) W.set_parent(ch[i], P);
    W.erase_child(P, k);
    W.bad[(size_t)k] = 1;
    return 0;
}

// The list over one map.  Outputs as slamit_kf_erase_apply documents them: *n_edits_out, *n_child_out and *status are always written;
// with a gate's bit in *status nothing else is.
static inline void ke_apply_seq(const LmMap& M, const KeIndex& X, int n, const KeOp* ops, int32_t* op_status, int edit_cap, MeEdit* edits,
                                int32_t* n_edits_out, int32_t* n_child_out, int32_t* status) {
    const size_t nk = (size_t)M.n_kf, rc = (size_t)X.row_cap;
    KeWorldSeq W;
    W.M = &M; W.call = 0;
    W.cw_kf.assign(X.cw_kf, X.cw_kf + nk * rc); W.cw_w.assign(X.cw_w, X.cw_w + nk * rc); W.cw_n.assign(X.cw_n, X.cw_n + nk);
    W.ord_kf.assign(X.ord_kf, X.ord_kf + nk * rc); W.ord_w.assign(X.ord_w, X.ord_w + nk * rc); W.ord_n.assign(X.ord_n, X.ord_n + nk);
    if (X.kf_best) W.best.assign(X.kf_best, X.kf_best + nk * LM_BEST); else W.best.assign(nk * LM_BEST + 1, -1);
    W.parent.assign(X.kf_parent, X.kf_parent + nk); W.bad.assign(X.kf_bad, X.kf_bad + nk); W.tbe.assign(X.kf_to_be_erased, X.kf_to_be_erased + nk);
    W.dirty.assign(nk, 0); W.keys.assign(rc + 1, 0);
    W.child.resize(nk);
    for (size_t j = 0; j < nk; ++j) W.child[j].assign(M.kf_child + M.kf_child_ptr[j], M.kf_child + M.kf_child_ptr[j + 1]);
    W.G = ke_graph(X.row_cap, W.cw_kf.data(), W.cw_w.data(), W.cw_n.data(), W.ord_kf.data(), W.ord_w.data(), W.ord_n.data(), W.best.data());
    std::vector<int32_t> ost((size_t)n + 1, 0);
    std::vector<uint8_t> emits((size_t)n + 1, 0);
    long long n_edits = 0, need = 0;
    for (int i = 0; i < n; ++i) {
        bool em;
        ost[(size_t)i] = ke_walk_op_seq(W, X, ops[i], &em);
        emits[(size_t)i] = em;
        if (em)
            for (int e = M.kf_mp_ptr[ops[i].kf]; e < M.kf_mp_ptr[ops[i].kf + 1]; ++e) n_edits += M.kf_mp[e] != -1;
    }
    for (size_t j = 0; j < nk; ++j) need += (long long)W.child[j].size();
    bool committed;
    *status = ke_call_status(need > X.child_cap_out, n_edits > edit_cap, W.call, committed);
    *n_edits_out = (int32_t)n_edits; *n_child_out = (int32_t)need;
    if (!committed) return;
    int at = 0;
    for (int i = 0; i < n; ++i) {
        op_status[i] = ost[(size_t)i];
        if (!emits[(size_t)i]) continue;
        const int k = ops[i].kf;
        for (int e = M.kf_mp_ptr[k]; e < M.kf_mp_ptr[k + 1]; ++e)
            if (M.kf_mp[e] != -1) edits[at++] = ke_edit(M.kf_mp[e], k);
    }
    at = 0;
    for (size_t j = 0; j < nk; ++j) {
        X.child_ptr_out[j] = at;
        for (size_t e = 0; e < W.child[j].size(); ++e) X.child_out[at++] = W.child[j][e];
        X.kf_bad[j] = W.bad[j]; X.kf_parent[j] = W.parent[j]; X.kf_to_be_erased[j] = W.tbe[j];
        if (!W.dirty[j]) continue;
        const size_t ncw = (size_t)cv_clamp(W.cw_n[j], X.row_cap), no = (size_t)cv_clamp(W.ord_n[j], X.row_cap);
        for (size_t e = 0; e < ncw; ++e) { X.cw_kf[j * rc + e] = W.cw_kf[j * rc + e]; X.cw_w[j * rc + e] = W.cw_w[j * rc + e]; }
        for (size_t e = 0; e < no; ++e) { X.ord_kf[j * rc + e] = W.ord_kf[j * rc + e]; X.ord_w[j * rc + e] = W.ord_w[j * rc + e]; }
        X.cw_n[j] = W.cw_n[j]; X.ord_n[j] = W.ord_n[j];
        if (X.kf_best)
            for (size_t b = 0; b < LM_BEST; ++b) X.kf_best[j * LM_BEST + b] = W.best[j * LM_BEST + b];
    }
    X.child_ptr_out[nk] = at;
}
#endif

#endif
