// map_grow.h — the map grows on the resident tables: KeyFrame::KeyFrame(Frame&, ...) + Map::AddKeyFrame, the map point constructor with its
// AddObservation / AddMapPoint / Map::AddMapPoint (ORB_SLAM2/src/LocalMapping.cc:486-500, Tracking.cc:1376-1383, :718-723, :875-891) and the
// association loop of LocalMapping::ProcessNewKeyFrame (:156-175), over the slot tables of local_map.h and the columns beside them.
// A list of ops is applied AS IF SEQUENTIALLY IN LIST ORDER.  Everything is integer work and copies but the camera centre, whose float
// evaluation order is stated at mg_center: the device equals this text exactly.  One header for host and device: the per-element
// functions below are what map_grow.hip calls from its one workgroup per map; mg_apply_seq is the same walk in plain loops, built by g++
// for the CPU tests.
//
// THE TABLES are appended IN PLACE, each within a stated capacity (MgIndex: kf_cap keyframes, mp_cap points, kfmp_cap keypoints).  The
// call does not move n_kf / n_mp of any record: the caller advances them by the NEW_KF ops it listed and by P, its NEW_POINT ops.
//
// THE OPS, in the fields of MgOp.
//   NEW_KF {kf, src, kf_id}      kf must be the next free slot (n_kf + the NEW_KF ops applied before it) and src a frame record with at most
//                                MG_MAX_KP keypoints; else the op is skipped whole, MG_OP_BAD, never dereferenced.  Appends kf_mp_ptr[kf + 1],
//                                the kf_mp row as mvpMapPoints is copied (bad points stay; an entry outside [-1, the points that exist at
//                                that moment) becomes -1 with MG_BAD_SLOT), kf_octave, kf_desc and kf_depth beside it (a source without
//                                depth: -1, a monocular keyframe's mvDepth), kf_bad = 0, kf_parent = -1, kf_to_be_erased = 0, kf_not_erase = 0,
//                                kf_th_depth, kf_best all -1, cw_n = ord_n = 0, kf_child_ptr[kf + 1] = kf_child_ptr[kf], kf_center (mg_center).
//                                kf_id is the caller's (the library keeps no mnId column of keyframes); it is carried for the shim.
//   NEW_POINT {kf = ref, kf_id = first_kf_id, (kf_a, idx_a, weight_a), (kf_b, idx_b, weight_b), cand, flags, pos}
//                                kf_b = -1: one observer.  A slot or index outside its table, a weight outside 1..2 or cand outside
//                                [-1, cand_cap): skipped whole, MG_OP_BAD.  The point EXISTS iff cand == -1 (position in the op) or
//                                cand_status[cand] == 0 (position cand_x3d[3 cand ..]); else MG_OP_REJECTED.  Accepted points take the slots
//                                n_mp, n_mp + 1, ... in list order: mp_pos, mp_normal = 0, both distances 0, mp_bad = 0, mp_nobs = 0,
//                                mp_ref_kf = ref, mp_found = mp_visible = 1, mp_first_kf, mp_replaced = -1, mp_desc = 0, an empty row of
//                                obs_ptr.  For a, then b: kf_mp[kf][idx] = the slot, unconditional (the last op of the list that names an
//                                entry wins), and one ME_ADD_OBS edit without MATCH is EMITTED (octave from kf_octave, weight as given):
//                                AddObservation is map_edit.h's walk over that list, the caller's next call.  MG_RECENT appends the slot
//                                to the recent list.
//   ASSOCIATE {kf, src}          kf a keyframe that exists at that moment whose row has src's n_kp entries, else MG_OP_BAD.  Over kf_mp[kf]
//                                as the ops before left it, in keypoint order: -1 and bad points are skipped (a slot outside the points
//                                that exist: skipped, MG_BAD_SLOT); a point for which IsInKeyFrame(kf) holds at that moment goes to the
//                                recent list; any other emits ME_ADD_OBS(p, kf, i, kf_octave, 2 where src.uright[i] >= 0 else 1).
//                                IsInKeyFrame(kf) holds when the point's row in the table the call was given holds kf, or an ADD_OBS(p, kf)
//                                was emitted earlier in this call (a NEW_POINT naming kf, an earlier ASSOCIATE, an earlier keypoint of this
//                                row: a point at two keypoints adds at the first and goes to the recent list at the second).
// The call READS THE TABLES AS THEY ARE: edits emitted by an earlier grow call must have been applied (map_edit + the swap of its buffer
// sets) before a call that depends on them.  UpdateNormalAndDepth / ComputeDistinctiveDescriptors are map_edit's `touched` handed to
// the upkeep call; UpdateConnections and SET_PARENT are the existing calls.
// THE INERT TAIL: of the P NEW_POINT ops A are accepted; slots n_mp + A .. n_mp + P - 1 become mp_bad = 1, mp_nobs = 0, mp_ref_kf =
// mp_replaced = -1, empty rows, everything else 0, so a record with n_mp + P is valid at once; *n_new = A.
// TRUSTED, as in local_map.h and its siblings: the pointer arrays kf_mp_ptr, obs_ptr and kf_child_ptr ascend from 0 and end inside their
// tables (kf_mp_ptr[n_kf] is where the next row begins; obs_kf holds obs_ptr[n_mp] entries).  Every SLOT, index, weight and record number
// read from an op, a row or a frame record is checked before use.
// COST: an ASSOCIATE looks through every edit the call has emitted so far for those that name its keyframe, so a list of A ASSOCIATE ops
// costs O(A x edits).  A keyframe cadence has one ASSOCIATE per list.
// ONE GATE, decided before anything is written, from the list and the frame records alone (upper bounds): keyframes n_kf + the NEW_KF
// ops with a frame record; points n_mp + P; keypoints kf_mp_ptr[n_kf] + their n_kp; edits 2 P + the n_kp of the ASSOCIATE ops; recent
// entries n_recent + the MG_RECENT ops + that same sum.  A bound that fails, a frame record above MG_MAX_KP named by an op, or a list
// above the capacity it was given: the five needs and a status bit per failure are written and NOTHING else.
#ifndef SLAMIT_MAP_GROW_H
#define SLAMIT_MAP_GROW_H
#include <stddef.h>
#include <stdint.h>

#include "local_map.h"
#include "map_edit.h"

#define MG_MAX_OPS 65536       // ops per list
#define MG_MAX_FRAMES 16       // frame records per call: they travel as the kernel's argument
#define MG_MAX_KP 30000        // keypoints of a frame record: SLAMIT_FRAME_MAX_KP

enum { MG_NEW_KF = 1, MG_NEW_POINT = 2, MG_ASSOCIATE = 3 };   // kind
enum { MG_RECENT = 1 };                                       // flags
enum { MG_OP_REJECTED = -1, MG_OP_BAD = -2 };                 // op_status below 0; else the slot given (NEW_KF, NEW_POINT) or kf (ASSOCIATE)
// per map: the first seven are the gate's
enum { MG_KF_OVERFLOW = 1, MG_MP_OVERFLOW = 2, MG_KFMP_OVERFLOW = 4, MG_EDIT_OVERFLOW = 8, MG_RECENT_OVERFLOW = 16, MG_KP_OVERFLOW = 32, MG_OPS_OVERFLOW = 64,
       MG_BAD_SLOT = 128 };
enum { MG_REFUSED = 127 };
enum { MG_NEED_KF = 0, MG_NEED_MP, MG_NEED_KFMP, MG_NEED_EDIT, MG_NEED_RECENT, MG_NNEED };

struct MgOp {   // the layout of slamit_grow_op
    int32_t kind, flags;
    int32_t kf, src, kf_id;        // NEW_KF / ASSOCIATE: the keyframe, its frame record, mnId.  NEW_POINT: kf = ref, kf_id = first_kf_id
    int32_t cand;
    int32_t kf_a, idx_a, kf_b, idx_b;
    uint8_t weight_a, weight_b, pad[2];
    float pos[3];
};

struct MgFrame {   // the layout of slamit_grow_frame
    int32_t n_kp; float th_depth;
    const int32_t* frame_mp; const uint8_t* octave; const uint8_t* desc; const float* depth; const float* uright; const float* Tcw;
};

struct MgIndex {   // the layout of slamit_grow_index
    int32_t kf_cap, mp_cap, kfmp_cap, reserved;
    int32_t* kf_mp_ptr; int32_t* kf_mp; uint8_t* kf_octave; uint8_t* kf_desc; float* kf_depth;
    uint8_t* kf_bad; int32_t* kf_parent; uint8_t* kf_to_be_erased; uint8_t* kf_not_erase; float* kf_th_depth;
    int32_t* kf_best; int32_t* cw_n; int32_t* ord_n; int32_t* kf_child_ptr; float* kf_center;
    float* mp_pos; float* mp_normal; float* mp_max_dist; float* mp_min_dist;
    uint8_t* mp_bad; int32_t* mp_nobs; int32_t* mp_ref_kf; int32_t* mp_found; int32_t* mp_visible; int32_t* mp_first_kf; int32_t* mp_replaced;
    uint8_t* mp_desc; int32_t* obs_ptr;
};

// KeyFrame::SetPose: Ow = -Rcw^T tcw of the row-major 3x4 Tcw, in float, each component as ((R0j t0 + R1j t1) + R2j t2) negated.  The
// build never contracts a multiply into an add (-ffp-contract=off), so g++ and the device give the same bits.
LM_HD void mg_center(const float* T, float* c) {
    for (int j = 0; j < 3; ++j) {
        const float a = T[j] * T[3], b = T[4 + j] * T[7], d = T[8 + j] * T[11];
        c[j] = -((a + b) + d);
    }
}
LM_HD bool mg_frame_ok(int src, int n_frames) { return (unsigned)src < (unsigned)n_frames; }
// what an op adds to the gate's five sums.  kp_over: a named frame record above MG_MAX_KP.
struct MgSums { int n_new_kf, kp_new, n_points, kp_assoc, n_recent_ops, kp_over; };
LM_HD void mg_gate_add(const MgOp& e, int n_frames, const MgFrame* frames, MgSums& s) {
    if (e.kind == MG_NEW_POINT) { ++s.n_points; s.n_recent_ops += (e.flags & MG_RECENT) != 0; return; }
    if ((e.kind != MG_NEW_KF && e.kind != MG_ASSOCIATE) || !mg_frame_ok(e.src, n_frames)) return;
    const int n_kp = frames[e.src].n_kp;
    if (n_kp < 0) return;
    if (n_kp > MG_MAX_KP) { s.kp_over = 1; return; }
    if (e.kind == MG_NEW_KF) { ++s.n_new_kf; s.kp_new += n_kp; } else s.kp_assoc += n_kp;
}
// the needs and the status of the gate; over_ops: the list was longer than the capacity it came in
LM_HD int mg_gate(const MgSums& s, bool over_ops, int n_kf, int n_mp, int n_kfmp, int n_recent, const MgIndex& X, int edit_cap, int recent_cap, int32_t* need) {
    need[MG_NEED_KF] = n_kf + s.n_new_kf; need[MG_NEED_MP] = n_mp + s.n_points; need[MG_NEED_KFMP] = n_kfmp + s.kp_new;
    need[MG_NEED_EDIT] = 2 * s.n_points + s.kp_assoc; need[MG_NEED_RECENT] = n_recent + s.n_recent_ops + s.kp_assoc;
    return (need[MG_NEED_KF] > X.kf_cap ? MG_KF_OVERFLOW : 0) | (need[MG_NEED_MP] > X.mp_cap ? MG_MP_OVERFLOW : 0) | (need[MG_NEED_KFMP] > X.kfmp_cap ? MG_KFMP_OVERFLOW : 0) |
           (need[MG_NEED_EDIT] > edit_cap ? MG_EDIT_OVERFLOW : 0) | (need[MG_NEED_RECENT] > recent_cap ? MG_RECENT_OVERFLOW : 0) | (s.kp_over ? MG_KP_OVERFLOW : 0) |
           (over_ops ? MG_OPS_OVERFLOW : 0);
}
// can the walk apply the op, with cur_kf keyframes at that moment?
LM_HD bool mg_new_kf_ok(const MgOp& e, int cur_kf, int n_frames, const MgFrame* frames) {
    return e.kf == cur_kf && mg_frame_ok(e.src, n_frames) && frames[e.src].n_kp >= 0 && frames[e.src].n_kp <= MG_MAX_KP;
}
LM_HD bool mg_obs_ok(const MgIndex& X, int cur_kf, int kf, int idx, int weight) {
    return (unsigned)kf < (unsigned)cur_kf && idx >= 0 && idx < X.kf_mp_ptr[kf + 1] - X.kf_mp_ptr[kf] && (weight == 1 || weight == 2);
}
LM_HD bool mg_new_point_ok(const MgOp& e, const MgIndex& X, int cur_kf, int cand_cap) {
    return (unsigned)e.kf < (unsigned)cur_kf && e.cand >= -1 && e.cand < cand_cap && mg_obs_ok(X, cur_kf, e.kf_a, e.idx_a, e.weight_a) &&
           (e.kf_b == -1 || mg_obs_ok(X, cur_kf, e.kf_b, e.idx_b, e.weight_b));
}
LM_HD bool mg_associate_ok(const MgOp& e, const MgIndex& X, int cur_kf, int n_frames, const MgFrame* frames) {
    return (unsigned)e.kf < (unsigned)cur_kf && mg_frame_ok(e.src, n_frames) && frames[e.src].n_kp >= 0 && frames[e.src].n_kp <= MG_MAX_KP &&
           X.kf_mp_ptr[e.kf + 1] - X.kf_mp_ptr[e.kf] == frames[e.src].n_kp;
}
// the edit an observation emits
LM_HD MeEdit mg_edit(const MgIndex& X, int p, int kf, int idx, int weight) {
    MeEdit e;
    e.kind = ME_ADD_OBS; e.flags = 0; e.mp = p; e.kf = kf; e.idx = idx; e.octave = X.kf_octave[X.kf_mp_ptr[kf] + idx]; e.weight = (uint8_t)weight;
    e.pad[0] = 0; e.pad[1] = 0;
    return e;
}
// the columns of a new keyframe whose row ends at `end` (one lane)
LM_HD void mg_kf_columns(const MgIndex& X, int kf, int end, const MgFrame& F) {
    X.kf_mp_ptr[kf + 1] = end;
    X.kf_bad[kf] = 0; X.kf_parent[kf] = -1; X.kf_to_be_erased[kf] = 0; X.kf_not_erase[kf] = 0;
    if (X.kf_th_depth) X.kf_th_depth[kf] = F.th_depth;
    for (int b = 0; b < LM_BEST; ++b) X.kf_best[(size_t)kf * LM_BEST + b] = -1;
    X.cw_n[kf] = 0; X.ord_n[kf] = 0;
    X.kf_child_ptr[kf + 1] = X.kf_child_ptr[kf];
    mg_center(F.Tcw, X.kf_center + (size_t)kf * 3);
}
// the columns of point slot p (one lane): a new point, or with inert the tail's
LM_HD void mg_point_columns(const MgIndex& X, int p, bool inert, const float* pos, int ref, int first_kf_id) {
    for (int c = 0; c < 3; ++c) { X.mp_pos[(size_t)p * 3 + c] = inert ? 0.0f : pos[c]; X.mp_normal[(size_t)p * 3 + c] = 0.0f; }
    X.mp_max_dist[p] = 0.0f; X.mp_min_dist[p] = 0.0f;
    X.mp_bad[p] = inert ? 1 : 0; X.mp_nobs[p] = 0; X.mp_ref_kf[p] = inert ? -1 : ref;
    X.mp_found[p] = inert ? 0 : 1; X.mp_visible[p] = inert ? 0 : 1; X.mp_first_kf[p] = inert ? 0 : first_kf_id; X.mp_replaced[p] = -1;
    for (int b = 0; b < 32; ++b) X.mp_desc[(size_t)p * 32 + b] = 0;
}
// an entry of a frame's point list as the new row takes it
LM_HD int mg_row_entry(int p, int n_points_now, int& bits) {
    if (p >= -1 && p < n_points_now) return p;
    bits |= MG_BAD_SLOT;
    return -1;
}

// ---- the sequential statement (host builds; the kernel does the same with the parallelism inside an op) ------------------------
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC__)
#include <set>
#include <utility>

// The list over one map.  obs_kf: the observation table beside X.obs_ptr.  recent[recent_cap] / *n_recent in / out.  need[MG_NNEED] and
// *status are always written; with a bit of MG_REFUSED nothing else is.
static inline void mg_apply_seq(int n_kf, int n_mp, const int32_t* obs_kf, const MgIndex& X, int n_frames, const MgFrame* frames, int n_given, int cap, const MgOp* ops,
                                int cand_cap, const uint8_t* cand_status, const float* cand_x3d, int32_t* op_status, int edit_cap, MeEdit* edits, int32_t* n_edits_out,
                                int recent_cap, int32_t* recent, int32_t* n_recent, int32_t* n_new, int32_t* need, int32_t* status) {
    const int n = lm_list_n(n_given, cap), nrec0 = lm_list_n(*n_recent, recent_cap);
    MgSums s = MgSums();
    for (int i = 0; i < n; ++i) mg_gate_add(ops[i], n_frames, frames, s);
    const int gate = mg_gate(s, n_given > cap, n_kf, n_mp, X.kf_mp_ptr[n_kf], nrec0, X, edit_cap, recent_cap, need);
    *status = gate;
    if (gate) return;
    int cur_kf = n_kf, end = X.kf_mp_ptr[n_kf], acc = 0, ned = 0, nrec = nrec0, bits = 0;
    std::set<std::pair<int, int> > added;   // the (point, keyframe) of every ADD_OBS emitted so far
    for (int i = 0; i < n; ++i) {
        const MgOp& e = ops[i];
        if (e.kind == MG_NEW_KF) {
            if (!mg_new_kf_ok(e, cur_kf, n_frames, frames)) { op_status[i] = MG_OP_BAD; bits |= MG_BAD_SLOT; continue; }
            const MgFrame& F = frames[e.src];
            for (int k = 0; k < F.n_kp; ++k) {
                X.kf_mp[end + k] = mg_row_entry(F.frame_mp[k], n_mp + acc, bits);
                X.kf_octave[end + k] = F.octave[k];
                for (int b = 0; b < 32; ++b) X.kf_desc[(size_t)(end + k) * 32 + b] = F.desc[(size_t)k * 32 + b];
                if (X.kf_depth) X.kf_depth[end + k] = F.depth ? F.depth[k] : -1.0f;
            }
            end += F.n_kp;
            mg_kf_columns(X, cur_kf, end, F);
            op_status[i] = cur_kf++;
        } else if (e.kind == MG_NEW_POINT) {
            if (!mg_new_point_ok(e, X, cur_kf, cand_cap)) { op_status[i] = MG_OP_BAD; bits |= MG_BAD_SLOT; continue; }
            if (e.cand >= 0 && cand_status[e.cand] != 0) { op_status[i] = MG_OP_REJECTED; continue; }
            const int p = n_mp + acc++;
            mg_point_columns(X, p, false, e.cand >= 0 ? cand_x3d + 3 * (size_t)e.cand : e.pos, e.kf, e.kf_id);
            X.kf_mp[X.kf_mp_ptr[e.kf_a] + e.idx_a] = p;
            edits[ned++] = mg_edit(X, p, e.kf_a, e.idx_a, e.weight_a);
            added.insert(std::make_pair(p, e.kf_a));
            if (e.kf_b != -1) {
                X.kf_mp[X.kf_mp_ptr[e.kf_b] + e.idx_b] = p;
                edits[ned++] = mg_edit(X, p, e.kf_b, e.idx_b, e.weight_b);
                added.insert(std::make_pair(p, e.kf_b));
            }
            if (e.flags & MG_RECENT) recent[nrec++] = p;
            op_status[i] = p;
        } else if (e.kind == MG_ASSOCIATE) {
            if (!mg_associate_ok(e, X, cur_kf, n_frames, frames)) { op_status[i] = MG_OP_BAD; bits |= MG_BAD_SLOT; continue; }
            const MgFrame& F = frames[e.src];
            const int r0 = X.kf_mp_ptr[e.kf];
            for (int k = 0; k < F.n_kp; ++k) {
                const int p = X.kf_mp[r0 + k];
                if (p == -1) continue;
                if ((unsigned)p >= (unsigned)(n_mp + acc)) { bits |= MG_BAD_SLOT; continue; }
                if (X.mp_bad[p]) continue;
                bool in = added.count(std::make_pair(p, (int)e.kf)) != 0;
                if (!in && p < n_mp)
                    for (int o = X.obs_ptr[p]; o < X.obs_ptr[p + 1] && !in; ++o) in = obs_kf[o] == e.kf;
                if (in) { recent[nrec++] = p; continue; }
                edits[ned++] = mg_edit(X, p, e.kf, k, F.uright && F.uright[k] >= 0.0f ? 2 : 1);
                added.insert(std::make_pair(p, (int)e.kf));
            }
            op_status[i] = e.kf;
        } else { op_status[i] = MG_OP_BAD; bits |= MG_BAD_SLOT; }
    }
    for (int t = 0; t < s.n_points; ++t) {
        X.obs_ptr[n_mp + t + 1] = X.obs_ptr[n_mp];
        if (t >= acc) mg_point_columns(X, n_mp + t, true, 0, -1, 0);
    }
    *n_edits_out = ned; *n_recent = nrec; *n_new = acc; *status = bits;
}
#endif

#endif
