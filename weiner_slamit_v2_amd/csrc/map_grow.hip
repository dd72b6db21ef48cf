// map_grow.hip — new keyframes and new map points appended to the resident tables by one call (include/slamit.h,
// slamit_map_grow_batch_dev; the walk is stated in map_grow.h, whose per-element functions the kernel calls).  The only float work is
// mg_center.  No workgroup waits on another: ONE workgroup of 512 threads per map does everything, in two phases.
//   the gate   the five sums of mg_gate_add over the list, a lane per op, each reduced by the workgroup scan of wave_ops.h; lane 0 writes the
//              needs and the status.  A refused map ends here: nothing else of it is written.
//   the walk   the list in order.  NEW_KF: the row, octaves and depths a lane per keypoint, the descriptors as 16-byte words, the columns by
//              lane 0.  A RUN of consecutive NEW_POINT ops: a lane per op, up to 512 at once; the slots, the places of the edits and of the
//              recent entries come from one packed workgroup scan over (accepted, second observers, recent); of two kf_mp writes to one
//              entry inside the run only the later is stored (keys in LDS, a lane looks at the entries behind its own).  ASSOCIATE: the
//              ADD_OBS edits emitted so far that name the keyframe stamp mark[p]; a lane per keypoint classifies its entry (class in LDS);
//              the first occurrence of a point in the row is the minimum of (op stamp, keypoint) under atomicMin, read back at agent
//              scope; then the row in chunks of 512, edits and recent entries placed by the packed scan, in keypoint order.
// Arrays written by some lanes and read by others of the same workgroup are read behind a workgroup barrier.
// The stamps count ASSOCIATE ops of the call, so the two workspace rows are cleared once, on the stream, not per op.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"
#include "map_check.h"
#include "map_grow.h"

static_assert(sizeof(MgOp) == sizeof(slamit_grow_op) && sizeof(MgOp) == 56 && offsetof(MgOp, cand) == offsetof(slamit_grow_op, cand) &&
                  offsetof(MgOp, kf_b) == offsetof(slamit_grow_op, kf_b) && offsetof(MgOp, weight_a) == offsetof(slamit_grow_op, weight_a) &&
                  offsetof(MgOp, pos) == offsetof(slamit_grow_op, pos) && offsetof(MgOp, kf_id) == offsetof(slamit_grow_op, kf_id),
              "slamit_grow_op is MgOp");
static_assert(sizeof(MgFrame) == sizeof(slamit_grow_frame) && sizeof(MgFrame) == 56 && offsetof(MgFrame, th_depth) == offsetof(slamit_grow_frame, th_depth) &&
                  offsetof(MgFrame, frame_mp) == offsetof(slamit_grow_frame, frame_mp) && offsetof(MgFrame, Tcw) == offsetof(slamit_grow_frame, Tcw),
              "slamit_grow_frame is MgFrame");
static_assert(sizeof(MgIndex) == sizeof(slamit_grow_index) && sizeof(MgIndex) == 240 && offsetof(MgIndex, kf_mp_ptr) == offsetof(slamit_grow_index, kf_mp_ptr) &&
                  offsetof(MgIndex, kf_center) == offsetof(slamit_grow_index, kf_center) && offsetof(MgIndex, mp_pos) == offsetof(slamit_grow_index, mp_pos) &&
                  offsetof(MgIndex, mp_desc) == offsetof(slamit_grow_index, mp_desc) && offsetof(MgIndex, obs_ptr) == offsetof(slamit_grow_index, obs_ptr),
              "slamit_grow_index is MgIndex");
static_assert(sizeof(MeEdit) == sizeof(slamit_map_edit), "slamit_map_edit is MeEdit");
static_assert(MG_NEW_KF == SLAMIT_GROW_NEW_KF && MG_NEW_POINT == SLAMIT_GROW_NEW_POINT && MG_ASSOCIATE == SLAMIT_GROW_ASSOCIATE && MG_RECENT == SLAMIT_GROW_RECENT &&
                  MG_OP_REJECTED == SLAMIT_GROW_OP_REJECTED && MG_OP_BAD == SLAMIT_GROW_OP_BAD && MG_KF_OVERFLOW == SLAMIT_GROW_KF_OVERFLOW &&
                  MG_MP_OVERFLOW == SLAMIT_GROW_MP_OVERFLOW && MG_KFMP_OVERFLOW == SLAMIT_GROW_KFMP_OVERFLOW && MG_EDIT_OVERFLOW == SLAMIT_GROW_EDIT_OVERFLOW &&
                  MG_RECENT_OVERFLOW == SLAMIT_GROW_RECENT_OVERFLOW && MG_KP_OVERFLOW == SLAMIT_GROW_KP_OVERFLOW && MG_OPS_OVERFLOW == SLAMIT_GROW_OPS_OVERFLOW &&
                  MG_BAD_SLOT == SLAMIT_GROW_BAD_SLOT && MG_MAX_OPS == SLAMIT_GROW_MAX_OPS && MG_MAX_FRAMES == SLAMIT_GROW_MAX_FRAMES &&
                  MG_MAX_KP == SLAMIT_FRAME_MAX_KP && MG_NNEED == SLAMIT_GROW_NEEDS,
              "map_grow.h restates the C-ABI's constants");

#define MG_NT 512
static_assert(MG_NT <= 1023, "three counts of at most MG_NT each share one scanned word, ten bits apiece");
#define MG_STAMP_MAX 0x1ffffu  // ASSOCIATE ops of one list are below MG_MAX_OPS <= this: 17 bits above the keypoint's 15
static_assert(MG_MAX_OPS <= MG_STAMP_MAX && MG_MAX_KP < (1 << 15), "the first-occurrence key: stamp << 15 | keypoint");
static_assert((long long)MG_MAX_OPS * MG_MAX_KP + 3LL * MG_MAX_OPS + SLAMIT_UPKEEP_MAX_RECENT < 0x7fffffffLL, "the gate's sums stay inside int32");

struct MgMapD { int32_t n_kf, n_mp; const int32_t* obs_kf; };

// The batch as the kernel's argument: below the 4 KiB a kernel takes.
struct MgBatch {
    int32_t n_maps, cap, n_frames, cand_cap, edit_cap, recent_cap, mp_cap, reserved;
    MgMapD maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    MgIndex X[SLAMIT_LOCAL_MAP_MAX_MAPS];
    MgFrame frames[MG_MAX_FRAMES];
    const MgOp* ops; const int32_t* n; const uint8_t* cand_status; const float* cand_x3d;
    int32_t* op_status; MeEdit* edits; int32_t* n_edits_out; int32_t* recent; int32_t* n_recent; int32_t* n_new; int32_t* need; int32_t* status;
    uint32_t* first;           // [n_maps][mp_cap]  set to ~0: the least (MG_STAMP_MAX - stamp) << 15 | keypoint that wants to add the point
    int32_t* mark;             // [n_maps][mp_cap]  cleared: stamp + 1 of the ASSOCIATE op for whose keyframe an ADD_OBS of the point was emitted
};
static_assert(sizeof(MgBatch) <= 4096, "the records travel as the kernel's argument");

static size_t mg_ws_layout(int n_maps, int mp_cap, unsigned char* base, MgBatch* B, size_t* first_bytes) {
    const size_t row = (((size_t)mp_cap * 4 + 15) & ~(size_t)15) * (size_t)n_maps;
    if (first_bytes) *first_bytes = row;
    if (B) { B->first = (uint32_t*)base; B->mark = (int32_t*)(base + row); }
    return 2 * row + 16;
}

__device__ __forceinline__ uint32_t mg_first_key(int stamp, int kp) { return ((MG_STAMP_MAX - (uint32_t)stamp) << 15) | (uint32_t)kp; }
// the workgroup's sum
__device__ __forceinline__ int mg_block_sum(int v) {
    int total;
    block_inclusive_scan_i32<MG_NT>(v, total);
    return total;
}

// ---- grid (maps), 512 threads -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MG_NT) void mg_walk_kernel(MgBatch B) {
    __shared__ unsigned long long wkey[2 * MG_NT];                      // the kf_mp entries a run of NEW_POINT ops names, in list order
    __shared__ uint8_t cls[MG_MAX_KP];                                  // ASSOCIATE: 0 skipped, 1 already in the keyframe, 2 wants to add
    __shared__ int32_t s_run, s_bits, s_gate;
    const int m = blockIdx.x, tid = threadIdx.x;
    const MgMapD M = B.maps[m];
    const MgIndex& X = B.X[m];
    const int n_raw = B.n[m], n = lm_list_n(n_raw, B.cap);
    const MgOp* const ops = B.ops + (size_t)m * B.cap;
    int32_t* const ost = B.op_status + (size_t)m * B.cap;
    MeEdit* const edits = B.edits + (size_t)m * B.edit_cap;
    int32_t* const recent = B.recent + (size_t)m * B.recent_cap;
    const uint8_t* const cand_status = B.cand_status + (size_t)m * B.cand_cap;
    const float* const cand_x3d = B.cand_x3d + (size_t)m * B.cand_cap * 3;
    uint32_t* const first = B.first + (size_t)m * (((size_t)B.mp_cap + 3) & ~(size_t)3);
    int32_t* const mark = B.mark + (size_t)m * (((size_t)B.mp_cap + 3) & ~(size_t)3);
    const int nrec0 = lm_list_n(B.n_recent[m], B.recent_cap);

    // ---- the gate
    MgSums s = MgSums();
    for (int i = tid; i < n; i += MG_NT) mg_gate_add(ops[i], B.n_frames, B.frames, s);
    s.n_new_kf = mg_block_sum(s.n_new_kf); s.kp_new = mg_block_sum(s.kp_new); s.n_points = mg_block_sum(s.n_points);
    s.kp_assoc = mg_block_sum(s.kp_assoc); s.n_recent_ops = mg_block_sum(s.n_recent_ops); s.kp_over = mg_block_sum(s.kp_over);
    if (tid == 0) {
        int32_t need[MG_NNEED];
        const int gate = mg_gate(s, n_raw > B.cap, M.n_kf, M.n_mp, X.kf_mp_ptr[M.n_kf], nrec0, X, B.edit_cap, B.recent_cap, need);
        for (int q = 0; q < MG_NNEED; ++q) B.need[MG_NNEED * m + q] = need[q];
        if (gate) B.status[m] = gate;
        s_gate = gate; s_bits = 0;
    }
    __syncthreads();
    if (s_gate) return;                                                 // the whole workgroup

    // ---- the walk: these five are the same in every thread
    int cur_kf = M.n_kf, end = X.kf_mp_ptr[M.n_kf], acc = 0, ned = 0, nrec = nrec0, stamp = 0;
    for (int i = 0; i < n;) {
        const MgOp e = ops[i];
        if (e.kind == MG_NEW_POINT) {
            // the run from i on, at most MG_NT ops: lane t has op i + t
            const int at = i + tid;
            const bool is = at < n && ops[at].kind == MG_NEW_POINT;
            if (tid == 0) s_run = MG_NT;
            int unused;
            const int before = block_inclusive_scan_i32<MG_NT>(is ? 0 : 1, unused);
            if (!is && before == 1) s_run = tid;                        // the first lane outside the run
            __syncthreads();
            const int run = s_run;
            const bool act = tid < run;
            MgOp o = MgOp();
            bool ok = false, take = false;
            if (act) {
                o = ops[at];
                ok = mg_new_point_ok(o, X, cur_kf, B.cand_cap);
                take = ok && (o.cand < 0 || cand_status[o.cand] == 0);
            }
            const bool two = take && o.kf_b != -1, rec = take && (o.flags & MG_RECENT);
            const int v = (take ? 1 : 0) | (two ? 1 << 10 : 0) | (rec ? 1 << 20 : 0);
            int total;
            const int excl = block_inclusive_scan_i32<MG_NT>(v, total) - v;
            const int p = M.n_mp + acc + (excl & 1023);
            const int ea = (act && take) ? X.kf_mp_ptr[o.kf_a] + o.idx_a : -1, eb = two ? X.kf_mp_ptr[o.kf_b] + o.idx_b : -1;
            wkey[2 * tid] = (unsigned long long)(long long)ea; wkey[2 * tid + 1] = (unsigned long long)(long long)eb;
            __syncthreads();
            if (act) {
                if (take) {
                    const bool from_cand = o.cand >= 0;                    // (selected by value: a pointer chosen between the op and the array keeps the op in scratch)
                    const size_t c3 = from_cand ? 3 * (size_t)o.cand : 0;
                    const float pos[3] = {from_cand ? cand_x3d[c3] : o.pos[0], from_cand ? cand_x3d[c3 + 1] : o.pos[1], from_cand ? cand_x3d[c3 + 2] : o.pos[2]};
                    mg_point_columns(X, p, false, pos, o.kf, o.kf_id);
                    int ep = ned + (excl & 1023) + ((excl >> 10) & 1023);
                    edits[ep++] = mg_edit(X, p, o.kf_a, o.idx_a, o.weight_a);
                    if (two) edits[ep] = mg_edit(X, p, o.kf_b, o.idx_b, o.weight_b);
                    if (rec) recent[nrec + (excl >> 20)] = p;
                    // the last write of the list to an entry wins: mine is stored unless one behind it names the same entry
                    bool wa = true, wb = two;
                    const unsigned long long ka = wkey[2 * tid], kb = wkey[2 * tid + 1];
                    for (int q = 2 * tid + 1; q < 2 * run; ++q) {
                        const unsigned long long k = wkey[q];
                        wa = wa && k != ka;
                        wb = wb && (q == 2 * tid + 1 || k != kb);
                    }
                    if (wa) X.kf_mp[ea] = p;
                    if (wb) X.kf_mp[eb] = p;
                }
                ost[at] = take ? p : (ok ? MG_OP_REJECTED : MG_OP_BAD);
                if (!ok) atomicOr(&s_bits, MG_BAD_SLOT);
            }
            acc += total & 1023; ned += (total & 1023) + ((total >> 10) & 1023); nrec += total >> 20;
            i += run;
            __syncthreads();
            continue;
        }
        if (e.kind == MG_NEW_KF && mg_new_kf_ok(e, cur_kf, B.n_frames, B.frames)) {
            const MgFrame& F = B.frames[e.src];
            int bits = 0;
            for (int k = tid; k < F.n_kp; k += MG_NT) {
                X.kf_mp[end + k] = mg_row_entry(F.frame_mp[k], M.n_mp + acc, bits);
                X.kf_octave[end + k] = F.octave[k];
                if (X.kf_depth) X.kf_depth[end + k] = F.depth ? F.depth[k] : -1.0f;
            }
            const uint4* const src = reinterpret_cast<const uint4*>(F.desc);
            uint4* const dst = reinterpret_cast<uint4*>(X.kf_desc + (size_t)end * 32);
            for (int q = tid; q < 2 * F.n_kp; q += MG_NT) dst[q] = src[q];
            if (bits) atomicOr(&s_bits, bits);
            end += F.n_kp;
            if (tid == 0) { mg_kf_columns(X, cur_kf, end, F); ost[i] = cur_kf; }
            ++cur_kf; ++i;
            __syncthreads();
            continue;
        }
        if (e.kind == MG_ASSOCIATE && mg_associate_ok(e, X, cur_kf, B.n_frames, B.frames)) {
            const MgFrame& F = B.frames[e.src];
            const int kf = e.kf, r0 = X.kf_mp_ptr[kf], n_kp = F.n_kp, n_now = M.n_mp + acc;
            // the points an emitted ADD_OBS already gave this keyframe
            for (int q = tid; q < ned; q += MG_NT) {
                const MeEdit d = edits[q];
                if (d.kf == kf && (unsigned)d.mp < (unsigned)n_now) mark[d.mp] = stamp + 1;
            }
            __syncthreads();
            int bits = 0;
            for (int k = tid; k < n_kp; k += MG_NT) {
                const int p = X.kf_mp[r0 + k];
                uint8_t c = 0;
                if (p != -1) {
                    if ((unsigned)p >= (unsigned)n_now) bits |= MG_BAD_SLOT;
                    else if (!X.mp_bad[p]) {
                        bool in = mark[p] == stamp + 1;
                        if (!in && p < M.n_mp)
                            for (int q = X.obs_ptr[p]; q < X.obs_ptr[p + 1] && !in; ++q) in = M.obs_kf[q] == kf;
                        c = in ? 1 : 2;
                        if (!in) atomicMin(&first[p], mg_first_key(stamp, k));
                    }
                }
                cls[k] = c;
            }
            if (bits) atomicOr(&s_bits, bits);
            __syncthreads();
            for (int k0 = 0; k0 < n_kp; k0 += MG_NT) {                  // every thread walks the same rounds
                const int k = k0 + tid;
                const int c = k < n_kp ? cls[k] : 0;
                const int p = c ? X.kf_mp[r0 + k] : -1;
                const bool add = c == 2 && __hip_atomic_load(&first[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mg_first_key(stamp, k);
                const bool rec = c != 0 && !add;
                const int v = (add ? 1 : 0) | (rec ? 1 << 10 : 0);
                int total;
                const int excl = block_inclusive_scan_i32<MG_NT>(v, total) - v;
                if (add) edits[ned + (excl & 1023)] = mg_edit(X, p, kf, k, F.uright && F.uright[k] >= 0.0f ? 2 : 1);
                if (rec) recent[nrec + (excl >> 10)] = p;
                ned += total & 1023; nrec += total >> 10;
            }
            if (tid == 0) ost[i] = kf;
            ++stamp; ++i;
            __syncthreads();
            continue;
        }
        if (tid == 0) { ost[i] = MG_OP_BAD; s_bits |= MG_BAD_SLOT; }    // a kind outside 1..3, or an op the walk cannot apply
        ++i;
        __syncthreads();
    }
    // ---- the rows of the new slots and the inert tail
    const int base = X.obs_ptr[M.n_mp];
    for (int t = tid; t < s.n_points; t += MG_NT) {
        X.obs_ptr[M.n_mp + t + 1] = base;
        if (t >= acc) mg_point_columns(X, M.n_mp + t, true, nullptr, -1, 0);
    }
    __syncthreads();
    if (tid == 0) { B.n_edits_out[m] = ned; B.n_recent[m] = nrec; B.n_new[m] = acc; B.status[m] = s_bits; }
}

static hipError_t mg_launch(const MgBatch& B, size_t first_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.first, 0xff, first_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(B.mark, 0, first_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_kernel, dim3((unsigned)B.n_maps), dim3(MG_NT), 0, st, B);
    return hipGetLastError();
}

// What the host form checks of a list before anything is launched: the walk's own rules over the slots and the row lengths as the ops
// before leave them, null for a list the walk applies whole.  A frame record above MG_MAX_KP ends the look: the gate refuses that call.
static const char* mg_list_error(const slamit_map_index* map, const slamit_grow_index* X, int n_frames, const slamit_grow_frame* frames, int n, const slamit_grow_op* ops,
                                 int cand_cap, const uint8_t* cand_status) {
    std::vector<int> new_len;                                            // the rows of the keyframes the list has added so far
    int acc = 0;
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    const auto row_len = [&](int k) { return k < n_kf ? X->kf_mp_ptr[k + 1] - X->kf_mp_ptr[k] : new_len[(size_t)(k - n_kf)]; };
    const auto obs_ok = [&](int k, int i, int w) { return k >= 0 && k < n_kf + (int)new_len.size() && i >= 0 && i < row_len(k) && (w == 1 || w == 2); };
    for (int i = 0; i < n; ++i) {
        const slamit_grow_op& e = ops[i];
        const int cur_kf = n_kf + (int)new_len.size();
        if (e.kind == SLAMIT_GROW_NEW_POINT) {
            if (e.kf < 0 || e.kf >= cur_kf) return "a NEW_POINT op whose ref lies outside the keyframes that exist at that moment";
            if (e.cand < -1 || e.cand >= cand_cap) return "a NEW_POINT op whose cand lies outside [-1, cand_cap)";
            if (!obs_ok(e.kf_a, e.idx_a, e.weight_a) || (e.kf_b != -1 && !obs_ok(e.kf_b, e.idx_b, e.weight_b)))
                return "a NEW_POINT op with an observer's keyframe, index or weight outside its range";
            acc += e.cand < 0 || cand_status[e.cand] == 0;
            continue;
        }
        if (e.kind != SLAMIT_GROW_NEW_KF && e.kind != SLAMIT_GROW_ASSOCIATE) return "an op's kind outside 1..3";
        if (e.src < 0 || e.src >= n_frames) return "an op's src lies outside [0, n_frames)";
        const slamit_grow_frame& F = frames[e.src];
        if (F.n_kp > SLAMIT_FRAME_MAX_KP) return nullptr;
        if (e.kind == SLAMIT_GROW_NEW_KF) {
            if (e.kf != cur_kf) return "a NEW_KF op does not name the next free slot";
            if (!map_slots_ok(F.frame_mp, (size_t)F.n_kp, -1, n_mp + acc)) return "a frame record's frame_mp holds a point slot outside [-1, the points that exist at that moment)";
            new_len.push_back(F.n_kp);
        } else {
            if (e.kf < 0 || e.kf >= cur_kf) return "an ASSOCIATE op whose keyframe lies outside the keyframes that exist at that moment";
            if (row_len(e.kf) != F.n_kp) return "an ASSOCIATE op whose frame record does not have its keyframe's keypoints";
        }
    }
    return nullptr;
}

extern "C" {

int slamit_map_grow_apply(int device, const slamit_map_index* map, const slamit_grow_index* X, int32_t n_frames, const slamit_grow_frame* frames, int32_t n,
                          const slamit_grow_op* ops, int32_t cand_cap, const uint8_t* cand_status, const float* cand_x3d, int32_t* op_status, int32_t edit_cap,
                          slamit_map_edit* edits, int32_t* n_edits_out, int32_t recent_cap, int32_t* recent, int32_t* n_recent, int32_t* n_new, int32_t* need, int32_t* status) {
    const char* const where = "slamit_map_grow_apply";
    if (n < 0 || n_frames < 0 || cand_cap < 0 || edit_cap < 0 || recent_cap < 0 || !n_edits_out || !n_recent || !n_new || !need || !status || (n && (!ops || !op_status)) ||
        (edit_cap && !edits) || (recent_cap && !recent) || (cand_cap && (!cand_status || !cand_x3d)) || (n_frames && !frames))
        return slamit_refuse(where, "null array or negative count");
    if (n > SLAMIT_GROW_MAX_OPS) return slamit_refuse(where, "more than SLAMIT_GROW_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
    if (n_frames > SLAMIT_GROW_MAX_FRAMES) return slamit_refuse(where, "n_frames above SLAMIT_GROW_MAX_FRAMES", SLAMIT_ERR_CAPACITY);
    if (recent_cap > SLAMIT_UPKEEP_MAX_RECENT) return slamit_refuse(where, "recent_cap above SLAMIT_UPKEEP_MAX_RECENT", SLAMIT_ERR_CAPACITY);
    if (edit_cap > SLAMIT_EDIT_MAX_EDITS) return slamit_refuse(where, "edit_cap above SLAMIT_EDIT_MAX_EDITS", SLAMIT_ERR_CAPACITY);
    if (!map || !X) return slamit_refuse(where, "null table");
    if (const char* bad = map_sizes_error(map)) return slamit_refuse(where, bad);
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (X->kf_cap < n_kf || X->kf_cap > SLAMIT_LOCAL_MAP_MAX_KF || X->mp_cap < n_mp || X->kfmp_cap < 0) return slamit_refuse(where, "kf_cap outside [n_kf, SLAMIT_LOCAL_MAP_MAX_KF], mp_cap below n_mp or negative kfmp_cap");
    if (!X->kf_mp_ptr || !X->obs_ptr || !X->kf_child_ptr || !X->kf_best || !X->kf_center || (!X->kf_depth != !X->kf_th_depth)) return slamit_refuse(where, "null table");
    if (!map_csr_ok(X->kf_mp_ptr, n_kf) || !map_csr_ok(X->obs_ptr, n_mp) || !map_csr_ok(X->kf_child_ptr, n_kf)) return slamit_refuse(where, "a CSR pointer array does not ascend from 0");
    const size_t n_kfmp = (size_t)X->kf_mp_ptr[n_kf], n_obs = (size_t)X->obs_ptr[n_mp], kc = (size_t)X->kf_cap, pc = (size_t)X->mp_cap, ec = (size_t)X->kfmp_cap;
    if (n_kfmp > ec) return slamit_refuse(where, "kfmp_cap below kf_mp_ptr[n_kf]");
    if ((ec && (!X->kf_mp || !X->kf_octave || !X->kf_desc)) || (kc && (!X->kf_bad || !X->kf_parent || !X->kf_to_be_erased || !X->kf_not_erase || !X->cw_n || !X->ord_n)) ||
        (pc && (!X->mp_pos || !X->mp_normal || !X->mp_max_dist || !X->mp_min_dist || !X->mp_bad || !X->mp_nobs || !X->mp_ref_kf || !X->mp_found || !X->mp_visible ||
                !X->mp_first_kf || !X->mp_replaced || !X->mp_desc)) || (n_obs && !map->obs_kf))
        return slamit_refuse(where, "null table");
    if (!map_slots_ok(X->kf_mp, n_kfmp, -1, n_mp)) return slamit_refuse(where, "kf_mp holds a point slot outside [-1, n_mp)");
    if (!map_slots_ok(map->obs_kf, n_obs, 0, n_kf)) return slamit_refuse(where, "obs_kf holds a keyframe slot outside [0, n_kf)");
    for (int f = 0; f < n_frames; ++f) {
        const slamit_grow_frame& F = frames[f];
        if (F.n_kp < 0) return slamit_refuse(where, "a frame record with negative n_kp");
        if ((F.n_kp && (!F.frame_mp || !F.octave || !F.desc)) || !F.Tcw) return slamit_refuse(where, "a frame record with a null array");
    }
    if (const char* bad = mg_list_error(map, X, n_frames, frames, n, ops, cand_cap, cand_status)) return slamit_refuse(where, bad);
    SLAMIT_USE_DEVICE(device);
    MgBatch H;
    size_t first_bytes = 0;
    const size_t ws_bytes = mg_ws_layout(1, X->mp_cap, nullptr, nullptr, &first_bytes);
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<MgBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, MgBatch& Q) {
            io.clear();
            Q.n_maps = 1; Q.cap = n; Q.n_frames = n_frames; Q.cand_cap = cand_cap; Q.edit_cap = edit_cap; Q.recent_cap = recent_cap; Q.mp_cap = X->mp_cap;
            Q.maps[0].n_kf = n_kf; Q.maps[0].n_mp = n_mp; Q.maps[0].obs_kf = b.in(map->obs_kf, n_obs);
            MgIndex& E = Q.X[0];
            E.kf_cap = X->kf_cap; E.mp_cap = X->mp_cap; E.kfmp_cap = X->kfmp_cap;
            E.kf_mp_ptr = slamit_inout(b, io, X->kf_mp_ptr, kc + 1); E.kf_mp = slamit_inout(b, io, X->kf_mp, ec); E.kf_octave = slamit_inout(b, io, X->kf_octave, ec);
            E.kf_desc = slamit_inout(b, io, X->kf_desc, 32 * ec); E.kf_depth = slamit_inout(b, io, X->kf_depth, ec);
            E.kf_bad = slamit_inout(b, io, X->kf_bad, kc); E.kf_parent = slamit_inout(b, io, X->kf_parent, kc); E.kf_to_be_erased = slamit_inout(b, io, X->kf_to_be_erased, kc);
            E.kf_not_erase = slamit_inout(b, io, X->kf_not_erase, kc); E.kf_th_depth = slamit_inout(b, io, X->kf_th_depth, kc);
            E.kf_best = slamit_inout(b, io, X->kf_best, kc * SLAMIT_LOCAL_MAP_BEST); E.cw_n = slamit_inout(b, io, X->cw_n, kc); E.ord_n = slamit_inout(b, io, X->ord_n, kc);
            E.kf_child_ptr = slamit_inout(b, io, X->kf_child_ptr, kc + 1); E.kf_center = slamit_inout(b, io, X->kf_center, 3 * kc);
            E.mp_pos = slamit_inout(b, io, X->mp_pos, 3 * pc); E.mp_normal = slamit_inout(b, io, X->mp_normal, 3 * pc);
            E.mp_max_dist = slamit_inout(b, io, X->mp_max_dist, pc); E.mp_min_dist = slamit_inout(b, io, X->mp_min_dist, pc);
            E.mp_bad = slamit_inout(b, io, X->mp_bad, pc); E.mp_nobs = slamit_inout(b, io, X->mp_nobs, pc); E.mp_ref_kf = slamit_inout(b, io, X->mp_ref_kf, pc);
            E.mp_found = slamit_inout(b, io, X->mp_found, pc); E.mp_visible = slamit_inout(b, io, X->mp_visible, pc); E.mp_first_kf = slamit_inout(b, io, X->mp_first_kf, pc);
            E.mp_replaced = slamit_inout(b, io, X->mp_replaced, pc); E.mp_desc = slamit_inout(b, io, X->mp_desc, 32 * pc); E.obs_ptr = slamit_inout(b, io, X->obs_ptr, pc + 1);
            for (int f = 0; f < n_frames; ++f) {
                const slamit_grow_frame& F = frames[f];
                const size_t k = (size_t)F.n_kp;
                MgFrame& D = Q.frames[f];
                D.n_kp = F.n_kp; D.th_depth = F.th_depth;
                D.frame_mp = b.in(F.frame_mp, k); D.octave = b.in(F.octave, k); D.desc = b.in(F.desc, 32 * k); D.depth = b.in(F.depth, k); D.uright = b.in(F.uright, k);
                D.Tcw = b.in(F.Tcw, 12);
            }
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.ops = reinterpret_cast<const MgOp*>(b.in(ops, (size_t)n));
            Q.cand_status = b.in(cand_status, (size_t)cand_cap); Q.cand_x3d = b.in(cand_x3d, 3 * (size_t)cand_cap);
            Q.op_status = slamit_inout(b, io, op_status, (size_t)n);
            Q.edits = reinterpret_cast<MeEdit*>(slamit_inout(b, io, edits, (size_t)edit_cap));
            Q.recent = slamit_inout(b, io, recent, (size_t)recent_cap);
            Q.n_edits_out = slamit_inout(b, io, n_edits_out, 1); Q.n_recent = slamit_inout(b, io, n_recent, 1); Q.n_new = slamit_inout(b, io, n_new, 1);
            Q.need = b.out(need, MG_NNEED); Q.status = b.out(status, 1);
            unsigned char* const ws = b.scratch<unsigned char>(ws_bytes);
            if (ws) mg_ws_layout(1, X->mp_cap, ws, &Q, nullptr);
            H = Q;
        },
        [&](const MgBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : mg_launch(H, first_bytes, S.st);
        });
}

size_t slamit_map_grow_workspace(int n_maps, int mp_cap) {
    if (n_maps < 1 || n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || mp_cap < 0) return 0;
    return mg_ws_layout(n_maps, mp_cap, nullptr, nullptr, nullptr);
}

int slamit_map_grow_batch_dev(int device, const slamit_map_grow_batch_rec* R, void* stream) {
    const char* const where = "slamit_map_grow_batch_dev";
    if (!R || R->n_maps < 0 || R->cap < 0 || R->n_frames < 0 || R->cand_cap < 0 || R->edit_cap < 0 || R->recent_cap < 0 || R->mp_cap < 0)
        return slamit_refuse(where, "bad argument");
    if (R->n_maps == 0) return SLAMIT_OK;
    if (R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->grow) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_GROW_MAX_OPS) return slamit_refuse(where, "cap above SLAMIT_GROW_MAX_OPS", SLAMIT_ERR_CAPACITY);
    if (R->n_frames > SLAMIT_GROW_MAX_FRAMES) return slamit_refuse(where, "n_frames above SLAMIT_GROW_MAX_FRAMES", SLAMIT_ERR_CAPACITY);
    if (R->recent_cap > SLAMIT_UPKEEP_MAX_RECENT) return slamit_refuse(where, "recent_cap above SLAMIT_UPKEEP_MAX_RECENT", SLAMIT_ERR_CAPACITY);
    if (R->edit_cap > SLAMIT_EDIT_MAX_EDITS) return slamit_refuse(where, "edit_cap above SLAMIT_EDIT_MAX_EDITS", SLAMIT_ERR_CAPACITY);
    if (R->n_frames && !R->frames) return slamit_refuse(where, "null array");
    for (int f = 0; f < R->n_frames; ++f) {
        const slamit_grow_frame& F = R->frames[f];
        if (F.n_kp < 0) return slamit_refuse(where, "a frame record with negative n_kp");
        if (F.n_kp && (!F.frame_mp || !F.octave || !F.desc)) return slamit_refuse(where, "a frame record with a null array");
        if (!F.Tcw) return slamit_refuse(where, "a frame record without Tcw");
        if ((uintptr_t)F.desc & 15) return slamit_refuse(where, "a frame record's desc is not 16-byte aligned");
    }
    for (int m = 0; m < R->n_maps; ++m) {
        const slamit_map_index& M = R->maps[m];
        const slamit_grow_index& X = R->grow[m];
        if (X.kf_cap < 0 || X.kf_cap > SLAMIT_LOCAL_MAP_MAX_KF || X.mp_cap < 0 || X.mp_cap > R->mp_cap || X.kfmp_cap < 0)
            return slamit_refuse(where, "a map with kf_cap outside [0, SLAMIT_LOCAL_MAP_MAX_KF], mp_cap outside [0, the batch's mp_cap] or negative kfmp_cap");
        if (M.n_kf < 0 || M.n_mp < 0 || M.n_kf > X.kf_cap || M.n_mp > X.mp_cap) return slamit_refuse(where, "a map with n_kf outside [0, kf_cap] or n_mp outside [0, mp_cap]");
        if (!X.kf_mp_ptr || !X.kf_mp || !X.kf_octave || !X.kf_desc || !X.kf_bad || !X.kf_parent || !X.kf_to_be_erased || !X.kf_not_erase || !X.kf_best || !X.cw_n ||
            !X.ord_n || !X.kf_child_ptr || !X.kf_center || !X.mp_pos || !X.mp_normal || !X.mp_max_dist || !X.mp_min_dist || !X.mp_bad || !X.mp_nobs || !X.mp_ref_kf ||
            !X.mp_found || !X.mp_visible || !X.mp_first_kf || !X.mp_replaced || !X.mp_desc || !X.obs_ptr || !M.obs_kf)
            return slamit_refuse(where, "null table");
        if (!X.kf_depth != !X.kf_th_depth) return slamit_refuse(where, "kf_depth and kf_th_depth are NULL together");
        if ((uintptr_t)X.kf_desc & 15) return slamit_refuse(where, "kf_desc is not 16-byte aligned");
    }
    if (!R->d_n || !R->d_n_edits_out || !R->d_n_recent || !R->d_n_new || !R->d_need || !R->d_status || (R->cap && (!R->d_ops || !R->d_op_status)) ||
        (R->edit_cap && !R->d_edits) || (R->recent_cap && !R->d_recent) || (R->cand_cap && (!R->d_cand_status || !R->d_cand_x3d)))
        return slamit_refuse(where, "null array");
    size_t first_bytes = 0;
    const size_t need = mg_ws_layout(R->n_maps, R->mp_cap, nullptr, nullptr, &first_bytes);
    if (!R->d_workspace || R->workspace_bytes < need || ((uintptr_t)R->d_workspace & 7)) return slamit_refuse(where, "workspace missing, misaligned or below slamit_map_grow_workspace()");
    SLAMIT_USE_DEVICE(device);
    MgBatch B;
    memset(&B, 0, sizeof(B));
    B.n_maps = R->n_maps; B.cap = R->cap; B.n_frames = R->n_frames; B.cand_cap = R->cand_cap; B.edit_cap = R->edit_cap; B.recent_cap = R->recent_cap; B.mp_cap = R->mp_cap;
    for (int m = 0; m < R->n_maps; ++m) { B.maps[m].n_kf = R->maps[m].n_kf; B.maps[m].n_mp = R->maps[m].n_mp; B.maps[m].obs_kf = R->maps[m].obs_kf; }
    memcpy(B.X, R->grow, sizeof(MgIndex) * (size_t)R->n_maps);
    if (R->n_frames) memcpy(B.frames, R->frames, sizeof(MgFrame) * (size_t)R->n_frames);
    B.ops = reinterpret_cast<const MgOp*>(R->d_ops); B.n = R->d_n; B.cand_status = R->d_cand_status; B.cand_x3d = R->d_cand_x3d;
    B.op_status = R->d_op_status; B.edits = reinterpret_cast<MeEdit*>(R->d_edits); B.n_edits_out = R->d_n_edits_out; B.recent = R->d_recent; B.n_recent = R->d_n_recent;
    B.n_new = R->d_n_new; B.need = R->d_need; B.status = R->d_status;
    mg_ws_layout(R->n_maps, R->mp_cap, (unsigned char*)R->d_workspace, &B, nullptr);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY_AT(where, hipMemsetAsync(B.first, 0xff, first_bytes, st));
    HIP_TRY_AT(where, hipMemsetAsync(B.mark, 0, first_bytes, st));
    hipLaunchKernelGGL(mg_walk_kernel, dim3((unsigned)B.n_maps), dim3(MG_NT), 0, st, B);
    HIP_TRY_AT(where, hipGetLastError());
    return SLAMIT_OK;
}

}  // extern "C"
