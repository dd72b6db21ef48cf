// kf_erase.hip — KeyFrame::SetBadFlag's graph rows and spanning tree applied to the resident tables by one call (include/slamit.h,
// slamit_kf_erase_apply / slamit_kf_erase_batch_dev; the walk is stated in kf_erase.h, whose per-element functions the kernels call).
// Nothing here is float.  No workgroup waits on another inside a kernel: the order between kernels is the stream's.
//
// The semantics are sequential and the gates are known only after the walk, so the walk runs over WORKING COPIES in the workspace and
// the caller's arrays are written by the kernels behind the gate.
// ke_init_kernel        a wavefront per keyframe: its graph rows up to their counts, its columns and its children row into the
//                       workspace; the children become a linked list (node e is entry e of the old CSR), so an insert moves nothing.
// ke_walk_kernel        ONE workgroup of 256 threads per map walks the list.  Lane 0 decides an op's early exits and loads k's children
//                       into LDS; the neighbours of k are dealt to the four wavefronts, each testing membership by ballot over the
//                       row, closing it up through its keys in LDS and placing them by cv_rank; a wavefront per child scans its ord row
//                       against the candidate bitset in LDS; the pick is wave_min_u64 of ke_pick_key, then the minimum over the
//                       wavefronts.  Lane 0 relinks the lists.  LDS: 4 x 8 KiB keys + 4 KiB children + 1 KiB flags + 8 KiB bitset,
//                       below the 64 KiB a static allocation may take.
// ke_edit_count_kernel  a wavefront per op: the non-null entries of an emitting op's kf_mp row.
// ke_finish_kernel      one workgroup per map: the scan of the edit counts, the lengths of the children lists and their scan, THE GATES,
//                       the needs and the call's status.
// ke_commit_kernel      reads the gate first.  A wavefront per op: its status and its edits by ballot; a wavefront per keyframe: the
//                       columns, the new children row, and the graph rows where the walk changed them.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"
#include "map_check.h"
#include "kf_erase.h"

static_assert(sizeof(KeOp) == sizeof(slamit_kf_op) && sizeof(KeOp) == 16 && offsetof(KeOp, kf) == offsetof(slamit_kf_op, kf) &&
                  offsetof(KeOp, parent) == offsetof(slamit_kf_op, parent),
              "slamit_kf_op is KeOp");
static_assert(sizeof(KeIndex) == sizeof(slamit_tree_index) && sizeof(KeIndex) == 120 && offsetof(KeIndex, kf_not_erase) == offsetof(slamit_tree_index, kf_not_erase) &&
                  offsetof(KeIndex, kf_bad) == offsetof(slamit_tree_index, kf_bad) && offsetof(KeIndex, kf_to_be_erased) == offsetof(slamit_tree_index, kf_to_be_erased) &&
                  offsetof(KeIndex, cw_kf) == offsetof(slamit_tree_index, cw_kf) && offsetof(KeIndex, ord_n) == offsetof(slamit_tree_index, ord_n) &&
                  offsetof(KeIndex, kf_best) == offsetof(slamit_tree_index, kf_best) && offsetof(KeIndex, child_ptr_out) == offsetof(slamit_tree_index, child_ptr_out) &&
                  offsetof(KeIndex, child_cap_out) == offsetof(slamit_tree_index, child_cap_out),
              "slamit_tree_index is KeIndex");
static_assert(sizeof(LmMap) == sizeof(slamit_map_index) && sizeof(MeEdit) == sizeof(slamit_map_edit), "slamit_map_index is LmMap, slamit_map_edit is MeEdit");
static_assert(KE_SET_PARENT == SLAMIT_KF_ERASE_SET_PARENT && KE_SET_BAD == SLAMIT_KF_ERASE_SET_BAD && KE_ORIGIN == SLAMIT_KF_ERASE_ORIGIN &&
                  KE_NOT_ERASE == SLAMIT_KF_ERASE_NOT_ERASE && KE_NO_PARENT == SLAMIT_KF_ERASE_NO_PARENT && KE_BAD_SLOT == SLAMIT_KF_ERASE_BAD_SLOT &&
                  KE_ROW_OVERFLOW == SLAMIT_KF_ERASE_ROW_OVERFLOW && KE_CHILD_OVERFLOW == SLAMIT_KF_ERASE_CHILD_OVERFLOW &&
                  KE_EDIT_OVERFLOW == SLAMIT_KF_ERASE_EDIT_OVERFLOW && KE_MAX_OPS == SLAMIT_KF_ERASE_MAX_OPS && KE_MAX_CHILD == SLAMIT_KF_ERASE_MAX_CHILD &&
                  CV_MAX_ROW == SLAMIT_COVIS_MAX_ROW,
              "kf_erase.h restates the C-ABI's constants");

#define KE_NT 256
#define KE_WALK_NT 256
#define KE_NW (KE_WALK_NT / 64)
#define KE_FIN_NT 1024
static_assert(KE_MAX_OPS <= KE_FIN_NT && KE_MAX_CHILD < 65536 && CV_MAX_ROW < 65536, "the edit counts are scanned in one pass; the pick key's fields are 16 bits");
enum { KE_F_BITS = 0, KE_F_COMMIT = 1, KE_NFLAGS = 4 };

// The batch as the kernels' argument.  The workspace rows of a map lie S = kf_cap apart, its graph rows S * row_cap (a map's own rows
// are X.row_cap <= row_cap apart inside), its list nodes `pool`.
struct KeBatch {
    int32_t n_maps, cap, kf_cap, row_cap, child_cap, edit_cap, pool, reserved;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    KeIndex X[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const KeOp* ops; const int32_t* n;
    int32_t* op_status; MeEdit* edits; int32_t* n_edits_out; int32_t* n_child_out; int32_t* status;
    int32_t* flags;            // [n_maps][KE_NFLAGS]        cleared
    uint8_t* dirty;            // [n_maps][S]                cleared: the walk changed the keyframe's graph rows
    int32_t* wcw_kf;           // [n_maps][S * row_cap]      the working graph, as the next three
    int32_t* wcw_w;
    int32_t* word_kf;
    int32_t* word_w;
    int32_t* wcw_n;            // [n_maps][S]
    int32_t* word_n;
    int32_t* wparent;
    int32_t* head;             // [n_maps][S]                the first node of the keyframe's children list, -1 for none
    int32_t* wbest;            // [n_maps][S * LM_BEST]
    uint8_t* wbad;             // [n_maps][S]
    uint8_t* wtbe;
    int32_t* node_kf;          // [n_maps][pool]
    int32_t* node_next;
    int32_t* ost;              // [n_maps][cap]              the ops' statuses
    int32_t* emit;             // [n_maps][cap]              does the op emit its keyframe's row
    int32_t* eoff;             // [n_maps][cap + 1]          the edits before the op's, the total at [n]
    int32_t* cptr;             // [n_maps][S + 1]            the new pointer array
};

static size_t ke_pool(int cap, int kf_cap, int child_cap) { return (size_t)child_cap + (size_t)cap * (size_t)std::min(KE_MAX_CHILD, kf_cap); }

static size_t ke_ws_layout(int n_maps, int cap, int kf_cap, int row_cap, int child_cap, unsigned char* base, KeBatch* B, size_t* clear_bytes) {
    const size_t S = (size_t)kf_cap, nm = (size_t)n_maps, c = (size_t)cap, rows = nm * S * (size_t)row_cap, pool = ke_pool(cap, kf_cap, child_cap);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) & ~(size_t)15; return base ? base + at : nullptr; };
    unsigned char* const flags = take(4 * nm * KE_NFLAGS);
    unsigned char* const dirty = take(nm * S);
    if (clear_bytes) *clear_bytes = off;
    unsigned char* const wcw_kf = take(4 * rows);
    unsigned char* const wcw_w = take(4 * rows);
    unsigned char* const word_kf = take(4 * rows);
    unsigned char* const word_w = take(4 * rows);
    unsigned char* const wcw_n = take(4 * nm * S);
    unsigned char* const word_n = take(4 * nm * S);
    unsigned char* const wparent = take(4 * nm * S);
    unsigned char* const head = take(4 * nm * S);
    unsigned char* const wbest = take(4 * nm * S * LM_BEST);
    unsigned char* const wbad = take(nm * S);
    unsigned char* const wtbe = take(nm * S);
    unsigned char* const node_kf = take(4 * nm * pool);
    unsigned char* const node_next = take(4 * nm * pool);
    unsigned char* const ost = take(4 * nm * c);
    unsigned char* const emit = take(4 * nm * c);
    unsigned char* const eoff = take(4 * nm * (c + 1));
    unsigned char* const cptr = take(4 * nm * (S + 1));
    if (B) {
        B->flags = (int32_t*)flags; B->dirty = dirty; B->wcw_kf = (int32_t*)wcw_kf; B->wcw_w = (int32_t*)wcw_w; B->word_kf = (int32_t*)word_kf;
        B->word_w = (int32_t*)word_w; B->wcw_n = (int32_t*)wcw_n; B->word_n = (int32_t*)word_n; B->wparent = (int32_t*)wparent; B->head = (int32_t*)head;
        B->wbest = (int32_t*)wbest; B->wbad = wbad; B->wtbe = wtbe; B->node_kf = (int32_t*)node_kf; B->node_next = (int32_t*)node_next;
        B->ost = (int32_t*)ost; B->emit = (int32_t*)emit; B->eoff = (int32_t*)eoff; B->cptr = (int32_t*)cptr; B->pool = (int32_t)pool;
    }
    return off;
}

// a map's working copies
struct KeView {
    CvIndex G;
    int32_t* parent; int32_t* head; uint8_t* bad; uint8_t* tbe; uint8_t* dirty; int32_t* node_kf; int32_t* node_next; int32_t* flags;
    int32_t pool;
};
__device__ __forceinline__ KeView ke_view(const KeBatch& B, int m) {
    const size_t S = (size_t)B.kf_cap, r0 = (size_t)m * S * (size_t)B.row_cap, p0 = (size_t)m * (size_t)B.pool;
    KeView V;
    V.G = ke_graph(B.X[m].row_cap, B.wcw_kf + r0, B.wcw_w + r0, B.wcw_n + m * S, B.word_kf + r0, B.word_w + r0, B.word_n + m * S, B.wbest + m * S * LM_BEST);
    V.parent = B.wparent + m * S; V.head = B.head + m * S; V.bad = B.wbad + m * S; V.tbe = B.wtbe + m * S; V.dirty = B.dirty + m * S;
    V.node_kf = B.node_kf + p0; V.node_next = B.node_next + p0; V.flags = B.flags + KE_NFLAGS * m; V.pool = B.pool;
    return V;
}

// ---- grid (ceil(kf_cap / 4), maps), 256 threads: a wavefront per keyframe ------------------------------------------------------
__global__ __launch_bounds__(KE_NT) void ke_init_kernel(KeBatch B) {
    const int m = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * (KE_NT / 64) + (threadIdx.x >> 6);
    const LmMap& M = B.maps[m];
    const KeIndex& X = B.X[m];
    if (j >= M.n_kf) return;                                            // the whole wavefront; n_kf <= kf_cap
    const KeView V = ke_view(B, m);
    const size_t r0 = (size_t)j * X.row_cap;
    const int ncw = cv_clamp(X.cw_n[j], X.row_cap), no = cv_clamp(X.ord_n[j], X.row_cap);
    for (int e = lane; e < ncw; e += 64) { V.G.cw_kf[r0 + e] = X.cw_kf[r0 + e]; V.G.cw_w[r0 + e] = X.cw_w[r0 + e]; }
    for (int e = lane; e < no; e += 64) { V.G.ord_kf[r0 + e] = X.ord_kf[r0 + e]; V.G.ord_w[r0 + e] = X.ord_w[r0 + e]; }
    if (lane < LM_BEST) V.G.kf_best[(size_t)j * LM_BEST + lane] = X.kf_best ? X.kf_best[(size_t)j * LM_BEST + lane] : -1;
    const int e0 = M.kf_child_ptr[j], e1 = M.kf_child_ptr[j + 1];
    const bool row_ok = e0 >= 0 && e1 >= e0 && e1 <= B.child_cap;       // a row outside the nodes is read as empty
    if (row_ok)
        for (int e = e0 + lane; e < e1; e += 64) { V.node_kf[e] = M.kf_child[e]; V.node_next[e] = e + 1 < e1 ? e + 1 : -1; }
    if (lane == 0) {
        V.G.cw_n[j] = ncw; V.G.ord_n[j] = no;
        V.parent[j] = X.kf_parent[j]; V.bad[j] = X.kf_bad[j]; V.tbe[j] = X.kf_to_be_erased[j];
        V.head[j] = row_ok && e0 < e1 ? e0 : -1;
        if (!row_ok) atomicOr(&V.flags[KE_F_BITS], KE_BAD_SLOT);
    }
}

// ---- the children lists: one lane -------------------------------------------------------------------------------------------------
// ChangeParent / AddChild: before the first entry with a larger slot, unless c is there
__device__ __forceinline__ void ke_set_parent_dev(const KeView& V, int c, int p, int& top) {
    V.parent[c] = p;
    int prev = -1, node = V.head[p];
    while (node != -1 && V.node_kf[node] < c) { prev = node; node = V.node_next[node]; }
    if (node != -1 && V.node_kf[node] == c) return;
    if (top >= V.pool) { atomicOr(&V.flags[KE_F_BITS], KE_BAD_SLOT); return; }   // cannot be: pool = the old table + every possible insert
    const int nn = top++;
    V.node_kf[nn] = c; V.node_next[nn] = node;
    if (prev < 0) V.head[p] = nn; else V.node_next[prev] = nn;
}
__device__ __forceinline__ void ke_erase_child_dev(const KeView& V, int p, int c) {
    int prev = -1, node = V.head[p];
    while (node != -1 && V.node_kf[node] != c) { prev = node; node = V.node_next[node]; }
    if (node == -1) return;
    if (prev < 0) V.head[p] = V.node_next[node]; else V.node_next[prev] = V.node_next[node];
}

// EraseConnection(k) on keyframe j by one wavefront; keys: its CV_MAX_ROW words of LDS
__device__ __forceinline__ void ke_erase_connection_dev(const KeView& V, int j, int k, unsigned long long* keys, int lane) {
    const CvIndex& G = V.G;
    int32_t* const ckf = G.cw_kf + (size_t)j * G.row_cap;
    int32_t* const cw = G.cw_w + (size_t)j * G.row_cap;
    const int n = __builtin_amdgcn_readfirstlane(cv_clamp(G.cw_n[j], G.row_cap));
    int pos = -1;
    for (int e0 = 0; e0 < n && pos < 0; e0 += 64) {
        const unsigned long long mask = __ballot(e0 + lane < n && ckf[e0 + lane] == k);
        if (mask) pos = e0 + __ffsll((long long)mask) - 1;
    }
    if (pos < 0) return;                                                // j stays byte for byte
    wave_mem_sync();                                                     // the keys of the neighbour before
    for (int e = lane; e < n; e += 64)
        if (e != pos) keys[e - (e > pos)] = cv_key(cw[e], ckf[e]);
    wave_mem_sync();
    const int n1 = n - 1;
    for (int e = lane; e < n1; e += 64) {
        ckf[e] = (int32_t)(uint32_t)keys[e]; cw[e] = (int32_t)(keys[e] >> 32);
        cv_place(G, j, keys, n1, e);
    }
    if (lane < LM_BEST) cv_pad_best(G, j, n1, lane);
    if (lane == 0) { G.cw_n[j] = n1; G.ord_n[j] = n1; V.dirty[j] = 1; }
}

// ---- grid (maps), 256 threads -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KE_WALK_NT) void ke_walk_kernel(KeBatch B) {
    __shared__ unsigned long long keys[KE_NW][CV_MAX_ROW];
    __shared__ int32_t child[KE_MAX_CHILD];
    __shared__ uint8_t alive[KE_MAX_CHILD];
    __shared__ uint32_t bits[(LM_MAX_KF + 32) / 32];                    // the neighbours seen, then the candidates
    __shared__ unsigned long long wave_pick[KE_NW];
    __shared__ int32_t s_nc[2], s_parent[2];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const LmMap& M = B.maps[m];
    const KeIndex& X = B.X[m];
    const KeView V = ke_view(B, m);
    const int n = lm_list_n(B.n[m], B.cap), rc = X.row_cap, nwords = (M.n_kf + 31) / 32;
    const KeOp* const ops = B.ops + (size_t)m * B.cap;
    int32_t* const ost = B.ost + (size_t)m * B.cap;
    int32_t* const emit = B.emit + (size_t)m * B.cap;
    int top = M.n_kf > 0 ? min(max(M.kf_child_ptr[M.n_kf], 0), B.child_cap) : 0;   // lane 0's: the first free node
    for (int i = 0; i < n; ++i) {
        const KeOp e = ops[i];
        if (tid == 0) {                                                 // the early exits, in the reference's order
            int st = 0, nc = -1, P = -1;
            if (!ke_op_ok(M, e)) st = KE_BAD_SLOT;
            else if (e.kind == KE_SET_PARENT) ke_set_parent_dev(V, e.kf, e.parent, top);
            else if (e.kf == X.origin_kf) st = KE_ORIGIN;
            else if (X.kf_not_erase[e.kf]) { V.tbe[e.kf] = 1; st = KE_NOT_ERASE; }
            else if ((P = V.parent[e.kf]) == -1) st = KE_NO_PARENT;
            else if (!lm_kf_ok(M, P)) st = KE_BAD_SLOT;
            else {
                nc = 0;
                for (int node = V.head[e.kf]; node != -1; node = V.node_next[node]) {
                    if (nc < KE_MAX_CHILD) { child[nc] = V.node_kf[node]; alive[nc] = 1; }
                    ++nc;
                }
                if (nc > KE_MAX_CHILD) { st = KE_ROW_OVERFLOW; nc = -1; }
            }
            if (st & (KE_BAD_SLOT | KE_ROW_OVERFLOW)) atomicOr(&V.flags[KE_F_BITS], st);
            s_nc[i & 1] = nc; s_parent[i & 1] = P;
            ost[i] = st; emit[i] = nc >= 0;
        }
        for (int q = tid; q < nwords; q += KE_WALK_NT) bits[q] = 0;
        __syncthreads();
        const int nc = s_nc[i & 1], P = s_parent[i & 1], k = e.kf;     // slot i & 1 is written again two barriers on
        if (nc < 0) continue;
        // 3: the neighbours, dealt to the wavefronts; each writes its neighbour's rows only, k's row is read
        const int nk = cv_clamp(V.G.cw_n[k], rc);
        for (int t = w; t < nk; t += KE_NW) {
            const int j = __builtin_amdgcn_readfirstlane(V.G.cw_kf[(size_t)k * rc + t]);
            if (!lm_kf_ok(M, j) || j == k) {
                if (lane == 0) atomicOr(&V.flags[KE_F_BITS], KE_BAD_SLOT);
                continue;
            }
            uint32_t was = 0;
            if (lane == 0) was = atomicOr(&bits[j >> 5], 1u << (j & 31));
            was = (uint32_t)__builtin_amdgcn_readfirstlane((int)was);
            if ((was >> (j & 31)) & 1u) continue;                       // listed twice: visited once
            ke_erase_connection_dev(V, j, k, keys[w], lane);
        }
        __syncthreads();
        // 5: the own rows
        if (tid == 0) { V.G.cw_n[k] = 0; V.G.ord_n[k] = 0; V.dirty[k] = 1; }
        if (tid < LM_BEST) V.G.kf_best[(size_t)k * LM_BEST + tid] = -1;
        // 6: the spanning tree
        for (int q = tid; q < nwords; q += KE_WALK_NT) bits[q] = 0;
        __syncthreads();
        if (tid == 0) bits[P >> 5] = 1u << (P & 31);
        __syncthreads();
        for (;;) {
            unsigned long long mine = KE_PICK_NONE;
            for (int ci = w; ci < nc; ci += KE_NW) {                    // a wavefront per child
                if (!alive[ci]) continue;
                const int c = child[ci];
                if (!lm_kf_ok(M, c)) {
                    if (lane == 0) atomicOr(&V.flags[KE_F_BITS], KE_BAD_SLOT);
                    continue;
                }
                if (V.bad[c]) continue;
                const int no = cv_clamp(V.G.ord_n[c], rc);
                for (int t0 = 0; t0 < no; t0 += 64) {
                    const int t = t0 + lane;
                    if (t >= no) continue;
                    const int kf = V.G.ord_kf[(size_t)c * rc + t];
                    if (!lm_kf_ok(M, kf) || !((bits[kf >> 5] >> (kf & 31)) & 1u)) continue;
                    const int wt = ke_weight(V.G, c, kf);
                    if (wt < 0) continue;                               // never above -1
                    const unsigned long long key = ke_pick_key(wt, ci, t);
                    mine = key < mine ? key : mine;
                }
            }
            mine = wave_min_u64(mine);
            if (lane == 0) wave_pick[w] = mine;
            __syncthreads();
            unsigned long long pick = KE_PICK_NONE;
            for (int u = 0; u < KE_NW; ++u) pick = wave_pick[u] < pick ? wave_pick[u] : pick;
            if (pick == KE_PICK_NONE) break;                            // the whole workgroup
            if (tid == 0) {
                const int ci = ke_pick_child(pick), c = child[ci], p = V.G.ord_kf[(size_t)c * rc + ke_pick_row(pick)];
                ke_set_parent_dev(V, c, p, top);
                ke_erase_child_dev(V, k, c);
                alive[ci] = 0;
                bits[c >> 5] |= 1u << (c & 31);
            }
            __syncthreads();
        }
        if (tid == 0) {
            for (int ci = 0; ci < nc; ++ci)
                if (alive[ci] && lm_kf_ok(M, child[ci])) ke_set_parent_dev(V, child[ci], P, top);
            ke_erase_child_dev(V, P, k);
            V.bad[k] = 1;
        }
        __syncthreads();
    }
}

// ---- grid (cap, maps), 64 threads: a wavefront per op -------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ke_edit_count_kernel(KeBatch B) {
    const int m = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    if (i >= lm_list_n(B.n[m], B.cap)) return;
    const LmMap& M = B.maps[m];
    int cnt = 0;
    if (B.emit[(size_t)m * B.cap + i]) {
        const int k = B.ops[(size_t)m * B.cap + i].kf;                  // inside the table: the walk took the op
        for (int e = M.kf_mp_ptr[k] + lane; e < M.kf_mp_ptr[k + 1]; e += 64) cnt += M.kf_mp[e] != -1;
    }
    cnt = __builtin_amdgcn_readlane(wave_inclusive_scan_i32(cnt), 63);
    if (lane == 0) B.eoff[(size_t)m * (B.cap + 1) + i] = cnt;
}

// ---- grid (maps), 1024 threads ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KE_FIN_NT) void ke_finish_kernel(KeBatch B) {
    const int m = blockIdx.x, tid = threadIdx.x;
    const LmMap& M = B.maps[m];
    const KeIndex& X = B.X[m];
    const KeView V = ke_view(B, m);
    const int n = lm_list_n(B.n[m], B.cap);
    int32_t* const eoff = B.eoff + (size_t)m * (B.cap + 1);
    int32_t* const cptr = B.cptr + (size_t)m * ((size_t)B.kf_cap + 1);
    int n_edits;
    {
        const int v = tid < n ? eoff[tid] : 0;                          // n <= KE_MAX_OPS <= the workgroup
        const int incl = block_inclusive_scan_i32<KE_FIN_NT>(v, n_edits);
        if (tid < n) eoff[tid] = incl - v;
        if (tid == 0) eoff[n] = n_edits;
    }
    int need = 0;
    for (int j0 = 0; j0 < M.n_kf; j0 += KE_FIN_NT) {                    // every thread walks the same rounds
        const int j = j0 + tid;
        int len = 0;
        if (j < M.n_kf)
            for (int node = V.head[j]; node != -1; node = V.node_next[node]) ++len;
        int total;
        const int incl = block_inclusive_scan_i32<KE_FIN_NT>(len, total);
        if (j < M.n_kf) cptr[j] = need + incl - len;
        need += total;
    }
    if (tid != 0) return;
    cptr[M.n_kf] = need;
    bool committed;
    B.status[m] = ke_call_status(need > X.child_cap_out, n_edits > B.edit_cap, V.flags[KE_F_BITS], committed);
    B.n_edits_out[m] = n_edits; B.n_child_out[m] = need;
    V.flags[KE_F_COMMIT] = committed;                                   // THE GATE of ke_commit_kernel
    if (committed) X.child_ptr_out[M.n_kf] = need;
}

// ---- grid (ceil(max(kf_cap, cap) / 4), maps), 256 threads: a wavefront per op and per keyframe -----------------------------------
__global__ __launch_bounds__(KE_NT) void ke_commit_kernel(KeBatch B) {
    const int m = blockIdx.y, lane = threadIdx.x & 63, q = blockIdx.x * (KE_NT / 64) + (threadIdx.x >> 6);
    const LmMap& M = B.maps[m];
    const KeIndex& X = B.X[m];
    const KeView V = ke_view(B, m);
    if (!V.flags[KE_F_COMMIT]) return;
    if (q < lm_list_n(B.n[m], B.cap)) {
        if (lane == 0) B.op_status[(size_t)m * B.cap + q] = B.ost[(size_t)m * B.cap + q];
        if (B.emit[(size_t)m * B.cap + q]) {
            const int k = B.ops[(size_t)m * B.cap + q].kf, e1 = M.kf_mp_ptr[k + 1];
            MeEdit* const out = B.edits + (size_t)m * B.edit_cap;
            int at = B.eoff[(size_t)m * (B.cap + 1) + q];               // at + the row's non-null entries <= the total <= edit_cap
            for (int e0 = M.kf_mp_ptr[k]; e0 < e1; e0 += 64) {
                const int e = e0 + lane, p = e < e1 ? M.kf_mp[e] : -1;
                const unsigned long long mask = __ballot(p != -1);
                if (p != -1) out[at + __popcll(mask & ((1ull << lane) - 1ull))] = ke_edit(p, k);
                at += __popcll(mask);
            }
        }
    }
    if (q >= M.n_kf) return;                                            // the whole wavefront
    const int j = q;
    if (lane == 0) {
        X.kf_bad[j] = V.bad[j]; X.kf_parent[j] = V.parent[j]; X.kf_to_be_erased[j] = V.tbe[j];
        int at = B.cptr[(size_t)m * ((size_t)B.kf_cap + 1) + j];        // the row ends below the need <= child_cap_out
        X.child_ptr_out[j] = at;
        for (int node = V.head[j]; node != -1; node = V.node_next[node]) X.child_out[at++] = V.node_kf[node];
    }
    if (!V.dirty[j]) return;
    const size_t r0 = (size_t)j * X.row_cap;
    const int ncw = cv_clamp(V.G.cw_n[j], X.row_cap), no = cv_clamp(V.G.ord_n[j], X.row_cap);
    for (int e = lane; e < ncw; e += 64) { X.cw_kf[r0 + e] = V.G.cw_kf[r0 + e]; X.cw_w[r0 + e] = V.G.cw_w[r0 + e]; }
    for (int e = lane; e < no; e += 64) { X.ord_kf[r0 + e] = V.G.ord_kf[r0 + e]; X.ord_w[r0 + e] = V.G.ord_w[r0 + e]; }
    if (lane == 0) { X.cw_n[j] = ncw; X.ord_n[j] = no; }
    if (X.kf_best && lane < LM_BEST) X.kf_best[(size_t)j * LM_BEST + lane] = V.G.kf_best[(size_t)j * LM_BEST + lane];
}

static hipError_t ke_launch(const KeBatch& B, size_t clear_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.flags, 0, clear_bytes, st);          // flags is the workspace's first byte
    if (e != hipSuccess) return e;
    const unsigned nm = (unsigned)B.n_maps;
    const auto blocks = [](int n, int per) { return (unsigned)std::max(1, (n + per - 1) / per); };
    hipLaunchKernelGGL(ke_init_kernel, dim3(blocks(B.kf_cap, KE_NT / 64), nm), dim3(KE_NT), 0, st, B);
    hipLaunchKernelGGL(ke_walk_kernel, dim3(nm), dim3(KE_WALK_NT), 0, st, B);
    hipLaunchKernelGGL(ke_edit_count_kernel, dim3(blocks(B.cap, 1), nm), dim3(64), 0, st, B);
    hipLaunchKernelGGL(ke_finish_kernel, dim3(nm), dim3(KE_FIN_NT), 0, st, B);
    hipLaunchKernelGGL(ke_commit_kernel, dim3(blocks(std::max(B.kf_cap, B.cap), KE_NT / 64), nm), dim3(KE_NT), 0, st, B);
    return hipGetLastError();
}

extern "C" {   // what the host forms check before anything is launched: map_check.h and their own arguments

int slamit_kf_erase_apply(int device, const slamit_map_index* map, const slamit_tree_index* X, int32_t n, const slamit_kf_op* ops, int32_t* op_status,
                          int32_t edit_cap, slamit_map_edit* edits, int32_t* n_edits_out, int32_t* n_child_out, int32_t* status) {
    const char* const where = "slamit_kf_erase_apply";
    if (n < 0 || edit_cap < 0 || !n_edits_out || !n_child_out || !status || (n && (!ops || !op_status)) || (edit_cap && !edits))
        return slamit_refuse(where, "null array or negative count");
    if (n > SLAMIT_KF_ERASE_MAX_OPS) return slamit_refuse(where, "more than SLAMIT_KF_ERASE_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
    if (!map || !X) return slamit_refuse(where, "null table");
    if (const char* bad = map_sizes_error(map)) return slamit_refuse(where, bad);
    if (X->row_cap < 1 || X->row_cap > SLAMIT_COVIS_MAX_ROW) return slamit_refuse(where, "row_cap outside [1, SLAMIT_COVIS_MAX_ROW]");
    if (X->child_cap_out < 0) return slamit_refuse(where, "negative child_cap_out");
    const int n_kf = map->n_kf, n_mp = map->n_mp, rc = X->row_cap;
    if (X->origin_kf < -1 || X->origin_kf >= n_kf) return slamit_refuse(where, "origin_kf holds a keyframe slot outside [-1, n_kf)");
    if (!map->kf_mp_ptr || !map->kf_child_ptr || !X->child_ptr_out) return slamit_refuse(where, "null table");
    if (!map_csr_ok(map->kf_mp_ptr, n_kf) || !map_csr_ok(map->kf_child_ptr, n_kf)) return slamit_refuse(where, "a CSR pointer array does not ascend from 0");
    const size_t n_kfmp = (size_t)map->kf_mp_ptr[n_kf], n_child = (size_t)map->kf_child_ptr[n_kf], cap_out = (size_t)X->child_cap_out, nk = (size_t)n_kf;
    if ((n_kfmp && !map->kf_mp) || (n_child && !map->kf_child) || (cap_out && !X->child_out) ||
        (n_kf && (!X->kf_not_erase || !X->kf_bad || !X->kf_parent || !X->kf_to_be_erased || !X->cw_kf || !X->cw_w || !X->cw_n || !X->ord_kf || !X->ord_w || !X->ord_n)))
        return slamit_refuse(where, "null table");
    if (!map_slots_ok(map->kf_mp, n_kfmp, -1, n_mp)) return slamit_refuse(where, "kf_mp holds a point slot outside [-1, n_mp)");
    if (!map_slots_ok(X->kf_parent, nk, -1, n_kf)) return slamit_refuse(where, "kf_parent holds a keyframe slot outside [-1, n_kf)");
    if (const char* bad = map_graph_rows_error(n_kf, rc, X->cw_kf, X->cw_n, X->ord_kf, X->ord_n)) return slamit_refuse(where, bad);
    if (const char* bad = map_children_error(map)) return slamit_refuse(where, bad);
    for (int i = 0; i < n; ++i) {
        const slamit_kf_op& e = ops[i];
        if (e.kind != SLAMIT_KF_ERASE_SET_PARENT && e.kind != SLAMIT_KF_ERASE_SET_BAD) return slamit_refuse(where, "an op's kind outside 1..2");
        if (e.kf < 0 || e.kf >= n_kf || (e.kind == SLAMIT_KF_ERASE_SET_PARENT && (e.parent < 0 || e.parent >= n_kf)))
            return slamit_refuse(where, "ops holds a keyframe slot outside [0, n_kf)");
    }
    SLAMIT_USE_DEVICE(device);
    KeBatch H;
    size_t clear_bytes = 0;
    const size_t ws_bytes = ke_ws_layout(1, n, n_kf, rc, (int)n_child, nullptr, nullptr, &clear_bytes);
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<KeBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, KeBatch& Q) {
            io.clear();
            Q.n_maps = 1; Q.cap = n; Q.kf_cap = n_kf; Q.row_cap = rc; Q.child_cap = (int)n_child; Q.edit_cap = edit_cap;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.kf_mp_ptr = b.in(map->kf_mp_ptr, nk + 1); M.kf_mp = b.in(map->kf_mp, n_kfmp);
            M.kf_child_ptr = b.in(map->kf_child_ptr, nk + 1); M.kf_child = b.in(map->kf_child, n_child);
            KeIndex& E = Q.X[0];
            E.row_cap = rc; E.origin_kf = X->origin_kf; E.child_cap_out = X->child_cap_out;
            E.kf_not_erase = b.in(X->kf_not_erase, nk);
            E.kf_bad = slamit_inout(b, io, X->kf_bad, nk); E.kf_parent = slamit_inout(b, io, X->kf_parent, nk);
            E.kf_to_be_erased = slamit_inout(b, io, X->kf_to_be_erased, nk);
            E.cw_kf = slamit_inout(b, io, X->cw_kf, nk * rc); E.cw_w = slamit_inout(b, io, X->cw_w, nk * rc); E.cw_n = slamit_inout(b, io, X->cw_n, nk);
            E.ord_kf = slamit_inout(b, io, X->ord_kf, nk * rc); E.ord_w = slamit_inout(b, io, X->ord_w, nk * rc); E.ord_n = slamit_inout(b, io, X->ord_n, nk);
            E.kf_best = X->kf_best ? slamit_inout(b, io, X->kf_best, nk * SLAMIT_LOCAL_MAP_BEST) : nullptr;
            E.child_ptr_out = slamit_inout(b, io, X->child_ptr_out, nk + 1); E.child_out = slamit_inout(b, io, X->child_out, cap_out);
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.ops = reinterpret_cast<const KeOp*>(b.in(ops, (size_t)n));
            Q.op_status = slamit_inout(b, io, op_status, (size_t)n);
            Q.edits = reinterpret_cast<MeEdit*>(slamit_inout(b, io, edits, (size_t)edit_cap));
            Q.n_edits_out = b.out(n_edits_out, 1); Q.n_child_out = b.out(n_child_out, 1); Q.status = b.out(status, 1);
            unsigned char* const ws = b.scratch<unsigned char>(ws_bytes);
            if (ws) ke_ws_layout(1, n, n_kf, rc, (int)n_child, ws, &Q, nullptr);
            H = Q;
        },
        [&](const KeBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : ke_launch(H, clear_bytes, S.st);
        });
}

size_t slamit_kf_erase_workspace(int n_maps, int cap, int kf_cap, int row_cap, int child_cap) {
    if (n_maps < 1 || cap < 0 || kf_cap < 0 || row_cap < 1 || child_cap < 0 || cap > SLAMIT_KF_ERASE_MAX_OPS || kf_cap > SLAMIT_LOCAL_MAP_MAX_KF || row_cap > SLAMIT_COVIS_MAX_ROW)
        return 0;
    return ke_ws_layout(n_maps, cap, kf_cap, row_cap, child_cap, nullptr, nullptr, nullptr);
}

int slamit_kf_erase_batch_dev(int device, const slamit_kf_erase_batch_rec* R, void* stream) {
    const char* const where = "slamit_kf_erase_batch_dev";
    if (!R || R->n_maps < 0 || R->cap < 0 || R->kf_cap < 0 || R->child_cap < 0 || R->edit_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->n_maps == 0) return SLAMIT_OK;
    if (R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->tree) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_KF_ERASE_MAX_OPS) return slamit_refuse(where, "cap above SLAMIT_KF_ERASE_MAX_OPS", SLAMIT_ERR_CAPACITY);
    if (R->row_cap < 1 || R->row_cap > SLAMIT_COVIS_MAX_ROW) return slamit_refuse(where, "row_cap outside [1, SLAMIT_COVIS_MAX_ROW]");
    if (R->kf_cap > SLAMIT_LOCAL_MAP_MAX_KF) return slamit_refuse(where, "kf_cap above SLAMIT_LOCAL_MAP_MAX_KF", SLAMIT_ERR_CAPACITY);
    for (int m = 0; m < R->n_maps; ++m) {
        const slamit_map_index& M = R->maps[m];
        const slamit_tree_index& X = R->tree[m];
        if (M.n_kf < 0 || M.n_mp < 0 || M.n_kf > R->kf_cap) return slamit_refuse(where, "a map with n_kf outside [0, kf_cap] or negative n_mp");
        if (X.row_cap < 1 || X.row_cap > R->row_cap) return slamit_refuse(where, "a map with row_cap outside [1, the batch's row_cap]");
        if (X.child_cap_out < 0) return slamit_refuse(where, "negative child_cap_out");
        if (!M.kf_mp_ptr || !M.kf_mp || !M.kf_child_ptr || !M.kf_child || !X.kf_not_erase || !X.kf_bad || !X.kf_parent || !X.kf_to_be_erased || !X.cw_kf || !X.cw_w ||
            !X.cw_n || !X.ord_kf || !X.ord_w || !X.ord_n || !X.child_ptr_out || !X.child_out)
            return slamit_refuse(where, "null table");
    }
    if (!R->d_n || !R->d_n_edits_out || !R->d_n_child_out || !R->d_status || (R->cap && (!R->d_ops || !R->d_op_status)) || (R->edit_cap && !R->d_edits))
        return slamit_refuse(where, "null array");
    size_t clear_bytes = 0;
    const size_t need = ke_ws_layout(R->n_maps, R->cap, R->kf_cap, R->row_cap, R->child_cap, nullptr, nullptr, &clear_bytes);
    if (!R->d_workspace || R->workspace_bytes < need || ((uintptr_t)R->d_workspace & 7)) return slamit_refuse(where, "workspace missing, misaligned or below slamit_kf_erase_workspace()");
    SLAMIT_USE_DEVICE(device);
    KeBatch B;
    memset(&B, 0, sizeof(B));
    B.n_maps = R->n_maps; B.cap = R->cap; B.kf_cap = R->kf_cap; B.row_cap = R->row_cap; B.child_cap = R->child_cap; B.edit_cap = R->edit_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.X, R->tree, sizeof(KeIndex) * (size_t)R->n_maps);
    B.ops = reinterpret_cast<const KeOp*>(R->d_ops); B.n = R->d_n;
    B.op_status = R->d_op_status; B.edits = reinterpret_cast<MeEdit*>(R->d_edits); B.n_edits_out = R->d_n_edits_out; B.n_child_out = R->d_n_child_out; B.status = R->d_status;
    ke_ws_layout(R->n_maps, R->cap, R->kf_cap, R->row_cap, R->child_cap, (unsigned char*)R->d_workspace, &B, nullptr);
    HIP_TRY_AT(where, ke_launch(B, clear_bytes, (hipStream_t)stream));
    return SLAMIT_OK;
}

}  // extern "C"
