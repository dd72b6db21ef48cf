// map_replace.hip — MapPoint::Replace and Fuse's AddObservation + AddMapPoint applied to the resident tables by one call
// (include/slamit.h, slamit_map_replace_apply / slamit_map_replace_batch_dev; the effect of an op is stated in map_replace.h, whose
// mr_walk_op the round kernel runs over working rows in the workspace), and Tracking::CheckReplacedInLastFrame, the reader of
// mp_replaced.  Nothing here is float.  No workgroup waits on another inside a kernel: the order between kernels is the stream's.
//
// mr_hist_kernel     a thread per op: is it one the walk can apply, does it act; the bucket sizes of its points, integer atomics.
// mr_scan_*          the device scan on wave_ops.h, used twice, two arrays at once: (ops per point, is the point involved) gives the
//                    buckets' first entries and the involved points' compact numbers; (new row length, received) gives the new pointer
//                    array and the places in `touched`.
// mr_scatter_kernel  a thread per op: its list index into the bucket of each of its points; a thread per point: the slot of a compact number.
// mr_prep_kernel     a wavefront per involved point: more than MR_MAX_PER_POINT ops sets the overflow word; else every op of the bucket
//                    learns its predecessor on this side (the largest list index below its own); the point's row and its five column
//                    values are copied into its working row.
// mr_round_kernel    ONE workgroup of 1024 threads per map.  Round r: a lane looks at one op; it is ready when it is not done and each
//                    predecessor finished in a round before r.  A wavefront applies the ready ops among its 64, one after the other:
//                    S's keyframes sorted in LDS by rank, membership in D's row, the moved entries placed by ballot, the kf_mp writes as
//                    atomicMax of (list index + 1) << 32 | (value + 1).  Ready ops name disjoint points, so which wavefront takes which
//                    op shows nowhere.  __syncthreads_or ends the round and says whether any op is left; the first op not done is always
//                    ready, so at most n rounds.  Data crosses rounds only inside the workgroup.  LDS: 16 x (2,048 + 1,024) = 49,152 bytes.
// mr_commit_kernel   a wavefront per involved point: the working row at its new offset, the five columns in place.
// mr_copy_kernel     the rows of the other points, 64 points to a wavefront; the new pointer array, touched, the counts and the
//                    call's status.
// mr_kfmp_kernel     the winners of the kf_mp words into kf_mp; moved / erased.
// THE GATE: every kernel that writes a caller's array first reads the two overflow words and the table's need from device memory.
// The working rows, the world over them, the scan bodies and the row copy are map_rows_dev.h's, shared with map_fuse.hip.
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
#include "map_replace.h"
#include "map_rows_dev.h"

static_assert(sizeof(MrOp) == sizeof(slamit_map_replace) && sizeof(MrOp) == 20 && offsetof(MrOp, a) == offsetof(slamit_map_replace, a) &&
                  offsetof(MrOp, idx) == offsetof(slamit_map_replace, idx) && offsetof(MrOp, octave) == offsetof(slamit_map_replace, octave) &&
                  offsetof(MrOp, weight) == offsetof(slamit_map_replace, weight),
              "slamit_map_replace is MrOp");
static_assert(sizeof(MrIndex) == sizeof(slamit_replace_index) && offsetof(MrIndex, obs_weight) == offsetof(slamit_replace_index, obs_weight) &&
                  offsetof(MrIndex, mp_bad) == offsetof(slamit_replace_index, mp_bad) && offsetof(MrIndex, mp_replaced) == offsetof(slamit_replace_index, mp_replaced) &&
                  offsetof(MrIndex, kf_mp) == offsetof(slamit_replace_index, kf_mp) && offsetof(MrIndex, obs_ptr_out) == offsetof(slamit_replace_index, obs_ptr_out) &&
                  offsetof(MrIndex, obs_weight_out) == offsetof(slamit_replace_index, obs_weight_out) && offsetof(MrIndex, obs_cap_out) == offsetof(slamit_replace_index, obs_cap_out),
              "slamit_replace_index is MrIndex");
static_assert(sizeof(LmMap) == sizeof(slamit_map_index), "slamit_map_index is LmMap");
static_assert(MR_REPLACE == SLAMIT_REPLACE_REPLACE && MR_ADD_OBS == SLAMIT_REPLACE_ADD_OBS && MR_OP_OVERFLOW == SLAMIT_REPLACE_OP_OVERFLOW &&
                  MR_OBS_OVERFLOW == SLAMIT_REPLACE_OBS_OVERFLOW && MR_TABLE_OVERFLOW == SLAMIT_REPLACE_TABLE_OVERFLOW && MR_BAD_SLOT == SLAMIT_REPLACE_BAD_SLOT &&
                  MR_MAX_OPS == SLAMIT_REPLACE_MAX_OPS && MR_MAX_PER_POINT == SLAMIT_REPLACE_MAX_PER_POINT && MR_MAX_OBS == SLAMIT_UPKEEP_MAX_OBS,
              "map_replace.h restates the C-ABI's constants");
static_assert(MR_MAX_PER_POINT == 64 && MR_SCAN_BLOCK == 256 && MR_MAX_OBS <= 65535, "a bucket is one wavefront; the scan's workgroup; a sorted position is 16 bits");

#define MR_NT 256
#define MR_ROUND_NT 1024

// The batch as the kernels' argument: W the workspace rows of map_rows_dev.h (cnt: the ops naming the point), then this module's own.
struct MrBatch {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    MrIndex X[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const MrOp* ops; const int32_t* n;
    int32_t* moved; int32_t* erased; int32_t* touched; int32_t* n_touched; int32_t* n_obs_out; int32_t* status;
    MapRows W;
    unsigned long long* kfw;   // [n_maps][kfmp_cap]      cleared
    int32_t* cursor;           // [n_maps][S]             cleared
    int32_t* bstart;           // [n_maps][S]             the buckets' first entries
    int32_t* bucket;           // [n_maps][2 cap]         list indices by point
    int32_t* pred;             // [n_maps][2][cap]        the predecessor on a's side, on b's side, -1 for none
    int32_t* done;             // [n_maps][cap]           0, or 1 + the round the op finished in
    int32_t* mv;               // [n_maps][cap]
    int32_t* er;               // [n_maps][cap]
};

static size_t mr_ws_layout(int n_maps, int cap, int mp_cap, int kfmp_cap, unsigned char* base, MrBatch* B, size_t* clear_bytes) {
    MapRowsLayout L(n_maps, cap, mp_cap, base);
    const size_t nm = L.nm, S = L.S, c = L.c;
    unsigned long long* const kfw = L.take<unsigned long long>(nm * (size_t)kfmp_cap);
    L.cleared();
    int32_t* const cursor = L.take<int32_t>(nm * S);
    if (clear_bytes) *clear_bytes = L.off;
    int32_t* const bstart = L.take<int32_t>(nm * S);
    L.scanned();
    int32_t* const bucket = L.take<int32_t>(nm * 2 * c);
    int32_t* const pred = L.take<int32_t>(nm * 2 * c);
    int32_t* const done = L.take<int32_t>(nm * c);
    int32_t* const mv = L.take<int32_t>(nm * c);
    int32_t* const er = L.take<int32_t>(nm * c);
    L.columns();
    L.rows();
    if (B) { B->W = L.W; B->kfw = kfw; B->cursor = cursor; B->bstart = bstart; B->bucket = bucket; B->pred = pred; B->done = done; B->mv = mv; B->er = er; }
    return L.off;
}

__device__ __forceinline__ bool mr_gate(const MrBatch& B, int m) {
    const int32_t* const f = B.W.flags + MR_NFLAGS * m;
    return f[MR_F_OP_OVER] != 0 || f[MR_F_OBS_OVER] != 0 || B.W.newptr[(size_t)m * (B.mp_cap + 1) + B.maps[m].n_mp] > B.X[m].obs_cap_out;
}

// ---- grid (ceil(cap / 256), maps) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_hist_kernel(MrBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * MR_NT + (int)threadIdx.x;
    if (i >= lm_list_n(B.n[m], B.cap)) return;
    const LmMap& M = B.maps[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    const MrOp e = B.ops[m * c + i];
    int d = 1;                                                          // an op that does nothing is done
    if (!mr_op_ok(M, e)) atomicOr(&B.W.flags[MR_NFLAGS * m + MR_F_OP_BAD], 1);
    else if (mr_op_acts(e)) {
        d = 0;
        atomicAdd(&B.W.cnt[m * S + e.a], 1);
        if (e.kind == MR_REPLACE) atomicAdd(&B.W.cnt[m * S + e.b], 1);
    }
    B.done[m * c + i] = d; B.mv[m * c + i] = 0; B.er[m * c + i] = 0;
    B.pred[(m * 2 + 0) * c + i] = -1; B.pred[(m * 2 + 1) * c + i] = -1;
}

// ---- the device scan ------------------------------------------------------------------------------------------------------------
// what is scanned.  mode 0: array 0 the ops naming point p, array 1 whether any does.  mode 1: array 0 the new length of p's row,
// array 1 whether p received an observation.
__device__ __forceinline__ int mr_scan_src(const MrBatch& B, int m, int mode, int z, int p) {
    const size_t S = (size_t)B.mp_cap + 1;
    const int c = B.W.cnt[m * S + p];
    if (mode == 0) return z ? (c > 0) : c;
    if (c == 0) return z ? 0 : B.maps[m].obs_ptr[p + 1] - B.maps[m].obs_ptr[p];
    const int ci = B.W.cidx[m * S + p];                                // < ninv: the involved points are counted there
    return map_rows_col(B.W, m, z ? MR_C_RECEIVED : MR_C_LEN)[ci];
}
// the three kernels over map_rows_dev.h's bodies.  grid (nparts, maps, 2), (maps, 2), (nparts, maps, 2)
__global__ __launch_bounds__(MR_NT) void mr_scan_sum_kernel(MrBatch B, int mode) {
    const int m = blockIdx.y;
    map_scan_sum<MR_NT>(B.W.parts, B.W.nparts, B.maps[m].n_mp, [&](int z, int p) { return mr_scan_src(B, m, mode, z, p); });
}
__global__ __launch_bounds__(MR_NT) void mr_scan_parts_kernel(MrBatch B) { map_scan_parts<MR_NT>(B.W.parts, B.W.nparts); }
__global__ __launch_bounds__(MR_NT) void mr_scan_add_kernel(MrBatch B, int mode) {
    const int m = blockIdx.y;
    int32_t* const out = (mode == 0 ? (blockIdx.z ? B.W.cidx : B.bstart) : (blockIdx.z ? B.W.tpos : B.W.newptr)) + m * ((size_t)B.mp_cap + 1);
    map_scan_add<MR_NT>(B.W.parts, B.W.nparts, B.maps[m].n_mp, [&](int z, int p) { return mr_scan_src(B, m, mode, z, p); }, out);   // n_mp <= mp_cap: inside the row
}

// ---- grid (ceil(max(cap, mp_cap) / 256), maps) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_scatter_kernel(MrBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * MR_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    if (i < lm_list_n(B.n[m], B.cap) && B.done[m * c + i] == 0) {                // an op the histogram counted
        const MrOp e = B.ops[m * c + i];
        int at = B.bstart[m * S + e.a] + atomicAdd(&B.cursor[m * S + e.a], 1);   // < the number bucketed <= 2 cap
        B.bucket[m * 2 * c + at] = i;
        if (e.kind == MR_REPLACE) {
            at = B.bstart[m * S + e.b] + atomicAdd(&B.cursor[m * S + e.b], 1);
            B.bucket[m * 2 * c + at] = i;
        }
    }
    if (i < M.n_mp && B.W.cnt[m * S + i] > 0) B.W.inv[(size_t)m * B.W.ninv + B.W.cidx[m * S + i]] = i;   // cidx < the involved points <= ninv
}

// ---- grid (ceil(ninv / 4), maps), 256 threads: a wavefront per involved point --------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_prep_kernel(MrBatch B) {
    __shared__ int32_t raw[MR_NT / 64][64];
    const int m = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, ci = blockIdx.x * (MR_NT / 64) + w;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    if (ci >= B.W.cidx[m * S + M.n_mp]) return;                         // the whole wavefront, here and below
    const int p = __builtin_amdgcn_readfirstlane(B.W.inv[(size_t)m * B.W.ninv + ci]);
    const int ne = __builtin_amdgcn_readfirstlane(B.W.cnt[m * S + p]);
    if (ne > MR_MAX_PER_POINT) {
        if (lane == 0) atomicOr(&B.W.flags[MR_NFLAGS * m + MR_F_OP_OVER], 1);
        return;
    }
    const int b0 = B.bstart[m * S + p];
    const int li = lane < ne ? B.bucket[m * 2 * c + b0 + lane] : 0x7fffffff;
    raw[w][lane] = li;
    wave_mem_sync();
    if (lane < ne) {
        int prev = -1;                                                  // list indices are distinct: the largest below mine
        for (int t = 0; t < ne; ++t) { const int o = raw[w][t]; if (o < li && o > prev) prev = o; }
        const MrOp e = B.ops[m * c + li];
        const int side = e.kind == MR_REPLACE && e.b == p;              // a != b in a bucketed REPLACE
        B.pred[(m * 2 + side) * c + li] = prev;
    }
    map_row_load(B.W, m, M, X, ci, p, lane);
}

// ---- the kf_mp writes of the world (MapWorldDev of map_rows_dev.h): ops of one round run at once, so the largest list index wins -
struct MrEmitDev {
    const LmMap* M; unsigned long long* kfw; int32_t* flags;
    int kfmp_cap, lane;
    __device__ __forceinline__ void mine(int k, int i, int value, int li) {   // this lane's write
        const long long at = mr_kfmp_at(*M, k, i);
        if (at < 0 || at >= kfmp_cap) { atomicOr(&flags[MR_F_OBS_BAD], 1); return; }
        atomicMax(&kfw[at], ((unsigned long long)(unsigned)(li + 1) << 32) | (unsigned)(value + 1));
    }
    __device__ __forceinline__ void one(int k, int i, int value, int li) {    // the wavefront's write
        if (lane == 0) mine(k, i, value, li);
    }
};

// ---- grid (maps), 1024 threads --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_ROUND_NT) void mr_round_kernel(MrBatch B) {
    __shared__ int32_t skf[MR_ROUND_NT / 64][MR_MAX_OBS];
    __shared__ uint16_t sord[MR_ROUND_NT / 64][MR_MAX_OBS];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const LmMap& M = B.maps[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    int32_t* const flags = B.W.flags + MR_NFLAGS * m;
    if (flags[MR_F_OP_OVER]) return;                                    // a bucket above a wavefront: no predecessors were made
    const int n = lm_list_n(B.n[m], B.cap);
    const MrOp* const ops = B.ops + m * c;
    int32_t* const done = B.done + m * c;
    const int32_t* const pred_a = B.pred + (m * 2 + 0) * c;
    const int32_t* const pred_b = B.pred + (m * 2 + 1) * c;
    MapWorldDev world;
    world.bind(B.W, m, S, skf[w], sord[w], lane);
    MrEmitDev emit = {&M, B.kfw + (size_t)m * B.kfmp_cap, flags, B.kfmp_cap, lane};
    for (int round = 0; round < n; ++round) {                           // the first op not done is ready: at most n rounds
        int pending = 0;
        for (int base = 0; base < n; base += MR_ROUND_NT) {
            const int i = base + tid;
            bool ready = false;
            if (i < n && __hip_atomic_load(&done[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) {
                const int pa = pred_a[i], pb = pred_b[i];               // < i: inside the list
                const int da = pa < 0 ? 1 : __hip_atomic_load(&done[pa], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int db = pb < 0 ? 1 : __hip_atomic_load(&done[pb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // finished in a round before this one (a predecessor never is a skipped op, so its stamp is its round's)
                ready = (pa < 0 || (da > 0 && da <= round)) && (pb < 0 || (db > 0 && db <= round));
                if (!ready) pending = 1;
            }
            unsigned long long mask = __ballot(ready);
            while (mask) {                                              // wave-uniform
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int j = base + w * 64 + l;
                const MrOp e = ops[j];
                int moved, erased;
                mr_walk_op(world, e, j, emit, moved, erased);
                if (lane == 0) {
                    B.mv[m * c + j] = moved; B.er[m * c + j] = erased;
                    __hip_atomic_store(&done[j], round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (!__syncthreads_or(pending)) break;                          // ends the round: what it wrote is the next round's to read
    }
}

// ---- grid (ceil(ninv / 4), maps), 256 threads: a wavefront per involved point --------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_commit_kernel(MrBatch B) {
    const int m = blockIdx.y, lane = threadIdx.x & 63, ci = blockIdx.x * (MR_NT / 64) + (threadIdx.x >> 6);
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    if (mr_gate(B, m)) return;
    if (ci >= B.W.cidx[m * S + M.n_mp]) return;
    map_row_commit(B.W, m, S, X, ci, lane);
}

// ---- grid (ceil((mp_cap + 1) / 256), maps) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_copy_kernel(MrBatch B) {
    const int m = blockIdx.y, p = blockIdx.x * MR_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    const int32_t* const newptr = B.W.newptr + m * S;
    const int32_t* const flags = B.W.flags + MR_NFLAGS * m;
    const int n_mp = M.n_mp, need = newptr[n_mp];
    const bool op_over = flags[MR_F_OP_OVER] != 0, obs_over = flags[MR_F_OBS_OVER] != 0, table_over = !op_over && !obs_over && need > X.obs_cap_out;
    bool committed;
    const int status = mr_call_status(op_over, obs_over, table_over, flags[MR_F_OP_BAD] != 0, flags[MR_F_OBS_BAD] != 0, committed);
    if (p == n_mp) {
        B.status[m] = status;
        if (table_over || committed) B.n_obs_out[m] = need;
    }
    if (!committed) return;
    if (p <= n_mp) X.obs_ptr_out[p] = newptr[p];
    if (p == n_mp) B.n_touched[m] = B.W.tpos[m * S + n_mp];
    bool sk = true;
    if (p < n_mp) {
        sk = B.W.cnt[m * S + p] > 0;                                    // mr_commit_kernel writes that row
        if (sk && mr_scan_src(B, m, 1, 1, p)) B.touched[(size_t)m * B.mp_cap + B.W.tpos[m * S + p]] = p;   // tpos < the receivers before p <= p
    }
    map_copy_unnamed_rows<MR_NT>(p & ~63, sk, M.obs_ptr, newptr, n_mp, M.obs_kf, X.obs_idx, X.obs_octave, X.obs_weight, X.obs_kf_out, X.obs_idx_out,
                                 X.obs_octave_out, X.obs_weight_out);
}

// ---- grid (ceil(max(kfmp_cap, cap) / 256), maps) --------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_NT) void mr_kfmp_kernel(MrBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * MR_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t c = (size_t)B.cap;
    if (mr_gate(B, m)) return;
    if (i < lm_list_n(B.n[m], B.cap)) { B.moved[m * c + i] = B.mv[m * c + i]; B.erased[m * c + i] = B.er[m * c + i]; }
    if (i >= min(M.kf_mp_ptr[M.n_kf], B.kfmp_cap)) return;
    const unsigned long long v = B.kfw[(size_t)m * B.kfmp_cap + i];
    if (v) X.kf_mp[i] = (int)(unsigned)v - 1;
}

static hipError_t mr_launch(const MrBatch& B, size_t clear_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.kfw, 0, clear_bytes, st);            // kfw is the workspace's first byte
    if (e != hipSuccess) return e;
    const unsigned nm = (unsigned)B.n_maps, nparts = (unsigned)B.W.nparts;
    const auto blocks = [](int n, int per) { return (unsigned)std::max(1, (n + per - 1) / per); };
    hipLaunchKernelGGL(mr_hist_kernel, dim3(blocks(B.cap, MR_NT), nm), dim3(MR_NT), 0, st, B);
    hipLaunchKernelGGL(mr_scan_sum_kernel, dim3(nparts, nm, 2), dim3(MR_NT), 0, st, B, 0);
    hipLaunchKernelGGL(mr_scan_parts_kernel, dim3(nm, 2), dim3(MR_NT), 0, st, B);
    hipLaunchKernelGGL(mr_scan_add_kernel, dim3(nparts, nm, 2), dim3(MR_NT), 0, st, B, 0);
    hipLaunchKernelGGL(mr_scatter_kernel, dim3(blocks(std::max(B.cap, B.mp_cap), MR_NT), nm), dim3(MR_NT), 0, st, B);
    if (B.W.ninv > 0) hipLaunchKernelGGL(mr_prep_kernel, dim3(blocks(B.W.ninv, MR_NT / 64), nm), dim3(MR_NT), 0, st, B);
    if (B.cap > 0) hipLaunchKernelGGL(mr_round_kernel, dim3(nm), dim3(MR_ROUND_NT), 0, st, B);
    hipLaunchKernelGGL(mr_scan_sum_kernel, dim3(nparts, nm, 2), dim3(MR_NT), 0, st, B, 1);
    hipLaunchKernelGGL(mr_scan_parts_kernel, dim3(nm, 2), dim3(MR_NT), 0, st, B);
    hipLaunchKernelGGL(mr_scan_add_kernel, dim3(nparts, nm, 2), dim3(MR_NT), 0, st, B, 1);
    if (B.W.ninv > 0) hipLaunchKernelGGL(mr_commit_kernel, dim3(blocks(B.W.ninv, MR_NT / 64), nm), dim3(MR_NT), 0, st, B);
    hipLaunchKernelGGL(mr_copy_kernel, dim3(nparts, nm), dim3(MR_NT), 0, st, B);
    if (std::max(B.kfmp_cap, B.cap) > 0) hipLaunchKernelGGL(mr_kfmp_kernel, dim3(blocks(std::max(B.kfmp_cap, B.cap), MR_NT), nm), dim3(MR_NT), 0, st, B);
    return hipGetLastError();
}

// ---- Tracking::CheckReplacedInLastFrame: grid (frames), 256 threads, a lane per entry ------------------------------------------
struct MrCheck {
    int32_t nframes, n_maps, cap, reserved;
    int32_t n_mp[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* replaced[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* frame_map; const int32_t* n; int32_t* frame_mp; int32_t* status;
};
__global__ __launch_bounds__(MR_NT) void mr_check_replaced_kernel(MrCheck Q) {
    const int f = blockIdx.x, fm = Q.frame_map ? Q.frame_map[f] : 0;
    const bool map_ok = (unsigned)fm < (unsigned)Q.n_maps;
    int bad = map_ok ? 0 : 1;
    if (map_ok) {
        const int n = min(max(Q.n[f], 0), Q.cap), n_mp = Q.n_mp[fm];
        const int32_t* const rep = Q.replaced[fm];
        int32_t* const list = Q.frame_mp + (size_t)f * Q.cap;
        for (int i = threadIdx.x; i < n; i += MR_NT) bad |= mr_check_replaced_entry(n_mp, rep, &list[i]);
    }
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) Q.status[f] = any ? MR_BAD_SLOT : 0;
}

extern "C" {   // what the host forms check before anything is launched: map_check.h and their own arguments

int slamit_map_replace_apply(int device, const slamit_map_index* map, const slamit_replace_index* X, int32_t n, const slamit_map_replace* ops, int32_t* moved,
                             int32_t* erased, int32_t* touched, int32_t* n_touched, int32_t* n_obs_out, int32_t* status) {
    const char* const where = "slamit_map_replace_apply";
    if (n < 0 || !n_touched || !n_obs_out || !status || (n && (!ops || !moved || !erased))) return slamit_refuse(where, "null array or negative n");
    if (n > SLAMIT_REPLACE_MAX_OPS) return slamit_refuse(where, "more than SLAMIT_REPLACE_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
    if (const char* bad = map_replace_tables_error(map, X, touched)) return slamit_refuse(where, bad);
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf];
    for (int i = 0; i < n; ++i) {
        const slamit_map_replace& e = ops[i];
        if (e.kind != SLAMIT_REPLACE_REPLACE && e.kind != SLAMIT_REPLACE_ADD_OBS) return slamit_refuse(where, "an op's kind outside 1..2");
        if (e.a < 0 || e.a >= n_mp) return slamit_refuse(where, "ops holds a point slot outside [0, n_mp)");
        if (e.kind == SLAMIT_REPLACE_REPLACE) {
            if (e.b < 0 || e.b >= n_mp) return slamit_refuse(where, "ops holds a point slot outside [0, n_mp)");
            continue;
        }
        if (e.b < 0 || e.b >= n_kf) return slamit_refuse(where, "ops holds a keyframe slot outside [0, n_kf)");
        if (e.idx < 0 || e.idx >= map->kf_mp_ptr[e.b + 1] - map->kf_mp_ptr[e.b]) return slamit_refuse(where, "ops holds a keypoint index outside its keyframe's row");
        if (e.weight != 1 && e.weight != 2) return slamit_refuse(where, "an op's weight other than 1 or 2");
    }
    if (n_obs + (size_t)n > (size_t)0x7fffffff) return slamit_refuse(where, "the new table may need more than 2^31 - 1 entries", SLAMIT_ERR_CAPACITY);
    SLAMIT_USE_DEVICE(device);
    MrBatch H;
    size_t clear_bytes = 0;
    const size_t ws_bytes = mr_ws_layout(1, n, n_mp, (int)n_kfmp, nullptr, nullptr, &clear_bytes);
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<MrBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, MrBatch& Q) {
            io.clear();
            Q.n_maps = 1; Q.cap = n; Q.mp_cap = n_mp; Q.kfmp_cap = (int)n_kfmp;
            map_stage_tables(b, io, map, X, Q.maps[0], Q.X[0]);
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.ops = reinterpret_cast<const MrOp*>(b.in(ops, (size_t)n));
            Q.moved = slamit_inout(b, io, moved, (size_t)n); Q.erased = slamit_inout(b, io, erased, (size_t)n);
            Q.touched = slamit_inout(b, io, touched, (size_t)n_mp);
            Q.n_touched = slamit_inout(b, io, n_touched, 1); Q.n_obs_out = slamit_inout(b, io, n_obs_out, 1);
            Q.status = b.out(status, 1);
            unsigned char* const ws = b.scratch<unsigned char>(ws_bytes);
            if (ws) mr_ws_layout(1, n, n_mp, (int)n_kfmp, ws, &Q, nullptr);
            H = Q;
        },
        [&](const MrBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : mr_launch(H, clear_bytes, S.st);
        });
}

size_t slamit_map_replace_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap) {
    if (n_maps < 1 || cap < 0 || mp_cap < 0 || kfmp_cap < 0 || cap > SLAMIT_REPLACE_MAX_OPS) return 0;
    return mr_ws_layout(n_maps, cap, mp_cap, kfmp_cap, nullptr, nullptr, nullptr);
}

int slamit_map_replace_batch_dev(int device, const slamit_map_replace_batch_rec* R, void* stream) {
    const char* const where = "slamit_map_replace_batch_dev";
    if (!R || R->n_maps < 0 || R->cap < 0 || R->mp_cap < 0 || R->kfmp_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->n_maps == 0) return SLAMIT_OK;
    if (R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->index) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_REPLACE_MAX_OPS) return slamit_refuse(where, "cap above SLAMIT_REPLACE_MAX_OPS", SLAMIT_ERR_CAPACITY);
    if (R->mp_cap == 0x7fffffff) return slamit_refuse(where, "mp_cap above 2^31 - 2", SLAMIT_ERR_CAPACITY);
    if (const char* bad = map_replace_batch_error(R->n_maps, R->mp_cap, R->maps, R->index)) return slamit_refuse(where, bad);
    if (!R->d_n || !R->d_n_touched || !R->d_n_obs_out || !R->d_status || (R->cap && (!R->d_ops || !R->d_moved || !R->d_erased)) || (R->mp_cap && !R->d_touched))
        return slamit_refuse(where, "null array");
    size_t clear_bytes = 0;
    const size_t need = mr_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, nullptr, nullptr, &clear_bytes);
    if (!R->d_workspace || R->workspace_bytes < need || ((uintptr_t)R->d_workspace & 7)) return slamit_refuse(where, "workspace missing, misaligned or below slamit_map_replace_workspace()");
    SLAMIT_USE_DEVICE(device);
    MrBatch B;
    memset(&B, 0, sizeof(B));
    B.n_maps = R->n_maps; B.cap = R->cap; B.mp_cap = R->mp_cap; B.kfmp_cap = R->kfmp_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.X, R->index, sizeof(MrIndex) * (size_t)R->n_maps);
    B.ops = reinterpret_cast<const MrOp*>(R->d_ops); B.n = R->d_n;
    B.moved = R->d_moved; B.erased = R->d_erased; B.touched = R->d_touched; B.n_touched = R->d_n_touched; B.n_obs_out = R->d_n_obs_out; B.status = R->d_status;
    mr_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, (unsigned char*)R->d_workspace, &B, nullptr);
    HIP_TRY_AT(where, mr_launch(B, clear_bytes, (hipStream_t)stream));
    return SLAMIT_OK;
}

int slamit_check_replaced(int device, int32_t n_mp, const int32_t* mp_replaced, int32_t n, int32_t* frame_mp, int32_t* status) {
    const char* const where = "slamit_check_replaced";
    if (n < 0 || n_mp < 0 || !status || (n && !frame_mp) || (n_mp && !mp_replaced)) return slamit_refuse(where, "null array or negative count");
    if (n > SLAMIT_CHECK_REPLACED_MAX_N) return slamit_refuse(where, "more than SLAMIT_CHECK_REPLACED_MAX_N entries", SLAMIT_ERR_CAPACITY);
    if (!map_slots_ok(frame_mp, (size_t)n, -1, n_mp)) return slamit_refuse(where, "frame_mp holds a point slot outside [-1, n_mp)");
    SLAMIT_USE_DEVICE(device);
    MrCheck H;
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<MrCheck>(
        where, S, device, 1,
        [&](StageBinder& b, int, MrCheck& Q) {
            io.clear();
            Q.nframes = 1; Q.n_maps = 1; Q.cap = n; Q.n_mp[0] = n_mp;
            Q.replaced[0] = b.in(mp_replaced, (size_t)n_mp);
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.frame_map = nullptr;
            Q.frame_mp = slamit_inout(b, io, frame_mp, (size_t)n);
            Q.status = b.out(status, 1);
            H = Q;
        },
        [&](const MrCheck*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(mr_check_replaced_kernel, dim3(1), dim3(MR_NT), 0, S.st, H);
            return hipGetLastError();
        });
}

int slamit_check_replaced_batch_dev(int device, const slamit_check_replaced_batch_rec* R, void* stream) {
    const char* const where = "slamit_check_replaced_batch_dev";
    if (!R || R->nframes < 0 || R->n_maps < 0 || R->cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nframes == 0) return SLAMIT_OK;
    if (R->n_maps < 1 || R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->n_mp || !R->d_mp_replaced) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_CHECK_REPLACED_MAX_N) return slamit_refuse(where, "cap above SLAMIT_CHECK_REPLACED_MAX_N", SLAMIT_ERR_CAPACITY);
    MrCheck Q;
    memset(&Q, 0, sizeof(Q));
    for (int m = 0; m < R->n_maps; ++m) {
        if (R->n_mp[m] < 0 || (R->n_mp[m] && !R->d_mp_replaced[m])) return slamit_refuse(where, "a map with negative n_mp or no mp_replaced");
        Q.n_mp[m] = R->n_mp[m]; Q.replaced[m] = R->d_mp_replaced[m];
    }
    if (!R->d_frame_map || !R->d_n || !R->d_status || (R->cap && !R->d_frame_mp)) return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    Q.nframes = R->nframes; Q.n_maps = R->n_maps; Q.cap = R->cap;
    Q.frame_map = R->d_frame_map; Q.n = R->d_n; Q.frame_mp = R->d_frame_mp; Q.status = R->d_status;
    hipLaunchKernelGGL(mr_check_replaced_kernel, dim3((unsigned)R->nframes), dim3(MR_NT), 0, (hipStream_t)stream, Q);
    HIP_TRY_AT(where, hipGetLastError());
    return SLAMIT_OK;
}

}  // extern "C"
