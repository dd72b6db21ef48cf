// map_fuse.hip — the tail of ORBmatcher::Fuse applied to the resident tables by one call (include/slamit.h, slamit_map_fuse_apply /
// slamit_map_fuse_batch_dev; the effect of an op is stated in map_fuse.h, whose mf_walk_op the walk kernel runs over working rows and a
// working image of kf_mp in the workspace), and the builder of FUSE lists from what the guided search left (slamit_fuse_list_batch_dev).
// Nothing here is float but the builder's one comparison.  No workgroup waits on another inside a kernel: the order between kernels is
// the stream's.
//
// mf_mark_kernel     a thread per op: is it one the walk can apply, does it act; its points -- P, the INITIAL kf_mp[k][idx], S and D of
//                    a plain op -- are marked involved (plain stores of 1).  A thread per entry of kf_mp: the working image.
// mf_scan_*          the device scan on wave_ops.h, used twice: (is the point involved) gives the compact numbers and their slots;
//                    (new row length, received) gives the new pointer array and the places in `touched`.
// mf_prep_kernel     a wavefront per involved point: its row and its five column values into its working row.
// mf_walk_kernel     ONE wavefront per map walks the list in order (which ops touch which points is only known while it
//                    runs, so there is no DAG to schedule).  A lane loads one op of the next 64; the wavefront takes the acting ones one
//                    after the other through mf_walk_op: membership by ballot, the moved entries placed by popcount, mp_nobs by the wave
//                    scan, kf_mp read and written in the working image.  LDS: 2,048 + 1,024 bytes.
// mf_commit_kernel   a wavefront per involved point: the working row at its new offset, the five columns in place.
// mf_copy_kernel     the rows of the other points, 64 points to a wavefront; the new pointer array, touched, the counts, the status.
// mf_finish_kernel   the working image into kf_mp; outcome / moved / erased.
// THE GATE: every kernel that writes a caller's array first reads the overflow word and the table's need from device memory.
// A row that holds one (keyframe, index) pair twice (no std::map does) has its two kf_mp writes in one store instruction.
// The working rows, the world over them (holds / push / fuse / retire), the scan bodies and the row copy are map_rows_dev.h's, the one
// text map_replace.hip runs too; MfWorldDev below adds what mf_walk_op asks for beyond mr_walk_op.
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
#include "map_fuse.h"
#include "map_rows_dev.h"

static_assert(sizeof(MrOp) == sizeof(slamit_map_replace) && sizeof(MrOp) == 20 && sizeof(MrIndex) == sizeof(slamit_replace_index) && sizeof(LmMap) == sizeof(slamit_map_index),
              "the records of map_replace.h are the C-ABI's");
static_assert(MF_FUSE == SLAMIT_FUSE_FUSE && MF_MAX_OPS == SLAMIT_FUSE_MAX_OPS && MF_OBS_OVERFLOW == SLAMIT_FUSE_OBS_OVERFLOW && MF_TABLE_OVERFLOW == SLAMIT_FUSE_TABLE_OVERFLOW &&
                  MF_BAD_SLOT == SLAMIT_FUSE_BAD_SLOT && MF_OBS_OVERFLOW == MR_OBS_OVERFLOW && MF_TABLE_OVERFLOW == MR_TABLE_OVERFLOW && MF_BAD_SLOT == MR_BAD_SLOT &&
                  MF_OUT_PLAIN == SLAMIT_FUSE_OUT_PLAIN && MF_OUT_NOMATCH == SLAMIT_FUSE_OUT_NOMATCH && MF_OUT_SKIP_BAD == SLAMIT_FUSE_OUT_SKIP_BAD &&
                  MF_OUT_SKIP_IN_KF == SLAMIT_FUSE_OUT_SKIP_IN_KF && MF_OUT_ADDED == SLAMIT_FUSE_OUT_ADDED && MF_OUT_OCCUPANT_BAD == SLAMIT_FUSE_OUT_OCCUPANT_BAD &&
                  MF_OUT_P_REPLACED == SLAMIT_FUSE_OUT_P_REPLACED && MF_OUT_Q_REPLACED == SLAMIT_FUSE_OUT_Q_REPLACED,
              "map_fuse.h restates the C-ABI's constants, and its status bits are map_replace.h's");

#define MF_NT 256
#define MF_TO_WALK (-1)   // an op's outcome word until the walk has taken it

// The batch as the kernels' argument: W the workspace rows of map_rows_dev.h (cnt: 1 for an involved point), then this module's own.
struct MfBatch {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    MrIndex X[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const MrOp* ops; const int32_t* n;
    int32_t* outcome; int32_t* moved; int32_t* erased; int32_t* touched; int32_t* n_touched; int32_t* n_fused; int32_t* n_obs_out; int32_t* status;
    MapRows W;
    int32_t* oc;               // [n_maps][cap]           MF_TO_WALK, then the outcome
    int32_t* mv;               // [n_maps][cap]
    int32_t* er;               // [n_maps][cap]
    int32_t* fused;            // [n_maps]
    int32_t* image;            // [n_maps][kfmp_cap]      kf_mp as the walk has it
};

static size_t mf_ws_layout(int n_maps, int cap, int mp_cap, int kfmp_cap, unsigned char* base, MfBatch* B, size_t* clear_bytes) {
    MapRowsLayout L(n_maps, cap, mp_cap, base);
    const size_t nm = L.nm, c = L.c;
    L.cleared();
    if (clear_bytes) *clear_bytes = L.off;
    L.scanned();
    int32_t* const oc = L.take<int32_t>(nm * c);
    int32_t* const mv = L.take<int32_t>(nm * c);
    int32_t* const er = L.take<int32_t>(nm * c);
    int32_t* const fused = L.take<int32_t>(nm);
    L.columns();
    int32_t* const image = L.take<int32_t>(nm * (size_t)kfmp_cap);
    L.rows();
    if (B) { B->W = L.W; B->oc = oc; B->mv = mv; B->er = er; B->fused = fused; B->image = image; }
    return L.off;
}

__device__ __forceinline__ bool mf_gate(const MfBatch& B, int m) {
    return B.W.flags[MR_NFLAGS * m + MR_F_OBS_OVER] != 0 || B.W.newptr[(size_t)m * (B.mp_cap + 1) + B.maps[m].n_mp] > B.X[m].obs_cap_out;
}

// ---- grid (ceil(max(cap, kfmp_cap) / 256), maps) --------------------------------------------------------------------------------
__global__ __launch_bounds__(MF_NT) void mf_mark_kernel(MfBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * MF_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    if (i < lm_list_n(B.n[m], B.cap)) {
        const MrOp e = B.ops[m * c + i];
        int out = MF_OUT_PLAIN;                                          // an op that is skipped or does nothing
        bool ok = mf_op_ok(M, e);
        long long at = -1;
        if (ok && e.kind == MF_FUSE && e.idx >= 0) {
            at = mr_kfmp_at(M, e.b, e.idx);
            ok = at < B.kfmp_cap;                                        // the occupant is read there
        }
        if (!ok) atomicOr(&B.W.flags[MR_NFLAGS * m + MR_F_OP_BAD], 1);
        else if (!mf_op_acts(e)) out = e.kind == MF_FUSE ? MF_OUT_NOMATCH : MF_OUT_PLAIN;
        else {
            out = MF_TO_WALK;
            B.W.cnt[m * S + e.a] = 1;
            if (e.kind == MR_REPLACE) B.W.cnt[m * S + e.b] = 1;
            if (e.kind == MF_FUSE) {
                const int q = X.kf_mp[at];                               // the INITIAL occupant
                if (lm_mp_ok(M, q)) B.W.cnt[m * S + q] = 1;
            }
        }
        B.oc[m * c + i] = out; B.mv[m * c + i] = 0; B.er[m * c + i] = 0;
    }
    if (i < min(M.kf_mp_ptr[M.n_kf], B.kfmp_cap)) B.image[(size_t)m * B.kfmp_cap + i] = X.kf_mp[i];
}

// ---- the device scan ------------------------------------------------------------------------------------------------------------
// what is scanned.  mode 0: whether point p is involved (one array).  mode 1: array 0 the new length of p's row, array 1 whether p
// received an observation.
__device__ __forceinline__ int mf_scan_src(const MfBatch& B, int m, int mode, int z, int p) {
    const size_t S = (size_t)B.mp_cap + 1;
    const int c = B.W.cnt[m * S + p];
    if (mode == 0) return c;
    if (c == 0) return z ? 0 : B.maps[m].obs_ptr[p + 1] - B.maps[m].obs_ptr[p];
    const int ci = B.W.cidx[m * S + p];                                // < ninv: the involved points are counted there
    return map_rows_col(B.W, m, z ? MR_C_RECEIVED : MR_C_LEN)[ci];
}
// the three kernels over map_rows_dev.h's bodies.  grid (nparts, maps, arrays), (maps, arrays), (nparts, maps, arrays); mode 0: one
// array, mode 1: two.  Mode 0 of the add pass also writes the slot of each compact number.
__global__ __launch_bounds__(MF_NT) void mf_scan_sum_kernel(MfBatch B, int mode) {
    const int m = blockIdx.y;
    map_scan_sum<MF_NT>(B.W.parts, B.W.nparts, B.maps[m].n_mp, [&](int z, int p) { return mf_scan_src(B, m, mode, z, p); });
}
__global__ __launch_bounds__(MF_NT) void mf_scan_parts_kernel(MfBatch B) { map_scan_parts<MF_NT>(B.W.parts, B.W.nparts); }
__global__ __launch_bounds__(MF_NT) void mf_scan_add_kernel(MfBatch B, int mode) {
    const int m = blockIdx.y, i = blockIdx.x * MF_NT + (int)threadIdx.x, n = B.maps[m].n_mp;
    int32_t* const out = (mode == 0 ? B.W.cidx : (blockIdx.z ? B.W.tpos : B.W.newptr)) + m * ((size_t)B.mp_cap + 1);
    const MapScanAt at = map_scan_add<MF_NT>(B.W.parts, B.W.nparts, n, [&](int z, int p) { return mf_scan_src(B, m, mode, z, p); }, out);   // n <= mp_cap: inside the row
    if (mode == 0 && at.v && at.before < B.W.ninv) B.W.inv[(size_t)m * B.W.ninv + at.before] = i;   // v != 0: i < n; at most 2 per op and n_mp are involved: always inside
}

// ---- grid (ceil(ninv / 4), maps), 256 threads: a wavefront per involved point --------------------------------------------------
__global__ __launch_bounds__(MF_NT) void mf_prep_kernel(MfBatch B) {
    const int m = blockIdx.y, lane = threadIdx.x & 63, ci = blockIdx.x * (MF_NT / 64) + (threadIdx.x >> 6);
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    if (ci >= min(B.W.cidx[m * S + M.n_mp], B.W.ninv)) return;          // the whole wavefront
    const int p = __builtin_amdgcn_readfirstlane(B.W.inv[(size_t)m * B.W.ninv + ci]);
    map_row_load(B.W, m, M, X, ci, p, lane);
}

// ---- the world of mf_walk_op on the device: MapWorldDev of map_rows_dev.h over the rows, and the working image of kf_mp ---------
struct MfEmitDev {   // one wavefront walks the list, so a later write simply comes later
    const LmMap* M; int32_t* image; int32_t* flags;
    int kfmp_cap, lane;
    __device__ __forceinline__ void mine(int k, int i, int value, int) {
        const long long at = mr_kfmp_at(*M, k, i);
        if (at < 0 || at >= kfmp_cap) { atomicOr(&flags[MR_F_OBS_BAD], 1); return; }
        image[at] = value;
    }
    __device__ __forceinline__ void one(int k, int i, int value, int li) {
        if (lane == 0) mine(k, i, value, li);
    }
};
struct MfWorldDev : MapWorldDev {   // what mf_walk_op asks for beyond mr_walk_op
    const LmMap* M; const int32_t* image;
    __device__ __forceinline__ bool bad(int p) const { return __builtin_amdgcn_readfirstlane(col[MR_C_BAD][cidx[p]]) != 0; }
    __device__ __forceinline__ int nobs(int p) const { return __builtin_amdgcn_readfirstlane(col[MR_C_NOBS][cidx[p]]); }
    __device__ __forceinline__ int occupant(int k, int i) const { return __builtin_amdgcn_readfirstlane(image[mr_kfmp_at(*M, k, i)]); }   // marked: inside the image
    __device__ __forceinline__ bool point_ok(int q) const { return lm_mp_ok(*M, q); }
    __device__ __forceinline__ void skipped() {
        if (lane == 0) atomicOr(&flags[MR_F_OP_BAD], 1);
    }
};

// ---- grid (maps), 64 threads ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mf_walk_kernel(MfBatch B) {
    __shared__ int32_t skf[MR_MAX_OBS];
    __shared__ uint16_t sord[MR_MAX_OBS];
    const int m = blockIdx.x, lane = threadIdx.x;
    const LmMap& M = B.maps[m];
    const size_t S = (size_t)B.mp_cap + 1, c = (size_t)B.cap;
    int32_t* const flags = B.W.flags + MR_NFLAGS * m;
    if (flags[MR_F_OBS_OVER]) return;                                   // an input row above the ceiling: the call is refused
    const int n = lm_list_n(B.n[m], B.cap);
    const int32_t* const raw = reinterpret_cast<const int32_t*>(B.ops + m * c);   // five words an op
    int32_t* const oc = B.oc + m * c;
    MfWorldDev world;
    world.bind(B.W, m, S, skf, sord, lane);
    world.M = &M; world.image = B.image + (size_t)m * B.kfmp_cap;
    MfEmitDev emit = {&M, B.image + (size_t)m * B.kfmp_cap, flags, B.kfmp_cap, lane};
    int fused = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool go = i < n && oc[i] == MF_TO_WALK;
        int w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0;
        if (go) { w0 = raw[5 * (size_t)i]; w1 = raw[5 * (size_t)i + 1]; w2 = raw[5 * (size_t)i + 2]; w3 = raw[5 * (size_t)i + 3]; w4 = raw[5 * (size_t)i + 4]; }
        unsigned long long mask = __ballot(go);
        while (mask) {                                                  // wave-uniform, in list order
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int j = base + l;
            MrOp e;
            e.kind = __builtin_amdgcn_readlane(w0, l); e.a = __builtin_amdgcn_readlane(w1, l); e.b = __builtin_amdgcn_readlane(w2, l);
            e.idx = __builtin_amdgcn_readlane(w3, l);
            const int ow = __builtin_amdgcn_readlane(w4, l);
            e.octave = (uint8_t)(ow & 0xff); e.weight = (uint8_t)((ow >> 8) & 0xff); e.pad[0] = e.pad[1] = 0;
            wave_mem_sync();                                             // what lane 0 wrote in the op before is every lane's to read
            int moved, erased;
            const int out = mf_walk_op(world, e, j, emit, moved, erased);
            fused += mf_counts(out) ? 1 : 0;
            if (lane == 0) { oc[j] = out; B.mv[m * c + j] = moved; B.er[m * c + j] = erased; }
        }
    }
    if (lane == 0) B.fused[m] = fused;
}

// ---- grid (ceil(ninv / 4), maps), 256 threads: a wavefront per involved point --------------------------------------------------
__global__ __launch_bounds__(MF_NT) void mf_commit_kernel(MfBatch B) {
    const int m = blockIdx.y, lane = threadIdx.x & 63, ci = blockIdx.x * (MF_NT / 64) + (threadIdx.x >> 6);
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    if (mf_gate(B, m)) return;
    if (ci >= min(B.W.cidx[m * S + M.n_mp], B.W.ninv)) return;
    map_row_commit(B.W, m, S, X, ci, lane);
}

// ---- grid (ceil((mp_cap + 1) / 256), maps) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(MF_NT) void mf_copy_kernel(MfBatch B) {
    const int m = blockIdx.y, p = blockIdx.x * MF_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    const int32_t* const newptr = B.W.newptr + m * S;
    const int32_t* const flags = B.W.flags + MR_NFLAGS * m;
    const int n_mp = M.n_mp, need = newptr[n_mp];
    const bool obs_over = flags[MR_F_OBS_OVER] != 0, table_over = !obs_over && need > X.obs_cap_out;
    bool committed;
    const int status = mr_call_status(false, obs_over, table_over, flags[MR_F_OP_BAD] != 0, flags[MR_F_OBS_BAD] != 0, committed);
    if (p == n_mp) {
        B.status[m] = status;
        if (table_over || committed) B.n_obs_out[m] = need;
    }
    if (!committed) return;
    if (p <= n_mp) X.obs_ptr_out[p] = newptr[p];
    if (p == n_mp) { B.n_touched[m] = B.W.tpos[m * S + n_mp]; B.n_fused[m] = B.fused[m]; }
    bool sk = true;
    if (p < n_mp) {
        sk = B.W.cnt[m * S + p] > 0;                                    // mf_commit_kernel writes that row
        if (sk && mf_scan_src(B, m, 1, 1, p)) B.touched[(size_t)m * B.mp_cap + B.W.tpos[m * S + p]] = p;   // tpos < the receivers before p <= p
    }
    map_copy_unnamed_rows<MF_NT>(p & ~63, sk, M.obs_ptr, newptr, n_mp, M.obs_kf, X.obs_idx, X.obs_octave, X.obs_weight, X.obs_kf_out, X.obs_idx_out,
                                 X.obs_octave_out, X.obs_weight_out);
}

// ---- grid (ceil(max(kfmp_cap, cap) / 256), maps) --------------------------------------------------------------------------------
__global__ __launch_bounds__(MF_NT) void mf_finish_kernel(MfBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * MF_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MrIndex& X = B.X[m];
    const size_t c = (size_t)B.cap;
    if (mf_gate(B, m)) return;
    if (i < lm_list_n(B.n[m], B.cap)) { B.outcome[m * c + i] = B.oc[m * c + i]; B.moved[m * c + i] = B.mv[m * c + i]; B.erased[m * c + i] = B.er[m * c + i]; }
    if (i >= min(M.kf_mp_ptr[M.n_kf], B.kfmp_cap)) return;
    const int v = B.image[(size_t)m * B.kfmp_cap + i];
    if (v != X.kf_mp[i]) X.kf_mp[i] = v;
}

static hipError_t mf_launch(const MfBatch& B, size_t clear_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.W.flags, 0, clear_bytes, st);        // flags is the workspace's first byte
    if (e != hipSuccess) return e;
    const unsigned nm = (unsigned)B.n_maps, nparts = (unsigned)B.W.nparts;
    const auto blocks = [](int n, int per) { return (unsigned)std::max(1, (n + per - 1) / per); };
    hipLaunchKernelGGL(mf_mark_kernel, dim3(blocks(std::max(B.cap, B.kfmp_cap), MF_NT), nm), dim3(MF_NT), 0, st, B);
    hipLaunchKernelGGL(mf_scan_sum_kernel, dim3(nparts, nm, 1), dim3(MF_NT), 0, st, B, 0);
    hipLaunchKernelGGL(mf_scan_parts_kernel, dim3(nm, 1), dim3(MF_NT), 0, st, B);
    hipLaunchKernelGGL(mf_scan_add_kernel, dim3(nparts, nm, 1), dim3(MF_NT), 0, st, B, 0);
    if (B.W.ninv > 0) hipLaunchKernelGGL(mf_prep_kernel, dim3(blocks(B.W.ninv, MF_NT / 64), nm), dim3(MF_NT), 0, st, B);
    hipLaunchKernelGGL(mf_walk_kernel, dim3(nm), dim3(64), 0, st, B);
    hipLaunchKernelGGL(mf_scan_sum_kernel, dim3(nparts, nm, 2), dim3(MF_NT), 0, st, B, 1);
    hipLaunchKernelGGL(mf_scan_parts_kernel, dim3(nm, 2), dim3(MF_NT), 0, st, B);
    hipLaunchKernelGGL(mf_scan_add_kernel, dim3(nparts, nm, 2), dim3(MF_NT), 0, st, B, 1);
    if (B.W.ninv > 0) hipLaunchKernelGGL(mf_commit_kernel, dim3(blocks(B.W.ninv, MF_NT / 64), nm), dim3(MF_NT), 0, st, B);
    hipLaunchKernelGGL(mf_copy_kernel, dim3(nparts, nm), dim3(MF_NT), 0, st, B);
    if (std::max(B.kfmp_cap, B.cap) > 0) hipLaunchKernelGGL(mf_finish_kernel, dim3(blocks(std::max(B.kfmp_cap, B.cap), MF_NT), nm), dim3(MF_NT), 0, st, B);
    return hipGetLastError();
}

// ---- the list builder: grid (ceil(q_cap / 256), frames), a lane per query ------------------------------------------------------
struct MfList {
    int32_t nframes, n_maps, kp_cap, q_cap, cap, reserved;
    const int32_t* m; const int32_t* match_kp; const int32_t* query_point; const slamit_kp* kps_un; const float* kp_ur;
    const int32_t* frame_map; const int32_t* frame_kf; const int32_t* base;
    MrOp* ops; int32_t* n; int32_t* status;
};
__device__ __forceinline__ bool mf_list_frame_ok(const MfList& Q, int f) {
    const int b = Q.base[f];
    return (unsigned)Q.frame_map[f] < (unsigned)Q.n_maps && b >= 0 && b <= Q.cap - Q.q_cap;
}
__global__ __launch_bounds__(MF_NT) void mf_list_kernel(MfList Q) {
    const int f = blockIdx.y, q = blockIdx.x * MF_NT + (int)threadIdx.x;
    const bool ok = mf_list_frame_ok(Q, f);
    if (q == 0) {
        Q.status[f] = ok ? 0 : MF_BAD_SLOT;
        if (ok) atomicMax(&Q.n[Q.frame_map[f]], Q.base[f] + Q.q_cap);    // the list ends where its last slice ends; d_n was cleared on the stream
    }
    if (!ok || q >= Q.q_cap) return;
    MrOp e;
    e.kind = MF_FUSE; e.a = -1; e.b = Q.frame_kf[f]; e.idx = -1; e.octave = 0; e.weight = 1; e.pad[0] = e.pad[1] = 0;
    if (q < lm_list_n(Q.m[f], Q.q_cap)) {
        const size_t fq = (size_t)f * Q.q_cap + q;
        e.a = Q.query_point[fq]; e.idx = Q.match_kp[fq];
        if (e.idx >= 0 && e.idx < Q.kp_cap) {
            const size_t fk = (size_t)f * Q.kp_cap + e.idx;
            e.octave = (uint8_t)Q.kps_un[fk].octave;
            e.weight = Q.kp_ur && Q.kp_ur[fk] >= 0.f ? 2 : 1;
        }
    }
    Q.ops[(size_t)Q.frame_map[f] * Q.cap + Q.base[f] + q] = e;           // base + q < cap
}
extern "C" {   // what the host form checks before anything is launched: map_check.h and its own arguments

int slamit_map_fuse_apply(int device, const slamit_map_index* map, const slamit_replace_index* X, int32_t n, const slamit_map_replace* ops, int32_t* outcome,
                          int32_t* moved, int32_t* erased, int32_t* touched, int32_t* n_touched, int32_t* n_fused, int32_t* n_obs_out, int32_t* status) {
    const char* const where = "slamit_map_fuse_apply";
    if (n < 0 || !n_touched || !n_fused || !n_obs_out || !status || (n && (!ops || !outcome || !moved || !erased))) return slamit_refuse(where, "null array or negative n");
    if (n > SLAMIT_FUSE_MAX_OPS) return slamit_refuse(where, "more than SLAMIT_FUSE_MAX_OPS ops", SLAMIT_ERR_CAPACITY);
    if (const char* bad = map_replace_tables_error(map, X, touched)) return slamit_refuse(where, bad);
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf];
    if (!map_slots_ok(X->kf_mp, n_kfmp, -1, n_mp)) return slamit_refuse(where, "kf_mp holds a point slot outside [-1, n_mp)");
    for (int i = 0; i < n; ++i) {
        const slamit_map_replace& e = ops[i];
        if (e.kind != SLAMIT_REPLACE_REPLACE && e.kind != SLAMIT_REPLACE_ADD_OBS && e.kind != SLAMIT_FUSE_FUSE) return slamit_refuse(where, "an op's kind outside 1..3");
        if (e.kind == SLAMIT_FUSE_FUSE && e.idx < 0) continue;           // no match: nothing else is read
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
    MfBatch H;
    size_t clear_bytes = 0;
    const size_t ws_bytes = mf_ws_layout(1, n, n_mp, (int)n_kfmp, nullptr, nullptr, &clear_bytes);
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<MfBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, MfBatch& Q) {
            io.clear();
            Q.n_maps = 1; Q.cap = n; Q.mp_cap = n_mp; Q.kfmp_cap = (int)n_kfmp;
            map_stage_tables(b, io, map, X, Q.maps[0], Q.X[0]);
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.ops = reinterpret_cast<const MrOp*>(b.in(ops, (size_t)n));
            Q.outcome = slamit_inout(b, io, outcome, (size_t)n); Q.moved = slamit_inout(b, io, moved, (size_t)n); Q.erased = slamit_inout(b, io, erased, (size_t)n);
            Q.touched = slamit_inout(b, io, touched, (size_t)n_mp);
            Q.n_touched = slamit_inout(b, io, n_touched, 1); Q.n_fused = slamit_inout(b, io, n_fused, 1); Q.n_obs_out = slamit_inout(b, io, n_obs_out, 1);
            Q.status = b.out(status, 1);
            unsigned char* const ws = b.scratch<unsigned char>(ws_bytes);
            if (ws) mf_ws_layout(1, n, n_mp, (int)n_kfmp, ws, &Q, nullptr);
            H = Q;
        },
        [&](const MfBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : mf_launch(H, clear_bytes, S.st);
        });
}

size_t slamit_map_fuse_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap) {
    if (n_maps < 1 || cap < 0 || mp_cap < 0 || kfmp_cap < 0 || cap > SLAMIT_FUSE_MAX_OPS) return 0;
    return mf_ws_layout(n_maps, cap, mp_cap, kfmp_cap, nullptr, nullptr, nullptr);
}

int slamit_map_fuse_batch_dev(int device, const slamit_map_fuse_batch_rec* R, void* stream) {
    const char* const where = "slamit_map_fuse_batch_dev";
    if (!R || R->n_maps < 0 || R->cap < 0 || R->mp_cap < 0 || R->kfmp_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->n_maps == 0) return SLAMIT_OK;
    if (R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->index) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_FUSE_MAX_OPS) return slamit_refuse(where, "cap above SLAMIT_FUSE_MAX_OPS", SLAMIT_ERR_CAPACITY);
    if (R->mp_cap == 0x7fffffff) return slamit_refuse(where, "mp_cap above 2^31 - 2", SLAMIT_ERR_CAPACITY);
    if (const char* bad = map_replace_batch_error(R->n_maps, R->mp_cap, R->maps, R->index)) return slamit_refuse(where, bad);
    if (!R->d_n || !R->d_n_touched || !R->d_n_fused || !R->d_n_obs_out || !R->d_status || (R->cap && (!R->d_ops || !R->d_outcome || !R->d_moved || !R->d_erased)) ||
        (R->mp_cap && !R->d_touched))
        return slamit_refuse(where, "null array");
    size_t clear_bytes = 0;
    const size_t need = mf_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, nullptr, nullptr, &clear_bytes);
    if (!R->d_workspace || R->workspace_bytes < need || ((uintptr_t)R->d_workspace & 7)) return slamit_refuse(where, "workspace missing, misaligned or below slamit_map_fuse_workspace()");
    SLAMIT_USE_DEVICE(device);
    MfBatch B;
    memset(&B, 0, sizeof(B));
    B.n_maps = R->n_maps; B.cap = R->cap; B.mp_cap = R->mp_cap; B.kfmp_cap = R->kfmp_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.X, R->index, sizeof(MrIndex) * (size_t)R->n_maps);
    B.ops = reinterpret_cast<const MrOp*>(R->d_ops); B.n = R->d_n;
    B.outcome = R->d_outcome; B.moved = R->d_moved; B.erased = R->d_erased; B.touched = R->d_touched; B.n_touched = R->d_n_touched; B.n_fused = R->d_n_fused;
    B.n_obs_out = R->d_n_obs_out; B.status = R->d_status;
    mf_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, (unsigned char*)R->d_workspace, &B, nullptr);
    HIP_TRY_AT(where, mf_launch(B, clear_bytes, (hipStream_t)stream));
    return SLAMIT_OK;
}

int slamit_fuse_list_batch_dev(int device, const slamit_fuse_list_batch_rec* R, void* stream) {
    const char* const where = "slamit_fuse_list_batch_dev";
    if (!R || R->nframes < 0 || R->n_maps < 0 || R->kp_cap < 0 || R->q_cap < 0 || R->cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nframes == 0) return SLAMIT_OK;
    if (R->n_maps < 1 || R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_FUSE_MAX_OPS) return slamit_refuse(where, "cap above SLAMIT_FUSE_MAX_OPS", SLAMIT_ERR_CAPACITY);
    if (R->nframes > 65535) return slamit_refuse(where, "more than 65,535 frames", SLAMIT_ERR_CAPACITY);
    if (!R->d_m || !R->d_frame_map || !R->d_frame_kf || !R->d_base || !R->d_n || !R->d_status ||
        (R->q_cap && (!R->d_match_kp || !R->d_query_point || !R->d_ops)) || (R->q_cap && R->kp_cap && !R->d_kps_un))
        return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    MfList Q;
    memset(&Q, 0, sizeof(Q));
    Q.nframes = R->nframes; Q.n_maps = R->n_maps; Q.kp_cap = R->kp_cap; Q.q_cap = R->q_cap; Q.cap = R->cap;
    Q.m = R->d_m; Q.match_kp = R->d_match_kp; Q.query_point = R->d_query_point; Q.kps_un = R->d_kps_un; Q.kp_ur = R->d_kp_ur;
    Q.frame_map = R->d_frame_map; Q.frame_kf = R->d_frame_kf; Q.base = R->d_base;
    Q.ops = reinterpret_cast<MrOp*>(R->d_ops); Q.n = R->d_n; Q.status = R->d_status;
    HIP_TRY_AT(where, hipMemsetAsync(R->d_n, 0, sizeof(int32_t) * (size_t)R->n_maps, (hipStream_t)stream));
    hipLaunchKernelGGL(mf_list_kernel, dim3((unsigned)std::max(1, (R->q_cap + MF_NT - 1) / MF_NT), (unsigned)R->nframes), dim3(MF_NT), 0, (hipStream_t)stream, Q);
    HIP_TRY_AT(where, hipGetLastError());
    return SLAMIT_OK;
}

}  // extern "C"
