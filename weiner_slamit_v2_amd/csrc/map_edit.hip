// map_edit.hip — MapPoint::AddObservation, ::EraseObservation and ::SetBadFlag applied to the resident tables by one call
// (include/slamit.h, slamit_map_edit_apply / slamit_map_edit_batch_dev; the walk is stated in map_edit.h, whose me_walk the kernel runs
// over a row in LDS).  Nothing here is float.  Every kernel takes grid.y = the map; no workgroup waits on another inside a kernel.
//
// me_hist_kernel       a thread per edit: the bucket sizes by point, integer atomics.
// me_scan_*            the device scan, used twice: per-workgroup sums of ME_SCAN_BLOCK entries, one workgroup scanning the sums, an add
//                      pass that rescans its block.  Exclusive, the total one past the end; two arrays at once (row lengths, touched flags).
// me_scatter_kernel    a thread per edit: its list index into the point's bucket through an atomic cursor, in arbitrary order; and a
//                      thread per point without edits: its row keeps its length.
// me_apply_kernel      one wavefront per point with edits (the wavefront of the bucket's first entry): the bucket ordered by list index in
//                      LDS, the row gathered into LDS, me_walk over it -- membership by wave ballot, the edits one after the other.  LDS:
//                      ME_ROW x (4 + 4 + 1 + 1) bytes of row + 2 x 256 bytes of bucket = 6,272 bytes per wavefront, so the 160 KiB of a CU
//                      hold 26 such wavefronts of its 32.  Instantiated twice: the COUNT pass leaves the new length, the WRITE pass, after the
//                      scan of the lengths, writes the row and its columns at the new offset, mp_bad / mp_nobs / mp_ref_kf, and issues the
//                      kf_mp writes as atomicMax of (list index + 1) << 32 | (value + 1) into the 64-bit workspace beside kf_mp.
// me_copy_kernel       the rows of the points without edits: a wavefront takes 64 consecutive points, whose entries are consecutive in the
//                      old table, and every lane finds its entry's point by bisection in LDS (map_rows_dev.h); the new pointer array,
//                      the per-point status, touched (compacted through the scan), the counts and the call's status.
// me_kfmp_kernel       the winners of the kf_mp workspace into kf_mp.
// THE GATE: every kernel that writes a caller's array first reads the table's need (the scan's total) from device memory and leaves
// when it exceeds obs_cap_out; me_copy_kernel writes n_obs_out and the status before it does.
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
#include "map_edit.h"
#include "map_rows_dev.h"

static_assert(sizeof(MeEdit) == sizeof(slamit_map_edit) && offsetof(MeEdit, mp) == offsetof(slamit_map_edit, mp) && offsetof(MeEdit, idx) == offsetof(slamit_map_edit, idx) &&
                  offsetof(MeEdit, octave) == offsetof(slamit_map_edit, octave) && offsetof(MeEdit, weight) == offsetof(slamit_map_edit, weight),
              "slamit_map_edit is MeEdit");
static_assert(sizeof(MeIndex) == sizeof(slamit_edit_index) && offsetof(MeIndex, obs_weight) == offsetof(slamit_edit_index, obs_weight) &&
                  offsetof(MeIndex, mp_bad) == offsetof(slamit_edit_index, mp_bad) && offsetof(MeIndex, kf_mp) == offsetof(slamit_edit_index, kf_mp) &&
                  offsetof(MeIndex, obs_ptr_out) == offsetof(slamit_edit_index, obs_ptr_out) && offsetof(MeIndex, obs_weight_out) == offsetof(slamit_edit_index, obs_weight_out) &&
                  offsetof(MeIndex, obs_cap_out) == offsetof(slamit_edit_index, obs_cap_out),
              "slamit_edit_index is MeIndex");
static_assert(sizeof(LmMap) == sizeof(slamit_map_index), "slamit_map_index is LmMap");
static_assert(ME_ADD_OBS == SLAMIT_EDIT_ADD_OBS && ME_ERASE_OBS == SLAMIT_EDIT_ERASE_OBS && ME_SET_BAD == SLAMIT_EDIT_SET_BAD && ME_MATCH == SLAMIT_EDIT_MATCH &&
                  ME_REF_END == SLAMIT_EDIT_REF_END && ME_EDIT_OVERFLOW == SLAMIT_EDIT_EDIT_OVERFLOW && ME_OBS_OVERFLOW == SLAMIT_EDIT_OBS_OVERFLOW &&
                  ME_BAD_SLOT == SLAMIT_EDIT_BAD_SLOT && ME_TABLE_OVERFLOW == SLAMIT_EDIT_TABLE_OVERFLOW && ME_MAX_PER_POINT == SLAMIT_EDIT_MAX_PER_POINT &&
                  ME_MAX_EDITS == SLAMIT_EDIT_MAX_EDITS && ME_MAX_OBS == SLAMIT_UPKEEP_MAX_OBS,
              "map_edit.h restates the C-ABI's constants");
static_assert(ME_MAX_PER_POINT == 64 && ME_ROW <= 32 * 64 && ME_SCAN_BLOCK == 256, "a bucket is one wavefront; a lane's alive bits are one word; the scan's workgroup");

#define ME_NT 256

// The batch as the kernels' argument: the maps' records travel with it, the arrays stay where the caller keeps them.  The workspace
// rows of a map lie S = mp_cap + 1 apart.
struct MeBatch {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    MeIndex X[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const MeEdit* edits; const int32_t* n;
    int32_t* status_mp; int32_t* touched; int32_t* n_touched; int32_t* n_obs_out; int32_t* status;
    unsigned long long* kfw;   // [n_maps][kfmp_cap]   cleared
    int32_t* flags;            // [n_maps][4]          cleared: the call's status bits
    int32_t* cnt;              // [n_maps][S]          cleared: edits per point
    int32_t* cursor;           // [n_maps][S]          cleared
    int32_t* bstart;           // [n_maps][S]          the buckets' first entries, the number bucketed at [n_mp]
    int32_t* bucket;           // [n_maps][cap]        list indices by point
    int32_t* newlen;           // [n_maps][S]
    int32_t* newptr;           // [n_maps][S]          the new pointer array, the table's need at [n_mp]
    int32_t* tflag;            // [n_maps][S]
    int32_t* tpos;             // [n_maps][S]
    int32_t* st;               // [n_maps][S]          the count pass's status of a point with edits
    int32_t* parts;            // [n_maps][2][nparts + 1]
    int32_t nparts, reserved;
};

// the workspace: what the call clears first, then the rest.  -> bytes; *clear_bytes the cleared head
static size_t me_ws_layout(int n_maps, int cap, int mp_cap, int kfmp_cap, unsigned char* base, MeBatch* B, size_t* clear_bytes) {
    const size_t S = (size_t)mp_cap + 1, nm = (size_t)n_maps, nparts = (S + ME_SCAN_BLOCK - 1) / ME_SCAN_BLOCK;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) & ~(size_t)15; return base ? base + at : nullptr; };
    unsigned char* const kfw = take(8 * nm * (size_t)kfmp_cap);
    unsigned char* const flags = take(4 * nm * 4);
    unsigned char* const cnt = take(4 * nm * S);
    unsigned char* const cursor = take(4 * nm * S);
    if (clear_bytes) *clear_bytes = off;
    unsigned char* const bstart = take(4 * nm * S);
    unsigned char* const bucket = take(4 * nm * (size_t)cap);
    unsigned char* const newlen = take(4 * nm * S);
    unsigned char* const newptr = take(4 * nm * S);
    unsigned char* const tflag = take(4 * nm * S);
    unsigned char* const tpos = take(4 * nm * S);
    unsigned char* const st = take(4 * nm * S);
    unsigned char* const parts = take(4 * nm * 2 * (nparts + 1));
    if (B) {
        B->kfw = (unsigned long long*)kfw; B->flags = (int32_t*)flags; B->cnt = (int32_t*)cnt; B->cursor = (int32_t*)cursor; B->bstart = (int32_t*)bstart;
        B->bucket = (int32_t*)bucket; B->newlen = (int32_t*)newlen; B->newptr = (int32_t*)newptr; B->tflag = (int32_t*)tflag; B->tpos = (int32_t*)tpos;
        B->st = (int32_t*)st; B->parts = (int32_t*)parts; B->nparts = (int32_t)nparts;
    }
    return off;
}

// ---- grid (ceil(cap / 256), maps) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_NT) void me_hist_kernel(MeBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * ME_NT + (int)threadIdx.x;
    if (i >= lm_list_n(B.n[m], B.cap)) return;
    const LmMap& M = B.maps[m];
    const int p = B.edits[(size_t)m * B.cap + i].mp;
    if (lm_mp_ok(M, p)) atomicAdd(&B.cnt[(size_t)m * (B.mp_cap + 1) + p], 1);
    else atomicOr(&B.flags[4 * m], ME_BAD_SLOT);
}

// ---- the device scan: the three kernels over map_rows_dev.h's bodies; a, b, out_a, out_b: rows S apart ---------------------------
// grid (nparts, maps, arrays), (maps, arrays), (nparts, maps, arrays)
__global__ __launch_bounds__(ME_NT) void me_scan_sum_kernel(MeBatch B, const int32_t* a, const int32_t* b) {
    const int m = blockIdx.y;
    const size_t r = m * ((size_t)B.mp_cap + 1);
    map_scan_sum<ME_NT>(B.parts, B.nparts, B.maps[m].n_mp, [&](int z, int i) { return (z ? b : a)[r + i]; });
}
__global__ __launch_bounds__(ME_NT) void me_scan_parts_kernel(MeBatch B) { map_scan_parts<ME_NT>(B.parts, B.nparts); }
__global__ __launch_bounds__(ME_NT) void me_scan_add_kernel(MeBatch B, const int32_t* a, const int32_t* b, int32_t* out_a, int32_t* out_b) {
    const int m = blockIdx.y;
    const size_t r = m * ((size_t)B.mp_cap + 1);
    map_scan_add<ME_NT>(B.parts, B.nparts, B.maps[m].n_mp, [&](int z, int i) { return (z ? b : a)[r + i]; }, (blockIdx.z ? out_b : out_a) + r);   // n_mp <= mp_cap: inside the row
}

// ---- grid (ceil(max(cap, mp_cap) / 256), maps) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_NT) void me_scatter_kernel(MeBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * ME_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const size_t S = (size_t)B.mp_cap + 1;
    if (i < lm_list_n(B.n[m], B.cap)) {
        const int p = B.edits[(size_t)m * B.cap + i].mp;
        if (lm_mp_ok(M, p)) {
            const int at = B.bstart[m * S + p] + atomicAdd(&B.cursor[m * S + p], 1);   // < bstart[p + 1] <= the list's length <= cap
            B.bucket[(size_t)m * B.cap + at] = i;
        }
    }
    if (i < M.n_mp && B.cnt[m * S + i] == 0) {
        B.newlen[m * S + i] = M.obs_ptr[i + 1] - M.obs_ptr[i];
        B.tflag[m * S + i] = 0;
    }
}

// ---- the row of me_walk in LDS: entry e is lane e & 63's, whose bit e >> 6 of `alive` says whether it is live --------------------
struct MeRowDev {
    int32_t* kf; int32_t* idx; uint8_t* octave; uint8_t* weight;
    int n, lane;
    uint32_t alive;
    __device__ __forceinline__ bool live(int c) const { return (alive >> c) & 1u; }
    __device__ __forceinline__ int uniform(int v) const { return __builtin_amdgcn_readfirstlane(v); }
    __device__ __forceinline__ int find(int k) const {
        for (int c = 0; c * 64 < n; ++c) {
            const int e = c * 64 + lane;
            const unsigned long long hit = __ballot(e < n && live(c) && kf[e] == k);
            if (hit) return c * 64 + __ffsll((long long)hit) - 1;
        }
        return -1;
    }
    __device__ __forceinline__ int idx_at(int pos) const { return idx[pos]; }
    __device__ __forceinline__ int weight_at(int pos) const { return weight[pos]; }
    __device__ __forceinline__ void push(int k, int i, uint8_t o, uint8_t w) {   // n < ME_ROW: at most ME_MAX_PER_POINT pushes onto ME_MAX_OBS
        if (lane == 0) { kf[n] = k; idx[n] = i; octave[n] = o; weight[n] = w; }
        if (lane == (n & 63)) alive |= 1u << (n >> 6);
        ++n;
        wave_mem_sync();
    }
    __device__ __forceinline__ void kill(int pos) {
        if (lane == (pos & 63)) alive &= ~(1u << (pos >> 6));
    }
    __device__ __forceinline__ int min_slot() const {
        uint32_t best = 0xffffffffu;
        for (int c = 0; c * 64 < n; ++c) {
            const int e = c * 64 + lane;
            if (e < n && live(c)) best = min(best, (uint32_t)kf[e]);
        }
        best = wave_min_u32(best);
        return best == 0xffffffffu ? -1 : (int)best;
    }
    template <class Emit>
    __device__ __forceinline__ void emit_live(Emit& emit, int li) const {
        for (int c = 0; c * 64 < n; ++c) {
            const int e = c * 64 + lane;
            if (e < n && live(c)) emit.mine(kf[e], idx[e], -1, li);
        }
    }
    __device__ __forceinline__ void clear() { alive = 0; }
};
struct MeEmitNoneDev {
    __device__ __forceinline__ void mine(int, int, int, int) {}
    __device__ __forceinline__ void one(int, int, int, int) {}
};
struct MeEmitDev {
    const LmMap* M; unsigned long long* kfw;
    int kfmp_cap, lane, bad;
    __device__ __forceinline__ void mine(int k, int i, int value, int li) {   // this lane's write
        const long long at = me_kfmp_at(*M, k, i);
        if (at < 0 || at >= kfmp_cap) { bad = 1; return; }
        atomicMax(&kfw[at], ((unsigned long long)(unsigned)(li + 1) << 32) | (unsigned)(value + 1));
    }
    __device__ __forceinline__ void one(int k, int i, int value, int li) {    // the wavefront's write
        if (lane == 0) mine(k, i, value, li);
    }
};

// ---- grid (cap, maps), 64 threads: wavefront j is the point's whose bucket starts at entry j ----------------------------------
template <bool WRITE>
__global__ __launch_bounds__(64) void me_apply_kernel(MeBatch B) {
    __shared__ int32_t rkf[ME_ROW], ridx[ME_ROW];
    __shared__ uint8_t roct[ME_ROW], rwgt[ME_ROW];
    __shared__ int32_t raw[ME_MAX_PER_POINT], order[ME_MAX_PER_POINT];
    const int m = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
    const LmMap& M = B.maps[m];
    const MeIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    const int32_t* const newptr = B.newptr + m * S;
    if (WRITE && newptr[M.n_mp] > X.obs_cap_out) return;                // the gate; the whole wavefront, here and at every return below
    const int32_t* const bstart = B.bstart + m * S;
    if (j >= bstart[M.n_mp]) return;
    const int32_t* const bucket = B.bucket + (size_t)m * B.cap;
    const MeEdit* const edits = B.edits + (size_t)m * B.cap;
    const int p = __builtin_amdgcn_readfirstlane(edits[bucket[j]].mp);   // inside the table: only such edits are bucketed
    if (j != bstart[p]) return;
    const int ne = __builtin_amdgcn_readfirstlane(B.cnt[m * S + p]);
    const int o0 = __builtin_amdgcn_readfirstlane(M.obs_ptr[p]), len0 = __builtin_amdgcn_readfirstlane(M.obs_ptr[p + 1]) - o0;
    int refused = 0;
    if (ne > ME_MAX_PER_POINT) refused = ME_EDIT_OVERFLOW;
    else if (len0 > ME_MAX_OBS) refused = ME_OBS_OVERFLOW;
    else if (WRITE && (B.st[m * S + p] & ME_OBS_OVERFLOW)) refused = ME_OBS_OVERFLOW;   // the count pass found an add past the ceiling
    if (refused) {                                                      // the row as it is, none of the edits
        if (!WRITE) {
            if (lane == 0) { B.newlen[m * S + p] = len0; B.tflag[m * S + p] = 0; B.st[m * S + p] = refused; }
            return;
        }
        const int d0 = newptr[p];                                       // d0 + len0 <= the need <= obs_cap_out
        for (int e = lane; e < len0; e += 64) {
            X.obs_kf_out[d0 + e] = M.obs_kf[o0 + e]; X.obs_idx_out[d0 + e] = X.obs_idx[o0 + e];
            X.obs_octave_out[d0 + e] = X.obs_octave[o0 + e]; X.obs_weight_out[d0 + e] = X.obs_weight[o0 + e];
        }
        if (lane == 0) B.status_mp[(size_t)m * B.mp_cap + p] = refused;
        return;
    }
    MeRowDev r = {rkf, ridx, roct, rwgt, len0, lane, 0u};
    for (int c = 0; c * 64 < len0; ++c) {                               // len0 <= ME_MAX_OBS
        const int e = c * 64 + lane;
        if (e < len0) {
            rkf[e] = M.obs_kf[o0 + e]; ridx[e] = X.obs_idx[o0 + e]; roct[e] = X.obs_octave[o0 + e]; rwgt[e] = X.obs_weight[o0 + e];
            r.alive |= 1u << c;
        }
    }
    if (lane < ne) raw[lane] = bucket[j + lane];                        // ne <= 64 entries from bstart[p] = j
    wave_mem_sync();
    if (lane < ne) {
        const int li = raw[lane];
        int rank = 0;                                                   // list indices are distinct
        for (int t = 0; t < ne; ++t) rank += raw[t] < li;
        order[rank] = li;
    }
    wave_mem_sync();
    MeState s = {len0, X.mp_nobs[p], X.mp_bad[p], X.mp_ref_kf[p], 0, 0};
    if (!WRITE) {
        MeEmitNoneDev none;
        me_walk(M, p, r, s, edits, order, ne, none);
        const bool over = (s.status & ME_OBS_OVERFLOW) != 0;
        if (lane == 0) { B.newlen[m * S + p] = over ? len0 : s.live; B.tflag[m * S + p] = over ? 0 : s.changed; B.st[m * S + p] = s.status; }
        return;
    }
    MeEmitDev emit = {&M, B.kfw + (size_t)m * B.kfmp_cap, B.kfmp_cap, lane, 0};
    me_walk(M, p, r, s, edits, order, ne, emit);
    int d = newptr[p];                                                  // d + s.live <= the need <= obs_cap_out
    for (int c = 0; c * 64 < r.n; ++c) {
        const int e = c * 64 + lane;
        const bool keep = e < r.n && r.live(c);
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int at = d + __popcll(mask & ((1ull << lane) - 1ull));
            X.obs_kf_out[at] = rkf[e]; X.obs_idx_out[at] = ridx[e]; X.obs_octave_out[at] = roct[e]; X.obs_weight_out[at] = rwgt[e];
        }
        d += __popcll(mask);
    }
    const bool bad = __ballot(emit.bad != 0) != 0;
    if (lane == 0) {
        X.mp_bad[p] = (uint8_t)s.bad; X.mp_nobs[p] = s.nobs; X.mp_ref_kf[p] = s.ref;
        B.status_mp[(size_t)m * B.mp_cap + p] = s.status | (bad ? ME_BAD_SLOT : 0);
    }
}

// ---- grid (ceil((mp_cap + 1) / 256), maps) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_NT) void me_copy_kernel(MeBatch B) {
    const int m = blockIdx.y, p = blockIdx.x * ME_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MeIndex& X = B.X[m];
    const size_t S = (size_t)B.mp_cap + 1;
    const int32_t* const newptr = B.newptr + m * S;
    const int n_mp = M.n_mp, need = newptr[n_mp];
    const bool gate = need > X.obs_cap_out;
    if (p == n_mp) { B.n_obs_out[m] = need; B.status[m] = B.flags[4 * m] | (gate ? ME_TABLE_OVERFLOW : 0); }
    if (gate) return;
    if (p <= n_mp) X.obs_ptr_out[p] = newptr[p];
    if (p == n_mp) B.n_touched[m] = B.tpos[m * S + n_mp];
    bool sk = true;
    if (p < n_mp) {
        sk = B.cnt[m * S + p] > 0;                                      // me_apply_kernel writes that row and that status
        if (!sk) B.status_mp[(size_t)m * B.mp_cap + p] = 0;
        if (B.tflag[m * S + p]) B.touched[(size_t)m * B.mp_cap + B.tpos[m * S + p]] = p;   // tpos < the touched before p <= p
    }
    map_copy_unnamed_rows<ME_NT>(p & ~63, sk, M.obs_ptr, newptr, n_mp, M.obs_kf, X.obs_idx, X.obs_octave, X.obs_weight, X.obs_kf_out, X.obs_idx_out,
                                 X.obs_octave_out, X.obs_weight_out);
}

// ---- grid (ceil(kfmp_cap / 256), maps) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_NT) void me_kfmp_kernel(MeBatch B) {
    const int m = blockIdx.y, i = blockIdx.x * ME_NT + (int)threadIdx.x;
    const LmMap& M = B.maps[m];
    const MeIndex& X = B.X[m];
    if (B.newptr[(size_t)m * (B.mp_cap + 1) + M.n_mp] > X.obs_cap_out) return;
    if (i >= min(M.kf_mp_ptr[M.n_kf], B.kfmp_cap)) return;
    const unsigned long long v = B.kfw[(size_t)m * B.kfmp_cap + i];
    if (v) X.kf_mp[i] = (int)(unsigned)v - 1;
}

static hipError_t me_launch(const MeBatch& B, size_t clear_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.kfw, 0, clear_bytes, st);            // kfw is the workspace's first byte
    if (e != hipSuccess) return e;
    const unsigned nm = (unsigned)B.n_maps, nparts = (unsigned)B.nparts;
    const auto blocks = [](int n) { return (unsigned)std::max(1, (n + ME_NT - 1) / ME_NT); };
    hipLaunchKernelGGL(me_hist_kernel, dim3(blocks(B.cap), nm), dim3(ME_NT), 0, st, B);
    hipLaunchKernelGGL(me_scan_sum_kernel, dim3(nparts, nm, 1), dim3(ME_NT), 0, st, B, (const int32_t*)B.cnt, (const int32_t*)nullptr);
    hipLaunchKernelGGL(me_scan_parts_kernel, dim3(nm, 1), dim3(ME_NT), 0, st, B);
    hipLaunchKernelGGL(me_scan_add_kernel, dim3(nparts, nm, 1), dim3(ME_NT), 0, st, B, (const int32_t*)B.cnt, (const int32_t*)nullptr, B.bstart, (int32_t*)nullptr);
    hipLaunchKernelGGL(me_scatter_kernel, dim3(blocks(std::max(B.cap, B.mp_cap)), nm), dim3(ME_NT), 0, st, B);
    if (B.cap > 0) hipLaunchKernelGGL(me_apply_kernel<false>, dim3((unsigned)B.cap, nm), dim3(64), 0, st, B);
    hipLaunchKernelGGL(me_scan_sum_kernel, dim3(nparts, nm, 2), dim3(ME_NT), 0, st, B, (const int32_t*)B.newlen, (const int32_t*)B.tflag);
    hipLaunchKernelGGL(me_scan_parts_kernel, dim3(nm, 2), dim3(ME_NT), 0, st, B);
    hipLaunchKernelGGL(me_scan_add_kernel, dim3(nparts, nm, 2), dim3(ME_NT), 0, st, B, (const int32_t*)B.newlen, (const int32_t*)B.tflag, B.newptr, B.tpos);
    if (B.cap > 0) hipLaunchKernelGGL(me_apply_kernel<true>, dim3((unsigned)B.cap, nm), dim3(64), 0, st, B);
    hipLaunchKernelGGL(me_copy_kernel, dim3(nparts, nm), dim3(ME_NT), 0, st, B);
    if (B.kfmp_cap > 0) hipLaunchKernelGGL(me_kfmp_kernel, dim3(blocks(B.kfmp_cap), nm), dim3(ME_NT), 0, st, B);
    return hipGetLastError();
}

extern "C" {   // what the host forms check before anything is launched: map_check.h and their own arguments

int slamit_map_edit_apply(int device, const slamit_map_index* map, const slamit_edit_index* X, int32_t n, const slamit_map_edit* edits, int32_t* status_mp,
                          int32_t* touched, int32_t* n_touched, int32_t* n_obs_out, int32_t* status) {
    const char* const where = "slamit_map_edit_apply";
    if (n < 0 || !n_touched || !n_obs_out || !status || (n && !edits)) return slamit_refuse(where, "null array or negative n");
    if (n > SLAMIT_EDIT_MAX_EDITS) return slamit_refuse(where, "more than SLAMIT_EDIT_MAX_EDITS edits", SLAMIT_ERR_CAPACITY);
    if (!map || !X) return slamit_refuse(where, "null table");
    if (const char* bad = map_sizes_error(map)) return slamit_refuse(where, bad);
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (n_mp && (!status_mp || !touched)) return slamit_refuse(where, "null array or negative n");
    if (X->obs_cap_out < 0) return slamit_refuse(where, "negative obs_cap_out");
    if (!map->obs_ptr || !map->kf_mp_ptr || !X->obs_ptr_out) return slamit_refuse(where, "null table");
    if (!map_csr_ok(map->obs_ptr, n_mp) || !map_csr_ok(map->kf_mp_ptr, n_kf)) return slamit_refuse(where, "a CSR pointer array does not ascend from 0");
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf], cap_out = (size_t)X->obs_cap_out;
    if ((n_obs && (!map->obs_kf || !X->obs_idx || !X->obs_octave || !X->obs_weight)) || (n_mp && (!X->mp_bad || !X->mp_nobs || !X->mp_ref_kf)) || (n_kfmp && !X->kf_mp) ||
        (cap_out && (!X->obs_kf_out || !X->obs_idx_out || !X->obs_octave_out || !X->obs_weight_out)))
        return slamit_refuse(where, "null table");
    if (const char* bad = map_obs_error(map, X->obs_idx, X->obs_weight)) return slamit_refuse(where, bad);
    if (!map_slots_ok(X->mp_ref_kf, (size_t)n_mp, -1, n_kf)) return slamit_refuse(where, "mp_ref_kf holds a keyframe slot outside [-1, n_kf)");
    for (int i = 0; i < n; ++i) {
        const slamit_map_edit& e = edits[i];
        if (e.kind < SLAMIT_EDIT_ADD_OBS || e.kind > SLAMIT_EDIT_SET_BAD) return slamit_refuse(where, "an edit's kind outside 1..3");
        if (e.flags < 0 || e.flags > SLAMIT_EDIT_MATCH) return slamit_refuse(where, "an edit's flags outside 0..1");
        if (e.mp < 0 || e.mp >= n_mp) return slamit_refuse(where, "edits holds a point slot outside [0, n_mp)");
        if (e.kind == SLAMIT_EDIT_SET_BAD) continue;
        if (e.kf < 0 || e.kf >= n_kf) return slamit_refuse(where, "edits holds a keyframe slot outside [0, n_kf)");
        if (e.kind == SLAMIT_EDIT_ERASE_OBS) continue;
        if (e.idx < 0 || e.idx >= map->kf_mp_ptr[e.kf + 1] - map->kf_mp_ptr[e.kf]) return slamit_refuse(where, "edits holds a keypoint index outside its keyframe's row");
        if (e.weight != 1 && e.weight != 2) return slamit_refuse(where, "an edit's weight other than 1 or 2");
    }
    if (n_obs + (size_t)n > (size_t)0x7fffffff) return slamit_refuse(where, "the new table may need more than 2^31 - 1 entries", SLAMIT_ERR_CAPACITY);
    SLAMIT_USE_DEVICE(device);
    MeBatch H;
    size_t clear_bytes = 0;
    const size_t ws_bytes = me_ws_layout(1, n, n_mp, (int)n_kfmp, nullptr, nullptr, &clear_bytes);
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<MeBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, MeBatch& Q) {
            io.clear();
            Q.n_maps = 1; Q.cap = n; Q.mp_cap = n_mp; Q.kfmp_cap = (int)n_kfmp;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.obs_ptr = b.in(map->obs_ptr, (size_t)n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs); M.kf_mp_ptr = b.in(map->kf_mp_ptr, (size_t)n_kf + 1);
            MeIndex& E = Q.X[0];
            E.obs_idx = b.in(X->obs_idx, n_obs); E.obs_octave = b.in(X->obs_octave, n_obs); E.obs_weight = b.in(X->obs_weight, n_obs);
            E.mp_bad = slamit_inout(b, io, X->mp_bad, (size_t)n_mp); E.mp_nobs = slamit_inout(b, io, X->mp_nobs, (size_t)n_mp);
            E.mp_ref_kf = slamit_inout(b, io, X->mp_ref_kf, (size_t)n_mp); E.kf_mp = slamit_inout(b, io, X->kf_mp, n_kfmp);
            E.obs_ptr_out = slamit_inout(b, io, X->obs_ptr_out, (size_t)n_mp + 1);
            E.obs_kf_out = slamit_inout(b, io, X->obs_kf_out, cap_out); E.obs_idx_out = slamit_inout(b, io, X->obs_idx_out, cap_out);
            E.obs_octave_out = slamit_inout(b, io, X->obs_octave_out, cap_out); E.obs_weight_out = slamit_inout(b, io, X->obs_weight_out, cap_out);
            E.obs_cap_out = X->obs_cap_out;
            int32_t* h1;
            Q.n = b.in_fill<int32_t>(1, &h1);
            if (h1) h1[0] = n;
            Q.edits = reinterpret_cast<const MeEdit*>(b.in(edits, (size_t)n));
            Q.status_mp = slamit_inout(b, io, status_mp, (size_t)n_mp); Q.touched = slamit_inout(b, io, touched, (size_t)n_mp);
            Q.n_touched = slamit_inout(b, io, n_touched, 1);
            Q.n_obs_out = b.out(n_obs_out, 1); Q.status = b.out(status, 1);
            unsigned char* const ws = b.scratch<unsigned char>(ws_bytes);
            if (ws) me_ws_layout(1, n, n_mp, (int)n_kfmp, ws, &Q, nullptr);
            H = Q;
        },
        [&](const MeBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : me_launch(H, clear_bytes, S.st);
        });
}

size_t slamit_map_edit_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap) {
    if (n_maps < 1 || cap < 0 || mp_cap < 0 || kfmp_cap < 0) return 0;
    return me_ws_layout(n_maps, cap, mp_cap, kfmp_cap, nullptr, nullptr, nullptr);
}

int slamit_map_edit_batch_dev(int device, const slamit_map_edit_batch_rec* R, void* stream) {
    const char* const where = "slamit_map_edit_batch_dev";
    if (!R || R->n_maps < 0 || R->cap < 0 || R->mp_cap < 0 || R->kfmp_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->n_maps == 0) return SLAMIT_OK;
    if (R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->edit) return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cap > SLAMIT_EDIT_MAX_EDITS) return slamit_refuse(where, "cap above SLAMIT_EDIT_MAX_EDITS", SLAMIT_ERR_CAPACITY);
    if (R->mp_cap == 0x7fffffff) return slamit_refuse(where, "mp_cap above 2^31 - 2", SLAMIT_ERR_CAPACITY);
    for (int m = 0; m < R->n_maps; ++m) {
        const slamit_map_index& M = R->maps[m];
        const slamit_edit_index& X = R->edit[m];
        if (const char* bad = map_batch_sizes_error(&M)) return slamit_refuse(where, bad);
        if (M.n_mp > R->mp_cap) return slamit_refuse(where, "a map with n_mp above mp_cap");
        if (X.obs_cap_out < 0) return slamit_refuse(where, "negative obs_cap_out");
        if (!M.obs_ptr || !M.obs_kf || !M.kf_mp_ptr || !X.obs_idx || !X.obs_octave || !X.obs_weight || !X.mp_bad || !X.mp_nobs || !X.mp_ref_kf || !X.kf_mp ||
            !X.obs_ptr_out || !X.obs_kf_out || !X.obs_idx_out || !X.obs_octave_out || !X.obs_weight_out)
            return slamit_refuse(where, "null table");
    }
    if (!R->d_n || !R->d_n_touched || !R->d_n_obs_out || !R->d_status || (R->cap && !R->d_edits) || (R->mp_cap && (!R->d_status_mp || !R->d_touched)))
        return slamit_refuse(where, "null array");
    size_t clear_bytes = 0;
    const size_t need = me_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, nullptr, nullptr, &clear_bytes);
    if (!R->d_workspace || R->workspace_bytes < need || ((uintptr_t)R->d_workspace & 7)) return slamit_refuse(where, "workspace missing, misaligned or below slamit_map_edit_workspace()");
    SLAMIT_USE_DEVICE(device);
    MeBatch B;
    memset(&B, 0, sizeof(B));
    B.n_maps = R->n_maps; B.cap = R->cap; B.mp_cap = R->mp_cap; B.kfmp_cap = R->kfmp_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.X, R->edit, sizeof(MeIndex) * (size_t)R->n_maps);
    B.edits = reinterpret_cast<const MeEdit*>(R->d_edits); B.n = R->d_n;
    B.status_mp = R->d_status_mp; B.touched = R->d_touched; B.n_touched = R->d_n_touched; B.n_obs_out = R->d_n_obs_out; B.status = R->d_status;
    me_ws_layout(R->n_maps, R->cap, R->mp_cap, R->kfmp_cap, (unsigned char*)R->d_workspace, &B, nullptr);
    HIP_TRY_AT(where, me_launch(B, clear_bytes, (hipStream_t)stream));
    return SLAMIT_OK;
}

}  // extern "C"
