// map_rows_dev.h — what the map modules that rebuild the observation table share on the device, each piece stated once (hipcc only).
// For map_edit.hip, map_replace.hip and map_fuse.hip: the three bodies of the device scan and the copy of the rows no op names.
// For the two that include map_replace.h before this file: the workspace rows over the points with their working rows (MapRows, laid out
// by MapRowsLayout), a point into its working row and back (map_row_load, map_row_commit), the host form's tables through the binder
// (map_stage_tables), and MapWorldDev, the wavefront form of the world mr_walk_op asks for.  Nothing here knows its caller: what
// differs between the modules (the gates, the bounds on a compact number, the emitters of kf_mp writes, the heads of the copy
// kernels) stays in their files.  No workgroup-wide barrier stands here: the scan bodies take theirs from wave_ops.h.
#ifndef SLAMIT_MAP_ROWS_DEV_H
#define SLAMIT_MAP_ROWS_DEV_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wave_ops.h"

// ---- the device scan: three kernels, grid.y = the map, two arrays at once (grid.z), parts rows of nparts + 1 entries -----------------
// src(z, i) -> entry i of array z of this map.  struct MapScanAt: entry i's value and what lies before it.
struct MapScanAt { int v, before; };
// grid (nparts, maps, arrays): the sum of block x of array z over the first n entries
template <int NT, class Src>
__device__ __forceinline__ void map_scan_sum(int32_t* parts, int nparts, int n, Src src) {
    const int i = blockIdx.x * NT + (int)threadIdx.x;
    int total;
    block_inclusive_scan_i32<NT>(i < n ? src((int)blockIdx.z, i) : 0, total);
    if (threadIdx.x == 0) parts[((size_t)blockIdx.y * 2 + blockIdx.z) * (nparts + 1) + blockIdx.x] = total;
}
// grid (maps, arrays): the sums scanned in place by one workgroup, the total at [nparts]
template <int NT>
__device__ __forceinline__ void map_scan_parts(int32_t* parts, int nparts) {
    block_scan_parts_i32<NT>(parts + ((size_t)blockIdx.x * 2 + blockIdx.y) * (nparts + 1), nparts);
}
// grid (nparts, maps, arrays): out[i] = what lies before entry i, out[n] = the total (out: this map's row of array z, n inside it)
template <int NT, class Src>
__device__ __forceinline__ MapScanAt map_scan_add(const int32_t* parts, int nparts, int n, Src src, int32_t* out) {
    const int i = blockIdx.x * NT + (int)threadIdx.x;
    parts += ((size_t)blockIdx.y * 2 + blockIdx.z) * (nparts + 1);
    const int v = i < n ? src((int)blockIdx.z, i) : 0;
    int total;
    const int incl = block_inclusive_scan_i32<NT>(v, total);
    const int before = parts[blockIdx.x] + incl - v;
    if (i < n) out[i] = before;
    else if (i == n) out[i] = parts[nparts];
    return {v, before};
}

// ---- the rows of the points no op names, NT / 64 wavefronts of 64 consecutive points: 2,336 bytes of LDS at NT = 256 ----------------
// The wavefront's points start at p0 (past n_mp: nothing to do) and their entries are consecutive in the old table; every lane finds its
// entry's point by bisection in LDS.  sk: this lane's point is written elsewhere.  The whole wavefront calls it.
template <int NT>
__device__ __forceinline__ void map_copy_unnamed_rows(int p0, bool sk, const int32_t* obs_ptr, const int32_t* newptr, int n_mp, const int32_t* kf, const int32_t* idx,
                                                      const uint8_t* octave, const uint8_t* weight, int32_t* kf_out, int32_t* idx_out, uint8_t* octave_out, uint8_t* weight_out) {
    __shared__ int32_t optr[NT / 64][65], nptr[NT / 64][65];
    __shared__ uint8_t skip[NT / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (p0 >= n_mp) return;
    optr[w][lane] = obs_ptr[min(p0 + lane, n_mp)]; nptr[w][lane] = newptr[min(p0 + lane, n_mp)];
    if (lane == 63) { optr[w][64] = obs_ptr[min(p0 + 64, n_mp)]; nptr[w][64] = newptr[min(p0 + 64, n_mp)]; }
    skip[w][lane] = sk;
    wave_mem_sync();
    const int e1 = optr[w][64];
    for (int e = optr[w][0] + lane; e < e1; e += 64) {
        int lo = 0, hi = 63;                                            // the row q with optr[q] <= e < optr[q + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (optr[w][mid + 1] > e) hi = mid; else lo = mid + 1;
        }
        if (skip[w][lo]) continue;
        const int at = nptr[w][lo] + (e - optr[w][lo]);                 // an unchanged row: inside the new table
        kf_out[at] = kf[e]; idx_out[at] = idx[e]; octave_out[at] = octave[e]; weight_out[at] = weight[e];
    }
}

#ifdef SLAMIT_MAP_REPLACE_H   // ---- from here on: working rows, for the files whose ops are map_replace.h's ----------------------------
#include <algorithm>
#include <vector>

#include "slamit_internal.h"

enum { MR_F_OP_BAD = 0, MR_F_OBS_BAD = 1, MR_F_OP_OVER = 2, MR_F_OBS_OVER = 3, MR_NFLAGS = 8 };
enum { MR_C_LEN = 0, MR_C_BAD, MR_C_NOBS, MR_C_FOUND, MR_C_VISIBLE, MR_C_REPLACED, MR_C_RECEIVED, MR_NCOLS };

// The workspace rows both modules keep.  The rows of a map lie S = mp_cap + 1 apart; an involved point has a compact number below
// ninv = min(2 cap, mp_cap) and a working row of MR_MAX_OBS entries.
struct MapRows {
    int32_t* flags;            // [n_maps][MR_NFLAGS]     cleared
    int32_t* cnt;              // [n_maps][S]             cleared: not 0 for an involved point
    int32_t* cidx;             // [n_maps][S]             the compact number of an involved point, their count at [n_mp]
    int32_t* newptr;           // [n_maps][S]             the new pointer array, the table's need at [n_mp]
    int32_t* tpos;             // [n_maps][S]
    int32_t* parts;            // [n_maps][2][nparts + 1]
    int32_t* inv;              // [n_maps][ninv]          the slot of a compact number
    int32_t* wcol;             // [n_maps][MR_NCOLS][ninv]
    int32_t* wkf;              // [n_maps][ninv][MR_MAX_OBS]
    int32_t* widx;
    uint8_t* woct;
    uint8_t* wwgt;
    int32_t nparts, ninv;
};

// The workspace handed out in 16-byte steps, a module's own arrays through take(), the shared ones in the four groups they stand in.
// base null: only the sizes.  off: the bytes handed out so far.
struct MapRowsLayout {
    size_t nm, S, c, nparts, ninv, off;
    unsigned char* base;
    MapRows W;
    MapRowsLayout(int n_maps, int cap, int mp_cap, unsigned char* base_)
        : nm((size_t)n_maps), S((size_t)mp_cap + 1), c((size_t)cap), nparts((S + MR_SCAN_BLOCK - 1) / MR_SCAN_BLOCK), ninv(std::min(2 * c, (size_t)mp_cap)), off(0), base(base_) {
        W.nparts = (int32_t)nparts; W.ninv = (int32_t)ninv;
    }
    template <class T>
    T* take(size_t count) {
        const size_t at = off;
        off += (sizeof(T) * count + 15) & ~(size_t)15;
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    void cleared() { W.flags = take<int32_t>(nm * MR_NFLAGS); W.cnt = take<int32_t>(nm * S); }
    void scanned() { W.cidx = take<int32_t>(nm * S); W.newptr = take<int32_t>(nm * S); W.tpos = take<int32_t>(nm * S); W.parts = take<int32_t>(nm * 2 * (nparts + 1)); }
    void columns() { W.inv = take<int32_t>(nm * ninv); W.wcol = take<int32_t>(nm * MR_NCOLS * ninv); }
    void rows() {
        const size_t n = nm * ninv * MR_MAX_OBS;
        W.wkf = take<int32_t>(n); W.widx = take<int32_t>(n); W.woct = take<uint8_t>(n); W.wwgt = take<uint8_t>(n);
    }
};

__device__ __forceinline__ int32_t* map_rows_col(const MapRows& W, int m, int col) { return W.wcol + ((size_t)m * MR_NCOLS + col) * (size_t)W.ninv; }

// Point p of map m into working row ci: its row and its five column values.  A row outside [0, MR_MAX_OBS] is noted and left empty.
// The whole wavefront calls it, p wave-uniform.
__device__ __forceinline__ void map_row_load(const MapRows& W, int m, const LmMap& M, const MrIndex& X, int ci, int p, int lane) {
    const int o0 = __builtin_amdgcn_readfirstlane(M.obs_ptr[p]);
    int len0 = __builtin_amdgcn_readfirstlane(M.obs_ptr[p + 1]) - o0;
    if (len0 > MR_MAX_OBS || len0 < 0) {
        if (lane == 0) atomicOr(&W.flags[MR_NFLAGS * m + MR_F_OBS_OVER], 1);
        len0 = 0;
    }
    const size_t r0 = ((size_t)m * W.ninv + ci) * MR_MAX_OBS;
    for (int e = lane; e < len0; e += 64) {
        W.wkf[r0 + e] = M.obs_kf[o0 + e]; W.widx[r0 + e] = X.obs_idx[o0 + e]; W.woct[r0 + e] = X.obs_octave[o0 + e]; W.wwgt[r0 + e] = X.obs_weight[o0 + e];
    }
    if (lane == 0) {
        map_rows_col(W, m, MR_C_LEN)[ci] = len0; map_rows_col(W, m, MR_C_BAD)[ci] = X.mp_bad[p]; map_rows_col(W, m, MR_C_NOBS)[ci] = X.mp_nobs[p];
        map_rows_col(W, m, MR_C_FOUND)[ci] = X.mp_found[p]; map_rows_col(W, m, MR_C_VISIBLE)[ci] = X.mp_visible[p]; map_rows_col(W, m, MR_C_REPLACED)[ci] = X.mp_replaced[p];
        map_rows_col(W, m, MR_C_RECEIVED)[ci] = 0;
    }
}
// Working row ci of map m at its point's new offset, the five columns in place.  The caller has passed its gate and bounded ci.
__device__ __forceinline__ void map_row_commit(const MapRows& W, int m, size_t S, const MrIndex& X, int ci, int lane) {
    const int p = W.inv[(size_t)m * W.ninv + ci];
    const int len = map_rows_col(W, m, MR_C_LEN)[ci], d0 = W.newptr[m * S + p];   // d0 + len <= the need <= obs_cap_out
    const size_t r0 = ((size_t)m * W.ninv + ci) * MR_MAX_OBS;
    for (int e = lane; e < len; e += 64) {
        X.obs_kf_out[d0 + e] = W.wkf[r0 + e]; X.obs_idx_out[d0 + e] = W.widx[r0 + e]; X.obs_octave_out[d0 + e] = W.woct[r0 + e]; X.obs_weight_out[d0 + e] = W.wwgt[r0 + e];
    }
    if (lane == 0) {
        X.mp_bad[p] = (uint8_t)map_rows_col(W, m, MR_C_BAD)[ci]; X.mp_nobs[p] = map_rows_col(W, m, MR_C_NOBS)[ci]; X.mp_found[p] = map_rows_col(W, m, MR_C_FOUND)[ci];
        X.mp_visible[p] = map_rows_col(W, m, MR_C_VISIBLE)[ci]; X.mp_replaced[p] = map_rows_col(W, m, MR_C_REPLACED)[ci];
    }
}

// ---- the world of mr_walk_op on the device: one wavefront, the rows in the workspace ------------------------------------------
// Emit: mine(kf, idx, value, li), this lane's kf_mp write, and one(kf, idx, value, li), the wavefront's.
struct MapWorldDev {
    const int32_t* cidx; int32_t* flags;
    int32_t* col[MR_NCOLS];
    int32_t* wkf; int32_t* widx; uint8_t* woct; uint8_t* wwgt;          // the map's working rows
    int32_t* skf; uint16_t* sord;                                       // this wavefront's LDS: S's keyframes, S's entries by rank
    int lane;
    // map m of the rows W; skf_, sord_: MR_MAX_OBS entries each of this wavefront's own
    __device__ __forceinline__ void bind(const MapRows& W, int m, size_t S, int32_t* skf_, uint16_t* sord_, int lane_) {
        const size_t r0 = (size_t)m * W.ninv * MR_MAX_OBS;
        cidx = W.cidx + m * S; flags = W.flags + MR_NFLAGS * m;
        for (int q = 0; q < MR_NCOLS; ++q) col[q] = map_rows_col(W, m, q);
        wkf = W.wkf + r0; widx = W.widx + r0; woct = W.woct + r0; wwgt = W.wwgt + r0;
        skf = skf_; sord = sord_; lane = lane_;
    }
    __device__ __forceinline__ int len_of(int ci) const { return __builtin_amdgcn_readfirstlane(col[MR_C_LEN][ci]); }
    __device__ __forceinline__ bool holds(int p, int k) const {
        const int ci = cidx[p], len = len_of(ci);
        const size_t r0 = (size_t)ci * MR_MAX_OBS;
        for (int e0 = 0; e0 < len; e0 += 64)
            if (__ballot(e0 + lane < len && wkf[r0 + e0 + lane] == k)) return true;
        return false;
    }
    __device__ __forceinline__ int push(int p, int k, int i, uint8_t o, uint8_t wt) {
        const int ci = cidx[p], len = len_of(ci);
        if (len >= MR_MAX_OBS) {
            if (lane == 0) atomicOr(&flags[MR_F_OBS_OVER], 1);
            return 0;
        }
        if (lane == 0) {
            const size_t at = (size_t)ci * MR_MAX_OBS + len;
            wkf[at] = k; widx[at] = i; woct[at] = o; wwgt[at] = wt;
            col[MR_C_LEN][ci] = len + 1; col[MR_C_NOBS][ci] += wt; col[MR_C_RECEIVED][ci] = 1;
        }
        return 1;
    }
    template <class Emit>
    __device__ __forceinline__ void fuse(int S, int D, Emit& emit, int li, int& moved, int& erased) {
        const int cs = cidx[S], cd = cidx[D], len_s = len_of(cs), len_d = len_of(cd);
        const size_t rs = (size_t)cs * MR_MAX_OBS, rd = (size_t)cd * MR_MAX_OBS;
        wave_mem_sync();                                                 // the LDS of the op before
        for (int e = lane; e < len_s; e += 64) skf[e] = wkf[rs + e];
        wave_mem_sync();
        for (int e = lane; e < len_s; e += 64) {                        // ascending slot, row order among equals
            const uint32_t key = (uint32_t)skf[e];
            int rank = 0;
            for (int f = 0; f < len_s; ++f) { const uint32_t o = (uint32_t)skf[f]; rank += (o < key) || (o == key && f < e); }
            sord[rank] = (uint16_t)e;
        }
        wave_mem_sync();
        int n_moved = 0, add = 0, over = 0;
        for (int j0 = 0; j0 < len_s; j0 += 64) {
            const int j = j0 + lane;
            const bool act = j < len_s;
            const int e = act ? sord[j] : 0, k = act ? skf[e] : 0;
            bool go = act && (j == 0 || skf[sord[j - 1]] != k);         // the first of a run of one keyframe decides
            if (go)
                for (int f = 0; f < len_d; ++f) go = go && wkf[rd + f] != k;     // D's row as the op met it: the received keyframes are S's own
            const int i = act ? widx[rs + e] : 0, wt = act ? wwgt[rs + e] : 0;
            const unsigned long long mask = __ballot(go);
            if (go) {
                const int at = len_d + n_moved + __popcll(mask & ((1ull << lane) - 1ull));
                if (at >= MR_MAX_OBS) over = 1;
                else { wkf[rd + at] = k; widx[rd + at] = i; woct[rd + at] = woct[rs + e]; wwgt[rd + at] = (uint8_t)wt; }
            }
            if (act) emit.mine(k, i, go ? D : -1, li);
            add += __builtin_amdgcn_readlane(wave_inclusive_scan_i32(go ? wt : 0), 63);
            n_moved += __popcll(mask);
        }
        if (__ballot(over != 0)) {
            if (lane == 0) atomicOr(&flags[MR_F_OBS_OVER], 1);
            n_moved = MR_MAX_OBS - len_d;
        }
        if (lane == 0 && n_moved > 0) { col[MR_C_LEN][cd] = len_d + n_moved; col[MR_C_NOBS][cd] += add; col[MR_C_RECEIVED][cd] = 1; }
        moved = n_moved; erased = len_s - n_moved;
    }
    __device__ __forceinline__ void retire(int S, int D) {
        if (lane != 0) return;
        const int cs = cidx[S], cd = cidx[D];
        col[MR_C_LEN][cs] = 0; col[MR_C_BAD][cs] = 1; col[MR_C_REPLACED][cs] = D;
        col[MR_C_FOUND][cd] = (int32_t)((uint32_t)col[MR_C_FOUND][cd] + (uint32_t)col[MR_C_FOUND][cs]);
        col[MR_C_VISIBLE][cd] = (int32_t)((uint32_t)col[MR_C_VISIBLE][cd] + (uint32_t)col[MR_C_VISIBLE][cs]);
    }
};

// ---- the host form's tables through the binder (both *_apply, inside describe): the tables and the read-only columns staged down,
// the in-place columns and the new table both ways.  map and X have passed map_replace_tables_error.
static void map_stage_tables(StageBinder& b, std::vector<SlamitInOut>& io, const slamit_map_index* map, const slamit_replace_index* X, LmMap& M, MrIndex& E) {
    const size_t n_kf = (size_t)map->n_kf, n_mp = (size_t)map->n_mp;
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf], cap_out = (size_t)X->obs_cap_out;
    M.n_kf = map->n_kf; M.n_mp = map->n_mp;
    M.obs_ptr = b.in(map->obs_ptr, n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs); M.kf_mp_ptr = b.in(map->kf_mp_ptr, n_kf + 1);
    E.obs_idx = b.in(X->obs_idx, n_obs); E.obs_octave = b.in(X->obs_octave, n_obs); E.obs_weight = b.in(X->obs_weight, n_obs);
    E.mp_bad = slamit_inout(b, io, X->mp_bad, n_mp); E.mp_nobs = slamit_inout(b, io, X->mp_nobs, n_mp);
    E.mp_found = slamit_inout(b, io, X->mp_found, n_mp); E.mp_visible = slamit_inout(b, io, X->mp_visible, n_mp);
    E.mp_replaced = slamit_inout(b, io, X->mp_replaced, n_mp); E.kf_mp = slamit_inout(b, io, X->kf_mp, n_kfmp);
    E.obs_ptr_out = slamit_inout(b, io, X->obs_ptr_out, n_mp + 1);
    E.obs_kf_out = slamit_inout(b, io, X->obs_kf_out, cap_out); E.obs_idx_out = slamit_inout(b, io, X->obs_idx_out, cap_out);
    E.obs_octave_out = slamit_inout(b, io, X->obs_octave_out, cap_out); E.obs_weight_out = slamit_inout(b, io, X->obs_weight_out, cap_out);
    E.obs_cap_out = X->obs_cap_out;
}
#endif   // SLAMIT_MAP_REPLACE_H

#endif
