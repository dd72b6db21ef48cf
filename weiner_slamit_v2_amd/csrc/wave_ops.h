// wave_ops.h — what the kernels do across the 64 lanes of a wavefront: DPP exchanges, v_readlane broadcasts, the reductions and the
// scan built from them, the workgroup scan on top of the wave scan, and the two idioms of the matchers (256-bit Hamming distance, two
// smallest keys).
//
// Why DPP: __shfl_xor / __shfl_up compile to ds_bpermute, an LDS round trip per step, six dependent steps per reduction (twelve for a
// 64-bit value).  In the serial loops that reduce -- one query, one vocabulary node, one Levenberg sum after the other -- those round
// trips WERE the loop time (the whole microsecond the guided search spent per query; 27-35 sums per optimiser iteration).  A DPP operand
// reads another lane of the 16-lane row for free, so every reduction here is four exchanges that leave each row uniform (xor 1, xor 2,
// half-row mirror, row mirror), then four v_readlane (lanes 0 / 16 / 32 / 48) joined on the scalar side: a wave-uniform result.
#ifndef SLAMIT_WAVE_OPS_H
#define SLAMIT_WAVE_OPS_H
#include <hip/hip_runtime.h>

// ---- exchanges and broadcasts ---------------------------------------------------------------------------------------------------
// lane's partner under DPP control CTRL (0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror);
// a lane without a source reads 0.  64-bit values are two 32-bit exchanges.
template <int CTRL>
__device__ __forceinline__ int dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// quad_perm exchange in which every lane has a source (CTRL < 0x100): no zero-initialised "old" operand to set up
template <int CTRL>
__device__ __forceinline__ double dpp_quad_d(double v) {
    const int l = __double2loint(v), h = __double2hiint(v);
    const int lo = __builtin_amdgcn_update_dpp(l, l, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(h, h, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// value of lane `l` (compile-time constant or wave-uniform) as a wave-uniform scalar: v_readlane_b32 x2, no LDS
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
// the same for a lane index the compiler cannot prove uniform
__device__ __forceinline__ double readlane_dyn_d(double v, int l) {
    const int ls = __builtin_amdgcn_readfirstlane(l);
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), ls);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), ls);
    return __hiloint2double(hi, lo);
}

// ---- reductions over the 64 lanes, the same value in every lane -----------------------------------------------------------------
__device__ __forceinline__ double row16_sum(double v) {   // all 16 lanes of a DPP row end up with the row's sum
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {   // in a fixed order, part of the numerics: BA, pose and Sim3 depend on it bit for bit
    v = row16_sum(v);
    return ((readlane_d(v, 0) + readlane_d(v, 16)) + readlane_d(v, 32)) + readlane_d(v, 48);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = min(v, dpp<0xB1>(v));
    v = min(v, dpp<0x4E>(v));
    v = min(v, dpp<0x141>(v));
    v = min(v, dpp<0x140>(v));
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    unsigned long long o;
    o = dpp<0xB1>(v); v = o < v ? o : v;
    o = dpp<0x4E>(v); v = o < v ? o : v;
    o = dpp<0x141>(v); v = o < v ? o : v;
    o = dpp<0x140>(v); v = o < v ? o : v;
    const unsigned long long a = readlane_u64(v, 0), b = readlane_u64(v, 16), c = readlane_u64(v, 32), d = readlane_u64(v, 48);
    const unsigned long long ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// minimum over a lane group of 16 (one DPP row) or 32 (two rows), the same value in every lane of the group; groups are independent,
// so a wavefront reduces four (two) of them at once.  The step between the two rows of a 32-group is a ds_swizzle (xor 16), which
// goes through the LDS crossbar without touching LDS memory.  Every lane of a group must be active.
__device__ __forceinline__ unsigned long long row16_min_u64(unsigned long long v) {
    unsigned long long o;
    o = dpp<0xB1>(v); v = o < v ? o : v;
    o = dpp<0x4E>(v); v = o < v ? o : v;
    o = dpp<0x141>(v); v = o < v ? o : v;
    o = dpp<0x140>(v); v = o < v ? o : v;
    return v;
}
template <int G>
__device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v) {
    static_assert(G == 16 || G == 32, "lane groups are one or two DPP rows");
    v = row16_min_u64(v);
    if (G == 32) {
        const int lo = __builtin_amdgcn_ds_swizzle((int)(unsigned)v, 0x401F);           // and 0x1F, or 0, xor 0x10
        const int hi = __builtin_amdgcn_ds_swizzle((int)(unsigned)(v >> 32), 0x401F);
        const unsigned long long o = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
        v = o < v ? o : v;
    }
    return v;
}

// inclusive prefix sum over the wavefront: four DPP row shifts scan each 16-lane row, two row broadcasts carry the row totals on
// (lane 15 -> rows 1 and 3, lane 31 -> rows 2 and 3); shifted-out and masked-off lanes contribute the 0 of `old`.  Lane 63 holds the total.
__device__ __forceinline__ int wave_inclusive_scan_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2, 3
    return v;
}

// memory (LDS or global) written by some lanes of the wavefront, read by others
__device__ __forceinline__ void wave_mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- the workgroup on top of the wave scan --------------------------------------------------------------------------------------
// inclusive scan over the NT threads of the workgroup; total = the workgroup's sum.  Every thread calls it.
template <int NT>
__device__ __forceinline__ int block_inclusive_scan_i32(int v, int& total) {
    __shared__ int wave_total[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int incl = wave_inclusive_scan_i32(v);
    if (lane == 63) wave_total[w] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
    for (int u = 0; u < NT / 64; ++u) { const int t = wave_total[u]; off += u < w ? t : 0; total += t; }
    __syncthreads();
    return off + incl;
}
// parts[nparts] scanned in place by one workgroup of NT threads (exclusive), the total at parts[nparts]
template <int NT>
__device__ __forceinline__ void block_scan_parts_i32(int32_t* parts, int nparts) {
    int base = 0;
    for (int c0 = 0; c0 < nparts; c0 += NT) {   // every thread walks the same rounds
        const int t = c0 + (int)threadIdx.x;
        const int v = t < nparts ? parts[t] : 0;
        int total;
        const int incl = block_inclusive_scan_i32<NT>(v, total);
        if (t < nparts) parts[t] = base + incl - v;
        base += total;
    }
    if (threadIdx.x == 0) parts[nparts] = base;
}

// ---- matcher idioms -------------------------------------------------------------------------------------------------------------
// Hamming distance of two 256-bit ORB descriptors held as uint4 halves
__device__ __forceinline__ int hamming256(uint4 a0, uint4 a1, uint4 t0, uint4 t1) {
    return __popc(a0.x ^ t0.x) + __popc(a0.y ^ t0.y) + __popc(a0.z ^ t0.z) + __popc(a0.w ^ t0.w) +
           __popc(a1.x ^ t1.x) + __popc(a1.y ^ t1.y) + __popc(a1.z ^ t1.z) + __popc(a1.w ^ t1.w);
}
// (k1, k2) = this lane's two smallest keys so far; keys are unique, ~0 = none
__device__ __forceinline__ void keep2(unsigned long long& k1, unsigned long long& k2, unsigned long long k) {
    // (selects on the values: as an if / else on the two references the stores merge into one through a selected address,
    //  and the pair then lives in scratch memory)
    const bool first = k < k1;
    k2 = first ? k1 : (k < k2 ? k : k2);
    k1 = first ? k : k1;
}
// the two smallest keys of the wavefront from every lane's pair: one lane holds the best, its runner-up competes for second
__device__ __forceinline__ void wave_min2(unsigned long long k1, unsigned long long k2, unsigned long long& best, unsigned long long& second) {
    best = wave_min_u64(k1);
    second = wave_min_u64(k1 == best ? k2 : k1);
}

#endif
