// hamming.hip — 256-bit Hamming matching (include/slamit.h, slamit_hamming_*).
//
// Replaces ORBmatcher::DescriptorDistance (ORB_SLAM2/src/ORBmatcher.cc:1651-1667) and the
// best / second-best selection loops that call it (:85-117, :440-461, :1404-1428):
//     if (d < best) { second = best; best = d; idx = j; } else if (d < second) second = d;
// i.e. best = minimum distance with the FIRST index on ties, second = second smallest value of
// the multiset.  That pair is an associative reduction, so the train set is split over 4 lanes
// per query and merged with cross-lane shuffles:
//     merge((b1,i1,s1),(b2,i2,s2)) = (b1,i1,min(s1,b2)) if (b1,i1) < (b2,i2) else (b2,i2,min(s2,b1)).
// Workgroup = 256 threads = 64 queries x 4 train slices; train descriptors stream through LDS in
// tiles of 256 rows (8 KB), read as broadcast ds_read_b128; distance = 8 x (v_xor + v_bcnt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"
#include "distinctive.h"

#define HM_TILE 256      // train rows per LDS tile: two uint4 per thread
#ifndef HM_SLICES
#define HM_SLICES 8     // lanes per query: each takes every HM_SLICES-th train row of a tile
#endif
#define HM_QPB (256 / HM_SLICES)   // queries per workgroup

// popcount(x) + acc in ONE instruction; left to itself the compiler builds a tree of 8 v_bcnt + 3 v_add3 per distance
__device__ __forceinline__ unsigned bcnt_acc(unsigned x, unsigned acc) {
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {   // v_med3_u32 (no builtin for the unsigned form)
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__global__ __launch_bounds__(256) void hamming_best2_kernel(
    const uint8_t* __restrict__ q, const int* __restrict__ nq_arr, int nq_fixed, size_t q_stride,
    const uint8_t* __restrict__ t, const int* __restrict__ nt_arr, int nt_fixed, size_t t_stride,
    int* __restrict__ best_idx, int* __restrict__ best, int* __restrict__ second, size_t out_stride) {
    __shared__ uint4 tile[HM_TILE * 2];
    const int pair = blockIdx.y;
    const int nq = nq_arr ? nq_arr[pair] : nq_fixed;
    const int nt = nt_arr ? nt_arr[pair] : nt_fixed;
    const int tid = threadIdx.x;
    const int qi = blockIdx.x * HM_QPB + tid / HM_SLICES;
    const int slice = tid % HM_SLICES;
    if (blockIdx.x * HM_QPB >= nq) return;  // uniform
    const uint4* Q = reinterpret_cast<const uint4*>(q + (size_t)pair * q_stride);
    const uint4* T = reinterpret_cast<const uint4*>(t + (size_t)pair * t_stride);
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    const bool live = qi < nq;
    if (live) { a0 = Q[2 * (size_t)qi]; a1 = Q[2 * (size_t)qi + 1]; }
    // (best, second) are the two smallest keys (distance << 16 | train index): strict '<' with the first index
    // winning ties is exactly the order of these keys, and a median / min pair updates both without a branch
    unsigned kb = 0xFFFFFFFFu, ks = 0xFFFFFFFFu;
    // the next tile of train descriptors travels HBM -> registers while the current one is being scanned
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // (Two named registers, not an array: the compiler moves a small array to LDS and then waits for the load at once.
    // Indices are clamped, not predicated: a select between a load and zero turns into a FLAT load, which also counts
    // in lgkmcnt and would make every LDS wait of the scan wait for the prefetch.  Rows >= nt of a tile are never read.)
    uint4 p0 = zero, p1 = zero;
    if (nt > 0) {
        const int last = 2 * min(nt, HM_TILE) - 1;
        p0 = T[min(tid, last)]; p1 = T[min(tid + 256, last)];
    }
    for (int base = 0; base < nt; base += HM_TILE) {
        const int rows = min(HM_TILE, nt - base);
        __syncthreads();
        tile[tid] = p0; tile[tid + 256] = p1;
        __syncthreads();
        if (base + HM_TILE < nt) {
            const int last = 2 * min(HM_TILE, nt - base - HM_TILE) - 1;
            const uint4* Tn = T + 2 * (size_t)(base + HM_TILE);
            p0 = Tn[min(tid, last)]; p1 = Tn[min(tid + 256, last)];
        }
#define HM_DIST(T0, T1) bcnt_acc(a1.w ^ T1.w, bcnt_acc(a1.z ^ T1.z, bcnt_acc(a1.y ^ T1.y, bcnt_acc(a1.x ^ T1.x, \
                        bcnt_acc(a0.w ^ T0.w, bcnt_acc(a0.z ^ T0.z, bcnt_acc(a0.y ^ T0.y, bcnt_acc(a0.x ^ T0.x, 0u))))))))
#define HM_TAKE(D, J) do { const unsigned k = ((D) << 16) | (unsigned)(base + (J)); \
            ks = umed3(kb, ks, k);   /* kb <= ks: the median of the three is the new second smallest */ \
            kb = min(kb, k); } while (0)
        int j = slice;
        // four rows per trip, their eight LDS reads issued before the first popcount (unrolled by hand: the asm in umed3
        // stops the unroller)
        for (; j + 3 * HM_SLICES < rows; j += 4 * HM_SLICES) {
            const uint4 t00 = tile[2 * j], t01 = tile[2 * j + 1], t10 = tile[2 * (j + HM_SLICES)], t11 = tile[2 * (j + HM_SLICES) + 1];
            const uint4 t20 = tile[2 * (j + 2 * HM_SLICES)], t21 = tile[2 * (j + 2 * HM_SLICES) + 1];
            const uint4 t30 = tile[2 * (j + 3 * HM_SLICES)], t31 = tile[2 * (j + 3 * HM_SLICES) + 1];
            const unsigned d0 = HM_DIST(t00, t01), d1 = HM_DIST(t10, t11), d2 = HM_DIST(t20, t21), d3 = HM_DIST(t30, t31);
            HM_TAKE(d0, j); HM_TAKE(d1, j + HM_SLICES); HM_TAKE(d2, j + 2 * HM_SLICES); HM_TAKE(d3, j + 3 * HM_SLICES);
        }
        for (; j < rows; j += HM_SLICES) { const uint4 t0 = tile[2 * j], t1 = tile[2 * j + 1]; const unsigned d = HM_DIST(t0, t1); HM_TAKE(d, j); }
#undef HM_DIST
#undef HM_TAKE
    }
    // merge the slices of each query (adjacent lanes): two smallest of the union
#pragma unroll
    for (int m = 1; m < HM_SLICES; m <<= 1) {
        const unsigned ob = (unsigned)__shfl_xor((int)kb, m, 64), os = (unsigned)__shfl_xor((int)ks, m, 64);
        ks = min(min(ks, os), max(kb, ob));
        kb = min(kb, ob);
    }
    const int b = kb == 0xFFFFFFFFu ? 256 : (int)(kb >> 16), bi = kb == 0xFFFFFFFFu ? -1 : (int)(kb & 0xFFFFu);
    const int s = ks == 0xFFFFFFFFu ? 256 : (int)(ks >> 16);
    if (live && slice == 0) {
        size_t o = (size_t)pair * out_stride + qi;
        best_idx[o] = bi; best[o] = b; second[o] = s;
    }
}

// ---- the same reduction on the matrix cores -------------------------------------------------------------------
// 256-bit Hamming distance as a block-scaled FP4 dot product: a descriptor bit becomes the e2m1 nibble 0x2 (+1.0) or 0xA
// (-1.0) (query: 1 -> -1, train: 1 -> +1) and each operand carries the constant block scale 2^6 (e8m0 byte 133), so a
// product is -4096 where the bits agree and +4096 where they differ and the sum over the 256 positions is
// 4096 * (2 d - 256) = 8192 d - 2^20.  The 13 low bits of that sum are zero, so the train index j (< 8192) rides in the
// accumulator's initial value: v_mfma_scale_f32_32x32x64_f8f6f4 leaves  8192 d - 2^20 + j  = the (distance, first index)
// key itself (plus HMM_BIAS = 2^21, which keeps it positive).  Every term and every partial sum is an integer below 2^22,
// inside f32's 24-bit significand, so the f32 accumulator holds that key exactly in whatever order the hardware adds; the epilogue per
// distance is a v_min_i32 and a v_med3_f32 (2 VALU ops instead of the 19 of the xor / popcount kernel) and the keys turn
// into integers once, in the final write-out.  Unpacking costs one shift + one v_bitop3 per EIGHT positions:
//     nibbles = ((w << (3 - s)) & 0x88888888) | 0x22222222            (query; train uses ~w)
// Position order inside the K = 256 axis is whatever (lane half, shift class s, dword) gives -- the same for both operands.
// A = train tile (32 rows), B = queries (32 columns): a lane's 16 accumulators are 16 train rows of ONE query, so the
// running (best, second) keys are two registers per lane and query tile.
typedef int hm_v8i __attribute__((ext_vector_type(8)));
typedef float hm_v16f __attribute__((ext_vector_type(16)));
#define HMM_MAX_TRAIN 8192
// Sentinels are powers of two: a sum of +-4096 products on top of one, and the +-32 HMM_WAVES rebasing of the running
// keys, stay multiples of its ulp (128 at most), so nothing is ever rounded and none can come near the 2^29 test below.
#define HMM_NONE 0x1p30f             // accumulator start of a train row >= nt: its key stays above every real one
#define HMM_EMPTY 0x1p30f            // "no key yet"
#define HMM_BIAS 0x1p21f             // added to every key through the accumulator start: real keys lie in (2^20 - 2^13, 2^22)
#define HMM_LIVE 0x1p29f             // ... and anything that started from a sentinel is above this
#define HMM_FP4 4                    // cbsz / blgp: both operands are e2m1, four VGPRs each
#define HMM_SCALE 133                // e8m0 block scale 2^6 of both operands (byte 0 of the scale register)

__device__ __forceinline__ hm_v8i hm_unpack_q(const uint4 w, const int s) {   // bit 1 -> 0xA (-1.0), bit 0 -> 0x2 (+1.0)
    const unsigned sign = 0x88888888u, one = 0x22222222u;
    hm_v8i r = {};                                                             // (FP4 operands: the upper four dwords are not read)
    r[0] = (int)__builtin_amdgcn_bitop3_b32(w.x << (3 - s), sign, one, 0xEA);
    r[1] = (int)__builtin_amdgcn_bitop3_b32(w.y << (3 - s), sign, one, 0xEA);
    r[2] = (int)__builtin_amdgcn_bitop3_b32(w.z << (3 - s), sign, one, 0xEA);
    r[3] = (int)__builtin_amdgcn_bitop3_b32(w.w << (3 - s), sign, one, 0xEA);
    return r;
}
__device__ __forceinline__ hm_v8i hm_unpack_t(const uint4 w, const int s) {   // bit 1 -> 0x2 (+1.0), bit 0 -> 0xA (-1.0)
    const unsigned sign = 0x88888888u, one = 0x22222222u;
    hm_v8i r = {};
    r[0] = (int)__builtin_amdgcn_bitop3_b32(w.x << (3 - s), sign, one, 0xAE);
    r[1] = (int)__builtin_amdgcn_bitop3_b32(w.y << (3 - s), sign, one, 0xAE);
    r[2] = (int)__builtin_amdgcn_bitop3_b32(w.z << (3 - s), sign, one, 0xAE);
    r[3] = (int)__builtin_amdgcn_bitop3_b32(w.w << (3 - s), sign, one, 0xAE);
    return r;
}
__device__ __forceinline__ hm_v16f hm_mfma(const hm_v8i a, const hm_v8i b, const hm_v16f c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, HMM_FP4, HMM_FP4, 0, HMM_SCALE, 0, HMM_SCALE);
}

// The kernel is bound by the matrix pipe and by vector-instruction ISSUE, which add up (the two waves of a SIMD run in
// step; staggering them or interleaving epilogue and MFMAs inside a wave changed nothing on the int8 form of this kernel).
// Per HMM_NG = 4 query tiles (128 queries) x 32 train rows a wave issues 16 MFMAs + 128 epilogue instructions + the train
// tile's unpacking (28) and the keys' rebasing (8), both shared by all the query tiles of the wave.  Measured
// (tools/diag/ubench/mfma_fp4_rate.hip, beside mfma_i8_rate.hip in the same run): the FP4 MFMA issues every 16.0-16.8 ns
// per SIMD, one or two waves, dependent or not -- the time of v_mfma_i32_32x32x32_i8 (15.7-16.0 ns) at twice its K, so
// 0.26 us per group where the int8 form took 0.51; a 64-key epilogue (add + v_med3_f32 + v_min_i32 per key) takes 305 ns
// per SIMD, 1.6 ns per instruction, and unpacking the operand between the MFMAs costs them 2-4 %.
// A wave carries HMM_NT query tiles, their unpacked queries held in 16 VGPRs each, and runs them against a train tile
// in groups of HMM_NG (64 VGPRs of accumulators) -> 2 waves per SIMD.
// Workgroup = 4 wavefronts = 4 train slices (a slice takes every 4th train tile) of the same queries, one wave per
// SIMD; they merge through LDS at the end.
#define HMM_WAVES 4                   // train slices = wavefronts per workgroup
#ifndef HMM_NT
#define HMM_NT 4                      // query tiles (32 queries each) per wavefront.  8 (256 VGPRs, no scratch) shares the train unpack
#endif                                // between twice the queries: 40.8 -> 40.4 us per 256 pairs of 1000 x 1000, 35.1 -> 33.0 us per 64 of
                                      // 2000 x 2000, but the single-pair call (4 workgroups instead of 8) 0.038 -> 0.0415 ms: not kept
#define HMM_NG 4                      // query tiles per group of accumulators

// Keys are positive floats (HMM_BIAS), which order like their bit patterns: the running minimum is a bare v_min_i32.
// (fminf on an MFMA result first quiets a possible signalling NaN, a v_max_f32 x, x: a third instruction per distance.)
__device__ __forceinline__ float hm_min(float a, float b) { return __int_as_float(min(__float_as_int(a), __float_as_int(b))); }
__device__ __forceinline__ float hm_max(float a, float b) { return __int_as_float(max(__float_as_int(a), __float_as_int(b))); }

__device__ __forceinline__ void hm_merge2(float& kb, float& ks, float ob, float os) {   // two smallest of the union of two (best, second) pairs
    ks = hm_min(hm_min(ks, os), hm_max(kb, ob));
    kb = hm_min(kb, ob);
}

__global__ __launch_bounds__(64 * HMM_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void hamming_best2_mfma_kernel(
    const uint8_t* __restrict__ q, const int* __restrict__ nq_arr, int nq_fixed, size_t q_stride,
    const uint8_t* __restrict__ t, const int* __restrict__ nt_arr, int nt_fixed, size_t t_stride,
    int* __restrict__ best_idx, int* __restrict__ best, int* __restrict__ second, size_t out_stride) {
    __shared__ float s_keys[HMM_WAVES - 1][64][2 * HMM_NT];     // slices 1..: (kb, ks) per query tile and lane
    const int pair = blockIdx.y;
    const int nq = __builtin_amdgcn_readfirstlane(nq_arr ? nq_arr[pair] : nq_fixed);
    const int nt = __builtin_amdgcn_readfirstlane(min(nt_arr ? nt_arr[pair] : nt_fixed, HMM_MAX_TRAIN));
    const int qbase = blockIdx.x * 32 * HMM_NT;
    if (qbase >= nq) return;  // uniform over the workgroup
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int col = lane & 31, h = lane >> 5;
    const uint4* Q = reinterpret_cast<const uint4*>(q + (size_t)pair * q_stride);
    const uint4* T = reinterpret_cast<const uint4*>(t + (size_t)pair * t_stride);
    // this lane's half (dwords 4h .. 4h+3) of its queries, unpacked once: 4 k-steps x 4 VGPRs per query tile
    hm_v8i bq[HMM_NT][4];
#pragma unroll
    for (int u = 0; u < HMM_NT; ++u) {
        const uint4 w = Q[2 * (size_t)min(qbase + 32 * u + col, nq - 1) + h];
#pragma unroll
        for (int s = 0; s < 4; ++s) bq[u][s] = hm_unpack_q(w, s);
    }
    // Accumulator start = row of (register r, lane half h) inside the tile: (r & 3) + 8 (r >> 2) + 4 h -- the same 16
    // registers for every tile.  The running keys are kept RELATIVE to the current tile's first row (stepping to the next
    // tile subtracts the stride from them) and the last tile's base is added back at the end.
    hm_v16f cinit;
#pragma unroll
    for (int r = 0; r < 16; ++r) cinit[r] = HMM_BIAS + (float)(4 * h + (r & 3) + 8 * (r >> 2));
    float kb[HMM_NT], ks[HMM_NT];
#pragma unroll
    for (int u = 0; u < HMM_NT; ++u) kb[u] = ks[u] = HMM_EMPTY;
    const int ntiles = (nt + 31) >> 5;
    uint4 wt = make_uint4(0u, 0u, 0u, 0u);
    if (wv < ntiles) wt = T[2 * (size_t)min(wv * 32 + col, nt - 1) + h];
    int tile = wv;
    for (; tile < ntiles; tile += HMM_WAVES) {
        const uint4 w = wt;
        if (tile + HMM_WAVES < ntiles) wt = T[2 * (size_t)min((tile + HMM_WAVES) * 32 + col, nt - 1) + h];   // travels during this tile
        hm_v8i a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = hm_unpack_t(w, s);
        if (tile * 32 + 32 > nt) {   // the set's last, partial tile (no tile follows it): rows >= nt start above every real key
#pragma unroll
            for (int r = 0; r < 16; ++r) cinit[r] = tile * 32 + 4 * h + (r & 3) + 8 * (r >> 2) < nt ? cinit[r] : HMM_NONE;
        }
        if (tile != wv) {
#pragma unroll
            for (int u = 0; u < HMM_NT; ++u) { kb[u] -= 32 * HMM_WAVES; ks[u] -= 32 * HMM_WAVES; }
        }
#pragma unroll
        for (int g = 0; g < HMM_NT; g += HMM_NG) {
            hm_v16f c[HMM_NG];
#pragma unroll
            for (int u = 0; u < HMM_NG; ++u) c[u] = hm_mfma(a[0], bq[g + u][0], cinit);
#pragma unroll
            for (int s = 1; s < 4; ++s) {
#pragma unroll
                for (int u = 0; u < HMM_NG; ++u) c[u] = hm_mfma(a[s], bq[g + u][s], c[u]);
            }
#pragma unroll
            for (int u = 0; u < HMM_NG; ++u) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float k = c[u][r];
                    ks[g + u] = __builtin_amdgcn_fmed3f(kb[g + u], ks[g + u], k);   // kb <= ks: the median of the three is the new second smallest
                    kb[g + u] = hm_min(kb[g + u], k);
                }
            }
        }
    }
    if (tile != wv) {   // this wave saw at least one tile: back to absolute train indices (base of its last tile)
        const float base = (float)((tile - HMM_WAVES) * 32);
#pragma unroll
        for (int u = 0; u < HMM_NT; ++u) { kb[u] += base; ks[u] += base; }
    }
    // the two lane halves hold different train rows of the same query
#pragma unroll
    for (int u = 0; u < HMM_NT; ++u) hm_merge2(kb[u], ks[u], __shfl_xor(kb[u], 32, 64), __shfl_xor(ks[u], 32, 64));
    if (wv > 0) {
#pragma unroll
        for (int u = 0; u < HMM_NT; ++u) { s_keys[wv - 1][lane][2 * u] = kb[u]; s_keys[wv - 1][lane][2 * u + 1] = ks[u]; }
    }
    __syncthreads();
    if (wv != 0 || h != 0) return;
#pragma unroll
    for (int o = 0; o < HMM_WAVES - 1; ++o) {
#pragma unroll
        for (int u = 0; u < HMM_NT; ++u) hm_merge2(kb[u], ks[u], s_keys[o][lane][2 * u], s_keys[o][lane][2 * u + 1]);
    }
    // key = HMM_BIAS + 8192 d - 2^20 + j, an integer held exactly; anything from HMM_NONE / the empty start is far above 2^29
#pragma unroll
    for (int u = 0; u < HMM_NT; ++u) {
        const int qi = qbase + 32 * u + col;
        if (qi >= nq) continue;
        const bool hb = kb[u] < HMM_LIVE, hs = ks[u] < HMM_LIVE;
        const int ib = (int)kb[u] - (1 << 20), is = (int)ks[u] - (1 << 20);   // - HMM_BIAS + 2^20
        const size_t o = (size_t)pair * out_stride + qi;
        best_idx[o] = hb ? (ib & 8191) : -1;
        best[o] = hb ? (ib >> 13) : 256;
        second[o] = hs ? (is >> 13) : 256;
    }
}

__global__ __launch_bounds__(256) void hamming_matrix_kernel(const uint8_t* __restrict__ q, int nq,
                                                             const uint8_t* __restrict__ t, int nt,
                                                             uint16_t* __restrict__ out) {
    __shared__ uint4 tile[64 * 2];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    const uint4* Q = reinterpret_cast<const uint4*>(q);
    const uint4* T = reinterpret_cast<const uint4*>(t);
    const int rows = min(64, nt - j0);
    for (int i = tid; i < rows * 2; i += 256) tile[i] = T[2 * (size_t)j0 + i];
    __syncthreads();
    const int j = tid & 63;
    for (int ii = tid >> 6; ii < 64; ii += 4) {
        int i = i0 + ii;
        if (i >= nq || j >= rows) continue;
        uint4 a0 = Q[2 * (size_t)i], a1 = Q[2 * (size_t)i + 1];
        uint4 t0 = tile[2 * j], t1 = tile[2 * j + 1];
        int d = hamming256(a0, a1, t0, t1);
        out[(size_t)i * nt + j0 + j] = (uint16_t)d;
    }
}

// MapPoint::ComputeDistinctiveDescriptors: one wavefront per map point.  Descriptors and the N x N
// distance matrix (u16) sit in LDS; each lane owns rows lane, lane+64 and finds its row's median by
// bisection on the value range [0, 256] (count of entries <= mid), then the wave takes the
// lexicographic minimum of (median, row) so the first least-median row wins like the reference's loop.
__global__ __launch_bounds__(64) void distinctive_kernel(const uint8_t* __restrict__ desc, const int* __restrict__ offsets,
                                                         int* __restrict__ best_idx, int* __restrict__ best_median) {
    __shared__ uint4 rowsd[SLAMIT_DISTINCTIVE_MAX * 2];
    __shared__ unsigned short D[SLAMIT_DISTINCTIVE_MAX * SLAMIT_DISTINCTIVE_MAX];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int o = offsets[p], n = offsets[p + 1] - o;
    if (n <= 0) { if (lane == 0) { best_idx[p] = -1; best_median[p] = 0; } return; }
    const uint4* G = reinterpret_cast<const uint4*>(desc + (size_t)o * 32);
    for (int i = lane; i < 2 * n; i += 64) rowsd[i] = G[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    DISTINCTIVE_SELECT(rowsd, D, n, lane, bestkey)   // distinctive.h: the distances, each row's median, the first least one
    if (lane == 0) { best_idx[p] = (int)(bestkey & 0xFFFF); best_median[p] = (int)(bestkey >> 16); }
}

// the matrix-core kernel carries the train index in 13 bits; larger train sets take the xor / popcount kernel.  Both give
// the same (index, best, second).
static bool hm_use_mfma(int max_train) { return max_train <= HMM_MAX_TRAIN; }

extern "C" {

int slamit_distinctive_batch(const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx,
                             int32_t* best_median) {
    if (npoints < 0 || (npoints && (!offsets || !best_idx || !best_median))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_distinctive_batch: bad argument");
    if (npoints == 0) return SLAMIT_OK;
    for (int p = 0; p < npoints; ++p) {
        const int n = offsets[p + 1] - offsets[p];
        if (n < 0 || offsets[0] < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_distinctive_batch: offsets must be non-decreasing");
        if (n > SLAMIT_DISTINCTIVE_MAX) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_distinctive_batch: more than SLAMIT_DISTINCTIVE_MAX rows for one point");
    }
    const int total = offsets[npoints];
    if (total && !desc) return slamit_fail(SLAMIT_ERR_ARG, "slamit_distinctive_batch: null descriptors");
    const int cur_dev = slamit_default_device();   // slamit_set_device() of this thread, else the current device
    SLAMIT_USE_DEVICE(cur_dev);
    StageLayout L;
    const StageSpan<uint8_t> d = L.take<uint8_t>(32 * (size_t)total);
    const StageSpan<int> off = L.take<int>((size_t)npoints + 1);
    L.end_inputs();
    const StageSpan<int> idx = L.take<int>(npoints), med = L.take<int>(npoints, alignof(int));
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_distinctive_batch", slamit_stage_reserve(S, cur_dev, L));
    if (total) memcpy(d.at(S.host), desc, d.bytes());
    memcpy(off.at(S.host), offsets, off.bytes());
    HIP_TRY_AT("slamit_distinctive_batch", slamit_stage_upload(S, L));
    hipLaunchKernelGGL(distinctive_kernel, dim3(npoints), dim3(64), 0, S.st, d.at(S.dev), off.at(S.dev), idx.at(S.dev), med.at(S.dev));
    HIP_TRY_AT("slamit_distinctive_batch", slamit_stage_download_and_wait(S, L));
    memcpy(best_idx, idx.at(S.host), idx.bytes());
    memcpy(best_median, med.at(S.host), med.bytes());
    return SLAMIT_OK;
}

int slamit_hamming_best2_batch_dev(const uint8_t* d_q, const int32_t* d_nq, size_t q_stride, const uint8_t* d_t,
                                   const int32_t* d_nt, size_t t_stride, int npairs, int max_n,
                                   int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, size_t out_stride,
                                   int device, void* stream) {
    if (npairs < 0 || max_n < 0 || !d_q || !d_t || !d_nq || !d_nt || !d_best_idx || !d_best || !d_second)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_hamming_best2_batch_dev: bad argument");
    if ((q_stride & 15) || (t_stride & 15) || ((uintptr_t)d_q & 15) || ((uintptr_t)d_t & 15))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_hamming_best2_batch_dev: descriptors must be 16-byte aligned");
    if (npairs == 0 || max_n == 0) return SLAMIT_OK;
    if (max_n > SLAMIT_HAMMING_MAX_TRAIN) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_hamming_best2_batch_dev: more than SLAMIT_HAMMING_MAX_TRAIN descriptors per set");
    SLAMIT_USE_DEVICE(device);
    if (hm_use_mfma(max_n)) {
        hipLaunchKernelGGL(hamming_best2_mfma_kernel, dim3((max_n + 32 * HMM_NT - 1) / (32 * HMM_NT), npairs), dim3(64 * HMM_WAVES), 0, (hipStream_t)stream, d_q, d_nq, 0, q_stride,
                           d_t, d_nt, 0, t_stride, d_best_idx, d_best, d_second, out_stride);
    } else {
        dim3 grid((max_n + HM_QPB - 1) / HM_QPB, npairs);
        hipLaunchKernelGGL(hamming_best2_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_q, d_nq, 0, q_stride, d_t, d_nt,
                           0, t_stride, d_best_idx, d_best, d_second, out_stride);
    }
    HIP_TRY(hipGetLastError());
    return SLAMIT_OK;
}

int slamit_hamming_best2(const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* best_idx, int32_t* best,
                         int32_t* second) {
    if (nq < 0 || nt < 0 || (nq && (!q || !best_idx || !best || !second)) || (nt && !t))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_hamming_best2: bad argument");
    if (nq == 0) return SLAMIT_OK;
    if (nt > SLAMIT_HAMMING_MAX_TRAIN) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_hamming_best2: more than SLAMIT_HAMMING_MAX_TRAIN train descriptors");
    const int cur_dev = slamit_default_device();   // slamit_set_device() of this thread, else the current device
    SLAMIT_USE_DEVICE(cur_dev);
    StageLayout L;
    const StageSpan<uint8_t> dq = L.take<uint8_t>(32 * (size_t)nq), dt = L.take<uint8_t>(32 * (size_t)std::max(nt, 1));
    L.end_inputs();
    const StageSpan<int> idx = L.take<int>(nq), b1 = L.take<int>(nq, alignof(int)), b2 = L.take<int>(nq, alignof(int));   // contiguous
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_hamming_best2", slamit_stage_reserve(S, cur_dev, L));
    memcpy(dq.at(S.host), q, dq.bytes());
    if (nt) memcpy(dt.at(S.host), t, 32 * (size_t)nt);
    HIP_TRY_AT("slamit_hamming_best2", slamit_stage_upload(S, L));
    if (hm_use_mfma(nt))
        hipLaunchKernelGGL(hamming_best2_mfma_kernel, dim3((nq + 32 * HMM_NT - 1) / (32 * HMM_NT), 1), dim3(64 * HMM_WAVES), 0, S.st, dq.at(S.dev), (const int*)nullptr, nq,
                           (size_t)0, dt.at(S.dev), (const int*)nullptr, nt, (size_t)0, idx.at(S.dev), b1.at(S.dev), b2.at(S.dev), (size_t)0);
    else
        hipLaunchKernelGGL(hamming_best2_kernel, dim3((nq + HM_QPB - 1) / HM_QPB, 1), dim3(256), 0, S.st, dq.at(S.dev), (const int*)nullptr, nq,
                           (size_t)0, dt.at(S.dev), (const int*)nullptr, nt, (size_t)0, idx.at(S.dev), b1.at(S.dev), b2.at(S.dev), (size_t)0);
    HIP_TRY_AT("slamit_hamming_best2", slamit_stage_download_and_wait(S, L));
    memcpy(best_idx, idx.at(S.host), idx.bytes()); memcpy(best, b1.at(S.host), b1.bytes()); memcpy(second, b2.at(S.host), b2.bytes());
    return SLAMIT_OK;
}

int slamit_hamming_matrix(const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* out) {
    if (nq < 0 || nt < 0 || ((nq && nt) && (!q || !t || !out))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_hamming_matrix: bad argument");
    if (nq == 0 || nt == 0) return SLAMIT_OK;
    const int cur_dev = slamit_default_device();
    SLAMIT_USE_DEVICE(cur_dev);
    StageLayout L;
    const StageSpan<uint8_t> dq = L.take<uint8_t>(32 * (size_t)nq), dt = L.take<uint8_t>(32 * (size_t)nt);
    L.end_inputs();
    const StageSpan<uint16_t> d = L.take<uint16_t>((size_t)nq * nt);
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_hamming_matrix", slamit_stage_reserve(S, cur_dev, L));
    memcpy(dq.at(S.host), q, dq.bytes());
    memcpy(dt.at(S.host), t, dt.bytes());
    HIP_TRY_AT("slamit_hamming_matrix", slamit_stage_upload(S, L));
    hipLaunchKernelGGL(hamming_matrix_kernel, dim3((nt + 63) / 64, (nq + 63) / 64), dim3(256), 0, S.st, dq.at(S.dev), nq, dt.at(S.dev), nt, d.at(S.dev));
    HIP_TRY_AT("slamit_hamming_matrix", slamit_stage_download_and_wait(S, L));
    memcpy(out, d.at(S.host), d.bytes());
    return SLAMIT_OK;
}

}  // extern "C"
