// distinctive.h — the selection of MapPoint::ComputeDistinctiveDescriptors by one wavefront over n descriptors in LDS, shared by
// distinctive_kernel (hamming.hip: rows packed by the caller) and the map-point update pass (upkeep.hip: rows gathered from the tables).
// rowsd holds the descriptors as uint4 halves, D the n x n distance matrix (u16).  Each lane owns rows lane, lane + 64 and finds its
// row's median by bisection on the value range [0, 256] (count of entries <= mid); the wave takes the lexicographic minimum of
// (median, row), so the first least-median row wins like the reference's loop.
//
// A macro and not a function: as the text of the kernel it came from, distinctive_kernel compiles to the instruction stream it had
// (an inlined function came out scheduled differently).  The caller has made rowsd[0 .. 2n) visible to the wave; n and lane are ints;
// it declares `unsigned bestkey` = (median << 16) | row, the same in every lane.
#ifndef SLAMIT_DISTINCTIVE_H
#define SLAMIT_DISTINCTIVE_H
#include <hip/hip_runtime.h>

#include "wave_ops.h"

#define DISTINCTIVE_SELECT(rowsd, D, n, lane, bestkey)                                                                         \
    for (int i = lane; i < n; i += 64) {                                                                                       \
        const uint4 a0 = rowsd[2 * i], a1 = rowsd[2 * i + 1];                                                                  \
        for (int j = 0; j < n; ++j) {                                                                                          \
            const uint4 t0 = rowsd[2 * j], t1 = rowsd[2 * j + 1];                                                              \
            const int d = hamming256(a0, a1, t0, t1);                                                                          \
            D[i * n + j] = (unsigned short)d;                                                                                  \
        }                                                                                                                      \
    }                                                                                                                          \
    const int k = (int)(0.5 * (n - 1)); /* index of the median in the sorted row */                                            \
    unsigned bestkey = 0xFFFFFFFFu;      /* (median << 16) | row */                                                             \
    for (int i = lane; i < n; i += 64) {                                                                                       \
        int lo = 0, hi = 256;                                                                                                  \
        while (lo < hi) {                                                                                                      \
            const int mid = (lo + hi) >> 1;                                                                                    \
            int c = 0;                                                                                                         \
            for (int j = 0; j < n; ++j) c += D[i * n + j] <= mid;                                                              \
            if (c >= k + 1) hi = mid; else lo = mid + 1;                                                                       \
        }                                                                                                                      \
        bestkey = min(bestkey, ((unsigned)lo << 16) | (unsigned)i);                                                            \
    }                                                                                                                          \
    _Pragma("unroll")                                                                                                          \
    for (int d = 32; d >= 1; d >>= 1) bestkey = min(bestkey, (unsigned)__shfl_xor((int)bestkey, d, 64));

#endif
