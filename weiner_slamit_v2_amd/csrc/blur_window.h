// blur_window.h — how one lane of an EDGE strip of blur_stream_kernel (orb_kernels.hip) obtains its 12-byte window from ONE 12-byte
// load per row.  A lane owns output columns x0 .. x0 + 3 (x0 a multiple of 4) of a level w columns wide whose rows are `pitch`
// bytes apart (a multiple of 4, >= w); its window is columns x0 - 4 .. x0 + 7, three dwords, of which output o reads columns
// o - 3 .. o + 3 through BORDER_REFLECT_101.  Only outputs o < w are stored, so only their bytes matter.
//
//   load       12 bytes at byte offset lb = min(max(x0 - 4, 0), pitch - 12) of the row: the leftmost lane of a level loads columns
//              0 .. 11 (its window shifted right by 4), a lane whose window would pass the row's pitch loads the row's last 12 bytes
//              (shifted left by 4), every other lane its window itself.  No byte outside [row, row + pitch) is touched.
//   window     every byte a stored output reads lies in those 12 bytes (w >= 62: a level is never narrower, slamit_orb_create), and
//              each window dword draws on at most two of the three loaded dwords -- dword 0 on loaded (0, 1), dwords 1 and 2 on
//              (0, 1) or (1, 2), by lane.  The choice of operands is folded into the selectors of TWO chained byte permutes:
//                  win[0] = perm(l1, l0, s0)
//                  win[k] = perm(l2, perm(l1, l0, a[k]), b[k])      k = 1, 2
//              (the inner permute gathers what comes from loaded dwords 0 and 1, the outer one keeps those bytes and takes the rest
//              from loaded dword 2): five v_perm_b32 per row and five selector registers per lane, no select, no second load.
//   don't care a window byte no stored output reads whose REFLECT_101 source lies outside the 12 loaded bytes is 0.
//
// The kernel and tests/test_blur_window.py (through a g++ driver) run the same text.  Plain integer C++.
#ifndef SLAMIT_BLUR_WINDOW_H
#define SLAMIT_BLUR_WINDOW_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BLURWIN_HD __host__ __device__ __forceinline__
#else
#define BLURWIN_HD static inline
#endif

struct BlurWindow {
    uint32_t lb;           // byte offset of the 12-byte load inside the row
    uint32_t s0;           // win[0] = perm(l1, l0, s0)
    uint32_t a1, b1;       // win[1] = perm(l2, perm(l1, l0, a1), b1)
    uint32_t a2, b2;       // win[2] = perm(l2, perm(l1, l0, a2), b2)
};

#define BLURWIN_ZERO 0x0Cu   // the selector byte of v_perm_b32 that yields 0x00

// v_perm_b32 for the selector bytes the plan uses: 0 .. 3 = byte of lo, 4 .. 7 = byte of hi, 0x0C = 0
BLURWIN_HD uint32_t blurwin_perm(const uint32_t hi, const uint32_t lo, const uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int j = 0; j < 4; ++j) {
        const uint32_t s = (sel >> (8 * j)) & 0xFFu;
        if (s < 8u) r |= (uint32_t)((src >> (8 * s)) & 0xFFu) << (8 * j);
    }
    return r;
#endif
}

// The plan of the lane at x0 (a multiple of 4, 0 <= x0 < w) of a level w >= 62 columns wide with rows `pitch` bytes apart.
BLURWIN_HD BlurWindow blur_window(const int x0, const int w, const int pitch) {
    BlurWindow p;
    const int lb = x0 - 4 < 0 ? 0 : (x0 + 8 > pitch ? pitch - 12 : x0 - 4);
    p.lb = (uint32_t)lb;
    uint32_t sa[3] = {0u, 0u, 0u}, sb[3] = {0u, 0u, 0u};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 12; ++i) {
        int c = x0 - 4 + i;                       // the window column, through REFLECT_101 (one reflection: |overshoot| <= 4 < w)
        c = c < 0 ? -c : c;
        c = c >= w ? 2 * w - 2 - c : c;
        const uint32_t b = (uint32_t)(c - lb);    // its place among the 12 loaded bytes, if it is there
        const int sh = 8 * (i & 3);
        sa[i >> 2] |= (b < 8u ? b : BLURWIN_ZERO) << sh;
        sb[i >> 2] |= (b < 8u ? (uint32_t)(i & 3) : b < 12u ? b - 4u : BLURWIN_ZERO) << sh;
    }
    p.s0 = sa[0];   // (dword 0 never draws on loaded dword 2: its sources lie at or left of column x0 + 4 <= lb + 8)
    p.a1 = sa[1]; p.b1 = sb[1];
    p.a2 = sa[2]; p.b2 = sb[2];
    return p;
}

// The window of a row from its three loaded dwords.
BLURWIN_HD void blur_window_apply(const BlurWindow& p, const uint32_t l0, const uint32_t l1, const uint32_t l2, uint32_t win[3]) {
    win[0] = blurwin_perm(l1, l0, p.s0);
    win[1] = blurwin_perm(l2, blurwin_perm(l1, l0, p.a1), p.b1);
    win[2] = blurwin_perm(l2, blurwin_perm(l1, l0, p.a2), p.b2);
}

#endif
