// lm_layout.h — where one problem of the two single-block LM entry points (pose.hip, sim3.hip) sits in the staging block, by name.
// Plain C++17 (no HIP): slamit_pose_optimize_batch / slamit_sim3_optimize_batch pack, point the kernel's record at and unpack
// these spans, and the CPU test (tests/test_stage_layout.py) checks them.  A batch is [doubles of every problem | ints |
// records | flags of every problem]; the doubles are contiguous, so a problem costs exactly the sizes quoted below.
// This is the host half of what the two entry points share; the device half is lm_block.h (the workgroup's Levenberg driver) over
// lm_step.h (its scalar rules, also CPU-tested: tests/test_lm_step.py).
#ifndef SLAMIT_LM_LAYOUT_H
#define SLAMIT_LM_LAYOUT_H
#include <stdint.h>

#include "stage_layout.h"

// one frame of slamit_pose_optimize_batch: 32 + 7 n doubles, 32 + 8 n when it has right-image columns
struct PoseSpans { StageSpan<double> pose_in, intr, xw, uv, w, chi2, pose_out, chi2_round, ur; };
inline PoseSpans pose_take(StageLayout& L, size_t n, bool stereo) {
    PoseSpans s;
    s.pose_in = L.take<double>(12, 8); s.intr = L.take<double>(4, 8);
    s.xw = L.take<double>(3 * n, 8); s.uv = L.take<double>(2 * n, 8); s.w = L.take<double>(n, 8); s.chi2 = L.take<double>(n, 8);
    s.pose_out = L.take<double>(12, 8); s.chi2_round = L.take<double>(4, 8); s.ur = L.take<double>(stereo ? n : 0, 8);
    return s;
}

// one problem of slamit_sim3_optimize_batch: 14 n + 16 doubles; out = R (9), t (3), s, chi2[2], pad
struct Sim3Spans { StageSpan<double> p1, p2, o1, o2, w1, w2, chi12, chi21, out; };
inline Sim3Spans sim3_take(StageLayout& L, size_t n) {
    Sim3Spans s;
    s.p1 = L.take<double>(3 * n, 8); s.p2 = L.take<double>(3 * n, 8); s.o1 = L.take<double>(2 * n, 8); s.o2 = L.take<double>(2 * n, 8);
    s.w1 = L.take<double>(n, 8); s.w2 = L.take<double>(n, 8); s.chi12 = L.take<double>(n, 8); s.chi21 = L.take<double>(n, 8); s.out = L.take<double>(16, 8);
    return s;
}

// the n outlier / inlier flags of one problem: (n + 15) & ~7 bytes, so the next problem's start on an 8-byte boundary
inline StageSpan<uint8_t> lm_take_flags(StageLayout& L, size_t n) {
    StageSpan<uint8_t> s = L.take<uint8_t>((n + 15) & ~(size_t)7, 1);
    s.count = n;
    return s;
}

#endif
