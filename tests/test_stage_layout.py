"""The staging-block layouts of the host-pointer entry points on the CPU: csrc/stage_layout.h and csrc/lm_layout.h are built with g++
together with a small C driver (no HIP), and checked against the rules the entry points rely on and the sizes the pose / Sim3 blocks
have always had."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")

# element types a take can be asked for: code -> (sizeof, alignof)
TYPES = {0: (1, 1), 1: (2, 2), 2: (4, 4), 3: (8, 8), 4: (20, 4), 5: (112, 16)}

DRIVER = r'''
#include <stdint.h>
#include "lm_layout.h"

struct Kp20 { float a, b, c, d; int32_t e; };
struct alignas(16) Rec112 { unsigned char b[112]; };
static_assert(sizeof(Kp20) == 20 && alignof(Kp20) == 4 && sizeof(Rec112) == 112 && alignof(Rec112) == 16, "the test's element types");

template <typename T>
static void put(StageLayout& L, uint64_t count, uint64_t align, uint64_t* o) {
    const StageSpan<T> s = align ? L.take<T>(count, align) : L.take<T>(count);
    unsigned char* const base = reinterpret_cast<unsigned char*>(uintptr_t(1) << 20);
    o[0] = s.off; o[1] = s.count; o[2] = s.bytes();
    o[3] = reinterpret_cast<uintptr_t>(s.at(base)) - reinterpret_cast<uintptr_t>(base);
}

// takes k spans (type code, count, align; align 0 = the default), the first n_in of them inputs, the next n_out outputs, the rest
// device-only; spans: k x (off, count, bytes, at - base); sizes: in_bytes, out_off, io_bytes, dev_bytes
extern "C" void drv_take(int k, int n_in, int n_out, const int32_t* type, const uint64_t* count, const uint64_t* align, uint64_t* spans,
                         uint64_t* sizes) {
    StageLayout L;
    for (int i = 0; i < k; ++i) {
        if (i == n_in) L.end_inputs();
        if (i == n_in + n_out) L.end_outputs();
        uint64_t* o = spans + 4 * i;
        switch (type[i]) {
            case 0: put<uint8_t>(L, count[i], align[i], o); break;
            case 1: put<uint16_t>(L, count[i], align[i], o); break;
            case 2: put<int32_t>(L, count[i], align[i], o); break;
            case 3: put<double>(L, count[i], align[i], o); break;
            case 4: put<Kp20>(L, count[i], align[i], o); break;
            default: put<Rec112>(L, count[i], align[i], o); break;
        }
    }
    if (k <= n_in) L.end_inputs();
    if (k <= n_in + n_out) L.end_outputs();
    sizes[0] = L.in_bytes; sizes[1] = L.out_off; sizes[2] = L.io_bytes; sizes[3] = L.dev_bytes;
}

static void span_out(const StageSpan<double>& s, uint64_t*& o) { *o++ = s.off; *o++ = s.count; }

// two problems of the same size one after the other, then their flags; out: 2 x 9 x (off, count) in the order
// pose_in, intr, xw, uv, w, chi2, pose_out, chi2_round, ur | bytes after the doubles | 2 x (off, count) of the flags | bytes at the end
extern "C" void drv_pose(uint64_t n, int stereo, uint64_t* o) {
    StageLayout L;
    for (int f = 0; f < 2; ++f) {
        const PoseSpans s = pose_take(L, n, stereo != 0);
        span_out(s.pose_in, o); span_out(s.intr, o); span_out(s.xw, o); span_out(s.uv, o); span_out(s.w, o); span_out(s.chi2, o);
        span_out(s.pose_out, o); span_out(s.chi2_round, o); span_out(s.ur, o);
    }
    *o++ = L.dev_bytes;
    for (int f = 0; f < 2; ++f) { const StageSpan<uint8_t> fl = lm_take_flags(L, n); *o++ = fl.off; *o++ = fl.count; }
    *o++ = L.dev_bytes;
}

// the same for Sim3: p1, p2, o1, o2, w1, w2, chi12, chi21, out
extern "C" void drv_sim3(uint64_t n, uint64_t* o) {
    StageLayout L;
    for (int f = 0; f < 2; ++f) {
        const Sim3Spans s = sim3_take(L, n);
        span_out(s.p1, o); span_out(s.p2, o); span_out(s.o1, o); span_out(s.o2, o); span_out(s.w1, o); span_out(s.w2, o);
        span_out(s.chi12, o); span_out(s.chi21, o); span_out(s.out, o);
    }
    *o++ = L.dev_bytes;
    for (int f = 0; f < 2; ++f) { const StageSpan<uint8_t> fl = lm_take_flags(L, n); *o++ = fl.off; *o++ = fl.count; }
    *o++ = L.dev_bytes;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("stage_layout"))
    drv = os.path.join(tmp, "stage_driver.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libstage_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, drv, "-o", so])
    L = C.CDLL(so)
    for f in (L.drv_take, L.drv_pose, L.drv_sim3):
        f.restype = None
    return L


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def take(lib, reqs, n_in, n_out):
    """reqs: [(type code, count, align or 0)] -> ([(off, count, bytes, at - base)], (in_bytes, out_off, io_bytes, dev_bytes))"""
    k = len(reqs)
    ty = np.array([r[0] for r in reqs] + [0], np.int32)
    cnt = np.array([r[1] for r in reqs] + [0], np.uint64)
    al = np.array([r[2] for r in reqs] + [0], np.uint64)
    spans = np.zeros(4 * k + 4, np.uint64)
    sizes = np.zeros(4, np.uint64)
    lib.drv_take.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.drv_take(k, n_in, n_out, _ptr(ty), _ptr(cnt), _ptr(al), _ptr(spans), _ptr(sizes))
    return [tuple(int(v) for v in spans[4 * i:4 * i + 4]) for i in range(k)], tuple(int(v) for v in sizes)


def check_take(lib, reqs, n_in, n_out):
    spans, (in_bytes, out_off, io_bytes, dev_bytes) = take(lib, reqs, n_in, n_out)
    assert in_bytes <= out_off <= io_bytes <= dev_bytes, (reqs, n_in, n_out)
    end = 0
    for i, ((ty, count, align), (off, cnt, nbytes, at)) in enumerate(zip(reqs, spans)):
        size, alignof = TYPES[ty]
        what = (reqs, n_in, n_out, i)
        assert cnt == count and nbytes == size * count and at == off, what   # exact in Python's integers: nothing wrapped
        assert off % (align or 256) == 0 and off % alignof == 0, what
        assert off >= end, what                                              # in order, never overlapping
        end = off + nbytes
        # the three sections: [0, in_bytes) | [out_off, io_bytes) | [io_bytes, dev_bytes)
        if i < n_in:
            assert end <= in_bytes, what
        elif i < n_in + n_out:
            assert out_off <= off and end <= io_bytes, what
        else:
            assert io_bytes <= off and end <= dev_bytes, what
    assert dev_bytes == max(end, out_off), (reqs, n_in, n_out)
    if n_in:
        assert in_bytes == spans[n_in - 1][0] + spans[n_in - 1][2], (reqs, n_in, n_out)   # the copy up ends with the last input
    if n_out and len(reqs) >= n_in + n_out:
        last = spans[n_in + n_out - 1]
        assert io_bytes == last[0] + last[2], (reqs, n_in, n_out)


COUNTS = [0, 1, 2, 3, 7, 8, 9, 31, 33, 255, 256, 257, 1000, 4099, 65537]


def test_spans_are_aligned_ordered_and_disjoint(lib):
    rs = np.random.RandomState(5)
    for c in COUNTS:   # one count through every type and a few alignments, empty neighbours included
        reqs = [(ty, c, al) for ty in TYPES for al in (0, 1, 8, 16, 256)] + [(0, 0, 0), (3, 0, 8), (2, 1, 0)]
        for n_in, n_out in ((0, 0), (1, 0), (7, 5), (len(reqs), 0), (len(reqs) - 2, 2), (10, len(reqs))):
            check_take(lib, reqs, n_in, n_out)
    for _ in range(200):
        k = int(rs.randint(1, 12))
        reqs = [(int(rs.randint(0, 6)), int(rs.choice(COUNTS)), int(rs.choice([0, 1, 2, 4, 8, 16, 64, 256, 4096]))) for _ in range(k)]
        n_in = int(rs.randint(0, k + 1))
        check_take(lib, reqs, n_in, int(rs.randint(0, k - n_in + 1)))


def test_an_empty_layout_and_empty_spans(lib):
    assert take(lib, [], 0, 0) == ([], (0, 0, 0, 0))
    spans, sizes = take(lib, [(3, 0, 0), (0, 0, 0), (2, 0, 0)], 1, 1)
    assert spans == [(0, 0, 0, 0)] * 3 and sizes == (0, 0, 0, 0)


def test_offsets_do_not_wrap_past_32_bits(lib):
    big = (1 << 29) + 3   # doubles: 4 GiB + 24 bytes
    reqs = [(0, 5, 0), (3, big, 0), (4, 3, 0), (1, (1 << 31) + 1, 0), (2, 7, 0), (5, 1 << 26, 0), (0, 1, 0)]
    check_take(lib, reqs, 3, 2)
    spans, sizes = take(lib, reqs, 3, 2)
    rup = lambda v: -(-v // 256) * 256
    assert spans[1][:3] == (256, big, 8 * big)
    assert spans[2][0] == rup(256 + 8 * big) and spans[2][0] > 1 << 32
    assert sizes[0] == spans[2][0] + 60 and sizes[1] == rup(sizes[0])
    assert spans[4][0] == rup(spans[3][0] + 2 * ((1 << 31) + 1)) and sizes[2] == spans[4][0] + 28
    assert sizes[3] == spans[6][0] + 1 and spans[6][0] == rup(spans[5][0] + 112 * (1 << 26))


LM_SIZES = [0, 1, 7, 8, 9, 1000]


def _lm(fn, *args):
    o = np.zeros(2 * 9 * 2 + 1 + 4 + 1, np.uint64)
    fn(*args, _ptr(o))
    o = [int(v) for v in o]
    frames = [[(o[18 * f + 2 * i], o[18 * f + 2 * i + 1]) for i in range(9)] for f in range(2)]
    return frames, o[36], [(o[37], o[38]), (o[39], o[40])], o[41]


def _check_problem(spans, start, want, n):
    """spans: (off, count) of a problem's named regions; want: (first double, doubles) of each by the sizes quoted in lm_layout.h"""
    for (off, count), (first, doubles) in zip(spans, want):
        assert off % 8 == 0 and (off, count) == (start + 8 * first, doubles), (n, spans)
    for (off, count), (nxt, _) in zip(spans, spans[1:]):
        assert off + 8 * count <= nxt, (n, spans)


def test_pose_layout(lib):
    lib.drv_pose.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
    for n in LM_SIZES:
        for stereo in (0, 1):
            frames, dbl_bytes, flags, end = _lm(lib.drv_pose, n, stereo)
            per = 32 + (8 if stereo else 7) * n   # doubles per frame
            # pose 12 | intr 4 | xw 3n | uv 2n | w n | chi2 n | pose_out 12 | chi2_round 4 [| ur n]
            want = [(0, 12), (12, 4), (16, 3 * n), (16 + 3 * n, 2 * n), (16 + 5 * n, n), (16 + 6 * n, n), (16 + 7 * n, 12), (28 + 7 * n, 4),
                    (32 + 7 * n, n if stereo else 0)]
            for f in range(2):
                _check_problem(frames[f], 8 * per * f, want, n)
            assert dbl_bytes == 2 * 8 * per, (n, stereo)
            fb = (n + 15) & ~7   # flag bytes per frame
            assert flags == [(dbl_bytes, n), (dbl_bytes + fb, n)] and end == dbl_bytes + 2 * fb, (n, stereo)


def test_sim3_layout(lib):
    lib.drv_sim3.argtypes = [C.c_uint64, C.c_void_p]
    for n in LM_SIZES:
        probs, dbl_bytes, flags, end = _lm(lib.drv_sim3, n)
        per = 14 * n + 16   # doubles per problem
        # p1 3n | p2 3n | o1 2n | o2 2n | w1 n | w2 n | chi12 n | chi21 n | out 16
        want = [(0, 3 * n), (3 * n, 3 * n), (6 * n, 2 * n), (8 * n, 2 * n), (10 * n, n), (11 * n, n), (12 * n, n), (13 * n, n), (14 * n, 16)]
        for f in range(2):
            _check_problem(probs[f], 8 * per * f, want, n)
        assert dbl_bytes == 2 * 8 * per, n
        fb = (n + 15) & ~7
        assert flags == [(dbl_bytes, n), (dbl_bytes + fb, n)] and end == dbl_bytes + 2 * fb, n
