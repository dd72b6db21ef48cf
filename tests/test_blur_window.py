"""The per-lane window plan of the blur's edge strips (csrc/blur_window.h) on the CPU: the header is built with g++ together with a
small C driver, and for every level width 62 .. 1400, every lane x0 < w and three row pitches the window a lane assembles from its
ONE 12-byte load is compared with BORDER_REFLECT_101 computed here, byte by byte, at every position a stored output reads.

A lane owns outputs x0 .. x0 + 3; output o is stored when o < w and reads columns o - 3 .. o + 3.  Of the 12 window bytes (columns
x0 - 4 .. x0 + 7) a lane with four stored outputs therefore never needs two (x0 - 4 and x0 + 7), and a lane at the right edge with
n < 4 stored outputs needs n + 6: the don't-care positions are masked out explicitly, and their number per lane is asserted so
that the mask cannot grow silently.  The load must stay inside the row's pitch: level 0 is the caller's buffer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")

# every lane of one (w, pitch): the load offset, the five selectors, and the window assembled from `row`
DRIVER = r'''
#include <string.h>
#include "blur_window.h"

extern "C" int drv_lanes(int w, int pitch, const uint8_t* row, int32_t* lb, uint32_t* sel, uint8_t* win) {
    int n = 0;
    for (int x0 = 0; x0 < w; x0 += 4, ++n) {
        const BlurWindow p = blur_window(x0, w, pitch);
        lb[n] = (int32_t)p.lb;
        const uint32_t s[5] = {p.s0, p.a1, p.b1, p.a2, p.b2};
        memcpy(sel + 5 * n, s, sizeof(s));
        if ((int64_t)p.lb + 12 > pitch) { memset(win + 12 * n, 0, 12); continue; }   // (the test fails on lb; no read outside the row here either)
        uint32_t l[3], o[3];
        memcpy(l, row + p.lb, 12);
        blur_window_apply(p, l[0], l[1], l[2], o);
        memcpy(win + 12 * n, o, 12);
    }
    return n;
}
'''

IDENTITY = [0x03020100, 0x07060504, 0x03020100, 0x0C0C0C0C, 0x07060504]   # s0, a1, b1, a2, b2 of a lane whose window is its load
W_MIN, W_MAX = 62, 1400


@pytest.fixture(scope="module")
def wlib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("blur_window"))
    drv, so = os.path.join(tmp, "window_driver.cc"), os.path.join(tmp, "libwindow_driver.so")
    with open(drv, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, drv, "-o", so])
    L = C.CDLL(so)
    L.drv_lanes.restype = C.c_int
    return L


def _row(w, pitch):
    """Distinct bytes over any 250 adjacent image columns; the pad columns w .. pitch - 1 hold values no image column has."""
    row = np.empty(pitch, np.uint8)
    row[:w] = (np.arange(w) * 7 + 3) % 251
    row[w:] = 252 + (np.arange(pitch - w) & 3)
    return row


def _lanes(L, w, pitch, row):
    n = (w + 3) // 4
    lb, sel, win = np.zeros(n, np.int32), np.zeros((n, 5), np.uint32), np.zeros((n, 12), np.uint8)
    got = L.drv_lanes(w, pitch, row.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p), sel.ctypes.data_as(C.c_void_p),
                      win.ctypes.data_as(C.c_void_p))
    assert got == n
    return lb, sel, win


def _expect(w, row):
    """(window through REFLECT_101, needed mask) for every lane of a level w wide, straight from the definition."""
    x0 = np.arange(0, w, 4)[:, None]
    c = x0 - 4 + np.arange(12)[None, :]                 # the window's columns
    o = x0[:, :, None] + np.arange(4)[None, None, :]    # the lane's outputs
    needed = ((o < w) & (np.abs(c[:, :, None] - o) <= 3)).any(axis=2)
    r = np.where(c < 0, -c, c)
    r = np.where(r >= w, 2 * w - 2 - r, r)
    assert ((r >= 0) & (r < w))[needed].all()
    return row[np.clip(r, 0, w - 1)], needed


def _pitches(w):
    return sorted({(w + 3) & ~3, ((w + 3) & ~3) + 4, (w + 63) & ~63})


def test_window_of_every_lane(wlib):
    cases = lanes = dont_care = 0
    for w in range(W_MIN, W_MAX + 1):
        x0 = np.arange(0, w, 4)
        nout = np.minimum(4, w - x0)
        for pitch in _pitches(w):
            row = _row(w, pitch)
            lb, sel, win = _lanes(wlib, w, pitch, row)
            want, needed = _expect(w, row)
            tag = "w %d pitch %d" % (w, pitch)
            # the load stays inside the row, at the offset the design states
            assert (lb >= 0).all() and (lb + 12 <= pitch).all(), tag
            assert np.array_equal(lb, np.minimum(np.maximum(x0 - 4, 0), pitch - 12)), tag
            # a lane with n stored outputs reads n + 6 of its 12 window bytes: 2 don't-care positions for a full lane, up to 5 at the right edge
            assert np.array_equal((~needed).sum(axis=1), 6 - nout), tag
            bad = np.argwhere(needed & (win != want))
            assert len(bad) == 0, "%s: lane x0 %d window byte %d is %d, REFLECT_101 gives %d" % (
                tag, 4 * bad[0][0], bad[0][1], win[tuple(bad[0])], want[tuple(bad[0])])
            # lanes whose window lies inside the image load it as it is
            inner = (x0 >= 4) & (x0 + 8 <= w)
            assert np.array_equal(lb[inner], x0[inner] - 4), tag
            assert (sel[inner] == np.array(IDENTITY, np.uint32)).all(), tag
            assert np.array_equal(win[inner], want[inner]), tag
            cases += 1
            lanes += len(x0)
            dont_care += int((~needed).sum())
    assert cases == sum(len(_pitches(w)) for w in range(W_MIN, W_MAX + 1)) and lanes > 0 and dont_care >= 2 * lanes
    print("blur window: %d (w, pitch) cases, %d lanes, %d don't-care bytes excluded" % (cases, lanes, dont_care))


def test_the_shifted_loads_are_exercised(wlib):
    """The two shifted loads exist in the sweep: the leftmost lane (shifted right by 4) and a last lane whose window would pass the
    pitch (shifted left by 4); a last lane with room in the pad is not shifted."""
    for w, pitch, last_lb in ((128, 128, 116), (125, 128, 116), (125, 132, 120), (129, 132, 120), (129, 192, 124), (62, 64, 52)):
        lb, _, _ = _lanes(wlib, w, pitch, _row(w, pitch))
        assert lb[0] == 0 and lb[1] == 0 and lb[2] == 4, (w, pitch)
        assert lb[-1] == last_lb, (w, pitch, int(lb[-1]))
