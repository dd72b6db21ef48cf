"""csrc/stage_binder.h on the CPU: the binder that names every array of a staged call once is built with g++ together with a small driver
(tests/stage_binder_driver.cc, no HIP) that stands in for the device with a second malloc'ed block.  Checked: every input arrives at its
device pointer, every output lands in its destination and nowhere else, device-only arrays lie behind the pinned block, the offsets are
aligned, ordered and disjoint, empty and null arrays take no room, totals beyond 4 GiB do not wrap, and a describe function that changes
between the passes is reported."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "stage_binder_driver.cc")

TYPES = {0: (1, 1), 1: (2, 2), 2: (4, 4), 3: (8, 8), 4: (20, 4), 5: (112, 16)}   # code -> (sizeof, alignof), as in test_stage_layout.py
IN, IN_FILL, OUT, OUT_VIEW, SCRATCH = range(5)
REGION = {IN: 0, IN_FILL: 0, OUT: 1, OUT_VIEW: 1, SCRATCH: 2}
OK_PLAN_NULL, OK_INPUT, OK_OUTPUT, OK_GUARDS = 1, 2, 4, 8
NONE = (1 << 64) - 1
COUNTS = [0, 1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("stage_binder")), "libstage_binder_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, DRIVER, "-o", so])
    L = C.CDLL(so)
    L.drv_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    L.drv_run.restype = C.c_int
    return L


def run(lib, nprob, reqs, bump=(-1, 0), only_offsets=False):
    """reqs: [(problem, kind, type code, count, null)] -> (check that failed or 0, [(dev off, host off, flags, bytes)], (in_bytes, out_off,
    io_bytes, dev_bytes, bound))"""
    k = len(reqs)
    rq = np.array(list(reqs) + [(0, 0, 0, 0, 0)], np.int64)
    report = np.zeros(4 * k + 4, np.uint64)
    sizes = np.zeros(5, np.uint64)
    rc = lib.drv_run(nprob, k, rq.ctypes.data, bump[0], bump[1], int(only_offsets), report.ctypes.data, sizes.ctypes.data)
    return rc, [tuple(int(v) for v in report[4 * i:4 * i + 4]) for i in range(k)], tuple(int(v) for v in sizes)


def check(lib, nprob, reqs, only_offsets=False):
    rc, rep, (in_bytes, out_off, io_bytes, dev_bytes, bound) = run(lib, nprob, reqs, only_offsets=only_offsets)
    assert rc == 0 and bound == 1, (rc, reqs)
    assert in_bytes <= out_off <= io_bytes <= dev_bytes and out_off % 256 == 0, reqs
    # the order in which the binder meets the arrays: problem by problem, and within a problem as listed
    order = sorted(range(len(reqs)), key=lambda i: (reqs[i][0], i))
    base = [0, out_off, -(-io_bytes // 256) * 256]   # the device-only region starts on a boundary of its own, like the outputs
    ends = list(base)                        # where the next array of each region may start: the end of the last one that took room
    for i in order:
        (_, kind, ty, count, null), (dev, host, flags, nbytes) = reqs[i], rep[i]
        size, alignof = TYPES[ty]
        what = (reqs, i)
        assert flags & OK_PLAN_NULL, what                                        # the plan pass hands out nothing
        assert nbytes == size * count, what
        if null and kind in (IN, OUT):
            assert dev == NONE, what                                             # a null source / destination: null, and no room (below)
            continue
        assert dev != NONE, what
        r = REGION[kind]
        if count == 0:
            assert dev == ends[r], what                                          # an empty array sits at the cursor and moves nothing
            continue
        assert dev % 16 == 0 and dev % alignof == 0 and dev >= ends[r] and dev - ends[r] < 16, what   # aligned, in order, no gap but the padding
        ends[r] = dev + nbytes
        if kind in (IN_FILL, OUT_VIEW) or (only_offsets and kind in (IN, OUT)):
            assert host == dev, what                                             # one layout for both copies of the block
        if r == 0:
            assert dev + nbytes <= in_bytes, what
            assert only_offsets or flags & OK_INPUT, what
        elif r == 1:
            assert out_off <= dev and dev + nbytes <= io_bytes, what
            assert only_offsets or flags & OK_OUTPUT, what
            assert only_offsets or kind != OUT or flags & OK_GUARDS, what
        else:
            assert io_bytes <= dev and dev + nbytes <= dev_bytes, what           # device-only: behind the pinned block
    assert (in_bytes, io_bytes, dev_bytes) == tuple(ends), reqs   # nothing but the arrays takes room
    return rep, (in_bytes, out_off, io_bytes, dev_bytes)


def batch(nprob, c, null_every=0):
    """every call with every type, the counts rotating through COUNTS from position c; of three problems the middle one is empty"""
    reqs = []
    for f in range(nprob):
        for kind in range(5):
            for ty in TYPES:
                count = 0 if (nprob == 3 and f == 1) else COUNTS[(c + ty + kind + f) % len(COUNTS)]
                reqs.append((f, kind, ty, count, int(null_every and (kind + ty + c) % null_every == 0)))
    return reqs


@pytest.mark.parametrize("nprob", [1, 3])
def test_inputs_arrive_outputs_land_and_the_regions_hold(lib, nprob):
    for c in range(len(COUNTS)):
        check(lib, nprob, batch(nprob, c))
        check(lib, nprob, batch(nprob, c, null_every=4))
    for count in COUNTS:   # one count through everything
        check(lib, nprob, [(f, kind, ty, count, 0) for f in range(nprob) for kind in range(5) for ty in TYPES])


def test_interleaved_calls_keep_three_contiguous_regions(lib):
    rs = np.random.RandomState(7)
    for _ in range(100):
        nprob = int(rs.choice([1, 3]))
        reqs = [(int(rs.randint(0, nprob)), int(rs.randint(0, 5)), int(rs.randint(0, 6)), int(rs.choice(COUNTS)), int(rs.rand() < 0.15))
                for _ in range(int(rs.randint(1, 20)))]
        check(lib, nprob, reqs)


def test_empty_and_null_arrays_take_no_room(lib):
    rep, sizes = check(lib, 1, [(0, kind, ty, 0, 0) for kind in range(5) for ty in TYPES])
    assert sizes == (0, 0, 0, 0)
    rep, sizes = check(lib, 1, [(0, kind, ty, 65, 1) for kind in (IN, OUT) for ty in TYPES])
    assert sizes == (0, 0, 0, 0) and all(r[0] == NONE for r in rep)
    full = [(0, IN, 2, 65, 0), (0, OUT, 3, 64, 0), (0, SCRATCH, 0, 257, 0)]
    _, want = check(lib, 1, full)
    padded = [(0, IN, 3, 0, 0), full[0], (0, IN, 5, 63, 1), (0, OUT, 4, 0, 0), full[1], (0, OUT, 1, 257, 1), (0, OUT_VIEW, 2, 0, 0), full[2],
              (0, SCRATCH, 5, 0, 0)]
    _, got = check(lib, 1, padded)
    assert got == want == (260, 512, 512 + 512, 1024 + 257)


def test_offsets_do_not_wrap_past_32_bits(lib):
    big = (1 << 29) + 3   # doubles: 4 GiB + 24 bytes
    reqs = [(0, IN, 0, 5, 0), (0, IN, 3, big, 0), (0, IN_FILL, 4, 3, 0), (0, OUT, 1, (1 << 31) + 1, 0), (0, OUT_VIEW, 2, 7, 0),
            (0, SCRATCH, 5, 1 << 26, 0), (0, SCRATCH, 0, 1, 0)]
    rep, (in_bytes, out_off, io_bytes, dev_bytes) = check(lib, 1, reqs, only_offsets=True)
    up16, up256 = lambda v: -(-v // 16) * 16, lambda v: -(-v // 256) * 256
    assert rep[1][0] == 16 and rep[2][0] == up16(16 + 8 * big) > 1 << 32
    assert in_bytes == rep[2][0] + 60 and out_off == up256(in_bytes) == rep[3][0]
    assert rep[4][0] == up16(out_off + 2 * ((1 << 31) + 1)) and io_bytes == rep[4][0] + 28
    assert rep[5][0] == up256(io_bytes) and rep[6][0] == rep[5][0] + 112 * (1 << 26) > 3 << 32 and dev_bytes == rep[6][0] + 1


@pytest.mark.parametrize("kind", range(5))
def test_a_describe_function_that_changes_between_the_passes_is_reported(lib, kind):
    for nprob in (1, 3):
        reqs = batch(nprob, 2)
        for i, q in enumerate(reqs):
            if q[1] != kind or q[3] == 0:
                continue
            for by in (64, -q[3]):   # more than planned (the block has no room for it), and less
                rc, rep, sizes = run(lib, nprob, reqs, bump=(i, by))
                assert rc == 0 and sizes[4] == 0, (i, by)
    # more than the whole block holds: from the array that does not fit on, nothing is handed out and nothing copied
    reqs = [(0, IN, 0, 64, 0), (0, IN, 3, 65, 0), (0, OUT, 2, 63, 0)]
    rc, rep, sizes = run(lib, 1, reqs, bump=(0, 64 * 9))
    assert rc == 0 and sizes[4] == 0 and all(r[0] == NONE for r in rep)
