"""The chunk schedule of an LM stage (csrc/ba_schedule.h) on the CPU: a g++-built driver runs the state machine over a fake device, and
its Q/W trace is compared with a restatement of the loop the solve had before the schedule became a unit of its own.

    Q(n, buf, first)  n slots queued (the first flagged as the stage's first slot), states copied to host buffer buf, event buf recorded
    W(buf)            event buf waited for, the done flags of buffer buf read
    S                 the caller's stop flag seen: the solve ends

The fake device reports every window done once `t` slots of the stage have been queued; the stop flag is up from pass `k` of the
driver's loop on (the poll in front of chunk k).

"The last Q is followed by its W" holds on the budget's exit.  On the other exit the solve has always left the stage on the W that reports
every window done, with the single-slot chunk queued in front of that W still in flight and never inspected: Q(1, 0, first) Q(1, 1) W(0)
is the whole trace of stage 0 with its = 1 when the first slot finishes the stage.  test_trace_properties asserts exactly that: nothing
but this one chunk may go uninspected, and only after such a report."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")

STAGES = (0, 1)
ITS = (0, 1, 2, 3, 4, 5, 10, 32)
STOPS = (-1, 0, 1, 2, 5)   # -1: never

# records of four int32: {0, n, buf, first} = Q, {1, buf, 0, 0} = W, {2, 0, 0, 0} = S
DRIVER = r'''
#include <stdint.h>
#include "ba_schedule.h"

extern "C" int drv_schedule(int stage, int its, int t, int k, int32_t* out, int cap) {
    int n = 0, queued = 0, pass = 0;
    bool done[2] = {false, false};   // what the device copied into each host buffer
    auto put = [&](int a, int b, int c, int d) {
        if (n < cap) { out[4 * n] = a; out[4 * n + 1] = b; out[4 * n + 2] = c; out[4 * n + 3] = d; }
        ++n;
    };
    BaStageSchedule sch(stage, its);
    for (bool over = false; !over && n < cap; ++pass) {
        if (k >= 0 && pass >= k) { put(2, 0, 0, 0); break; }
        const BaChunk c = sch.next();
        if (c.nslots) {
            queued += c.nslots;
            done[c.qbuf] = queued >= t;
            put(0, c.nslots, c.qbuf, c.first);
        }
        bool all_done = false;
        if (c.wbuf >= 0) { all_done = done[c.wbuf]; put(1, c.wbuf, 0, 0); }
        over = sch.finished(all_done);
    }
    return n;
}
'''

# the same grid in a program of its own, for the sanitizer build
MAIN = r'''
#include <stdio.h>
#include <vector>
int main() {
    const int its_all[] = {0, 1, 2, 3, 4, 5, 10, 32}, stops[] = {-1, 0, 1, 2, 5};
    long records = 0;
    std::vector<int32_t> out(4 * 4096);
    for (int stage = 0; stage < 2; ++stage)
        for (int its : its_all)
            for (int t = 1; t <= 10 * its + 2; ++t)
                for (int k : stops) {
                    const int n = drv_schedule(stage, its, t, k, out.data(), 4096);
                    if (n <= 0 || n >= 4096) { printf("bad trace length %d\n", n); return 1; }
                    records += n;
                }
    printf("records %ld\n", records);
    return 0;
}
'''

CAP = 4096


def _gxx(tmp, text, name, extra):
    src = os.path.join(tmp, name + ".cc")
    with open(src, "w") as f:
        f.write(text)
    out = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", CSRC, src, "-o", out] + extra)
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = _gxx(str(tmp_path_factory.mktemp("ba_schedule")), DRIVER, "libsched.so", ["-shared", "-fPIC"])
    return C.CDLL(so)


def new_trace(L, stage, its, t, k):
    out = np.zeros(4 * CAP, np.int32)
    n = L.drv_schedule(stage, its, t, k, out.ctypes.data_as(C.c_void_p), CAP)
    assert 0 < n < CAP
    tr = []
    for a, b, c, d in out[:4 * n].reshape(-1, 4).tolist():
        tr.append({0: ("Q", b, c, bool(d)), 1: ("W", b), 2: ("S",)}[a])
    return tr


def parent_trace(stage, its, t, k):
    """The solve's loop as it stood in ba_api.hip before the schedule was moved out, line for line, over the fake device."""
    tr = []
    queued = 0
    hs_done = [False, False]
    npass = 0
    # for (int stage = 0; stage < 2 && !stopped; ++stage) {  -- one stage here
    budget = its * 10 + 1
    cur, pending = 0, -1
    all_done, first = False, True
    while not all_done:
        if k >= 0 and npass >= k:       # if (opts->stop && *opts->stop) { stopped = true; break; }
            tr.append(("S",))
            break
        npass += 1
        if budget > 0:
            want = max(1, min(its if stage == 0 else 3, min(its, 4))) if first else 1
            nslots = min(want, budget)
            was_first = first
            first = False
            # for (sl < nslots) bak_slot(..., was_first && sl == 0, ...)
            queued += nslots
            budget -= nslots
            hs_done[cur] = queued >= t  # hipMemcpyAsync(hs[cur], ...); hipEventRecord(h->ev[cur], st)
            tr.append(("Q", nslots, cur, was_first))
        if pending >= 0:
            tr.append(("W", pending))   # hipEventSynchronize(h->ev[pending]); all_done = all of hs[pending][b].done
            all_done = hs_done[pending]
        if budget <= 0 and pending == cur:
            break
        pending = cur
        if budget > 0:
            cur ^= 1
    return tr


def grid():
    for stage in STAGES:
        for its in ITS:
            for t in range(1, 10 * its + 3):
                for k in STOPS:
                    yield stage, its, t, k


def test_trace_equals_the_parent_loops(lib):
    n = 0
    for stage, its, t, k in grid():
        assert new_trace(lib, stage, its, t, k) == parent_trace(stage, its, t, k), (stage, its, t, k)
        n += 1
    assert n == 2 * len(STOPS) * sum(10 * its + 2 for its in ITS)


def _queued_before_w(tr, i):
    """Slots of the stage queued up to and with the chunk whose read-back the W at tr[i] inspects (what the fake device reports by)."""
    last_q = max(j for j in range(i) if tr[j][0] == "Q" and tr[j][2] == tr[i][1])
    return sum(r[1] for r in tr[:last_q + 1] if r[0] == "Q")


def test_trace_properties(lib):
    for stage, its, t, k in grid():
        tr = new_trace(lib, stage, its, t, k)
        case = (stage, its, t, k)
        qs = [r for r in tr if r[0] == "Q"]
        assert sum(q[1] for q in qs) <= 10 * its + 1, case
        if qs:
            assert qs[0][1] == min(max(1, min(its if stage == 0 else 3, its, 4)), 10 * its + 1) and qs[0][3], case
            assert all(q[1] == 1 and not q[3] for q in qs[1:]), case
        # a buffer is inspected before it is queued into again, and at most two chunks are queued between a Q and its W
        waiting = {}   # buffer -> chunks queued since its own Q (that one included)
        for r in tr:
            if r[0] == "Q":
                assert r[2] not in waiting, case
                for b in waiting:
                    waiting[b] += 1
                waiting[r[2]] = 1
                assert max(waiting.values()) <= 2, case
            elif r[0] == "W":
                assert r[1] in waiting, case          # (never a buffer nothing was queued into)
                del waiting[r[1]]
        if k < 0:
            # The last Q is followed by its W -- on the budget's exit, and whenever the report that ends the stage is the last chunk's
            # own.  The other exit (a W that reports every window done) leaves the stage at once, as the solve always has: the one
            # chunk queued in the same pass, in front of that W, is then never looked at.  That is all that may stay uninspected.
            assert tr[-1][0] == "W", case
            reported = _queued_before_w(tr, len(tr) - 1) >= t
            if tr[-1][1] == qs[-1][2]:
                assert not waiting, case
            else:
                assert reported and list(waiting) == [qs[-1][2]] and tr[-2] == ("Q", 1, qs[-1][2], False), case
            # ... and no W before the last one reported every window done; without such a report the whole budget is queued
            assert all(_queued_before_w(tr, i) < t for i, r in enumerate(tr[:-1]) if r[0] == "W"), case
            assert reported or sum(q[1] for q in qs) == 10 * its + 1, case
        else:
            assert ("S",) not in tr[:-1], case   # nothing is queued or waited for once the flag was seen


def test_stop_is_polled_in_front_of_every_chunk(lib):
    for stage, its, t, k in grid():
        if k < 0:
            continue
        full, cut = new_trace(lib, stage, its, t, -1), new_trace(lib, stage, its, t, k)
        if cut[-1] == ("S",):
            # everything in front of the poll is what the unstopped stage does in its first k passes
            assert cut[:-1] == full[:len(cut) - 1], (stage, its, t, k)
            assert len([r for r in cut if r[0] == "Q"]) <= k, (stage, its, t, k)
        else:
            assert cut == full, (stage, its, t, k)   # the stage was over before pass k


def test_sanitized_driver_runs_clean(tmp_path):
    exe = _gxx(str(tmp_path), DRIVER + MAIN, "sched_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().startswith("records "), r.stdout.decode()
