"""Times slamit_sim3_ransac_batch: 10 candidates x 300 hypotheses x {200, 600} correspondences, one call (what
LoopClosing::ComputeSim3 costs), against a single-core C++ -O3 port of the same loop built from this file.

    python tools/bench_sim3_ransac.py [--reps 50] [--warmup 10] [--out profiles/r06_sim3_ransac.json]

Warm-up calls first, then the median of the repetitions (wall clock around the synchronous call, host staging and both copies
included: that is what a caller pays).  Recorded, not gated."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU_PORT = r'''
// iterate()'s body for a batch on one core: ComputeSim3 + CheckInliers per hypothesis, in the arithmetic of csrc/sim3_horn.h
#include <stdint.h>
#include "sim3_horn.h"
extern "C" void cpu_sim3_ransac(int nprob, const int* n, const int* nh, const float* const* x1, const float* const* x2, const float* const* e1,
                                const float* const* e2, const float* K1, const float* K2, int fix, const int32_t* const* tri, int32_t* const* counts) {
    for (int p = 0; p < nprob; ++p)
        for (int h = 0; h < nh[p]; ++h) {
            float P1[3][3], P2[3][3];
            for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { P1[k][a] = x1[p][3 * tri[p][3 * h + k] + a]; P2[k][a] = x2[p][3 * tri[p][3 * h + k] + a]; }
            Sim3Hyp H;
            sim3h_solve(P1, P2, fix, H);
            int c = 0;
            for (int i = 0; i < n[p]; ++i) { float a, b; sim3h_errors(H, x1[p] + 3 * i, x2[p] + 3 * i, K1, K2, &a, &b); c += (a < e1[p][i] && b < e2[p][i]); }
            counts[p][h] = c;
        }
}
'''


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_sim3_ransac.json"))
    a = ap.parse_args()
    from weiner_slamit_v2_amd import api, synth

    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    res = {"workload": "10 problems x 300 hypotheses, one slamit_sim3_ransac_batch call", "comparator": "single-core C++ -O3 port of the same loop (g++, this tool's source)",
           "reps": a.reps, "warmup": a.warmup, "cases": []}
    nprob, nh = 10, 300
    for n in (200, 600):
        probs = []
        for k in range(nprob):
            pr = synth.synth_sim3_ransac(n, 0.3, 500 + k, 0.5, False)
            rs = np.random.RandomState(k)
            pr["triples"] = api.Sim3Solver.sample_triples(n, nh, lambda lo, hi: int(rs.randint(lo, hi + 1)))
            probs.append(pr)
        got = api.Sim3Solver.evaluate(probs, want_bits=False)
        gpu_ms, gpu_min = median_ms(lambda: api.Sim3Solver.evaluate(probs, want_bits=False), a.warmup, a.reps)
        # the bare C call, arrays prepared once (what the C++ shim pays)
        P = (api.Sim3RansacProblem * nprob)()
        R = (api.Sim3RansacResult * nprob)()
        keep = []
        for i, pr in enumerate(probs):
            o = (np.zeros((nh, 13), np.float32), np.zeros(nh, np.int32))
            keep.append(o)
            P[i].n, P[i].n_hyp, P[i].fix_scale = n, nh, 0
            for key in ("x1", "x2", "max_err1", "max_err2", "triples"):
                setattr(P[i], key, pr[key].ctypes.data)
            P[i].intr1 = (C.c_float * 4)(*pr["intr1"]); P[i].intr2 = (C.c_float * 4)(*pr["intr2"])
            R[i].t12, R[i].n_inliers = o[0].ctypes.data, o[1].ctypes.data
        L = api.lib()
        call_ms, call_min = median_ms(lambda: L.slamit_sim3_ransac_batch(0, nprob, P, R), a.warmup, a.reps)
        # CPU port
        arr = lambda ct, xs: (ct * nprob)(*xs)   # noqa: E731
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        counts = [np.zeros(nh, np.int32) for _ in range(nprob)]
        args = [nprob, arr(C.c_int, [n] * nprob), arr(C.c_int, [nh] * nprob)]
        for key in ("x1", "x2", "max_err1", "max_err2"):
            args.append(arr(fp, [pr[key].ctypes.data_as(fp) for pr in probs]))
        args += [probs[0]["intr1"].ctypes.data_as(fp), probs[0]["intr2"].ctypes.data_as(fp), 0,
                 arr(ip, [pr["triples"].ctypes.data_as(ip) for pr in probs]), arr(ip, [c.ctypes.data_as(ip) for c in counts])]
        cpu_ms, cpu_min = median_ms(lambda: port.cpu_sim3_ransac(*args), 2, max(5, a.reps // 5))
        same = all(np.array_equal(c, g["n_inliers"]) for c, g in zip(counts, got))
        res["cases"].append({"n": n, "gpu_binding_ms_median": gpu_ms, "gpu_c_call_ms_median": call_ms, "gpu_c_call_ms_min": call_min, "cpu_port_ms_median": cpu_ms,
                             "speedup_c_call_vs_cpu_port": cpu_ms / call_ms, "pairs_per_call": nprob * nh * n, "counts_equal_cpu_port": bool(same)})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
