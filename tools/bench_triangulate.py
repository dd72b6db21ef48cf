"""Times slamit_triangulate_batch: 20 and 160 keyframe pairs x 300 matched pairs in one call (one keyframe's twenty neighbours, and
eight streams' worth), against csrc/triangulate.h itself compiled with g++ -O3 and run on one core.

    python tools/bench_triangulate.py [--reps 50] [--warmup 10] [--out profiles/r13_triangulate.json]

Warm-up calls first, then the median of the repetitions (wall clock around the synchronous call, host staging and both copies
included: that is what a caller pays).  The comparator's statuses must equal the device's on every pair, or the tool fails.
Recorded, not gated."""
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
// the kernel's per-pair text on one core, over the same records the C-ABI takes
#include <stdint.h>
#include "slamit.h"
#include "triangulate.h"
extern "C" void cpu_triangulate(int nprob, const slamit_triangulate_problem* probs, slamit_triangulate_result* res) {
    for (int p = 0; p < nprob; ++p) {
        const slamit_triangulate_problem& P = probs[p];
        TriView c1, c2;
        for (int k = 0; k < 12; ++k) { c1.T[k] = P.Tcw1[k]; c2.T[k] = P.Tcw2[k]; }
        c1.fx = P.intr1[0]; c1.fy = P.intr1[1]; c1.cx = P.intr1[2]; c1.cy = P.intr1[3]; c1.invfx = P.intr1[4]; c1.invfy = P.intr1[5];
        c2.fx = P.intr2[0]; c2.fy = P.intr2[1]; c2.cx = P.intr2[2]; c2.cy = P.intr2[3]; c2.invfx = P.intr2[4]; c2.invfy = P.intr2[5];
        tri_centre(c1); tri_centre(c2);
        int acc = 0;
        for (int i = 0; i < P.n; ++i) {
            const int o1 = P.octave1[i], o2 = P.octave2[i];
            const int st = tri_pair(c1, c2, P.kp1_xy + 2 * i, P.kp2_xy + 2 * i, P.level_sigma2_1[o1], P.level_sigma2_2[o2], P.scale_factors1[o1],
                                    P.scale_factors2[o2], P.ratio_factor, res[p].x3d + 3 * i);
            res[p].status[i] = (uint8_t)st;
            acc += st == 0;
        }
        res[p].n_accepted = acc;
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


def records(api, probs):
    """The C records of a list of problem dicts, with their output arrays: (P, R, outputs, keep-alive)."""
    m = len(probs)
    P, R = (api.TriangulateProblem * m)(), (api.TriangulateResult * m)()
    outs, keep = [], []
    for i, pr in enumerate(probs):
        n = int(pr["n"])
        k = {key: np.ascontiguousarray(pr[key]) for key in ("kp1_xy", "kp2_xy", "octave1", "octave2", "scale_factors1", "level_sigma2_1", "scale_factors2", "level_sigma2_2")}
        for key, arr in k.items():
            setattr(P[i], key, arr.ctypes.data)
        P[i].n, P[i].n_levels, P[i].ratio_factor = n, int(pr["n_levels"]), float(pr["ratio_factor"])
        P[i].Tcw1, P[i].Tcw2 = (C.c_float * 12)(*pr["Tcw1"]), (C.c_float * 12)(*pr["Tcw2"])
        P[i].intr1, P[i].intr2 = (C.c_float * 6)(*pr["intr1"]), (C.c_float * 6)(*pr["intr2"])
        o = (np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))
        R[i].status, R[i].x3d = o[0].ctypes.data, o[1].ctypes.data
        outs.append(o)
        keep.append(k)
    return P, R, outs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_triangulate.json"))
    a = ap.parse_args()
    from weiner_slamit_v2_amd import api, synth

    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    res = {"workload": "N problems x 300 pairs, one slamit_triangulate_batch call", "comparator": "csrc/triangulate.h compiled with g++ -O3, one core",
           "reps": a.reps, "warmup": a.warmup, "cases": []}
    L = api.lib()
    for nprob in (20, 160):
        probs = [synth.synth_triangulation(300, 900 + k, 0.05 + 0.7 * (k % 20) / 19.0, 0.2, 0.7) for k in range(nprob)]
        bind_ms, _ = median_ms(lambda: api.triangulate_batch(probs), a.warmup, a.reps)
        P, R, outs, keep = records(api, probs)
        assert L.slamit_triangulate_batch(0, nprob, P, R) == 0, L.slamit_last_error()
        call_ms, call_min = median_ms(lambda: L.slamit_triangulate_batch(0, nprob, P, R), a.warmup, a.reps)
        Pc, Rc, outs_c, keep_c = records(api, probs)
        cpu_ms, cpu_min = median_ms(lambda: port.cpu_triangulate(nprob, Pc, Rc), 2, a.reps)
        same = all(np.array_equal(g[0], c[0]) for g, c in zip(outs, outs_c))
        same_x = all(np.array_equal(g[1].view(np.uint32), c[1].view(np.uint32)) for g, c in zip(outs, outs_c))
        res["cases"].append({"problems": nprob, "pairs_per_call": 300 * nprob, "accepted": int(sum(R[i].n_accepted for i in range(nprob))),
                             "gpu_binding_ms_median": bind_ms, "gpu_c_call_ms_median": call_ms, "gpu_c_call_ms_min": call_min,
                             "cpu_header_ms_median": cpu_ms, "cpu_header_ms_min": cpu_min, "speedup_c_call_vs_cpu_header": cpu_ms / call_ms,
                             "statuses_equal_cpu_header": bool(same), "points_bit_equal_cpu_header": bool(same_x),
                             "n_accepted_equal": all(R[i].n_accepted == Rc[i].n_accepted for i in range(nprob))})
        if not same:
            print(json.dumps(res))
            raise SystemExit("statuses differ between the device and the g++-built header")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
