"""Times the two launches of the device PnPsolver: slamit_pnp_ransac_batch and slamit_pnp_refine_batch for 1, 8 and 32 candidate
keyframes x 35 hypotheses (Tracking::Relocalization's parameters) x {100, 1000} correspondences, and one candidate x 300 hypotheses,
against csrc/epnp.h itself on one host core (g++ -O3 of the same header, built from this file).

    python tools/bench_pnp.py [--reps 50] [--warmup 10] [--out profiles/r20_pnp.json]

Warm-up calls first, then the median of the repetitions (wall clock around the synchronous C call, host staging and both copies
included: that is what a caller pays).  A run without a device fails; there is no fall-back.  Recorded, not gated."""
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
// the two device calls on one core: csrc/epnp.h with a team of one
#include <stdint.h>
#include "epnp.h"
static int check(const EpnpSet& S, const double pose[12], int n, const float* err) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += epnp_inlier(pose, S.p3d[3 * i], S.p3d[3 * i + 1], S.p3d[3 * i + 2], S.p2d[2 * i], S.p2d[2 * i + 1], S.fu, S.fv, S.uc, S.vc, err[i]);
    return c;
}
extern "C" void cpu_pnp(int nprob, const int* n, const int* nh, const float* const* p3d, const float* const* p2d, const float* const* err, const double* K,
                        const int32_t* const* quads, const uint32_t* const* subset, int32_t* const* counts, int32_t* refined) {
    static EpnpWork W;
    const EpnpTeam T = {0, 1};
    for (int p = 0; p < nprob; ++p) {
        EpnpSet S;
        S.p3d = p3d[p]; S.p2d = p2d[p]; S.fu = K[0]; S.fv = K[1]; S.uc = K[2]; S.vc = K[3];
        double pose[12];
        if (quads) {
            for (int h = 0; h < nh[p]; ++h) {
                S.quad = quads[p] + 4 * h; S.mask = 0; S.span = 4; S.nc = 4; S.first = 0;
                epnp_compute_pose(T, &W, S, pose);
                counts[p][h] = check(S, pose, n[p], err[p]);
            }
        } else {
            S.quad = 0; S.mask = subset[p]; S.span = n[p]; S.nc = 0; S.first = -1;
            for (int i = 0; i < n[p]; ++i)
                if ((S.mask[i >> 5] >> (i & 31)) & 1u) { if (S.first < 0) S.first = i; ++S.nc; }
            epnp_compute_pose(T, &W, S, pose);
            refined[p] = check(S, pose, n[p], err[p]);
        }
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_pnp.json"))
    a = ap.parse_args()
    from weiner_slamit_v2_amd import api, synth

    if api.device_count() < 1:
        raise SystemExit("bench_pnp: no HIP device")
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    L = api.lib()
    res = {"workload": "slamit_pnp_ransac_batch, then slamit_pnp_refine_batch on each candidate's true matches (70 % of n): one C call each, host pointers",
           "comparator": "csrc/epnp.h compiled with g++ -O3, one core (this tool's source)", "measured_on": "MI355X (device calls), the same host (one core)",
           "reps": a.reps, "warmup": a.warmup, "cases": []}
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    for nprob, nh, n in [(1, 35, 100), (8, 35, 100), (32, 35, 100), (1, 35, 1000), (8, 35, 1000), (32, 35, 1000), (1, 300, 100), (1, 300, 1000)]:
        probs = []
        for k in range(nprob):
            pr = synth.synth_pnp(n, 0.3, 600 + k, 0.5)
            rs = np.random.RandomState(k)
            pr["quads"] = api.PnPsolver.sample_quads(n, nh, lambda lo, hi: int(rs.randint(lo, hi + 1)))
            probs.append(pr)
        got = api.PnPsolver.ransac(probs)
        subsets = []                            # Refine() sees the inliers of a good hypothesis: here the true matches of the scene
        for pr in probs:
            f = np.zeros(((n + 31) // 32) * 32, np.uint8)
            f[:n] = ~pr["true"]["bad"]
            subsets.append(np.ascontiguousarray(np.packbits(f, bitorder="little").view(np.uint32)))
        ref = api.PnPsolver.refine([dict(pr, subset_bits=s) for pr, s in zip(probs, subsets)])
        # the bare C calls, arrays prepared once (what the C++ shim pays)
        P, R = (api.PnpProblem * nprob)(), (api.PnpResult * nprob)()
        Q, S = (api.PnpRefineProblem * nprob)(), (api.PnpRefineResult * nprob)()
        keep = []
        for i, pr in enumerate(probs):
            o = (np.zeros((nh, 12)), np.zeros(nh, np.int32), np.zeros((nh, (n + 31) // 32), np.uint32), np.zeros((n + 31) // 32, np.uint32))
            keep.append(o)
            for X in (P[i], Q[i]):
                X.n, X.p3d, X.p2d, X.max_err = n, pr["p3d"].ctypes.data, pr["p2d"].ctypes.data, pr["max_err"].ctypes.data
                X.intr = (C.c_double * 4)(*pr["intr"])
            P[i].n_hyp, P[i].quads = nh, pr["quads"].ctypes.data
            Q[i].subset_bits = subsets[i].ctypes.data
            R[i].pose, R[i].n_inliers, R[i].inlier_bits = o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data
            S[i].inlier_bits = o[3].ctypes.data
        hyp_ms, hyp_min = median_ms(lambda: L.slamit_pnp_ransac_batch(0, nprob, P, R), a.warmup, a.reps)
        ref_ms, ref_min = median_ms(lambda: L.slamit_pnp_refine_batch(0, nprob, Q, S), a.warmup, a.reps)
        # the same header on one core
        arr = lambda ct, xs: (ct * nprob)(*xs)   # noqa: E731
        counts, refined = [np.zeros(nh, np.int32) for _ in range(nprob)], np.zeros(nprob, np.int32)
        base = [nprob, arr(C.c_int, [n] * nprob), arr(C.c_int, [nh] * nprob)]
        for key in ("p3d", "p2d", "max_err"):
            base.append(arr(fp, [pr[key].ctypes.data_as(fp) for pr in probs]))
        base.append(np.asarray(probs[0]["intr"], np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        quads, masks = arr(ip, [pr["quads"].ctypes.data_as(ip) for pr in probs]), arr(up, [s.ctypes.data_as(up) for s in subsets])
        cnts = arr(ip, [c.ctypes.data_as(ip) for c in counts])
        few = max(5, a.reps // 5)
        cpu_hyp_ms, _ = median_ms(lambda: port.cpu_pnp(*(base + [quads, None, cnts, refined.ctypes.data_as(ip)])), 2, few)
        cpu_ref_ms, _ = median_ms(lambda: port.cpu_pnp(*(base + [None, masks, cnts, refined.ctypes.data_as(ip)])), 2, few)
        same = all(np.array_equal(c, g["n_inliers"]) for c, g in zip(counts, got)) and all(int(r["n_inliers"]) == int(x) for r, x in zip(ref, refined))
        res["cases"].append({"candidates": nprob, "hypotheses": nh, "n": n,
                             "hypotheses_c_call_ms_median": hyp_ms, "hypotheses_c_call_ms_min": hyp_min, "hypotheses_cpu_header_ms_median": cpu_hyp_ms,
                             "refine_c_call_ms_median": ref_ms, "refine_c_call_ms_min": ref_min, "refine_cpu_header_ms_median": cpu_ref_ms,
                             "both_launches_ms_median": hyp_ms + ref_ms, "cpu_header_both_ms_median": cpu_hyp_ms + cpu_ref_ms,
                             "counts_equal_cpu_header": bool(same)})
        del keep
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
