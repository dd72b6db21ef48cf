"""Times the two launches of the device Initializer: slamit_init_hyp_batch (200 hypotheses, H and F) and
slamit_init_reconstruct_batch for 1, 8, 64 and 256 frame pairs x {150, 1000} matches, separately and together, against
csrc/two_view.h itself on one host core (g++ -O3 of tests/initializer_driver.cc, the same header).

    python tools/bench_initializer.py [--reps 50] [--warmup 10] [--out profiles/r32_initializer.json]

Warm-up calls first, then the median of the repetitions (wall clock around the synchronous C call, host staging and both copies
included: that is what a caller pays).  The outputs of the first frame pair of every shape are asserted equal to the host build's.
A run without a device fails; there is no fall-back.  Recorded, not gated."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_initializer.json"))
    ap.add_argument("--batches", default="1,8,64,256")
    a = ap.parse_args()
    import ctypes as C

    from tests import initializer_ref as ref
    from weiner_slamit_v2_amd import api

    if api.device_count() < 1:
        raise SystemExit("bench_initializer: no HIP device")
    L = api.lib()
    d = tempfile.mkdtemp(prefix="bench_initializer_")
    exe = os.path.join(d, "host")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-I", ref.CSRC, ref.DRIVER, "-o", exe])
    rows = []
    for n in (150, 1000):
        scenes = [ref.scene("b", "general", n, 0.2, 200, 500 + s, (0.8, 0.3, 0.4)) for s in range(8)]
        # the host core: one frame pair, both passes (mode 2), by the difference of two repeat counts
        ref.write_problem(os.path.join(d, "in.bin"), scenes[0], 2)
        def host(rep):
            t0 = time.perf_counter()
            subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), str(rep)])
            return (time.perf_counter() - t0) * 1e3
        host(1)
        cpu_ms = float(np.median([(host(6) - host(1)) / 5 for _ in range(5)]))
        h_hyp, h_pick, h_reco = ref.host_run(scenes[0], 2, exe=exe)
        for nb in [int(x) for x in a.batches.split(",")]:
            probs = [scenes[i % len(scenes)] for i in range(nb)]
            hyps = api.init_hypotheses(probs)
            assert np.array_equal(hyps[0]["score"].view(np.uint32), h_hyp["score"].view(np.uint32)) and np.array_equal(hyps[0]["inlier_bits"], h_hyp["inlier_bits"])
            recos_in = []
            for pr, hy in zip(probs, hyps):
                sel = api.init_select(hy)
                kind = sel["kind"]
                b = sel["best_h"] if kind == api.INIT_H else sel["best_f"]
                recos_in.append(dict(pr, kind=kind, model=hy["model"][kind][b], subset_bits=hy["inlier_bits"][kind][b]))
            recos = api.init_reconstruct(recos_in)
            nm = len(recos[0]["n_good"])
            assert np.array_equal(recos[0]["status"], h_reco["status"][:nm]) and np.array_equal(recos[0]["n_good"], h_reco["n_good"][:nm])
            assert np.array_equal(recos[0]["points"].view(np.uint32), h_reco["points"][:nm].view(np.uint32))
            # the C calls alone: records and output arrays built once
            keep = []
            P, R = (api.InitProblem * nb)(), (api.InitResult * nb)()
            Q, S = (api.InitReconstructProblem * nb)(), (api.InitReconstructResult * nb)()
            for i, (pr, q) in enumerate(zip(probs, recos_in)):
                k, nn = api._init_frames(pr, P[i])
                sets = np.ascontiguousarray(pr["sets"], np.int32)
                w = (nn + 31) // 32
                o = [np.zeros((2, 200, 9), np.float32), np.zeros((2, 200), np.float32), np.zeros((2, 200), np.int32), np.zeros((2, 200, w), np.uint32)]
                P[i].n_hyp, P[i].sets = 200, sets.ctypes.data
                R[i].model, R[i].score, R[i].n_inliers, R[i].inlier_bits = (x.ctypes.data for x in o)
                k2, _ = api._init_frames(pr, Q[i])
                sub = np.ascontiguousarray(q["subset_bits"], np.uint32)
                Q[i].kind, Q[i].subset_bits = int(q["kind"]), sub.ctypes.data
                Q[i].model = (C.c_float * 9)(*[float(v) for v in q["model"]])
                Q[i].K = (C.c_float * 9)(*[float(v) for v in np.asarray(pr["K"], np.float32).reshape(9)])
                o2 = [np.zeros((8, nn), np.uint8), np.zeros((8, nn, 3), np.float32), np.zeros((8, w), np.uint32)]
                S[i].status, S[i].points, S[i].good_bits = (x.ctypes.data for x in o2)
                keep.append((k, k2, sets, sub, o, o2))
            def hyp_call():
                assert L.slamit_init_hyp_batch(0, nb, P, R) == 0
            def reco_call():
                assert L.slamit_init_reconstruct_batch(0, nb, Q, S) == 0
            def both():
                hyp_call()
                reco_call()
            row = {"n": n, "pairs": nb, "n_hyp": 200, "hyp_ms": median_ms(hyp_call, a.warmup, a.reps), "reconstruct_ms": median_ms(reco_call, a.warmup, a.reps),
                   "both_ms": median_ms(both, a.warmup, a.reps), "host_core_both_ms_per_pair": cpu_ms, "host_core_both_ms": cpu_ms * nb}
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = {"what": "Initializer: hypotheses + motions, device against one host core on the same header", "warmup": a.warmup, "reps": a.reps, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
