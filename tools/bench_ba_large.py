"""Times map-sized bundle adjustment on one slamit_ba_create_ex handle (max_free_kf = 341) and prints one JSON line: per window (the
large-BA test windows, tests/test_gpu_ba_large.py) ms per solve, LM trials and iterations per second, the phase times of a profiled solve
(slamit_ba_profile), and the CPU oracle's time for the same solve on this host as a comparator (one core, dense LDLt).

    python tools/bench_ba_large.py [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weiner_slamit_v2_amd import api, synth  # noqa: E402

LOCAL, GLOBAL = (5, 10, api.HUBER_MONO), (10, 0, float(np.float32(np.sqrt(5.99))))
WINDOWS = {
    "fixed150": (dict(n_kf=170, n_pt=2000, obs_per_pt=6, n_fixed=150, seed=11), LOCAL),
    "free90": (dict(n_kf=150, n_pt=1500, obs_per_pt=6, n_fixed=60, seed=13), LOCAL),
    "sparse100": (dict(n_kf=100, n_pt=1000, obs_per_pt=2, n_fixed=1, seed=1), LOCAL),
    "global150": (dict(n_kf=150, n_pt=1500, obs_per_pt=6, n_fixed=1, seed=14), GLOBAL),
    "global300": (dict(n_kf=300, n_pt=3000, obs_per_pt=6, n_fixed=1, seed=15), GLOBAL),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", nargs="*", default=None, help="these windows only (a profiling run)")
    a = ap.parse_args()
    opt = api.Optimizer(max_kf=342, max_pt=3200, max_edge=24000, max_batch=1, max_free_kf=341)
    out = {"metric": "ba_large", "reps": a.reps, "windows": {}}
    for name, (kw, sched) in WINDOWS.items():
        if a.only and name not in a.only:
            continue
        prob = synth.synth_map(**kw)
        run = lambda: opt.LocalBundleAdjustment(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2])
        r = run()   # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = run()
            ts.append((time.perf_counter() - t0) * 1e3)
        trials = int(sum(sum(t) for t in r["stats"]["trials"]))
        its = int(sum(r["stats"]["n_its"]))
        opt.profile(True)
        run()
        prof = opt.profile_read()
        opt.profile(False)
        ms = float(np.median(ts))
        rec = {"n_kf": kw["n_kf"], "n_free": kw["n_kf"] - kw["n_fixed"], "nS": 6 * (kw["n_kf"] - kw["n_fixed"]), "n_edge": len(prob["edge_kf"]),
               "ms_per_solve": round(ms, 3), "ms_min": round(min(ts), 3), "lm_its": its, "lm_trials": trials,
               "lm_it_per_s": round(its / ms * 1e3, 1), "ms_per_trial": round(ms / max(trials, 1), 3),
               "phase_ms": {k: round(v, 3) for k, v in prof["phase_ms"].items()}, "slots": prof["slots"]}
        if not a.no_cpu:
            from oracle import bindings as ob
            t0 = time.perf_counter()
            ob.ba_solve(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2])
            rec["cpu_oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["windows"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
