"""Times Optimizer::OptimizeEssentialGraph on the device: the resident call (api.essential_graph_dev: problem, result and workspace on
the device, what a caller with a resident map pays) at 64, 256 and 1,024 free keyframes on a ring with covisibility edges and a
closing loop, against the numpy restatement (tests/essential_ref.py) on the host and, where oracle/_ref holds the harness
(tools/gen_essential_golden.py built it), the reference's g2o on one core.

    python tools/bench_essential.py [--reps 5] [--warmup 1] [--out profiles/r36_essential.json]

Warm-up calls first, then the median of the repetitions (wall clock around the synchronous call).  No time here is a pass criterion:
the dense factor is expected to lose to g2o's sparse one at the large end, and the file records what was measured.  A run without a
device fails; there is no fall-back."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36_essential.json"))
    ap.add_argument("--sizes", default="64,256,1024")
    a = ap.parse_args()
    import torch

    from tests import essential_ref as er
    from tests.essential_host import dev_result, dev_tensors
    from weiner_slamit_v2_amd import api, synth

    ref = None
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libeg_ref.so")):
        import gen_essential_golden as gg

        L = C.CDLL(gg.LIB)
        L.eg_ref_solve.argtypes = [C.POINTER(api.EgProblem), C.POINTER(api.EgResult), C.c_void_p]
        ref = lambda g: gg.ref_solve(L, g)
    rows = []
    for nf in [int(s) for s in a.sizes.split(",")]:
        g = synth.synth_essential(n_kf=nf + 1, seed=21, drift=0.001, scale_drift=0.002, n_pt=4 * nf)
        g.update(api.essential_plan(g))
        t, n_free = dev_tensors(g)
        st = torch.cuda.Stream()

        def dev():
            api.essential_graph_dev(t, n_free, int(g["fix_scale"]), int(g["max_its"]), float(g["lambda_init"]), stream=st.cuda_stream)
            st.synchronize()

        dev()
        r = dev_result(t)
        row = dict(free_keyframes=nf, unknowns=7 * nf, edges=len(g["edge_v0"]), points=4 * nf, n_its=r["n_its"], trials=int(r["n_trials"]),
                   workspace_MB=round(api.essential_graph_workspace(n_free, nf + 1, len(g["edge_v0"]), 4 * nf) / 1e6, 1))
        row["device_resident_ms"], row["device_resident_min_ms"] = median_ms(dev, a.warmup, a.reps)
        row["device_ms_per_trial"] = row["device_resident_ms"] / max(row["trials"], 1)
        row["host_form_ms"], _ = median_ms(lambda: api.essential_graph(g), a.warmup, max(a.reps // 2, 1))
        t0 = time.perf_counter()
        w = er.optimize(g)
        row["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        row["numpy_trials"] = int(len(w["trial_rho"]))
        # where each implementation ends: chi2 of its corrected Sim3s on ONE evaluator (the restatement's), and the device's failed pivots
        key = ("sim3_r", "sim3_t", "sim3_s")
        row["chi2_start"] = er.cost(g, g["scw_r"], g["scw_t"], g["scw_s"])
        row["device_final_chi2"] = er.cost(g, *[r[k] for k in key])
        row["numpy_final_chi2"] = er.cost(g, *[w[k] for k in key])
        row["device_failed_pivots"] = int((r["trial_chi2"] >= np.finfo(np.float64).max).sum())
        row["device_trials_per_iteration"] = [int(v) for v in r["trials"]]
        row["numpy_trials_per_iteration"] = [int(v) for v in w["trials"]]
        if ref:
            q = ref(g)
            row["g2o_one_core_ms"], _ = median_ms(lambda: ref(g), 0, 3)
            row["g2o_trials"] = int(q["n_trials"])
            row["g2o_final_chi2"] = er.cost(g, *[q[k] for k in key])
            row["g2o_trials_per_iteration"] = [int(v) for v in q["trials"]]
            row["g2o_failed_solves"] = int(q["trial_failed"].sum())
            row["worst_rel_vs_g2o"] = float(max(np.abs(r[k] - q[k]).max() / np.abs(q[k]).max() for k in ("sim3_r", "sim3_t", "sim3_s", "pose")))
        print(row)
        rows.append(row)
    out = dict(what="Optimizer::OptimizeEssentialGraph: resident device call vs the numpy restatement and the reference's g2o on one core; recorded, not gated",
               device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
