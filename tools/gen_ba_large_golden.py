"""Writes tests/golden/ba_large_ref.json.gz: map-sized BA windows (synth.synth_map) solved by the reference's own g2o
(oracle/_ref/libba_ref.so, which build() makes where the reference source exists).  Per window: the synth_map arguments and the
schedule, CRC32s of the problem's arrays, and the result -- every pose, a seeded sample of points, both outlier flag sets (packed
bits), the LM path (iterations, trials, chi2 and lambda per iteration) and the stage start costs.  Float64 values are stored as
base64 of their little-endian bytes (exact, and the fixture stays small).

HARD windows (synth.synth_map_hard: mirrored observations of points on the far side of the circle, a free keyframe whose
observations are all gross outliers) go to a sibling file, tests/golden/ba_large_hard_ref.json.gz, with their post-processing
arguments ("hard"), the mirrored edges' indices and every pose between the two stages ("kf_pose_stage1").

    python tools/gen_ba_large_golden.py
"""
import base64
import gzip
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bindings as ob  # noqa: E402
from weiner_slamit_v2_amd import api, synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ba_large_ref.json.gz")
LOCAL = [5, 10, api.HUBER_MONO]                         # Optimizer.cc:660, :707, :569
GLOBAL = [10, 0, float(np.float32(np.sqrt(5.99)))]      # BundleAdjustment(nIterations = 10, bRobust), Optimizer.cc:143
# name -> synth_map arguments, schedule.  Rows of the reduced system nS = 6 n_free, Npad = rup(nS + 1, 64)
WINDOWS = {
    "fixed150": (dict(n_kf=170, n_pt=2000, obs_per_pt=6, n_fixed=150, seed=11), LOCAL),                     # 120 / 128
    "stereo_fixed70": (dict(n_kf=82, n_pt=900, obs_per_pt=6, n_fixed=70, seed=12, stereo_frac=0.5), LOCAL),  # 72 / 128
    "free90": (dict(n_kf=150, n_pt=1500, obs_per_pt=6, n_fixed=60, seed=13), LOCAL),                         # 540 / 576: tiled
    "sparse100": (dict(n_kf=100, n_pt=1000, obs_per_pt=2, n_fixed=1, seed=1), LOCAL),                        # 594 / 640: a narrow band, tiled
    "global150": (dict(n_kf=150, n_pt=1500, obs_per_pt=6, n_fixed=1, seed=14), GLOBAL),                      # 894 / 896: side table
    "global300": (dict(n_kf=300, n_pt=3000, obs_per_pt=6, n_fixed=1, seed=15), GLOBAL),                      # 1794 / 1856
}
OUT_HARD = os.path.join(ROOT, "tests", "golden", "ba_large_hard_ref.json.gz")
# name -> synth_map arguments, synth_map_hard's post-processing, schedule
HARD = {
    "starved100": (dict(n_kf=100, n_pt=1000, obs_per_pt=6, n_fixed=1, seed=21), dict(mirror=dict(n=60, seed=121), starve_kf=[[50, 124]]), LOCAL),   # 594 / 640: tiled
}
PROBLEM_KEYS = ("kf_pose", "kf_fixed", "kf_intr", "pt_xyz", "edge_kf", "edge_pt", "edge_uv", "edge_inv_sigma2", "edge_ur", "kf_bf")
N_SAMPLE = 300


def crcs(prob):
    return {k: zlib.crc32(np.ascontiguousarray(prob[k]).tobytes()) for k in PROBLEM_KEYS if k in prob}


def b64(a):
    return base64.b64encode(np.ascontiguousarray(a, "<f8").tobytes()).decode()


def point_sample(name, n_pt):
    return np.sort(np.random.RandomState(zlib.crc32(name.encode())).choice(n_pt, min(N_SAMPLE, n_pt), replace=False))


def solve_all(windows, out, what):
    cases = {}
    for name, spec in windows.items():
        kw, sched = spec[0], spec[-1]
        extra = {}
        if len(spec) == 3:
            prob, mirrored = synth.synth_map_hard(kw, **spec[1])
            extra = {"hard": spec[1], "mirror_edges": mirrored.tolist()}
        else:
            prob = synth.synth_map(**kw)
        r = ob.ba_ref_solve(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2], stage1=len(spec) == 3)
        if len(spec) == 3:
            extra["kf_pose_stage1"] = b64(r["kf_pose_stage1"])
            extra["mirror_edge_chi2"] = b64(r["edge_chi2"][mirrored])
        idx = point_sample(name, len(prob["pt_xyz"]))
        s = r["stats"]
        cases[name] = {
            **extra, "synth_map": kw, "schedule": sched, "crc32": crcs(prob),
            "kf_pose": b64(r["kf_pose"]), "pt_index": idx.tolist(), "pt_xyz": b64(r["pt_xyz"][idx]),
            "edge_outlier": base64.b64encode(np.packbits(r["edge_outlier"].astype(bool))).decode(),
            "edge_stage1_outlier": base64.b64encode(np.packbits(r["edge_stage1_outlier"].astype(bool))).decode(),
            "edge_chi2_near_gate": np.flatnonzero(np.abs(r["edge_chi2"] - 5.991) <= 1e-6 * 5.991).tolist(),
            "n_its": s["n_its"], "trials": s["trials"], "chi2": [b64(c) for c in s["chi2"]], "lambda": [b64(c) for c in s["lambda"]],
            "chi2_init": b64(s["chi2_init"]),
        }
        print(name, "its", s["n_its"], "trials", s["trials"], "outliers", int(r["edge_outlier"].sum()))
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"what": what, "cases": cases}, sort_keys=True).encode())
    print(out, os.path.getsize(out), "bytes")


def main():
    if not ob.ba_ref_available():
        raise SystemExit("oracle/_ref/libba_ref.so is not built (build() makes it where the reference source exists)")
    if "hard" not in sys.argv[1:]:   # (`hard`: only the sibling file)
        solve_all(WINDOWS, OUT, "map-sized BA windows solved by the reference's g2o (tools/gen_ba_large_golden.py)")
    solve_all(HARD, OUT_HARD, "map-sized BA windows with mirrored observations and a starved keyframe, solved by the reference's g2o "
                              "(tools/gen_ba_large_golden.py)")


if __name__ == "__main__":
    main()
