#!/usr/bin/env python3
"""Bit parity of two builds of the library on the Levenberg paths (pose, Sim3, local BA).

    SLAMIT_LIB=<build A> python3 tools/lm_parity.py dump a.npz        # one fresh process per build
    SLAMIT_LIB=<build B> python3 tools/lm_parity.py dump b.npz
    python3 tools/lm_parity.py compare a.npz b.npz [--out parity.json]

`dump` solves every pose_*, sim3_* and ba_* golden and the synthetic batches of tests/test_gpu_pose.py and tests/test_gpu_sim3.py and
stores every output (states, flags, iteration counts, per-round chi2, the BA's lambda and trial sequences).  `compare` reports, per
case, whether all of them are identical bit for bit (np.array_equal on the raw bytes: NaN and -0 count as themselves), and the largest
deviation where they are not; exit status 1 when a case differs."""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cases():
    from tests.helpers import load_ba_golden, load_pose_golden, load_sim3_golden
    from weiner_slamit_v2_amd import api, synth
    gold = lambda pat: sorted(glob.glob(os.path.join(ROOT, "tests", "golden", pat)))
    out = {}

    def put(tag, res, keys):
        for k in keys:
            out["%s/%s" % (tag, k)] = np.asarray(res[k])

    pose_keys = ("pose", "outlier", "n_inliers", "n_its", "chi2")
    for p in gold("pose_*.npz"):
        put("pose_golden:" + os.path.basename(p)[5:-4], api.Optimizer.PoseOptimization(load_pose_golden(p)[0]), pose_keys)
    batches = {
        "pose_batch": [synth.synth_pose(100 + 150 * i, 0.1 + 0.05 * i, 60 + i, 0.02 + 0.01 * i) for i in range(8)],
        "pose_mixed": [synth.synth_pose(200 + 100 * i, 0.1 + 0.04 * i, 80 + i, 0.02 + 0.01 * i, stereo_frac=(0.0, 1.0, 0.5, 0.8, 0.0, 0.3)[i]) for i in range(6)],
        "pose_full64": [synth.synth_pose(1000, 0.25, 100 + (i % 4), 0.04) for i in range(64)],
    }
    for name, probs in batches.items():
        for i, r in enumerate(api.Optimizer.PoseOptimization(probs)):
            put("%s[%d]" % (name, i), r, pose_keys)
    sim3_keys = ("r12", "t12", "s12", "inlier", "n_inliers", "n_its", "chi2")
    for p in gold("sim3_*.npz"):
        put("sim3_golden:" + os.path.basename(p)[5:-4], api.Optimizer.OptimizeSim3(load_sim3_golden(p)[0]), sim3_keys)
    probs = [synth.synth_sim3(int(30 + 61 * (s % 7)), 0.08 * (s % 5), 100 + s, 0.02 + 0.015 * (s % 4), fix_scale=(s % 6 == 0)) for s in range(24)]
    for i, r in enumerate(api.Optimizer.OptimizeSim3(probs)):
        put("sim3_batch[%d]" % i, r, sim3_keys)
    put("sim3_true", api.Optimizer.OptimizeSim3(synth.synth_sim3(400, 0.2, 5, 0.05)), sim3_keys)
    put("sim3_nine", api.Optimizer.OptimizeSim3(synth.synth_sim3(9, 0.0, 4)), sim3_keys)
    opt = api.Optimizer(max_kf=64, max_pt=2048, max_edge=110000, max_batch=4)
    for p in gold("ba_*.npz"):
        prob, ref = load_ba_golden(p)
        res = opt.LocalBundleAdjustment(prob, *ref.get("schedule", (5, 10, api.HUBER_MONO)))
        tag = "ba_golden:" + os.path.basename(p)[3:-4]
        put(tag, res, ("kf_pose", "pt_xyz", "edge_chi2", "edge_outlier", "edge_stage1_outlier"))
        st = res["stats"]
        out[tag + "/n_its"] = np.asarray(st["n_its"])
        for s in range(2):
            for k in ("chi2", "lambda", "trials"):
                out["%s/%s%d" % (tag, k, s)] = np.asarray(st[k][s])
        out[tag + "/chi2_init"] = np.asarray(st["chi2_init"], np.float64)
    return out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(pa, pb, out_path):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    cases = {}
    for key in sorted(a.files):
        tag, field = key.rsplit("/", 1)
        c = cases.setdefault(tag, {"identical": True, "differs": {}})
        if not _same(a[key], b[key]):
            c["identical"] = False
            x, y = a[key].astype(np.float64), b[key].astype(np.float64)
            c["differs"][field] = float(np.nanmax(np.abs(x - y))) if x.shape == y.shape and x.size else "shape"
    groups = {}
    for tag, c in cases.items():
        g = groups.setdefault(tag.split(":")[0].split("[")[0], {"cases": 0, "identical": 0})
        g["cases"] += 1
        g["identical"] += c["identical"]
    doc = {"arrays": len(a.files), "groups": groups, "all_identical": all(c["identical"] for c in cases.values()),
           "cases": {t: (True if c["identical"] else c["differs"]) for t, c in sorted(cases.items())}}
    txt = json.dumps(doc, indent=1, sort_keys=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(txt + "\n")
    print(json.dumps({"groups": groups, "all_identical": doc["all_identical"],
                      "differing": {t: c["differs"] for t, c in cases.items() if not c["identical"]}}))
    return 0 if doc["all_identical"] else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        np.savez(sys.argv[2], **_cases())
        sys.exit(0)
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None))
    sys.exit(__doc__)
