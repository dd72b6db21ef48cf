"""Times slamit_guided_search_batch_dev with and without the right-image gate on the shape
profiles/r10_search_resolve.json used for the batch form: 64 frames of n = 1000 keypoints and m = 1000 queries, kp_cap 2048, q_cap 3072.

  parent      the old symbol of a library built from the parent commit (--parent-lib; skipped without it)
  head        the old symbol of this tree's library: the monocular instantiation of the kernels
  head_radius slamit_guided_search_stereo_batch_dev, SLAMIT_SEARCH_ER_RADIUS, on synth_search_stereo's mvuRight / q_ur for the same frames

    python tools/bench_search_stereo.py [--parent-lib PATH] [--rounds 9] [--launches 20] [--warmup 3] [--out profiles/r18_search_stereo.json]

The variants alternate within a round (parent, head, head_radius, parent, ...), every figure is device-event time around `launches`
back-to-back calls divided by their number, and a variant's result is the median over the rounds with its minimum and maximum.  The
monocular answer of the two libraries must be bit-equal, or the tool fails.  `within_parent_spread`: |head - parent| <= the parent's
own max - min.  The RADIUS time is recorded, not bounded."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, M, KP_CAP, Q_CAP = 64, 1000, 1000, 2048, 3072


def tensors(torch, api, problems):
    kps = np.zeros((B, KP_CAP), api.KP_DTYPE)
    t = dict(n=np.zeros(B, np.int32), desc=np.zeros((B, KP_CAP, 32), np.uint8), kp_taken=np.zeros((B, KP_CAP), np.uint8), m=np.zeros(B, np.int32),
             uvr=np.zeros((B, Q_CAP, 3), np.float32), level_min=np.zeros((B, Q_CAP), np.int32), level_max=np.zeros((B, Q_CAP), np.int32),
             qdesc=np.zeros((B, Q_CAP, 32), np.uint8), valid=np.zeros((B, Q_CAP), np.uint8), takes=np.ones((B, Q_CAP), np.uint8),
             kp_ur=np.full((B, KP_CAP), -1, np.float32), q_ur=np.zeros((B, Q_CAP), np.float32))
    for i, (f, q, st) in enumerate(problems):
        n, m = len(f["kp_xy"]), len(q["uvr"])
        t["n"][i], t["m"][i] = n, m
        kps["x"][i, :n], kps["y"][i, :n], kps["octave"][i, :n] = f["kp_xy"][:, 0], f["kp_xy"][:, 1], f["kp_octave"]
        t["desc"][i, :n], t["kp_taken"][i, :n] = f["desc"], f["kp_taken"]
        t["uvr"][i, :m], t["level_min"][i, :m], t["level_max"][i, :m] = q["uvr"], q["level_min"], q["level_max"]
        t["qdesc"][i, :m], t["valid"][i, :m], t["takes"][i, :m] = q["desc"], q["valid"], q["takes"]
        t["kp_ur"][i, :n], t["q_ur"][i, :m] = st["kp_ur"], st["q_ur"]
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, KP_CAP, 7)).cuda()
    d["match_kp"] = torch.full((B, Q_CAP), -7, dtype=torch.int32, device="cuda")
    d["nmatches"] = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    d["out4"] = torch.zeros((B, Q_CAP, 4), dtype=torch.int32, device="cuda")
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, Q_CAP), dtype=torch.uint8, device="cuda")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_search_stereo: no GPU (there is no CPU path to time)")
    distinct = [synth.synth_search_stereo(N, M, 100 + i, er_mode=1, displaced_frac=0.1) for i in range(8)]   # 8 distinct frames, each 8 times
    problems = [distinct[i % 8] for i in range(B)]
    bounds = tuple(float(problems[0][0][k]) for k in ("min_x", "min_y", "inv_w", "inv_h"))
    d = tensors(torch, api, problems)
    sb = api.SearchBatch(B, KP_CAP, Q_CAP, d["n"].data_ptr(), d["kps_un"].data_ptr(), d["desc"].data_ptr(), d["kp_taken"].data_ptr(), *bounds,
                         d["m"].data_ptr(), d["uvr"].data_ptr(), d["level_min"].data_ptr(), d["level_max"].data_ptr(), d["qdesc"].data_ptr(),
                         d["valid"].data_ptr(), d["takes"].data_ptr())
    rule = api._search_rule(100, True, 0.8)
    st = api.SearchStereoDev(api.SEARCH_ER_RADIUS, 7.8, d["kp_ur"].data_ptr(), d["q_ur"].data_ptr(), 1)
    stream = torch.cuda.Stream()
    outs = (d["match_kp"].data_ptr(), d["nmatches"].data_ptr(), d["out4"].data_ptr(), d["workspace"].data_ptr(), d["workspace"].numel(), stream.cuda_stream)
    head = api.lib()
    vp, sz = C.c_void_p, C.c_size_t
    variants = {}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.slamit_guided_search_batch_dev.argtypes = [C.c_int, C.POINTER(api.SearchBatch), C.POINTER(api.SearchRule), vp, vp, vp, vp, sz, vp]
        variants["parent"] = lambda: parent.slamit_guided_search_batch_dev(0, C.byref(sb), C.byref(rule), *outs)
    variants["head"] = lambda: head.slamit_guided_search_batch_dev(0, C.byref(sb), C.byref(rule), *outs)
    variants["head_radius"] = lambda: head.slamit_guided_search_stereo_batch_dev(0, C.byref(sb), C.byref(rule), C.byref(st), *outs)

    answers = {}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            if fn() != 0:
                raise SystemExit("bench_search_stereo: %s failed" % name)
        stream.synchronize()
        answers[name] = (d["match_kp"].cpu().numpy().copy(), d["nmatches"].cpu().numpy().copy())
    if "parent" in answers and not (np.array_equal(answers["parent"][0], answers["head"][0]) and np.array_equal(answers["parent"][1], answers["head"][1])):
        raise SystemExit("bench_search_stereo: the monocular answers of the two libraries differ")
    runs = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.launches):
                fn()
            e1.record(stream)
            stream.synchronize()
            runs[name].append(e0.elapsed_time(e1) / a.launches)
    res = {"what": "slamit_guided_search_batch_dev, %d frames x n = %d keypoints x m = %d queries (kp_cap %d, q_cap %d), ms per call of the whole batch; "
                   "%d rounds alternating the variants, %d back-to-back calls between two device events per round" % (B, N, M, KP_CAP, Q_CAP, a.rounds, a.launches),
           "matches": {name: int(v[1].sum()) for name, v in answers.items()}}
    for name, r in runs.items():
        res[name] = {"median_ms": round(float(np.median(r)), 4), "min_ms": round(float(np.min(r)), 4), "max_ms": round(float(np.max(r)), 4),
                     "runs_ms": [round(float(x), 4) for x in r]}
    if "parent" in runs:
        spread = res["parent"]["max_ms"] - res["parent"]["min_ms"]
        res["parent_spread_ms"] = round(spread, 4)
        res["within_parent_spread"] = bool(abs(res["head"]["median_ms"] - res["parent"]["median_ms"]) <= spread)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
