"""Times the vocabulary transform (slamit_voc_transform_batch_dev) on a vocabulary of the ORB file's shape: k = 10, L = 6, a full tree of
1,111,110 nodes with random centroids and random positive weights (the real ORBvoc.txt is not needed: the work per descriptor depends on
the shape alone), 1000 and 2000 random descriptors per frame, 1 and 256 frames.

    python tools/bench_bow.py [--reps 30] [--warmup 5] [--out profiles/r11_bow_transform.json]

Device events around `reps` back-to-back calls on one stream, after `warmup` calls of the same shape; the outputs of every shape are first
compared with the host-pointer form frame by frame.  Three variants per shape split the time: descent only (no output pair), descent +
BowVector, descent + both vectors.  The bytes are the ones the descent algorithmically reads, n x sum over levels of fan-out x 32 B,
set against the 8.6 TB/s at which random rows of a 38 MB table are gathered through the Infinity Cache (the lane groups also read
8 B of child links per centroid, not counted).  Recorded, not gated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L = 10, 6
GATHER_TBS = 8.6   # 38 MB table, uniformly random rows, served from the Infinity Cache


def orb_shaped_vocabulary(seed=0):
    """The array form, nodes numbered breadth first."""
    rs = np.random.RandomState(seed)
    sizes = [K ** l for l in range(1, L + 1)]
    starts = np.concatenate([[1], 1 + np.cumsum(sizes)])          # first id of level 1 .. L (+ the end)
    parent = np.concatenate([np.zeros(K, np.int64)] + [starts[l - 1] + np.arange(sizes[l]) // K for l in range(1, L)]).astype(np.int32)
    n = len(parent)
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[starts[L - 1] - 1:] = 1
    desc = rs.randint(0, 256, (n, 32)).astype(np.uint8)
    weight = rs.uniform(0.1, 12.0, n)
    return parent, is_leaf, desc, weight


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_bow_transform.json"))
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api

    if api.device_count() < 1:
        raise SystemExit("bench_bow: no HIP device (there is no CPU path to time)")
    parent, is_leaf, desc, weight = orb_shaped_vocabulary()
    voc = api.ORBVocabulary.from_arrays(K, L, parent, is_leaf, desc, weight)
    info = voc.info()
    table_mb = (info["n_nodes"] + 1) * 32 / 1e6
    res = {"workload": "slamit_voc_transform_batch_dev, k = 10, L = 6 full tree (%d nodes, %d words, %.1f MB of centroids), random descriptors, levelsup 4"
                       % (info["n_nodes"], info["n_words"], table_mb),
           "timing": "device events around reps back-to-back calls on one stream, after warmup calls of the same shape",
           "reps": a.reps, "warmup": a.warmup, "gather_rate_TBs_reference": GATHER_TBS, "cases": []}
    rs = np.random.RandomState(1)
    for n in (1000, 2000):
        for nframes in (1, 256):
            cap = n
            q = rs.randint(0, 256, (nframes, cap, 32)).astype(np.uint8)
            i32 = dict(dtype=torch.int32, device="cuda")
            t = {"desc": torch.from_numpy(q).cuda(), "n": torch.full((nframes,), n, **i32), "word_id": torch.zeros((nframes, cap), **i32),
                 "node_id": torch.zeros((nframes, cap), **i32), "workspace": torch.zeros(voc.transform_workspace(nframes, cap), dtype=torch.uint8, device="cuda"),
                 "bow_n": torch.zeros(nframes, **i32), "bow_word": torch.zeros((nframes, cap), **i32),
                 "bow_value": torch.zeros((nframes, cap), dtype=torch.float64, device="cuda"), "fv_n": torch.zeros(nframes, **i32),
                 "fv_node": torch.zeros((nframes, cap), **i32), "fv_ptr": torch.zeros((nframes, cap + 1), **i32), "fv_items": torch.zeros((nframes, cap), **i32)}
            s = torch.cuda.Stream()
            variants = {"descent": {k: v for k, v in t.items() if not k.startswith(("bow_", "fv_"))},
                        "descent_bow": {k: v for k, v in t.items() if not k.startswith("fv_")}, "full": t}
            ms = {}
            for name, tv in variants.items():
                for _ in range(a.warmup):
                    voc.transform_batch_dev(tv, 4, stream=s.cuda_stream)
                s.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(s):
                    e0.record()
                    for _ in range(a.reps):
                        voc.transform_batch_dev(tv, 4, stream=s.cuda_stream)
                    e1.record()
                s.synchronize()
                ms[name] = e0.elapsed_time(e1) / a.reps
            # the timed outputs against the host-pointer form, on the first and the last frame
            same = True
            for f in sorted({0, nframes - 1}):
                one = voc.transform(q[f, :n], 4)
                nb, nf = int(t["bow_n"][f]), int(t["fv_n"][f])
                same &= np.array_equal(t["word_id"][f, :n].cpu().numpy(), one["word_id"]) and nb == len(one["bow_word"]) and nf == len(one["fv_node"])
                same &= np.array_equal(t["bow_value"][f, :nb].cpu().numpy().view(np.uint64), one["bow_value"].view(np.uint64))
                same &= np.array_equal(t["fv_items"][f, :n].cpu().numpy()[:len(one["fv_items"])], one["fv_items"])
            nd = n * nframes
            gather_bytes = nd * L * K * 32
            res["cases"].append({
                "descriptors_per_frame": n, "frames": nframes, "ms_per_call": ms["full"], "us_per_frame": 1e3 * ms["full"] / nframes,
                "descriptors_per_second": nd / (ms["full"] * 1e-3), "ms_descent_only": ms["descent"], "ms_bowvector_pass": ms["descent_bow"] - ms["descent"],
                "ms_featurevector_pass": ms["full"] - ms["descent_bow"], "descent_gather_bytes": gather_bytes,
                "descent_gather_TBs": gather_bytes / (ms["descent"] * 1e-3) / 1e12, "descent_share_of_gather_rate": gather_bytes / (ms["descent"] * 1e-3) / 1e12 / GATHER_TBS,
                "unique_words_frame0": int(t["bow_n"][0]), "equals_host_form": bool(same)})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
