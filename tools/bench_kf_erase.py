#!/usr/bin/env python3
"""Time the resident KeyFrame::SetBadFlag call against what a caller does without it.

Workload: the eight maps of tools/bench_covis.py -- 200 keyframes x about 1,000 keypoints, 40,000 points each -- with every keyframe in
the graph and a spanning tree that hangs a keyframe under its best covisible keyframe of smaller slot.  Two lists per map: (i) one
keyframe culled, (ii) ten.
  (a) slamit_kf_erase_batch_dev, one call over the eight maps: HIP events around the call, median of --reps after --warmup with the
      10th-90th percentile spread; the in-place arrays are put back outside the events.
  (b) csrc/kf_erase.h's sequential form under g++ -O3 on one core, the eight maps one after the other.
  (c) (b) plus the upload of the tables the walk changed (kf_bad, kf_parent, kf_to_be_erased, the seven graph arrays, the children
      table, the emitted edits), the way api.MapIndex puts a table on the device.
All three in the same run; the results (every array) are compared before anything is reported.

  python3 tools/bench_kf_erase.py [--reps 30] [--warmup 5] [--no-cpu] [--out profiles/r29_kf_erase.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LISTS = (("one_keyframe", [100]), ("ten_keyframes", [40 + 12 * i for i in range(10)]))
CHANGED = ("kf_bad", "kf_parent", "kf_to_be_erased", "cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best", "child_ptr_out", "child_out", "edits")


def make_fixture(seed, ks):
    """A bench_covis map with every keyframe in the graph, a spanning tree, and SET_BAD ops for ks."""
    import bench_covis

    t, x, absent = bench_covis.make_map(seed)
    n_kf, rc = t["n_kf"], x["row_cap"]
    # the keyframes bench_covis leaves out of the graph: their rows from the tables, as UpdateConnections would have left them
    W = np.zeros((n_kf, n_kf), np.int32)
    who = t["obs_kf"].reshape(t["n_mp"], -1)[t["mp_bad"] == 0]
    for a in range(who.shape[1]):
        for b in range(who.shape[1]):
            if a != b:
                np.add.at(W, (who[:, a], who[:, b]), 1)
    for k in range(n_kf):
        nb = np.flatnonzero(W[k])
        srt = nb[np.lexsort((-nb, -W[k, nb]))]
        assert len(nb) <= rc
        x["cw_n"][k] = x["ord_n"][k] = len(nb)
        x["cw_kf"][k, :len(nb)], x["cw_w"][k, :len(nb)] = nb, W[k, nb]
        x["ord_kf"][k, :len(nb)], x["ord_w"][k, :len(nb)] = srt, W[k, srt]
        x["kf_best"][k] = -1
        x["kf_best"][k, :min(10, len(nb))] = srt[:10]
    parent = np.full(n_kf, -1, np.int32)
    for k in range(1, n_kf):
        below = [j for j in x["ord_kf"][k, :x["ord_n"][k]] if j < k]
        parent[k] = below[0] if below else k - 1
    rows = [[c for c in range(n_kf) if parent[c] == k] for k in range(n_kf)]
    t = dict(t, kf_parent=parent, kf_child_ptr=np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), kf_child=np.array([c for r in rows for c in r], np.int32),
             kf_best=x["kf_best"])
    x = dict(x, kf_to_be_erased=np.zeros(n_kf, np.uint8))
    return {"name": "bench", "t": t, "x": x, "ops": [(2, int(k), -1) for k in ks]}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "reps": len(a)}


def cpu_run(jobs, reps):
    """-> (the sum over the maps of the median walk, of the fastest, per map the arrays the header leaves)."""
    from tests import kf_erase_host as host

    exe = host.host_exe(False, "-O3")
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "bench_in.bin"), os.path.join(d, "bench_out.bin")
    open(pin, "wb").write(b"".join(host.job_bytes(fx, cc, ec) for fx, cc, ec in jobs))
    lines = subprocess.check_output([exe, pin, pout, str(reps)]).decode().split("\n")
    per = [[float(v) for v in ln.split()] for ln in lines if ln.strip()]
    assert len(per) == len(jobs)
    return sum(p[0] for p in per), sum(p[1] for p in per), host.parse(open(pout, "rb").read(), jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tests import kf_erase_host as host
    from weiner_slamit_v2_amd import api

    n_maps = 8
    result = {"lists": {}}
    for label, ks in LISTS:
        fxs = [make_fixture(100 + m, ks) for m in range(n_maps)]
        t0, x0 = fxs[0]["t"], fxs[0]["x"]
        result["workload"] = {"maps": n_maps, "keyframes": t0["n_kf"], "points": t0["n_mp"], "kf_mp_entries": int(len(t0["kf_mp"])), "row_cap": int(x0["row_cap"]),
                              "graph_entries": int(x0["cw_n"].sum()), "children_entries": int(len(t0["kf_child"]))}
        caps = [host.default_caps(fx) for fx in fxs]
        edit_cap = max(c[1] for c in caps)
        caps = [(c[0], edit_cap) for c in caps]
        mis = [api.MapIndex(fx["t"]) for fx in fxs]
        cis = [api.CovisIndex({k: v for k, v in fx["x"].items() if k != "kf_to_be_erased"}, mi) for fx, mi in zip(fxs, mis)]
        tis = [api.TreeIndex(fx["x"], mi, ci, cc) for fx, mi, ci, (cc, _) in zip(fxs, mis, cis, caps)]
        inplace = [[mi.t["kf_bad"], mi.t["kf_parent"], ti.t["kf_to_be_erased"]] + [ci.t[k] for k in api.COVIS_GRAPH] for mi, ci, ti in zip(mis, cis, tis)]
        saved = [[v.clone() for v in arrs] for arrs in inplace]
        cap, kf_cap, row_cap = len(ks), t0["n_kf"], int(x0["row_cap"])
        child_cap = max(len(fx["t"]["kf_child"]) for fx in fxs)
        h = np.zeros((n_maps, cap, 16), np.uint8)
        for m, fx in enumerate(fxs):
            h[m] = host.records(fx["ops"]).view(np.uint8).reshape(-1, 16)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
        tt = {"ops": torch.from_numpy(h).cuda(), "n": torch.full((n_maps,), cap, dtype=torch.int32, device="cuda"), "op_status": i32(n_maps, cap),
              "edits": torch.zeros((n_maps, edit_cap, 24), dtype=torch.uint8, device="cuda"), "n_edits_out": i32(n_maps), "n_child_out": i32(n_maps), "status": i32(n_maps),
              "kf_cap": kf_cap, "row_cap": row_cap, "child_cap": child_cap,
              "workspace": torch.zeros(api.kf_erase_workspace(n_maps, cap, kf_cap, row_cap, child_cap), dtype=torch.uint8, device="cuda")}
        stream = torch.cuda.current_stream()
        ms = []
        for r in range(a.warmup + a.reps):
            for arrs, sv in zip(inplace, saved):
                for v, s in zip(arrs, sv):
                    v.copy_(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            api.kf_erase_batch_dev(mis, tis, tt, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        assert not tt["status"].any().item() and not tt["op_status"].any().item()
        entry = {"keyframes_per_map": len(ks), "edits_per_map": [int(v) for v in tt["n_edits_out"].cpu()], "device": stats(ms), "workspace_bytes": int(tt["workspace"].numel())}
        if not a.no_cpu:
            med, best, outs = cpu_run([(fx, cc, ec) for fx, (cc, ec) in zip(fxs, caps)], max(5, a.reps))
            for m, (out, fx, mi, ci, ti) in enumerate(zip(outs, fxs, mis, cis, tis)):
                n_kf, rc, need, ne = fx["t"]["n_kf"], fx["x"]["row_cap"], out["n_child_out"], out["n_edits_out"]
                assert out["status"] == 0 and int(tt["n_child_out"][m]) == need and int(tt["n_edits_out"][m]) == ne
                got = {"child_ptr_out": ti.sets[1]["kf_child_ptr"][:n_kf + 1], "child_out": ti.sets[1]["kf_child"][:need], "kf_bad": mi.t["kf_bad"][:n_kf],
                       "kf_parent": mi.t["kf_parent"][:n_kf], "kf_to_be_erased": ti.t["kf_to_be_erased"][:n_kf], "kf_best": mi.t["kf_best"][:n_kf * 10],
                       "op_status": tt["op_status"][m], "edits": tt["edits"][m].reshape(-1)[:ne * 24]}
                for key in ("cw_kf", "cw_w", "ord_kf", "ord_w"):
                    got[key] = ci.t[key][:n_kf * rc]
                for key in ("cw_n", "ord_n"):
                    got[key] = ci.t[key][:n_kf]
                for key, v in got.items():
                    assert np.array_equal(v.cpu().numpy().reshape(-1), out[key][:v.numel()]), (label, m, key)
            # (c)'s upload: the tables the walk changed, the way api.MapIndex puts a table on the device
            hosts = [[np.ascontiguousarray(out[k][:out["n_child_out"]] if k == "child_out" else out[k][:out["n_edits_out"] * 24] if k == "edits" else out[k]) for k in CHANGED]
                     for out in outs]
            up = []
            for r in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t_0 = time.perf_counter()
                keep = [[torch.from_numpy(v).to("cuda:0") for v in hm] for hm in hosts]
                torch.cuda.synchronize()
                if r >= a.warmup:
                    up.append((time.perf_counter() - t_0) * 1e3)
                del keep
            entry["upload"] = dict(stats(up), bytes=int(sum(v.nbytes for hm in hosts for v in hm)), tables=list(CHANGED))
            entry["cpu_one_core"] = {"median_ms": med, "min_ms": best}
            entry["walk_and_upload_ms"] = med + entry["upload"]["median_ms"]
            entry["results_equal"] = True
            entry["resident_beats_walk_and_upload"] = bool(entry["device"]["median_ms"] < entry["walk_and_upload_ms"])
            entry["resident_beats_walk_alone"] = bool(entry["device"]["median_ms"] < med)
        result["lists"][label] = entry
        print(label, json.dumps(entry))
    if a.out:
        json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
