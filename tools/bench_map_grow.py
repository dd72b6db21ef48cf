#!/usr/bin/env python3
"""Time the resident map-growth call against what a caller does without it.

Workload: eight maps of 200 keyframes x 1,000 keypoints, 40,000 points each with five observers.  One keyframe per map: NEW_KF (1,000
keypoints, 400 of them tracked points) + ASSOCIATE + candidate pairs with the new keyframe, about half of them accepted.  Two lists: (i) 600
pairs, (ii) a hundred times as many, 60,000 pairs, in one call.
  (a) slamit_map_grow_batch_dev, one call over the eight maps: HIP events around the call, median of --reps after --warmup with the
      10th-90th percentile spread; the arrays the call writes are put back outside the events.
  (b) csrc/map_grow.h's sequential form under g++ -O3 on one core, the eight maps one after the other.
  (c) (b) plus the upload of the tables the walk changed (every appendable array: a caller without the call rebuilds and uploads them
      whole, the way api.MapIndex puts a table on the device).
All three in the same run; the results (every array) are compared before anything is reported.

  python3 tools/bench_map_grow.py [--reps 30] [--warmup 5] [--out profiles/r37_map_grow.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LISTS = (("pairs_600", 600), ("pairs_60000", 60000))
N_KF, N_KP, N_MP, N_OBS = 200, 1000, 40000, 5


def make_fixture(seed, n_pairs):
    from tests.map_grow_fixtures import fixture, frame, op
    from tests.map_grow_ref import ASSOCIATE, NEW_KF, NEW_POINT, RECENT

    rng = np.random.RandomState(seed)
    p = np.repeat(np.arange(N_MP), N_OBS)
    kf = (p * 7 + np.tile(np.arange(N_OBS), N_MP) * 37) % N_KF           # five different keyframes per point, 1,000 observations per keyframe
    order = np.argsort(kf, kind="stable")
    idx = np.empty(len(kf), np.int64)
    idx[order] = np.tile(np.arange(N_KP), N_KF)
    kf_mp = np.empty(N_KF * N_KP, np.int32)
    kf_mp[kf * N_KP + idx] = p
    octave = rng.randint(0, 8, N_KF * N_KP).astype(np.uint8)
    f32 = lambda *s: rng.randn(*s).astype(np.float32)
    t = {"n_kf": N_KF, "n_mp": N_MP, "kf_mp_ptr": (np.arange(N_KF + 1) * N_KP).astype(np.int32), "kf_mp": kf_mp, "kf_octave": octave,
         "kf_desc": rng.randint(0, 256, (N_KF * N_KP, 32)).astype(np.uint8), "kf_depth": f32(N_KF * N_KP), "kf_bad": np.zeros(N_KF, np.uint8),
         "kf_parent": np.arange(-1, N_KF - 1, dtype=np.int32), "kf_to_be_erased": np.zeros(N_KF, np.uint8), "kf_not_erase": np.zeros(N_KF, np.uint8),
         "kf_th_depth": np.full(N_KF, 35.0, np.float32), "kf_best": np.full((N_KF, 10), -1, np.int32), "cw_n": np.zeros(N_KF, np.int32), "ord_n": np.zeros(N_KF, np.int32),
         "kf_child_ptr": np.minimum(np.arange(N_KF + 1), N_KF - 1).astype(np.int32), "kf_child": np.arange(1, N_KF, dtype=np.int32), "kf_center": f32(N_KF, 3),
         "mp_pos": f32(N_MP, 3), "mp_normal": f32(N_MP, 3), "mp_max_dist": f32(N_MP), "mp_min_dist": f32(N_MP), "mp_bad": (rng.rand(N_MP) < 0.02).astype(np.uint8),
         "mp_nobs": np.full(N_MP, N_OBS, np.int32), "mp_ref_kf": kf[::N_OBS].astype(np.int32), "mp_found": np.ones(N_MP, np.int32), "mp_visible": np.ones(N_MP, np.int32),
         "mp_first_kf": kf[::N_OBS].astype(np.int32), "mp_replaced": np.full(N_MP, -1, np.int32), "mp_desc": rng.randint(0, 256, (N_MP, 32)).astype(np.uint8),
         "obs_ptr": (np.arange(N_MP + 1) * N_OBS).astype(np.int32), "obs_kf": kf.astype(np.int32), "obs_idx": idx.astype(np.int32),
         "obs_octave": octave[kf * N_KP + idx], "obs_weight": np.ones(len(kf), np.uint8)}
    fm = np.full(N_KP, -1, np.int32)
    tracked = rng.permutation(N_KP)[:400]
    fm[tracked] = rng.permutation(N_MP)[:400]
    free = np.flatnonzero(fm == -1)
    ops = [op(NEW_KF, kf=N_KF, src=0, kf_id=N_KF), op(ASSOCIATE, kf=N_KF, src=0)]
    for i in range(n_pairs):
        ops.append(op(NEW_POINT, flags=RECENT, kf=N_KF, kf_id=N_KF, kf_a=N_KF, idx_a=int(free[i % len(free)]), kf_b=int(rng.randint(N_KF)), idx_b=int(rng.randint(N_KP)), cand=i))
    return fixture("bench", t, [frame(fm.tolist(), seed)], ops, cand_status=(rng.rand(n_pairs) < 0.5).astype(np.uint8) * 3)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "reps": len(a)}


def cpu_run(jobs, reps):
    from tests import map_grow_host as host

    exe = host.host_exe(False, "-O3")
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "bench_in.bin"), os.path.join(d, "bench_out.bin")
    open(pin, "wb").write(b"".join(host.job_bytes(fx, caps) for fx, caps in jobs))
    lines = subprocess.check_output([exe, pin, pout, str(reps)]).decode().split("\n")
    per = [[float(v) for v in ln.split()] for ln in lines if ln.strip()]
    assert len(per) == len(jobs)
    return sum(p[0] for p in per), sum(p[1] for p in per), host.parse(open(pout, "rb").read(), jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tests import map_grow_host as host
    from weiner_slamit_v2_amd import api

    n_maps = 8
    result = {"workload": {"maps": n_maps, "keyframes": N_KF, "keypoints_per_keyframe": N_KP, "points": N_MP, "observers_per_point": N_OBS}, "lists": {}}
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    for label, n_pairs in LISTS:
        fxs = [make_fixture(100 + m, n_pairs) for m in range(n_maps)]
        caps = [host.default_caps(fx, pad=0, cap_pad=0) for fx in fxs]
        ins = [host.inputs(fx, c) for fx, c in zip(fxs, caps)]
        names = [k for k, _, _ in host.INDEX]
        dev = [{k: cu(v) for k, v in x.items() if k in names + ["obs_kf"]} for x in ins]
        saved = [{k: v.clone() for k, v in d.items()} for d in dev]
        frames = [{k: cu(v) for k, v in fx["frames"][0].items() if k != "th_depth"} for fx in fxs]
        frame_recs = [api.grow_frame_rec(dict(f, th_depth=fx["frames"][0]["th_depth"])) for f, fx in zip(frames, fxs)]
        map_recs, grow_recs = [], []
        for fx, d, c in zip(fxs, dev, caps):
            mr = api.MapIndexRec(N_KF, N_MP)
            mr.obs_kf, mr.obs_ptr = d["obs_kf"].data_ptr(), d["obs_ptr"].data_ptr()
            map_recs.append(mr)
            grow_recs.append(api.grow_index_rec(d, c["kf_cap"], c["mp_cap"], c["kfmp_cap"]))
        h = np.stack([host.records(fx["ops"]).view(np.uint8).reshape(-1, host.OP_DTYPE.itemsize) for fx in fxs])
        for m in range(n_maps):
            h[m].view(host.OP_DTYPE)["src"][:2] = m                        # every map's own frame record
        stack = lambda key: cu(np.stack([x[key] for x in ins]))
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
        mp_cap = caps[0]["mp_cap"]
        tt = {"ops": cu(h), "n": torch.full((n_maps,), h.shape[1], dtype=torch.int32, device="cuda"), "cand_status": stack("cand_status"), "cand_x3d": stack("cand_x3d"),
              "op_status": stack("op_status"), "edits": stack("edits").reshape(n_maps, caps[0]["edit_cap"], 24), "n_edits_out": i32(n_maps), "recent": stack("recent"),
              "n_recent": i32(n_maps), "n_new": i32(n_maps), "need": i32(n_maps, api.GROW_NEEDS), "status": i32(n_maps), "mp_cap": mp_cap,
              "workspace": torch.zeros(api.map_grow_workspace(n_maps, mp_cap), dtype=torch.uint8, device="cuda")}
        stream = torch.cuda.current_stream()
        ms = []
        for r in range(a.warmup + a.reps):
            for d, sv in zip(dev, saved):
                for k in d:
                    d[k].copy_(sv[k])
            tt["n_recent"].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            api.map_grow_batch_dev(map_recs, grow_recs, frame_recs, tt, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        assert not tt["status"].any().item()
        entry = {"pairs_per_map": n_pairs, "accepted_per_map": [int(v) for v in tt["n_new"].cpu()], "edits_per_map": [int(v) for v in tt["n_edits_out"].cpu()],
                 "device": stats(ms), "workspace_bytes": int(tt["workspace"].numel())}
        med, best, outs = cpu_run(list(zip(fxs, caps)), max(5, a.reps))
        for m, (out, d) in enumerate(zip(outs, dev)):
            assert out["status"] == 0 and out["n_new"] == int(tt["n_new"][m]) and out["n_edits_out"] == int(tt["n_edits_out"][m]) and out["n_recent"] == int(tt["n_recent"][m])
            for k in names:
                assert np.array_equal(d[k].cpu().numpy().reshape(-1).view(np.uint8), out[k].view(np.uint8)), (label, m, k)
            for k in ("op_status", "edits", "recent"):
                assert np.array_equal(tt[k][m].cpu().numpy().reshape(-1), out[k]), (label, m, k)
        hosts = [[out[k] for k in names] + [out["edits"], out["recent"]] for out in outs]
        up = []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            keep = [[torch.from_numpy(v).to("cuda:0") for v in hm] for hm in hosts]
            torch.cuda.synchronize()
            if r >= a.warmup:
                up.append((time.perf_counter() - t_0) * 1e3)
            del keep
        entry["upload"] = dict(stats(up), bytes=int(sum(v.nbytes for hm in hosts for v in hm)))
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
