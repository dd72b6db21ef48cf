#!/usr/bin/env python3
"""Time slamit_map_edit_batch_dev against the two other ways to get the same tables.

Workload: the maps of tools/bench_upkeep.py -- 8 maps x 200 keyframes x about 1,140 keypoints, 40,000 points each -- with SPARE free
keypoints appended to every keyframe's row, for adds.  One keyframe of local mapping is taken to produce, per map, ADDS observations of
points its neighbours see (ProcessNewKeyFrame, CreateNewMapPoints, Fuse: ADD_OBS | MATCH), ERASES outlier observations (local BA:
ERASE_OBS | MATCH) and CULLS culled points (MapPointCulling: SET_BAD), in shuffled order.  Two lists are timed: that one, and one 100
times as long (the same recipe over 100 keyframes).  Three routes to the new tables:
  (a) slamit_map_edit_batch_dev, one call over the eight maps: HIP events around the call after --warmup calls, the in-place arrays put
      back before every call outside the events; median of --reps with the minimum and the 10th / 90th percentiles;
  (b) the same walk, me_apply_seq of csrc/map_edit.h, under g++ -O3 on one core, the eight maps one after the other;
  (c) what the library offered before: the host rebuilds the tables -- taken at (b)'s time, which favours this route: a host that keeps
      objects has to flatten them as well -- and uploads every table the edits changed the way api.MapIndex does (one host-to-device copy
      per table, then a synchronisation).
(a)'s results are compared with (b)'s, every array, before anything is reported.

  python3 tools/bench_map_edit.py [--reps 30] [--warmup 5] [--no-cpu] [--out profiles/r26_map_edit.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
SPARE, ADDS, ERASES, CULLS = 700, 600, 60, 40
CHANGED = (("obs_ptr", np.int32), ("obs_kf", np.int32), ("obs_idx", np.int32), ("obs_octave", np.uint8), ("obs_weight", np.uint8), ("mp_bad", np.uint8),
           ("mp_nobs", np.int32), ("mp_ref_kf", np.int32), ("kf_mp", np.int32))


def with_spare(t):
    """Every keyframe's row with SPARE free keypoints at its end; obs_idx stays what it was."""
    n_kf, old = t["n_kf"], t["kf_mp_ptr"]
    ptr = (old + SPARE * np.arange(n_kf + 1)).astype(np.int32)
    kf_mp = np.full(ptr[-1], -1, np.int32)
    for k in range(n_kf):
        kf_mp[ptr[k]:ptr[k] + old[k + 1] - old[k]] = t["kf_mp"][old[k]:old[k + 1]]
    return dict(t, kf_mp_ptr=ptr, kf_mp=kf_mp)


def edits_of(t, x, keyframes, rng):
    from weiner_slamit_v2_amd import api

    rows = []
    old_len = np.diff(t["kf_mp_ptr"]) - SPARE
    for k in keyframes:
        mine = t["kf_mp"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k] + old_len[k]]
        near = np.concatenate([t["kf_mp"][t["kf_mp_ptr"][j]:t["kf_mp_ptr"][j] + old_len[j]] for j in range(max(k - 3, 0), min(k + 4, t["n_kf"])) if j != k])
        cand = np.setdiff1d(near, mine)
        for j, p in enumerate(rng.permutation(cand)[:ADDS]):
            rows.append((api.EDIT_ADD_OBS, api.EDIT_MATCH, int(p), int(k), int(old_len[k] + j), int(rng.integers(0, 8)), 1))
        for p in rng.permutation(mine)[:ERASES]:
            rows.append((api.EDIT_ERASE_OBS, api.EDIT_MATCH, int(p), int(k), 0, 0, 0))
        for p in rng.permutation(mine)[ERASES:ERASES + CULLS]:
            rows.append((api.EDIT_SET_BAD, 0, int(p), 0, 0, 0, 0))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return api.edit_records(rows)


CPU_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "map_edit.h"
template <typename T> static std::vector<T> rd(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v((size_t)n + 1);
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) exit(2);
    v.resize((size_t)n);
    return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v, size_t n) { fwrite(v.data(), sizeof(T), n, f); }
struct Map {
    std::vector<int32_t> h, obs_ptr, obs_kf, kf_mp_ptr, kf_mp, obs_idx, mp_nobs, mp_ref_kf;
    std::vector<uint8_t> mp_bad, obs_octave, obs_weight;
    std::vector<MeEdit> edits;
};
int main(int argc, char** argv) {
    if (argc != 4) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    const int reps = atoi(argv[3]);
    std::vector<int32_t> head = rd<int32_t>(f);   // maps
    std::vector<Map> maps(head[0]);
    for (Map& A : maps) {
        A.h = rd<int32_t>(f);                      // n_kf n_mp obs_cap_out
        A.obs_ptr = rd<int32_t>(f); A.obs_kf = rd<int32_t>(f); A.kf_mp_ptr = rd<int32_t>(f); A.kf_mp = rd<int32_t>(f); A.mp_bad = rd<uint8_t>(f);
        A.obs_idx = rd<int32_t>(f); A.obs_octave = rd<uint8_t>(f); A.obs_weight = rd<uint8_t>(f); A.mp_nobs = rd<int32_t>(f); A.mp_ref_kf = rd<int32_t>(f);
        A.edits = rd<MeEdit>(f);
    }
    fclose(f);
    std::vector<double> ms;
    FILE* o = fopen(argv[2], "wb");
    for (int r = 0; r < reps; ++r) {
        double total = 0;
        for (Map& A : maps) {
            std::vector<int32_t> kf_mp = A.kf_mp, mp_nobs = A.mp_nobs, mp_ref_kf = A.mp_ref_kf;   // the in-place arrays, fresh
            std::vector<uint8_t> mp_bad = A.mp_bad;
            const size_t cap = (size_t)A.h[2], n_mp = (size_t)A.h[1];
            std::vector<int32_t> optr(n_mp + 1), okf(cap + 1), oidx(cap + 1), status_mp(n_mp + 1), touched(n_mp + 1), bucket(A.edits.size() + 1), start(n_mp + 2), stamp(kf_mp.size() + 1);
            std::vector<uint8_t> ooct(cap + 1), owgt(cap + 1);
            int32_t tail[3] = {0, 0, 0};
            LmMap M = LmMap();
            MeIndex X = MeIndex();
            M.n_kf = A.h[0]; M.n_mp = A.h[1]; M.obs_ptr = A.obs_ptr.data(); M.obs_kf = A.obs_kf.data(); M.kf_mp_ptr = A.kf_mp_ptr.data();
            X.obs_idx = A.obs_idx.data(); X.obs_octave = A.obs_octave.data(); X.obs_weight = A.obs_weight.data();
            X.mp_bad = mp_bad.data(); X.mp_nobs = mp_nobs.data(); X.mp_ref_kf = mp_ref_kf.data(); X.kf_mp = kf_mp.data();
            X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
            X.obs_cap_out = A.h[2];
            auto t0 = std::chrono::steady_clock::now();
            me_apply_seq(M, X, (int)A.edits.size(), A.edits.data(), status_mp.data(), touched.data(), &tail[0], &tail[1], &tail[2], bucket.data(), start.data(), stamp.data());
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r == 0) {
                const size_t need = (size_t)tail[1], nt = (size_t)tail[0];
                fwrite(tail, 4, 3, o);
                wr(o, optr, n_mp + 1); wr(o, okf, need); wr(o, oidx, need); wr(o, ooct, need); wr(o, owgt, need);
                wr(o, mp_bad, n_mp); wr(o, mp_nobs, n_mp); wr(o, mp_ref_kf, n_mp); wr(o, kf_mp, kf_mp.size()); wr(o, status_mp, n_mp); wr(o, touched, nt);
            }
        }
        ms.push_back(total);
    }
    fclose(o);
    std::sort(ms.begin(), ms.end());
    printf("%.6f %.6f\n", ms[ms.size() / 2], ms[0]);
    return 0;
}
"""


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return np.int32(len(a)).tobytes() + a.tobytes()


def cpu_run(maps, lists, caps, reps):
    """-> (median ms, min ms, per map the arrays in the order the driver writes them)."""
    d = tempfile.mkdtemp(prefix="bench_map_edit_")
    src, exe, pin, pout = (os.path.join(d, n) for n in ("cpu.cc", "cpu", "in.bin", "out.bin"))
    open(src, "w").write(CPU_DRIVER)
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), src, "-o", exe])
    blob = _arr([len(maps)], np.int32)
    for (t, x), ed, cap in zip(maps, lists, caps):
        blob += _arr([t["n_kf"], t["n_mp"], cap], np.int32)
        for key, dt, s in (("obs_ptr", np.int32, t), ("obs_kf", np.int32, t), ("kf_mp_ptr", np.int32, t), ("kf_mp", np.int32, t), ("mp_bad", np.uint8, t),
                           ("obs_idx", np.int32, x), ("obs_octave", np.uint8, x), ("obs_weight", np.uint8, x), ("mp_nobs", np.int32, x), ("mp_ref_kf", np.int32, x)):
            blob += _arr(s[key], dt)
        blob += np.int32(len(ed)).tobytes() + ed.tobytes()
    open(pin, "wb").write(blob)
    med, best = (float(v) for v in subprocess.check_output([exe, pin, pout, str(reps)]).split())
    raw, o, outs = open(pout, "rb").read(), 0, []
    for (t, x) in maps:
        nt, need, st = np.frombuffer(raw, np.int32, 3, o)
        o += 12
        n_mp, n_kfmp = t["n_mp"], len(t["kf_mp"])
        out = {"n_touched": int(nt), "n_obs_out": int(need), "status": int(st)}
        for key, dt, count in (("obs_ptr", np.int32, n_mp + 1), ("obs_kf", np.int32, need), ("obs_idx", np.int32, need), ("obs_octave", np.uint8, need), ("obs_weight", np.uint8, need),
                               ("mp_bad", np.uint8, n_mp), ("mp_nobs", np.int32, n_mp), ("mp_ref_kf", np.int32, n_mp), ("kf_mp", np.int32, n_kfmp), ("status_mp", np.int32, n_mp),
                               ("touched", np.int32, nt)):
            out[key] = np.frombuffer(raw, dt, int(count), o).copy()
            o += out[key].nbytes
        outs.append(out)
    assert o == len(raw)
    return med, best, outs


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "reps": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bench_upkeep import N_MAPS, make_map
    from weiner_slamit_v2_amd import api

    maps = []
    for m in range(N_MAPS):
        t, x, _ = make_map(500 + m)
        x = dict(x, obs_weight=np.ones(len(t["obs_kf"]), np.uint8), mp_nobs=np.diff(t["obs_ptr"]).astype(np.int32))
        maps.append((with_spare(t), x))
    result = {"workload": {"maps": N_MAPS, "keyframes": maps[0][0]["n_kf"], "points": maps[0][0]["n_mp"], "observations": int(len(maps[0][0]["obs_kf"])),
                           "kf_mp_entries": int(len(maps[0][0]["kf_mp"])), "per_keyframe": {"adds": ADDS, "erases": ERASES, "set_bad": CULLS}}, "lists": {}}
    for label, n_keyframes in (("one_keyframe", 1), ("hundred_keyframes", 100)):
        rng = np.random.default_rng(77 + n_keyframes)
        lists = [edits_of(t, x, np.arange(5, 5 + n_keyframes), rng) for t, x in maps]
        caps = [len(t["obs_kf"]) + len(ed) for (t, x), ed in zip(maps, lists)]
        mis = [api.MapIndex(t) for t, _ in maps]
        eis = [api.EditIndex(x, mi, cap) for (_, x), mi, cap in zip(maps, mis, caps)]
        saved = [{k: ei.t[k].clone() for k in ("mp_bad", "mp_nobs", "mp_ref_kf", "kf_mp")} for ei in eis]
        cap, mp_cap, kfmp_cap = max(len(ed) for ed in lists), maps[0][0]["n_mp"], max(len(t["kf_mp"]) for t, _ in maps)
        h = np.zeros((N_MAPS, cap, 24), np.uint8)
        for m, ed in enumerate(lists):
            h[m, :len(ed)] = ed.view(np.uint8).reshape(-1, 24)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
        tt = {"edits": torch.from_numpy(h).cuda(), "n": torch.tensor([len(ed) for ed in lists], dtype=torch.int32, device="cuda"), "status_mp": i32(N_MAPS, mp_cap),
              "touched": i32(N_MAPS, mp_cap), "n_touched": i32(N_MAPS), "n_obs_out": i32(N_MAPS), "status": i32(N_MAPS), "kfmp_cap": kfmp_cap,
              "workspace": torch.zeros(api.map_edit_workspace(N_MAPS, cap, mp_cap, kfmp_cap), dtype=torch.uint8, device="cuda")}
        stream = torch.cuda.current_stream()
        ms = []
        for r in range(a.warmup + a.reps):
            for ei, sv in zip(eis, saved):
                for k, v in sv.items():
                    ei.t[k].copy_(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            api.map_edit_batch_dev(mis, eis, tt, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        entry = {"edits_per_map": [int(len(ed)) for ed in lists], "device": stats(ms), "workspace_bytes": int(tt["workspace"].numel())}
        assert not tt["status"].any().item()
        # (c)'s upload: the tables the edits changed, the way api.MapIndex puts a table on the device
        up = []
        host = [{k: np.ascontiguousarray((x if k in x else t)[k], dt).reshape(-1) for k, dt in CHANGED} for t, x in maps]
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = [[torch.from_numpy(v).to("cuda:0") for v in hm.values()] for hm in host]
            torch.cuda.synchronize()
            if r >= a.warmup:
                up.append((time.perf_counter() - t0) * 1e3)
            del keep
        entry["upload"] = dict(stats(up), bytes=int(sum(v.nbytes for hm in host for v in hm.values())), tables=[k for k, _ in CHANGED])
        if not a.no_cpu:
            med, best, outs = cpu_run(maps, lists, caps, max(3, a.reps // 3))
            for m, (out, ei, (t, x)) in enumerate(zip(outs, eis, maps)):
                need, nt, n_mp = out["n_obs_out"], out["n_touched"], t["n_mp"]
                assert int(tt["n_obs_out"][m]) == need and int(tt["n_touched"][m]) == nt and out["status"] == 0
                for key, got in (("obs_ptr", ei.sets[1]["obs_ptr"][:n_mp + 1]), ("obs_kf", ei.sets[1]["obs_kf"][:need]), ("obs_idx", ei.sets[1]["obs_idx"][:need]),
                                 ("obs_octave", ei.sets[1]["obs_octave"][:need]), ("obs_weight", ei.sets[1]["obs_weight"][:need]), ("mp_bad", ei.t["mp_bad"][:n_mp]),
                                 ("mp_nobs", ei.t["mp_nobs"][:n_mp]), ("mp_ref_kf", ei.t["mp_ref_kf"][:n_mp]), ("kf_mp", ei.t["kf_mp"][:len(t["kf_mp"])]),
                                 ("status_mp", tt["status_mp"][m, :n_mp]), ("touched", tt["touched"][m, :nt])):
                    assert np.array_equal(got.cpu().numpy(), out[key]), (label, m, key)
            entry["cpu_one_core"] = {"median_ms": med, "min_ms": best}
            entry["rebuild_and_upload_ms"] = med + entry["upload"]["median_ms"]
            entry["results_equal"] = True
        result["lists"][label] = entry
        print(label, json.dumps(entry))
    if a.out:
        json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
