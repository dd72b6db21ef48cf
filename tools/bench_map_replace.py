#!/usr/bin/env python3
"""Time slamit_map_replace_batch_dev against the two other ways to get the same tables.

Workload: the maps of tools/bench_map_edit.py -- 8 maps x 200 keyframes x about 1,140 keypoints, 40,000 points each, SPARE free
keypoints at the end of every keyframe's row.  One Fuse pass of local mapping (SearchInNeighbors) is taken, per map, as REPLACES
Replace ops -- a point of one of the keyframe's 20 neighbours gives way to a point of the keyframe -- and ADDS AddObservation +
AddMapPoint ops of the keyframe's points into neighbours' free keypoints, in shuffled order.  Two lists are timed: that one, and the
longest list of whole passes the ceiling of SLAMIT_REPLACE_MAX_OPS admits (23 passes over 23 keyframes; a hundred passes are five
calls).  Three routes to the new tables:
  (a) slamit_map_replace_batch_dev, one call over the eight maps: HIP events around the call after --warmup calls, the in-place arrays
      put back before every call outside the events; median of --reps with the minimum and the 10th / 90th percentiles;
  (b) the same walk, mr_apply_seq of csrc/map_replace.h, under g++ -O3 on one core, the eight maps one after the other;
  (c) what the library offered before: the host walks the tables -- taken at (b)'s time -- and uploads every table the list changed the
      way api.MapIndex does (one host-to-device copy per table, then a synchronisation).
(a)'s results are compared with (b)'s, every array, before anything is reported.

  python3 tools/bench_map_replace.py [--reps 30] [--warmup 5] [--no-cpu] [--out profiles/r27_map_replace.json]"""
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
REPLACES, ADDS, NEIGHBOURS = 400, 300, 20
CHANGED = (("obs_ptr", np.int32), ("obs_kf", np.int32), ("obs_idx", np.int32), ("obs_octave", np.uint8), ("obs_weight", np.uint8), ("mp_bad", np.uint8),
           ("mp_nobs", np.int32), ("mp_found", np.int32), ("mp_visible", np.int32), ("mp_replaced", np.int32), ("kf_mp", np.int32))
INPLACE = ("mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "kf_mp")


def ops_of(t, keyframes, rng, spare):
    from weiner_slamit_v2_amd import api

    rows, used = [], {}
    old_len = np.diff(t["kf_mp_ptr"]) - spare
    row = lambda k: t["kf_mp"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k] + old_len[k]]
    for k in keyframes:
        mine = np.unique(row(k)[row(k) >= 0])
        nb = [j for j in range(max(k - NEIGHBOURS // 2, 0), min(k + NEIGHBOURS // 2 + 1, t["n_kf"])) if j != k]
        near = np.setdiff1d(np.concatenate([row(j) for j in nb]), np.concatenate([mine, [-1]]))
        for s, d in zip(rng.permutation(near)[:REPLACES], rng.permutation(mine)[:REPLACES]):
            rows.append((api.REPLACE_REPLACE, int(s), int(d), 0, 0, 0))
        for i, p in enumerate(rng.permutation(mine)[:ADDS]):
            j = nb[i % len(nb)]
            used[j] = used.get(j, 0) + 1
            assert used[j] <= spare
            rows.append((api.REPLACE_ADD_OBS, int(p), int(j), int(old_len[j] + used[j] - 1), int(rng.integers(0, 8)), 1))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return api.replace_records(rows)


CPU_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "map_replace.h"
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
    std::vector<int32_t> h, obs_ptr, obs_kf, kf_mp_ptr, kf_mp, obs_idx, mp_nobs, mp_found, mp_visible, mp_replaced;
    std::vector<uint8_t> mp_bad, obs_octave, obs_weight;
    std::vector<MrOp> ops;
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
        A.obs_idx = rd<int32_t>(f); A.obs_octave = rd<uint8_t>(f); A.obs_weight = rd<uint8_t>(f); A.mp_nobs = rd<int32_t>(f); A.mp_found = rd<int32_t>(f);
        A.mp_visible = rd<int32_t>(f); A.mp_replaced = rd<int32_t>(f);
        A.ops = rd<MrOp>(f);
    }
    fclose(f);
    std::vector<double> ms;
    FILE* o = fopen(argv[2], "wb");
    for (int r = 0; r < reps; ++r) {
        double total = 0;
        for (Map& A : maps) {
            std::vector<int32_t> kf_mp = A.kf_mp, mp_nobs = A.mp_nobs, mp_found = A.mp_found, mp_visible = A.mp_visible, mp_replaced = A.mp_replaced;   // the in-place arrays, fresh
            std::vector<uint8_t> mp_bad = A.mp_bad;
            const size_t cap = (size_t)A.h[2], n_mp = (size_t)A.h[1], n = A.ops.size();
            std::vector<int32_t> optr(n_mp + 1), okf(cap + 1), oidx(cap + 1), moved(n + 1), erased(n + 1), touched(n_mp + 1);
            std::vector<uint8_t> ooct(cap + 1), owgt(cap + 1);
            int32_t tail[3] = {0, 0, 0};
            LmMap M = LmMap();
            MrIndex X = MrIndex();
            M.n_kf = A.h[0]; M.n_mp = A.h[1]; M.obs_ptr = A.obs_ptr.data(); M.obs_kf = A.obs_kf.data(); M.kf_mp_ptr = A.kf_mp_ptr.data();
            X.obs_idx = A.obs_idx.data(); X.obs_octave = A.obs_octave.data(); X.obs_weight = A.obs_weight.data();
            X.mp_bad = mp_bad.data(); X.mp_nobs = mp_nobs.data(); X.mp_found = mp_found.data(); X.mp_visible = mp_visible.data(); X.mp_replaced = mp_replaced.data();
            X.kf_mp = kf_mp.data();
            X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
            X.obs_cap_out = A.h[2];
            auto t0 = std::chrono::steady_clock::now();
            mr_apply_seq(M, X, (int)n, A.ops.data(), moved.data(), erased.data(), touched.data(), &tail[0], &tail[1], &tail[2]);
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r == 0) {
                const size_t need = (size_t)tail[1], nt = (size_t)tail[0];
                fwrite(tail, 4, 3, o);
                wr(o, optr, n_mp + 1); wr(o, okf, need); wr(o, oidx, need); wr(o, ooct, need); wr(o, owgt, need);
                wr(o, mp_bad, n_mp); wr(o, mp_nobs, n_mp); wr(o, mp_found, n_mp); wr(o, mp_visible, n_mp); wr(o, mp_replaced, n_mp); wr(o, kf_mp, kf_mp.size());
                wr(o, moved, n); wr(o, erased, n); wr(o, touched, nt);
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
    d = tempfile.mkdtemp(prefix="bench_map_replace_")
    src, exe, pin, pout = (os.path.join(d, n) for n in ("cpu.cc", "cpu", "in.bin", "out.bin"))
    open(src, "w").write(CPU_DRIVER)
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), src, "-o", exe])
    blob = _arr([len(maps)], np.int32)
    for (t, x), ed, cap in zip(maps, lists, caps):
        blob += _arr([t["n_kf"], t["n_mp"], cap], np.int32)
        for key, dt, s in (("obs_ptr", np.int32, t), ("obs_kf", np.int32, t), ("kf_mp_ptr", np.int32, t), ("kf_mp", np.int32, t), ("mp_bad", np.uint8, t),
                           ("obs_idx", np.int32, x), ("obs_octave", np.uint8, x), ("obs_weight", np.uint8, x), ("mp_nobs", np.int32, x), ("mp_found", np.int32, x),
                           ("mp_visible", np.int32, x), ("mp_replaced", np.int32, x)):
            blob += _arr(s[key], dt)
        blob += np.int32(len(ed)).tobytes() + ed.tobytes()
    open(pin, "wb").write(blob)
    med, best = (float(v) for v in subprocess.check_output([exe, pin, pout, str(reps)]).split())
    raw, o, outs = open(pout, "rb").read(), 0, []
    for (t, x), ed in zip(maps, lists):
        nt, need, st = np.frombuffer(raw, np.int32, 3, o)
        o += 12
        n_mp, n_kfmp, n = t["n_mp"], len(t["kf_mp"]), len(ed)
        out = {"n_touched": int(nt), "n_obs_out": int(need), "status": int(st)}
        for key, dt, count in (("obs_ptr", np.int32, n_mp + 1), ("obs_kf", np.int32, need), ("obs_idx", np.int32, need), ("obs_octave", np.uint8, need), ("obs_weight", np.uint8, need),
                               ("mp_bad", np.uint8, n_mp), ("mp_nobs", np.int32, n_mp), ("mp_found", np.int32, n_mp), ("mp_visible", np.int32, n_mp),
                               ("mp_replaced", np.int32, n_mp), ("kf_mp", np.int32, n_kfmp), ("moved", np.int32, n), ("erased", np.int32, n), ("touched", np.int32, nt)):
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
    from bench_map_edit import SPARE, with_spare
    from bench_upkeep import N_MAPS, make_map
    from weiner_slamit_v2_amd import api

    maps = []
    for m in range(N_MAPS):
        t, x, _ = make_map(500 + m)
        n_mp = t["n_mp"]
        rng = np.random.default_rng(900 + m)
        x = dict(x, obs_weight=np.ones(len(t["obs_kf"]), np.uint8), mp_nobs=np.diff(t["obs_ptr"]).astype(np.int32), mp_found=rng.integers(0, 50, n_mp).astype(np.int32),
                 mp_visible=rng.integers(50, 100, n_mp).astype(np.int32), mp_replaced=np.full(n_mp, -1, np.int32))
        maps.append((with_spare(t), x))
    passes_max = api.REPLACE_MAX_OPS // (REPLACES + ADDS)
    result = {"workload": {"maps": N_MAPS, "keyframes": maps[0][0]["n_kf"], "points": maps[0][0]["n_mp"], "observations": int(len(maps[0][0]["obs_kf"])),
                           "kf_mp_entries": int(len(maps[0][0]["kf_mp"])), "per_pass": {"replace": REPLACES, "add_obs": ADDS, "neighbours": NEIGHBOURS}}, "lists": {}}
    for label, n_passes in (("one_pass", 1), ("%d_passes" % passes_max, passes_max)):
        rng = np.random.default_rng(77 + n_passes)
        lists = [ops_of(t, np.arange(15, 15 + n_passes), rng, SPARE) for t, x in maps]
        caps = [len(t["obs_kf"]) + int(np.count_nonzero(ed["kind"] == api.REPLACE_ADD_OBS)) for (t, x), ed in zip(maps, lists)]
        mis = [api.MapIndex(t) for t, _ in maps]
        eis = [api.EditIndex(x, mi, cap) for (_, x), mi, cap in zip(maps, mis, caps)]
        ris = [api.ReplaceIndex(ei, x) for (_, x), ei in zip(maps, eis)]
        tens = lambda ei, ri, k: (ri.t if k in ri.t else ei.t)[k]
        saved = [{k: tens(ei, ri, k).clone() for k in INPLACE} for ei, ri in zip(eis, ris)]
        cap, mp_cap, kfmp_cap = max(len(ed) for ed in lists), maps[0][0]["n_mp"], max(len(t["kf_mp"]) for t, _ in maps)
        h = np.zeros((N_MAPS, cap, 20), np.uint8)
        for m, ed in enumerate(lists):
            h[m, :len(ed)] = ed.view(np.uint8).reshape(-1, 20)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
        tt = {"ops": torch.from_numpy(h).cuda(), "n": torch.tensor([len(ed) for ed in lists], dtype=torch.int32, device="cuda"), "moved": i32(N_MAPS, cap),
              "erased": i32(N_MAPS, cap), "touched": i32(N_MAPS, mp_cap), "n_touched": i32(N_MAPS), "n_obs_out": i32(N_MAPS), "status": i32(N_MAPS), "kfmp_cap": kfmp_cap,
              "workspace": torch.zeros(api.map_replace_workspace(N_MAPS, cap, mp_cap, kfmp_cap), dtype=torch.uint8, device="cuda")}
        stream = torch.cuda.current_stream()
        ms = []
        for r in range(a.warmup + a.reps):
            for ei, ri, sv in zip(eis, ris, saved):
                for k, v in sv.items():
                    tens(ei, ri, k).copy_(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            api.map_replace_batch_dev(mis, ris, tt, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        entry = {"ops_per_map": [int(len(ed)) for ed in lists], "device": stats(ms), "workspace_bytes": int(tt["workspace"].numel())}
        assert not tt["status"].any().item(), tt["status"]
        # (c)'s upload: the tables the list changed, the way api.MapIndex puts a table on the device
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
            for m, (out, ei, ri, (t, x), ed) in enumerate(zip(outs, eis, ris, maps, lists)):
                need, nt, n_mp, n = out["n_obs_out"], out["n_touched"], t["n_mp"], len(ed)
                assert int(tt["n_obs_out"][m]) == need and int(tt["n_touched"][m]) == nt and out["status"] == 0
                pairs = [(k, ei.sets[1][k][:n_mp + 1 if k == "obs_ptr" else need]) for k in ("obs_ptr", "obs_kf", "obs_idx", "obs_octave", "obs_weight")]
                pairs += [(k, tens(ei, ri, k)[:len(t["kf_mp"]) if k == "kf_mp" else n_mp]) for k in INPLACE]
                pairs += [("moved", tt["moved"][m, :n]), ("erased", tt["erased"][m, :n]), ("touched", tt["touched"][m, :nt])]
                for key, got in pairs:
                    assert np.array_equal(got.cpu().numpy(), out[key]), (label, m, key)
            entry["cpu_one_core"] = {"median_ms": med, "min_ms": best}
            entry["rebuild_and_upload_ms"] = med + entry["upload"]["median_ms"]
            entry["results_equal"] = True
            entry["moved"], entry["erased"], entry["touched"] = int(sum(o["moved"].sum() for o in outs)), int(sum(o["erased"].sum() for o in outs)), int(sum(o["n_touched"] for o in outs))
        result["lists"][label] = entry
        print(label, json.dumps(entry))
    if a.out:
        json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
