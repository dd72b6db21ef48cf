#!/usr/bin/env python3
"""Time slamit_fuse_list_batch_dev + slamit_map_fuse_batch_dev against the other ways to get the same tables.

Workload: the maps of tools/bench_map_edit.py -- 8 maps x 200 keyframes x about 1,140 keypoints, 40,000 points each, SPARE free
keypoints at the end of every keyframe's row.  One SearchInNeighbors pass per map: QUERIES points of keyframe 15 projected into each of
its 20 neighbours, then QUERIES of the neighbours' points into keyframe 15, 21 targets back to back; per target MATCHED queries found a
keypoint (half of them an occupied one, half a free one), the others none (-1): about 700 matched ops in a list of 5,376.  Routes:
  (a) the builder and slamit_map_fuse_batch_dev, one call each over the eight maps: HIP events around the pair after --warmup calls, the
      in-place arrays put back before every call outside the events; median of --reps with the minimum and the 10th / 90th percentiles;
  (b) the same walk, mf_apply_seq of csrc/map_fuse.h, under g++ -O3 on one core, the eight maps one after the other;
  (c) (b) and the upload of every table the list changed the way api.MapIndex does it;
  (d) what the library offered before this module: d_match_kp brought to the host, the tail of Fuse walked there over host mirrors to
      learn the directions (that walk IS (b): a direction depends on what the ops before it did), the list of plain ops uploaded, and
      slamit_map_replace_batch_dev.  Its device part is timed on the REPLACE / ADD_OBS list the walk resolves into (which source a
      'Q replaced' op had is taken from mp_replaced; the order among the sources of one receiver is not the walk's, so (d)'s tables are
      not compared).
(a)'s results are compared with (b)'s, every array, before anything is reported.

  python3 tools/bench_map_fuse.py [--reps 30] [--warmup 5] [--out profiles/r33_map_fuse.json]"""
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
KF, NEIGHBOURS, QUERIES, MATCHED = 15, 20, 256, 34
INPLACE = ("mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "kf_mp")
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def search_of(t, rng, spare):
    """What the batch search of one SearchInNeighbors pass leaves for one map -> dict of host arrays, one row per target."""
    old_len = np.diff(t["kf_mp_ptr"]) - spare
    row = lambda k: t["kf_mp"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k] + old_len[k]]
    mine = np.unique(row(KF)[row(KF) >= 0])
    nb = [j for j in range(KF - NEIGHBOURS // 2, KF + NEIGHBOURS // 2 + 1) if j != KF]
    near = np.setdiff1d(np.concatenate([row(j) for j in nb]), np.concatenate([mine, [-1]]))
    targets = [(j, mine) for j in nb] + [(KF, near)]
    nf, kp_cap = len(targets), int(np.diff(t["kf_mp_ptr"]).max())
    point, match = np.zeros((nf, QUERIES), np.int32), np.full((nf, QUERIES), -1, np.int32)
    for f, (k, pool) in enumerate(targets):
        point[f] = rng.permutation(pool)[:QUERIES]
        taken = np.flatnonzero((row(k) >= 0) & ~np.isin(row(k), pool))
        hit = rng.permutation(QUERIES)[:MATCHED]
        match[f, hit[:MATCHED // 2]] = rng.permutation(taken)[:MATCHED // 2]
        match[f, hit[MATCHED // 2:]] = old_len[k] + rng.permutation(spare)[:MATCHED - MATCHED // 2]
    kps = np.zeros((nf, kp_cap), KP_DTYPE)
    kps["octave"] = rng.integers(0, 8, (nf, kp_cap))
    return {"m": np.full(nf, QUERIES, np.int32), "kf": np.array([k for k, _ in targets], np.int32), "point": point, "match": match, "kps": kps, "kp_cap": kp_cap}


def ops_of(s):
    from weiner_slamit_v2_amd import api

    nf = len(s["m"])
    ed = np.zeros((nf, QUERIES), api.REPLACE_DTYPE)
    ed["kind"], ed["a"], ed["b"], ed["idx"], ed["weight"] = api.FUSE_FUSE, s["point"], s["kf"][:, None], s["match"], 1
    ed["octave"] = np.where(s["match"] >= 0, np.take_along_axis(s["kps"]["octave"], np.maximum(s["match"], 0), 1), 0)
    return ed.reshape(-1)


CPU_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "map_fuse.h"
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
            std::vector<int32_t> optr(n_mp + 1), okf(cap + 1), oidx(cap + 1), outcome(n + 1), moved(n + 1), erased(n + 1), touched(n_mp + 1);
            std::vector<uint8_t> ooct(cap + 1), owgt(cap + 1);
            int32_t tail[4] = {0, 0, 0, 0};   // n_touched n_fused n_obs_out status
            LmMap M = LmMap();
            MrIndex X = MrIndex();
            M.n_kf = A.h[0]; M.n_mp = A.h[1]; M.obs_ptr = A.obs_ptr.data(); M.obs_kf = A.obs_kf.data(); M.kf_mp_ptr = A.kf_mp_ptr.data();
            X.obs_idx = A.obs_idx.data(); X.obs_octave = A.obs_octave.data(); X.obs_weight = A.obs_weight.data();
            X.mp_bad = mp_bad.data(); X.mp_nobs = mp_nobs.data(); X.mp_found = mp_found.data(); X.mp_visible = mp_visible.data(); X.mp_replaced = mp_replaced.data();
            X.kf_mp = kf_mp.data();
            X.obs_ptr_out = optr.data(); X.obs_kf_out = okf.data(); X.obs_idx_out = oidx.data(); X.obs_octave_out = ooct.data(); X.obs_weight_out = owgt.data();
            X.obs_cap_out = A.h[2];
            auto t0 = std::chrono::steady_clock::now();
            mf_apply_seq(M, X, (int)n, A.ops.data(), outcome.data(), moved.data(), erased.data(), touched.data(), &tail[0], &tail[1], &tail[2], &tail[3]);
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r == 0) {
                const size_t need = (size_t)tail[2], nt = (size_t)tail[0];
                fwrite(tail, 4, 4, o);
                wr(o, optr, n_mp + 1); wr(o, okf, need); wr(o, oidx, need); wr(o, ooct, need); wr(o, owgt, need);
                wr(o, mp_bad, n_mp); wr(o, mp_nobs, n_mp); wr(o, mp_found, n_mp); wr(o, mp_visible, n_mp); wr(o, mp_replaced, n_mp); wr(o, kf_mp, kf_mp.size());
                wr(o, outcome, n); wr(o, moved, n); wr(o, erased, n); wr(o, touched, nt);
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


def cpu_run(maps, lists, caps, reps):
    """-> (median ms, min ms, per map the arrays in the order the driver writes them)."""
    from bench_map_replace import _arr

    d = tempfile.mkdtemp(prefix="bench_map_fuse_")
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
        nt, nfused, need, st = np.frombuffer(raw, np.int32, 4, o)
        o += 16
        n_mp, n_kfmp, n = t["n_mp"], len(t["kf_mp"]), len(ed)
        out = {"n_touched": int(nt), "n_fused": int(nfused), "n_obs_out": int(need), "status": int(st)}
        for key, dt, count in (("obs_ptr", np.int32, n_mp + 1), ("obs_kf", np.int32, need), ("obs_idx", np.int32, need), ("obs_octave", np.uint8, need), ("obs_weight", np.uint8, need),
                               ("mp_bad", np.uint8, n_mp), ("mp_nobs", np.int32, n_mp), ("mp_found", np.int32, n_mp), ("mp_visible", np.int32, n_mp),
                               ("mp_replaced", np.int32, n_mp), ("kf_mp", np.int32, n_kfmp), ("outcome", np.int32, n), ("moved", np.int32, n), ("erased", np.int32, n),
                               ("touched", np.int32, nt)):
            out[key] = np.frombuffer(raw, dt, int(count), o).copy()
            o += out[key].nbytes
        outs.append(out)
    assert o == len(raw)
    return med, best, outs


def plain_list(ed, out, api):
    """The REPLACE / ADD_OBS ops the walk resolved the list into, for (d)'s device call."""
    oc, rows = out["outcome"], []
    sources = {}
    for q in np.flatnonzero(out["mp_replaced"] >= 0):
        sources.setdefault(int(out["mp_replaced"][q]), []).append(int(q))
    for i in np.flatnonzero(oc >= api.FUSE_OUT["ADDED"]):
        e = ed[i]
        if oc[i] == api.FUSE_OUT["ADDED"]:
            rows.append((api.REPLACE_ADD_OBS, int(e["a"]), int(e["b"]), int(e["idx"]), int(e["octave"]), int(e["weight"])))
        elif oc[i] == api.FUSE_OUT["P_REPLACED"]:
            rows.append((api.REPLACE_REPLACE, int(e["a"]), int(out["mp_replaced"][e["a"]]), 0, 0, 0))
        elif oc[i] == api.FUSE_OUT["Q_REPLACED"] and sources.get(int(e["a"])):
            rows.append((api.REPLACE_REPLACE, sources[int(e["a"])].pop(), int(e["a"]), 0, 0, 0))
    return api.replace_records(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bench_map_edit import SPARE, with_spare
    from bench_map_replace import CHANGED, stats
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
    searches = [search_of(t, np.random.default_rng(1300 + m), SPARE) for m, (t, _) in enumerate(maps)]
    lists = [ops_of(s) for s in searches]
    nf, n_ops = len(searches[0]["m"]), len(lists[0])
    caps = [len(t["obs_kf"]) + n_ops for t, _ in maps]
    mis = [api.MapIndex(t) for t, _ in maps]
    eis = [api.EditIndex(x, mi, cap) for (_, x), mi, cap in zip(maps, mis, caps)]
    ris = [api.ReplaceIndex(ei, x) for (_, x), ei in zip(maps, eis)]
    tens = lambda ei, ri, k: (ri.t if k in ri.t else ei.t)[k]
    saved = [{k: tens(ei, ri, k).clone() for k in INPLACE} for ei, ri in zip(eis, ris)]
    cap, mp_cap, kfmp_cap, kp_cap = n_ops, maps[0][0]["n_mp"], max(len(t["kf_mp"]) for t, _ in maps), max(s["kp_cap"] for s in searches)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    kps = np.zeros((N_MAPS * nf, kp_cap), KP_DTYPE)
    for m, s in enumerate(searches):
        kps[m * nf:(m + 1) * nf, :s["kp_cap"]] = s["kps"]
    tt = {"ops": torch.zeros((N_MAPS, cap, 20), dtype=torch.uint8, device="cuda"), "n": i32(N_MAPS), "outcome": i32(N_MAPS, cap), "moved": i32(N_MAPS, cap),
          "erased": i32(N_MAPS, cap), "touched": i32(N_MAPS, mp_cap), "n_touched": i32(N_MAPS), "n_fused": i32(N_MAPS), "n_obs_out": i32(N_MAPS), "status": i32(N_MAPS),
          "kfmp_cap": kfmp_cap, "workspace": torch.zeros(api.map_fuse_workspace(N_MAPS, cap, mp_cap, kfmp_cap), dtype=torch.uint8, device="cuda"),
          "m": cu(np.concatenate([s["m"] for s in searches])), "match_kp": cu(np.concatenate([s["match"] for s in searches])),
          "query_point": cu(np.concatenate([s["point"] for s in searches])), "kps_un": cu(kps.view(np.uint8).reshape(N_MAPS * nf, kp_cap, 28)), "kp_ur": None,
          "frame_map": cu(np.repeat(np.arange(N_MAPS), nf).astype(np.int32)), "frame_kf": cu(np.concatenate([s["kf"] for s in searches])),
          "base": cu(np.tile(np.arange(nf) * QUERIES, N_MAPS).astype(np.int32)), "list_status": i32(N_MAPS * nf)}
    stream = torch.cuda.current_stream()

    def put_back():
        for ei, ri, sv in zip(eis, ris, saved):
            for k, v in sv.items():
                tens(ei, ri, k).copy_(v)

    def timed(call):
        ms = []
        for r in range(a.warmup + a.reps):
            put_back()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms)

    def fuse_pair():
        api.fuse_list_batch_dev(tt, N_MAPS, stream=stream.cuda_stream)
        api.map_fuse_batch_dev(mis, ris, tt, stream=stream.cuda_stream)

    entry = {"ops_per_map": n_ops, "matched_per_map": int(np.count_nonzero(searches[0]["match"] >= 0)), "targets": nf, "a_builder_and_fuse": timed(fuse_pair),
             "a_fuse_alone": timed(lambda: api.map_fuse_batch_dev(mis, ris, tt, stream=stream.cuda_stream)), "workspace_bytes": int(tt["workspace"].numel())}
    put_back()
    fuse_pair()
    torch.cuda.synchronize()
    assert not tt["status"].any().item() and not tt["list_status"].any().item() and tt["n"].cpu().tolist() == [n_ops] * N_MAPS
    for m, ed in enumerate(lists):                                       # the builder wrote the list the host would have
        assert np.array_equal(tt["ops"][m].cpu().numpy().reshape(-1).view(api.REPLACE_DTYPE), ed), m
    med, best, outs = cpu_run(maps, lists, caps, max(3, a.reps // 3))
    for m, (out, ei, ri, (t, x), ed) in enumerate(zip(outs, eis, ris, maps, lists)):
        need, nt, n_mp, n = out["n_obs_out"], out["n_touched"], t["n_mp"], len(ed)
        assert int(tt["n_obs_out"][m]) == need and int(tt["n_touched"][m]) == nt and int(tt["n_fused"][m]) == out["n_fused"] and out["status"] == 0
        pairs = [(k, ei.sets[1][k][:n_mp + 1 if k == "obs_ptr" else need]) for k in ("obs_ptr", "obs_kf", "obs_idx", "obs_octave", "obs_weight")]
        pairs += [(k, tens(ei, ri, k)[:len(t["kf_mp"]) if k == "kf_mp" else n_mp]) for k in INPLACE]
        pairs += [("outcome", tt["outcome"][m, :n]), ("moved", tt["moved"][m, :n]), ("erased", tt["erased"][m, :n]), ("touched", tt["touched"][m, :nt])]
        for key, got in pairs:
            assert np.array_equal(got.cpu().numpy(), out[key]), (m, key)
    entry.update(results_equal=True, b_cpu_one_core={"median_ms": med, "min_ms": best}, n_fused=[o["n_fused"] for o in outs],
                 outcomes={k: int(sum(np.sum(o["outcome"] == v) for o in outs)) for k, v in api.FUSE_OUT.items()})
    # (c)'s upload: the tables the list changed, the way api.MapIndex puts a table on the device
    host = [{k: np.ascontiguousarray((x if k in x else t)[k], dt).reshape(-1) for k, dt in CHANGED} for t, x in maps]

    def wall(call):
        ms = []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = call()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            del keep
        return stats(ms)

    entry["upload_tables"] = dict(wall(lambda: [[torch.from_numpy(v).to("cuda:0") for v in hm.values()] for hm in host]), bytes=int(sum(v.nbytes for hm in host for v in hm.values())))
    entry["c_cpu_and_upload_ms"] = med + entry["upload_tables"]["median_ms"]
    # (d): the matches down, the walk on the host, the plain list up, slamit_map_replace_batch_dev
    plain = [plain_list(ed, out, api) for ed, out in zip(lists, outs)]
    pcap = max(len(p) for p in plain)
    hp = np.zeros((N_MAPS, pcap, 20), np.uint8)
    for m, p in enumerate(plain):
        hp[m, :len(p)] = p.view(np.uint8).reshape(-1, 20)
    rr = {"ops": cu(hp), "n": cu(np.array([len(p) for p in plain], np.int32)), "moved": i32(N_MAPS, pcap), "erased": i32(N_MAPS, pcap), "touched": i32(N_MAPS, mp_cap),
          "n_touched": i32(N_MAPS), "n_obs_out": i32(N_MAPS), "status": i32(N_MAPS), "kfmp_cap": kfmp_cap,
          "workspace": torch.zeros(api.map_replace_workspace(N_MAPS, pcap, mp_cap, kfmp_cap), dtype=torch.uint8, device="cuda")}
    entry["d_download_matches"] = wall(lambda: tt["match_kp"].cpu())
    entry["d_upload_list"] = wall(lambda: torch.from_numpy(hp).to("cuda:0"))
    entry["d_map_replace_batch_dev"] = dict(timed(lambda: api.map_replace_batch_dev(mis, ris, rr, stream=stream.cuda_stream)), ops_per_map=[int(len(p)) for p in plain],
                                            status=rr["status"].cpu().tolist())
    entry["d_total_ms"] = entry["d_download_matches"]["median_ms"] + med + entry["d_upload_list"]["median_ms"] + entry["d_map_replace_batch_dev"]["median_ms"]
    am = entry["a_builder_and_fuse"]["median_ms"]
    entry["a_beats_c"], entry["a_beats_d"] = bool(am < entry["c_cpu_and_upload_ms"]), bool(am < entry["d_total_ms"])
    result = {"workload": {"maps": N_MAPS, "keyframes": maps[0][0]["n_kf"], "points": maps[0][0]["n_mp"], "observations": int(len(maps[0][0]["obs_kf"])),
                           "kf_mp_entries": int(len(maps[0][0]["kf_mp"])), "per_pass": {"targets": nf, "queries_per_target": QUERIES, "matched_per_target": MATCHED}},
              "one_pass": entry}
    if a.out:
        json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
