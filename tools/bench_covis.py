#!/usr/bin/env python3
"""Time the two resident covisibility calls against csrc/covis.h's sequential statement on one core.

Workload: maps of 200 keyframes x about 1,000 keypoints, 40,000 points each, a point seen by five of eight consecutive keyframes.
slamit_update_connections_batch_dev takes one keyframe per map and at most eight maps a call, so 256 updates are 32 calls on one
stream over eight maps (keyframes 3, 9, 15, ... of each, which the graph does not know yet: every listed neighbour is inserted into
and re-sorted); slamit_keyframe_culling_batch_dev takes the 256 current keyframes -- the same ones, after their update -- in one call.
Each timing is from the first call to the end of a stream synchronisation, median of --reps after --warmup, with the graph rows
restored outside the timed region.  The comparator runs the same 256 + 256 problems through cv_*_seq under g++ -O3; the results
(every graph row, every verdict) are compared before anything is reported.

  python3 tools/bench_covis.py [--reps 30] [--warmup 5] [--no-cpu] [--out profiles/r24_covis.json]"""
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
N_MAPS, N_KF, N_KP, PER_POINT, WINDOW, ROW_CAP, STEP = 8, 200, 1000, 5, 8, 32, 6
GRAPH = ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best")


def make_map(seed):
    """-> (tables, covis, ks): ks are the keyframes to update, absent from the graph as it stands."""
    rng = np.random.default_rng(seed)
    n_mp = N_KF * N_KP // PER_POINT
    base = rng.integers(0, N_KF - WINDOW + 1, n_mp)
    who = np.sort(np.argsort(rng.random((n_mp, WINDOW)), axis=1)[:, :PER_POINT], axis=1) + base[:, None]      # (n_mp, 5) observers, ascending
    octave = rng.integers(0, 8, (n_mp, PER_POINT)).astype(np.uint8)
    # keyframe rows: the (point, octave) pairs grouped by keyframe, in a shuffled keypoint order
    flat_kf, flat_p, flat_o = who.reshape(-1), np.repeat(np.arange(n_mp), PER_POINT), octave.reshape(-1)
    order = np.lexsort((rng.random(len(flat_kf)), flat_kf))
    kf_mp, kf_octave = flat_p[order].astype(np.int32), flat_o[order]
    kf_mp_ptr = np.concatenate([[0], np.cumsum(np.bincount(flat_kf, minlength=N_KF))]).astype(np.int32)
    mp_bad = (rng.random(n_mp) < 0.02).astype(np.uint8)
    ks = np.arange(3, N_KF, STEP)[:32]
    # the graph: weights from the rows, every keyframe but ks
    W = np.zeros((N_KF, N_KF), np.int32)
    good = who[mp_bad == 0]
    for a in range(PER_POINT):
        for b in range(PER_POINT):
            if a != b:
                np.add.at(W, (good[:, a], good[:, b]), 1)
    W[ks, :] = 0
    W[:, ks] = 0
    x = {"row_cap": ROW_CAP, "origin_kf": 0, "obs_octave": octave.reshape(-1), "obs_weight": np.ones(n_mp * PER_POINT, np.uint8),
         "mp_nobs": np.full(n_mp, PER_POINT, np.int32), "kf_octave": kf_octave, "kf_depth": None, "kf_th_depth": None, "kf_not_erase": np.zeros(N_KF, np.uint8),
         "cw_kf": np.full((N_KF, ROW_CAP), -1, np.int32), "cw_w": np.zeros((N_KF, ROW_CAP), np.int32), "cw_n": np.zeros(N_KF, np.int32),
         "ord_kf": np.full((N_KF, ROW_CAP), -1, np.int32), "ord_w": np.zeros((N_KF, ROW_CAP), np.int32), "ord_n": np.zeros(N_KF, np.int32),
         "kf_best": np.full((N_KF, 10), -1, np.int32)}
    for k in range(N_KF):
        nb = np.flatnonzero(W[k])
        srt = nb[np.lexsort((-nb, -W[k, nb]))]
        x["cw_n"][k] = x["ord_n"][k] = len(nb)
        x["cw_kf"][k, :len(nb)], x["cw_w"][k, :len(nb)] = nb, W[k, nb]
        x["ord_kf"][k, :len(nb)], x["ord_w"][k, :len(nb)] = srt, W[k, srt]
        x["kf_best"][k, :min(10, len(nb))] = srt[:10]
    t = {"n_kf": N_KF, "n_mp": n_mp, "obs_ptr": (np.arange(n_mp + 1) * PER_POINT).astype(np.int32), "obs_kf": who.reshape(-1).astype(np.int32), "mp_bad": mp_bad,
         "kf_bad": np.zeros(N_KF, np.uint8), "kf_mp_ptr": kf_mp_ptr, "kf_mp": kf_mp, "kf_best": x["kf_best"], "kf_child_ptr": np.zeros(N_KF + 1, np.int32),
         "kf_child": np.zeros(0, np.int32), "kf_parent": np.full(N_KF, -1, np.int32), "mp_pos": np.zeros((n_mp, 3), np.float32),
         "mp_normal": np.zeros((n_mp, 3), np.float32), "mp_max_dist": np.ones(n_mp, np.float32), "mp_min_dist": np.zeros(n_mp, np.float32)}
    return t, x, ks


CPU_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "covis.h"
template <typename T> static std::vector<T> rd(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v((size_t)n + 1);
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) exit(2);
    return v;
}
struct Map {
    std::vector<int32_t> h, obs_ptr, obs_kf, kf_mp_ptr, kf_mp, mp_nobs, cw_kf, cw_w, cw_n, ord_kf, ord_w, ord_n, kf_best, ks;
    std::vector<uint8_t> mp_bad, obs_octave, obs_weight, kf_octave, kf_not_erase;
    std::vector<int32_t> g0[7];
    LmMap M; CvIndex X;
    void bind() {
        M = LmMap(); X = CvIndex();
        M.n_kf = h[0]; M.n_mp = h[1]; X.row_cap = h[2]; X.origin_kf = h[3];
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.data(); M.mp_bad = mp_bad.data(); M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.data();
        X.obs_octave = obs_octave.data(); X.obs_weight = obs_weight.data(); X.mp_nobs = mp_nobs.data(); X.kf_octave = kf_octave.data(); X.kf_not_erase = kf_not_erase.data();
        X.cw_kf = cw_kf.data(); X.cw_w = cw_w.data(); X.cw_n = cw_n.data(); X.ord_kf = ord_kf.data(); X.ord_w = ord_w.data(); X.ord_n = ord_n.data(); X.kf_best = kf_best.data();
    }
    std::vector<int32_t>* graph(int i) { std::vector<int32_t>* g[7] = {&cw_kf, &cw_w, &cw_n, &ord_kf, &ord_w, &ord_n, &kf_best}; return g[i]; }
    void save() { for (int i = 0; i < 7; ++i) g0[i] = *graph(i); }
    void restore() { for (int i = 0; i < 7; ++i) *graph(i) = g0[i]; bind(); }
};
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
int main(int argc, char** argv) {
    if (argc != 4) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    const int reps = atoi(argv[3]);
    std::vector<int32_t> head = rd<int32_t>(f);
    std::vector<Map> maps(head[0]);
    for (size_t m = 0; m < maps.size(); ++m) {
        Map& A = maps[m];
        A.h = rd<int32_t>(f); A.ks = rd<int32_t>(f); A.ks.pop_back();
        A.obs_ptr = rd<int32_t>(f); A.obs_kf = rd<int32_t>(f); A.mp_bad = rd<uint8_t>(f); A.kf_mp_ptr = rd<int32_t>(f); A.kf_mp = rd<int32_t>(f);
        A.obs_octave = rd<uint8_t>(f); A.obs_weight = rd<uint8_t>(f); A.mp_nobs = rd<int32_t>(f); A.kf_octave = rd<uint8_t>(f); A.kf_not_erase = rd<uint8_t>(f);
        for (int i = 0; i < 7; ++i) *A.graph(i) = rd<int32_t>(f);
        A.bind(); A.save();
    }
    fclose(f);
    const int n_kf = maps[0].M.n_kf, cap = maps[0].X.row_cap, n_mp = maps[0].M.n_mp;
    std::vector<int32_t> counts(n_kf), n_mps(cap), n_red(cap);
    std::vector<unsigned long long> keys(cap), keys_j(cap);
    std::vector<uint8_t> verdict(cap), turned(n_mp);
    std::vector<uint32_t> S(n_kf / 32 + 2);
    std::vector<double> t_uc, t_cull;
    std::vector<int32_t> out;   // per problem: n_listed, parent; then n_cand and the verdicts
    for (int r = 0; r < reps; ++r) {
        for (size_t m = 0; m < maps.size(); ++m) maps[m].restore();
        out.clear();
        auto t0 = std::chrono::steady_clock::now();
        for (size_t m = 0; m < maps.size(); ++m)
            for (size_t i = 0; i < maps[m].ks.size(); ++i) {
                int status = 0;
                int32_t nc = 0, nl = 0, parent = -1;
                cv_counts_seq(maps[m].M, maps[m].ks[i], counts.data(), status);
                cv_connections_seq(maps[m].M, maps[m].X, maps[m].ks[i], true, counts.data(), &nc, &nl, &parent, keys.data(), keys_j.data(), status);
                out.push_back(nl); out.push_back(parent); out.push_back(status);
            }
        auto t1 = std::chrono::steady_clock::now();
        for (size_t m = 0; m < maps.size(); ++m)
            for (size_t i = 0; i < maps[m].ks.size(); ++i) {
                int status = 0;
                int32_t n_cand = 0;
                cv_culling_seq(maps[m].M, maps[m].X, maps[m].ks[i], true, verdict.data(), n_mps.data(), n_red.data(), &n_cand, turned.data(), S.data(), status);
                out.push_back(n_cand);
                for (int c = 0; c < n_cand; ++c) { out.push_back(verdict[c]); out.push_back(n_mps[c]); out.push_back(n_red[c]); }
            }
        auto t2 = std::chrono::steady_clock::now();
        t_uc.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        t_cull.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const double t[2] = {median(t_uc), median(t_cull)};
    fwrite(t, sizeof(double), 2, o);
    for (size_t m = 0; m < maps.size(); ++m)
        for (int i = 0; i < 7; ++i) fwrite(maps[m].graph(i)->data(), 4, maps[m].g0[i].size() - 1, o);
    fwrite(out.data(), 4, out.size(), o);
    fclose(o);
    return 0;
}
"""


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return np.int32(len(a)).tobytes() + a.tobytes()


def cpu_run(worlds, reps):
    d = tempfile.mkdtemp(prefix="bench_covis_")
    src, exe, pin, pout = (os.path.join(d, n) for n in ("cpu.cc", "cpu", "in.bin", "out.bin"))
    open(src, "w").write(CPU_DRIVER)
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"), src, "-o", exe])
    blob = _arr([len(worlds)], np.int32)
    for t, x, ks in worlds:
        blob += _arr([t["n_kf"], t["n_mp"], x["row_cap"], x["origin_kf"]], np.int32) + _arr(ks, np.int32)
        for key, dt in (("obs_ptr", np.int32), ("obs_kf", np.int32), ("mp_bad", np.uint8), ("kf_mp_ptr", np.int32), ("kf_mp", np.int32)):
            blob += _arr(t[key], dt)
        for key, dt in (("obs_octave", np.uint8), ("obs_weight", np.uint8), ("mp_nobs", np.int32), ("kf_octave", np.uint8), ("kf_not_erase", np.uint8)):
            blob += _arr(x[key], dt)
        for key in GRAPH:
            blob += _arr(x[key], np.int32)
    open(pin, "wb").write(blob)
    subprocess.check_call(["taskset", "-c", "0", exe, pin, pout, str(reps)] if os.path.exists("/usr/bin/taskset") else [exe, pin, pout, str(reps)])
    raw = open(pout, "rb").read()
    times = np.frombuffer(raw, np.float64, 2)
    return float(times[0]), float(times[1]), np.frombuffer(raw, np.int32, offset=16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_covis.json"))
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api

    worlds = [make_map(100 + m) for m in range(N_MAPS)]
    maps = [api.MapIndex(t) for t, _, _ in worlds]
    covis = [api.CovisIndex(x, mi) for (_, x, _), mi in zip(worlds, maps)]
    saved = [{key: ci.t[key].clone() for key in GRAPH} for ci in covis]
    calls = len(worlds[0][2])
    n_mp = worlds[0][0]["n_mp"]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    uc = [{"kf": torch.tensor([int(w[2][c]) for w in worlds], dtype=torch.int32, device="cuda"), "first": torch.ones(N_MAPS, dtype=torch.int32, device="cuda"),
           "counts": i32(N_MAPS, N_KF), "n_counted": i32(N_MAPS), "n_listed": i32(N_MAPS), "parent": i32(N_MAPS), "status": i32(N_MAPS)} for c in range(calls)]
    P = N_MAPS * calls
    cu = {"prob_map": torch.arange(N_MAPS, dtype=torch.int32, device="cuda").repeat_interleave(calls).contiguous(),
          "kf": torch.tensor([int(k) for w in worlds for k in w[2]], dtype=torch.int32, device="cuda"), "monocular": torch.ones(P, dtype=torch.int32, device="cuda"),
          "verdict": torch.zeros((P, ROW_CAP), dtype=torch.uint8, device="cuda"), "n_mps": i32(P, ROW_CAP), "n_redundant": i32(P, ROW_CAP), "n_cand": i32(P),
          "mp_turned_bad": torch.zeros((P, n_mp), dtype=torch.uint8, device="cuda"), "status": i32(P)}
    st = torch.cuda.Stream()

    def restore():
        for ci, s in zip(covis, saved):
            for key in GRAPH:
                ci.t[key].copy_(s[key])
        torch.cuda.synchronize()

    def run_uc():
        for c in range(calls):
            api.update_connections_batch_dev(maps, covis, range(N_MAPS), uc[c], stream=st.cuda_stream)
        st.synchronize()

    def run_cull():
        api.keyframe_culling_batch_dev(maps, covis, cu, stream=st.cuda_stream)
        st.synchronize()

    t_uc, t_cull = [], []
    for r in range(a.warmup + a.reps):
        restore()
        t0 = time.perf_counter(); run_uc(); t1 = time.perf_counter(); run_cull(); t2 = time.perf_counter()
        if r >= a.warmup:
            t_uc.append((t1 - t0) * 1e3)
            t_cull.append((t2 - t1) * 1e3)
    res = {"workload": {"maps": N_MAPS, "keyframes": N_KF, "keypoints": N_KP, "points_per_map": n_mp, "observers_per_point": PER_POINT, "row_cap": ROW_CAP,
                        "update_connections": "%d keyframes: %d calls of %d maps on one stream" % (P, calls, N_MAPS), "keyframe_culling": "%d problems in one call" % P},
           "reps": a.reps, "warmup": a.warmup,
           "gpu_ms": {"update_connections": {"median": float(np.median(t_uc)), "min": float(np.min(t_uc))},
                      "keyframe_culling": {"median": float(np.median(t_cull)), "min": float(np.min(t_cull))}},
           "listed_per_keyframe": float(np.mean([int(u["n_listed"][m]) for u in uc for m in range(N_MAPS)])),
           "candidates_per_problem": float(cu["n_cand"].float().mean()), "culled": int((cu["verdict"] == 1).sum()), "status_or": int(torch.stack([u["status"] for u in uc]).max()) | int(cu["status"].max())}
    if not a.no_cpu:
        c_uc, c_cull, out = cpu_run(worlds, a.reps)
        o = 0
        same = True
        for ci in covis:                                                                   # every graph row after the 256 updates
            for key in GRAPH:
                g = ci.t[key].cpu().numpy().reshape(-1)
                same &= bool(np.array_equal(out[o:o + len(g)], g))
                o += len(g)
        for m in range(N_MAPS):
            for c in range(calls):
                same &= [int(uc[c]["n_listed"][m]), int(uc[c]["parent"][m]), int(uc[c]["status"][m])] == out[o:o + 3].tolist()
                o += 3
        ncand, ver, nm, nr = (cu[k].cpu().numpy() for k in ("n_cand", "verdict", "n_mps", "n_redundant"))
        for p in range(P):
            n = int(out[o]); o += 1
            rows = out[o:o + 3 * n].reshape(n, 3); o += 3 * n
            same &= n == ncand[p] and np.array_equal(rows[:, 0], ver[p, :n]) and np.array_equal(rows[:, 1], nm[p, :n]) and np.array_equal(rows[:, 2], nr[p, :n])
        res["cpu_ms"] = {"update_connections": c_uc, "keyframe_culling": c_cull, "what": "cv_*_seq of csrc/covis.h, g++ -O3, one core, median of reps"}
        res["equal_to_cpu"] = bool(same and o == len(out))
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)
        open(a.out, "a").write("\n")
    return 0 if res.get("equal_to_cpu", True) else 1


if __name__ == "__main__":
    sys.exit(main())
