"""Times Tracking::UpdateLocalMap for 256 frames on maps of about 200 keyframes x 1,000 keypoints:

  (a) the host loops in plain C++ on one core, over pointer-linked objects with std::map and std::set as the reference has them
      (the comparator below; the objects are built once, outside the timed region, as a running tracker has them)
  (b) slamit_local_map_batch_dev, everything resident: votes, local keyframes, local points and the gathered frustum planes

    python tools/bench_local_map.py [--reps 30] [--warmup 5] [--out profiles/r23_local_map.json]
    python tools/bench_local_map.py --kernel-stats <rocprofv3 kernel_stats.csv> --out profiles/r23_local_map.json

(b) is wall clock from the call to the end of a stream synchronisation, median of the repetitions after warm-up; before each
repetition the in / out arrays are restored on the device, outside the timed region.  The device's lists must equal the
comparator's exactly or the tool fails.  The second form adds the three passes' kernel times, taken in a run of its own under
`rocprofv3 --kernel-trace --stats`, to the file the first form wrote.  Recorded, not gated."""
import argparse
import csv
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU_PORT = r'''
// Tracking::UpdateLocalMap as a host tracker runs it: objects linked by pointers, a std::map of votes, std::set children, marks by
// frame id.  Built from the same tables the device reads; a keyframe's address order is its slot order (one array).
#include <stddef.h>
#include <stdint.h>
#include <map>
#include <set>
#include <vector>
struct KF;
struct MP { bool bad; std::map<KF*, size_t> obs; long mark; int slot; };
struct KF { bool bad; std::vector<MP*> pts; std::vector<KF*> best; std::set<KF*> childs; KF* parent; long mark; int slot; };
struct World { std::vector<KF> kfs; std::vector<MP> mps; };
extern "C" void* cpu_build(int n_kf, int n_mp, const int32_t* obs_ptr, const int32_t* obs_kf, const uint8_t* mp_bad, const uint8_t* kf_bad, const int32_t* kf_mp_ptr,
                           const int32_t* kf_mp, const int32_t* kf_best, const int32_t* child_ptr, const int32_t* child, const int32_t* parent) {
    World* W = new World;
    W->kfs.resize(n_kf); W->mps.resize(n_mp);
    for (int p = 0; p < n_mp; ++p) {
        MP& m = W->mps[p];
        m.bad = mp_bad[p]; m.mark = -1; m.slot = p;
        for (int e = obs_ptr[p]; e < obs_ptr[p + 1]; ++e) m.obs[&W->kfs[obs_kf[e]]] = 0;
    }
    for (int k = 0; k < n_kf; ++k) {
        KF& f = W->kfs[k];
        f.bad = kf_bad[k]; f.mark = -1; f.slot = k; f.parent = parent[k] >= 0 ? &W->kfs[parent[k]] : NULL;
        for (int e = kf_mp_ptr[k]; e < kf_mp_ptr[k + 1]; ++e) f.pts.push_back(kf_mp[e] >= 0 ? &W->mps[kf_mp[e]] : NULL);
        for (int b = 0; b < 10; ++b) if (kf_best[10 * k + b] >= 0) f.best.push_back(&W->kfs[kf_best[10 * k + b]]);
        for (int e = child_ptr[k]; e < child_ptr[k + 1]; ++e) f.childs.insert(&W->kfs[child[e]]);
    }
    return W;
}
// nframes frames of kp_cap slots each (n[f] in use); writes per frame the two list sizes, the reference keyframe and the point list
extern "C" void cpu_run(void* world, int nframes, int kp_cap, const int32_t* n, const int32_t* frame_mp, int q_cap, int32_t* n_local_kf, int32_t* ref_kf,
                        int32_t* n_local_mp, int32_t* local_mp, long first_id) {
    World* W = (World*)world;
    std::vector<KF*> localKFs;
    std::vector<MP*> localMPs, mine;
    for (int f = 0; f < nframes; ++f) {
        const long id = first_id + f;
        mine.clear();
        for (int i = 0; i < n[f]; ++i) mine.push_back(frame_mp[(size_t)f * kp_cap + i] >= 0 ? &W->mps[frame_mp[(size_t)f * kp_cap + i]] : NULL);
        std::map<KF*, int> counter;
        for (size_t i = 0; i < mine.size(); ++i) {
            MP* p = mine[i];
            if (!p) continue;
            if (p->bad) { mine[i] = NULL; continue; }
            const std::map<KF*, size_t> obs = p->obs;   // GetObservations() returns a copy
            for (std::map<KF*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) counter[it->first]++;
        }
        KF* ref = NULL;
        if (!counter.empty()) {
            int best = 0;
            localKFs.clear();
            for (std::map<KF*, int>::const_iterator it = counter.begin(); it != counter.end(); ++it) {
                if (it->first->bad) continue;
                if (it->second > best) { best = it->second; ref = it->first; }
                localKFs.push_back(it->first);
                it->first->mark = id;
            }
            const size_t voted = localKFs.size();
            for (size_t v = 0; v < voted; ++v) {
                if (localKFs.size() > 80) break;
                KF* kf = localKFs[v];
                const std::vector<KF*> neigh = kf->best;
                for (size_t j = 0; j < neigh.size(); ++j)
                    if (!neigh[j]->bad && neigh[j]->mark != id) { localKFs.push_back(neigh[j]); neigh[j]->mark = id; break; }
                const std::set<KF*> childs = kf->childs;
                for (std::set<KF*>::const_iterator c = childs.begin(); c != childs.end(); ++c)
                    if (!(*c)->bad && (*c)->mark != id) { localKFs.push_back(*c); (*c)->mark = id; break; }
                if (kf->parent && kf->parent->mark != id) { localKFs.push_back(kf->parent); kf->parent->mark = id; break; }
            }
        }
        localMPs.clear();
        for (size_t k = 0; k < localKFs.size(); ++k) {
            const std::vector<MP*> pts = localKFs[k]->pts;   // GetMapPointMatches() returns a copy
            for (size_t i = 0; i < pts.size(); ++i) {
                MP* p = pts[i];
                if (!p || p->mark == id || p->bad) continue;
                localMPs.push_back(p);
                p->mark = id;
            }
        }
        n_local_kf[f] = (int32_t)localKFs.size(); ref_kf[f] = ref ? ref->slot : -1; n_local_mp[f] = (int32_t)localMPs.size();
        for (size_t i = 0; i < localMPs.size() && (int)i < q_cap; ++i) local_mp[(size_t)f * q_cap + i] = localMPs[i]->slot;
    }
}
'''

PASSES = {"a_votes": ("lm_votes_kernel",), "b_local_keyframes": ("lm_keyframes_kernel",),
          "c_local_points": ("lm_mark_kernel", "lm_keys_kernel", "lm_count_kernel", "lm_write_kernel")}


def merge_kernel_stats(path, out):
    res = json.load(open(out))
    rows = {r["Name"].split("(")[0].split()[-1]: r for r in csv.DictReader(open(path))}
    k = {}
    for name, kernels in PASSES.items():
        missing = [x for x in kernels if x not in rows]
        if missing:
            raise SystemExit("no such kernels in %s: %s" % (path, missing))
        k[name + "_us_per_call"] = sum(float(rows[x]["AverageNs"]) for x in kernels) / 1e3
        k[name + "_kernels"] = {x: {"calls": int(rows[x]["Calls"]), "average_us": float(rows[x]["AverageNs"]) / 1e3} for x in kernels}
    res["kernel_times_rocprofv3"] = k
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_local_map.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.kernel_stats, a.out)
    import torch

    from tests.local_map_fixtures import chain_map
    from weiner_slamit_v2_amd import api

    B, K, kps = a.frames, a.keyframes, a.keypoints
    n_mp = K * kps // 5                                   # a point is seen by about five keyframes
    maps = [chain_map(900 + i, K, n_mp, kps, kps + kps // 4) for i in range(2)]
    rs = np.random.RandomState(5)
    kp_cap, kf_cap, q_cap = kps, 128, 16384
    frame_map = (np.arange(B) % 2).astype(np.int32)
    frame_mp = np.full((B, kp_cap), -1, np.int32)
    for f in range(B):                                    # a frame tracks points of a stretch of the chain about three keyframes long
        lo = rs.randint(0, n_mp - 3 * n_mp // K)
        mp = rs.randint(lo, lo + 3 * n_mp // K, kp_cap)
        mp[rs.rand(kp_cap) < 0.5] = -1
        frame_mp[f] = mp
    n = np.full(B, kp_cap, np.int32)
    res = {"workload": "%d frames of %d keypoints on 2 maps of %d keyframes x %d keypoints, %d points each" % (B, kp_cap, K, kps, n_mp),
           "comparator": "the host loops in C++ (g++ -O3) on one core, std::map votes and std::set children over pointer-linked objects", "reps": a.reps,
           "warmup": a.warmup}

    # (b) resident
    mi = [api.MapIndex(t) for t in maps]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    d = {"frame_map": torch.from_numpy(frame_map).cuda(), "n": torch.from_numpy(n).cuda(), "frame_mp": torch.from_numpy(frame_mp).cuda(), "votes": i32(B, K),
         "local_kf": i32(B, kf_cap), "n_local_kf": i32(B), "ref_kf": i32(B), "local_mp": i32(B, q_cap), "n_local_mp": i32(B), "pos": f32(B, 3, q_cap),
         "normal": f32(B, 3, q_cap), "max_dist": f32(B, q_cap), "min_dist": f32(B, q_cap), "skip": torch.zeros((B, q_cap), dtype=torch.uint8, device="cuda"),
         "m": i32(B), "status": i32(B), "mp_cap": n_mp,
         "workspace": torch.zeros(api.local_map_workspace(B, n_mp, kf_cap), dtype=torch.uint8, device="cuda")}
    start = {k: d[k].clone() for k in ("frame_mp", "local_kf", "n_local_kf", "ref_kf")}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    t_dev = []
    for r in range(a.warmup + a.reps):
        for k, v in start.items():
            d[k].copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.local_map_batch_dev(mi, d, stream=s.cuda_stream)
        s.synchronize()
        if r >= a.warmup:
            t_dev.append((time.perf_counter() - t0) * 1e3)
    g = {k: d[k].cpu().numpy() for k in ("n_local_kf", "ref_kf", "n_local_mp", "local_mp", "status", "m")}
    res.update({"b_resident_ms_median": float(np.median(t_dev)), "b_resident_ms_min": float(np.min(t_dev)), "b_resident_us_per_frame": float(np.median(t_dev)) * 1e3 / B,
                "local_keyframes_mean": float(g["n_local_kf"].mean()), "local_points_mean": float(g["n_local_mp"].mean()), "status_bits_seen": int(np.bitwise_or.reduce(g["status"]))})
    if a.no_cpu:
        print(json.dumps(res))
        return

    # (a) the comparator
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-shared", "-fPIC", os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    shutil.rmtree(tmp, ignore_errors=True)                # the library stays mapped
    port.cpu_build.restype = C.c_void_p
    port.cpu_build.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 10
    port.cpu_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    ptr = lambda a_: a_.ctypes.data_as(C.c_void_p)
    worlds = []
    for t in maps:
        keep = [np.ascontiguousarray(t[k]) for k in ("obs_ptr", "obs_kf", "mp_bad", "kf_bad", "kf_mp_ptr", "kf_mp", "kf_best", "kf_child_ptr", "kf_child", "kf_parent")]
        worlds.append(port.cpu_build(t["n_kf"], t["n_mp"], *[ptr(x) for x in keep]))
    c = {"n_local_kf": np.zeros(B, np.int32), "ref_kf": np.zeros(B, np.int32), "n_local_mp": np.zeros(B, np.int32), "local_mp": np.zeros((B, q_cap), np.int32)}
    per_map = [np.flatnonzero(frame_map == i) for i in range(2)]
    sub = [{k: np.ascontiguousarray(v[idx]) for k, v in c.items()} for idx in per_map]
    sub_in = [(np.ascontiguousarray(n[idx]), np.ascontiguousarray(frame_mp[idx])) for idx in per_map]
    t_cpu, next_id = [], [1]

    def cpu_once():
        for i in range(2):
            o = sub[i]
            port.cpu_run(worlds[i], len(per_map[i]), kp_cap, ptr(sub_in[i][0]), ptr(sub_in[i][1]), q_cap, ptr(o["n_local_kf"]), ptr(o["ref_kf"]), ptr(o["n_local_mp"]),
                         ptr(o["local_mp"]), next_id[0])
            next_id[0] += B
    for r in range(2 + a.reps):
        t0 = time.perf_counter()
        cpu_once()
        if r >= 2:
            t_cpu.append((time.perf_counter() - t0) * 1e3)
    for i, idx in enumerate(per_map):
        for k in c:
            c[k][idx] = sub[i][k]
    same = all(np.array_equal(g[k], c[k]) for k in ("n_local_kf", "ref_kf", "n_local_mp"))
    same = same and all(np.array_equal(g["local_mp"][f, :g["m"][f]], c["local_mp"][f, :g["m"][f]]) for f in range(B))
    res.update({"a_cpu_loops_ms_median": float(np.median(t_cpu)), "a_cpu_loops_ms_min": float(np.min(t_cpu)), "a_cpu_us_per_frame": float(np.median(t_cpu)) * 1e3 / B,
                "speedup_resident_vs_cpu_loops": float(np.median(t_cpu) / np.median(t_dev)), "device_lists_equal_cpu_loops": bool(same)})
    print(json.dumps(res))
    if not same:
        raise SystemExit("the device's lists and the host loops' differ")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
