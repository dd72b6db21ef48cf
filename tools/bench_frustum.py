"""Times the frustum test of Tracking::SearchLocalPoints at 64 frames x 2,000 local map points:

  (a) csrc/frustum.h itself, compiled with g++ -O3, on one host core
  (b) slamit_frustum_batch: host pointers, staging and both copies included
  (c) slamit_frustum_batch_dev alone, everything resident
  (d) the chain slamit_frustum_batch_dev -> slamit_guided_search_batch_dev, against today's route on the same run: (a) on the host,
      the upload of the four query arrays (uvr, level_min, level_max, valid), then the same search

    python tools/bench_frustum.py [--reps 30] [--warmup 5] [--out profiles/r14_frustum.json]

Warm-up calls first, then the median of the repetitions; (c) and (d) are wall clock from the first launch to the end of a stream
synchronisation.  The device's statuses and query arrays must equal the host build's bit for bit, and the two routes of (d) must
give the same matches, or the tool fails.  Recorded, not gated."""
import argparse
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
// the kernel's per-point text on one core, over the same records the C-ABI takes
#include <stdint.h>
#include <string.h>
#include "slamit.h"
#include "frustum.h"
extern "C" void cpu_frustum(int nprob, const slamit_frustum_problem* probs, slamit_frustum_result* res) {
    for (int p = 0; p < nprob; ++p) {
        const slamit_frustum_problem& P = probs[p];
        FrustumFrame F;
        memcpy(&F, &P.frame, sizeof(F));
        int in = 0;
        for (int i = 0; i < P.n; ++i) {
            FrustumOut o;
            const int st = frustum_point(F, P.pos + 3 * i, P.normal + 3 * i, P.max_dist[i], P.min_dist[i], P.skip[i] != 0, o);
            res[p].status[i] = (uint8_t)st;
            res[p].proj[3 * i] = o.u; res[p].proj[3 * i + 1] = o.v; res[p].proj[3 * i + 2] = o.uR;
            res[p].view_cos[i] = o.viewCos; res[p].level[i] = o.level;
            int l0, l1;
            frustum_query(st, o, res[p].uvr + 3 * i, l0, l1, res[p].valid[i]);
            res[p].level_min[i] = l0; res[p].level_max[i] = l1;
            in += st == 0;
        }
        res[p].n_in_view = in;
    }
}
'''

OUT = (("status", np.uint8, 1), ("proj", np.float32, 3), ("view_cos", np.float32, 1), ("level", np.int32, 1), ("uvr", np.float32, 3),
       ("level_min", np.int32, 1), ("level_max", np.int32, 1), ("valid", np.uint8, 1))


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def records(api, probs):
    """The C records of a list of problem dicts, with their output arrays: (P, R, outputs, keep-alive)."""
    m = len(probs)
    P, R = (api.FrustumProblem * m)(), (api.FrustumResult * m)()
    outs, keep = [], []
    for i, pr in enumerate(probs):
        n = int(pr["n"])
        C.memmove(C.byref(P[i].frame), api.frustum_frame_record(pr).ctypes.data, C.sizeof(api.FrustumFrame))
        k = {key: np.ascontiguousarray(pr[key]) for key in ("pos", "normal", "max_dist", "min_dist", "skip")}
        for key, arr in k.items():
            setattr(P[i], key, arr.ctypes.data)
        P[i].n = n
        o = {name: np.zeros((n, w) if w > 1 else n, dt) for name, dt, w in OUT}
        for name, arr in o.items():
            setattr(R[i], name, arr.ctypes.data)
        outs.append(o)
        keep.append(k)
    return P, R, outs, keep


def keypoints_for(o, seed, clutter=300):
    """A frame's keypoints for the search: one near each point in view, at its predicted level, and clutter."""
    rs = np.random.RandomState(seed)
    seen = np.flatnonzero(o["status"] == 0)
    xy = o["uvr"][seen, :2] + rs.uniform(-0.5, 0.5, (len(seen), 2)) * o["uvr"][seen, 2:3]
    xy = np.concatenate([xy, np.stack([rs.uniform(0, 640, clutter), rs.uniform(0, 480, clutter)], 1)]).astype(np.float32)
    octave = np.concatenate([o["level"][seen], rs.randint(0, 8, clutter)]).astype(np.int32)
    return xy, octave, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_frustum.json"))
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api, synth

    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    shutil.rmtree(tmp, ignore_errors=True)   # the library stays mapped
    L = api.lib()
    B, n = a.frames, a.points
    probs = [synth.synth_frustum(2000 + k, n, (1.0, 3.0, 5.0)[k % 3]) for k in range(B)]
    res = {"workload": "%d frames x %d local map points" % (B, n), "comparator": "csrc/frustum.h compiled with g++ -O3, one core", "reps": a.reps, "warmup": a.warmup}

    # (a) and (b)
    Pc, Rc, outs_c, keep_c = records(api, probs)
    cpu_ms, cpu_min = median_ms(lambda: port.cpu_frustum(B, Pc, Rc), 2, a.reps)
    P, R, outs, keep = records(api, probs)
    assert L.slamit_frustum_batch(0, B, P, R) == 0, L.slamit_last_error()
    call_ms, call_min = median_ms(lambda: L.slamit_frustum_batch(0, B, P, R), a.warmup, a.reps)
    same = all(np.array_equal(g[name].view(np.uint8), c[name].view(np.uint8)) for g, c in zip(outs, outs_c) for name, _, _ in OUT)
    same = same and all(R[i].n_in_view == Rc[i].n_in_view for i in range(B))
    res.update({"a_cpu_header_ms_median": cpu_ms, "a_cpu_header_ms_min": cpu_min, "b_batch_host_pointers_ms_median": call_ms, "b_batch_host_pointers_ms_min": call_min,
                "in_view": int(sum(R[i].n_in_view for i in range(B))), "device_equals_cpu_header_bit_for_bit": bool(same)})
    if not same:
        print(json.dumps(res))
        raise SystemExit("the device and the g++-built header differ")

    # (c) and (d): everything resident
    q_cap = n
    kp = [keypoints_for(o, 500 + f) for f, o in enumerate(outs_c)]
    kp_cap = max(len(k[0]) for k in kp)
    rs = np.random.RandomState(1)
    t = dict(frames=np.concatenate([api.frustum_frame_record(pr) for pr in probs]).view(np.float32).reshape(B, -1), m=np.full(B, n, np.int32),
             pos=np.stack([pr["pos"].T for pr in probs]), normal=np.stack([pr["normal"].T for pr in probs]), max_dist=np.stack([pr["max_dist"] for pr in probs]),
             min_dist=np.stack([pr["min_dist"] for pr in probs]), skip=np.stack([pr["skip"] for pr in probs]), n=np.array([len(k[0]) for k in kp], np.int32),
             desc=np.zeros((B, kp_cap, 32), np.uint8), kp_taken=np.zeros((B, kp_cap), np.uint8), qdesc=rs.randint(0, 256, (B, q_cap, 32)).astype(np.uint8),
             takes=np.ones((B, q_cap), np.uint8))
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    for f, (xy, octave, seen) in enumerate(kp):
        kps["x"][f, :len(xy)], kps["y"][f, :len(xy)], kps["octave"][f, :len(xy)] = xy[:, 0], xy[:, 1], octave
        t["desc"][f, :len(xy)] = rs.randint(0, 256, (len(xy), 32))
        t["desc"][f, :len(seen)] = t["qdesc"][f, seen]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, q_cap), dtype=torch.uint8, device="cuda")
    for name, dt, w in OUT[4:]:
        d[name] = torch.zeros((B, q_cap, 3) if w > 1 else (B, q_cap), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
    d["n_in_view"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    d["match_kp"] = torch.zeros((B, q_cap), dtype=torch.int32, device="cuda")
    d["nmatches"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    pr0 = probs[0]
    bounds = (float(pr0["min_x"]), float(pr0["min_y"]), float(np.float32(64) / np.float32(pr0["max_x"] - pr0["min_x"])),
              float(np.float32(48) / np.float32(pr0["max_y"] - pr0["min_y"])))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def dev_only():
        api.frustum_batch_dev(d, stream=s.cuda_stream)
        s.synchronize()

    def chain():
        api.frustum_batch_dev(d, stream=s.cuda_stream)
        api.ORBmatcher.guided_search_batch_dev(d, bounds, 100, True, 0.8, stream=s.cuda_stream)
        s.synchronize()

    host_q = {name: np.stack([o[name] for o in outs_c]) for name, _, _ in OUT[4:]}

    # today's route: the header writes the four query arrays of all frames straight into one pinned [B][q_cap] block each (the layout
    # the search reads), which goes up in four copies on the search's stream; nothing else is inside the timed region
    pinned = {name: torch.zeros((B, q_cap, 3) if w > 1 else (B, q_cap), dtype=getattr(torch, np.dtype(dt).name)).pin_memory() for name, dt, w in OUT[4:]}
    Pt, Rt, outs_t, keep_t = records(api, probs)
    for name in pinned:
        view = pinned[name].numpy()
        for f in range(B):
            setattr(Rt[f], name, view[f].ctypes.data)

    def today():
        port.cpu_frustum(B, Pt, Rt)
        with torch.cuda.stream(s):
            for name in pinned:
                d[name].copy_(pinned[name], non_blocking=True)
        api.ORBmatcher.guided_search_batch_dev(d, bounds, 100, True, 0.8, stream=s.cuda_stream)
        s.synchronize()

    def search_only():
        api.ORBmatcher.guided_search_batch_dev(d, bounds, 100, True, 0.8, stream=s.cuda_stream)
        s.synchronize()

    dev_ms, dev_min = median_ms(dev_only, a.warmup, a.reps)
    same_q = all(np.array_equal(d[name].cpu().numpy().view(np.uint8), host_q[name].view(np.uint8)) for name, _, _ in OUT[4:])
    chain_ms, chain_min = median_ms(chain, a.warmup, a.reps)
    m_chain = (d["match_kp"].cpu().numpy().copy(), d["nmatches"].cpu().numpy().copy())
    today_ms, today_min = median_ms(today, a.warmup, a.reps)
    m_today = (d["match_kp"].cpu().numpy().copy(), d["nmatches"].cpu().numpy().copy())
    search_ms, search_min = median_ms(search_only, a.warmup, a.reps)
    same_m = np.array_equal(m_chain[0], m_today[0]) and np.array_equal(m_chain[1], m_today[1])
    res.update({"c_batch_dev_ms_median": dev_ms, "c_batch_dev_ms_min": dev_min, "d_chain_ms_median": chain_ms, "d_chain_ms_min": chain_min,
                "d_today_host_header_upload_search_ms_median": today_ms, "d_today_host_header_upload_search_ms_min": today_min,
                "search_alone_ms_median": search_ms, "speedup_chain_vs_today": today_ms / chain_ms, "matches": int(m_chain[1].sum()),
                "device_queries_equal_cpu_header_bit_for_bit": bool(same_q), "routes_give_the_same_matches": bool(same_m)})
    print(json.dumps(res))
    if not (same_q and same_m):
        raise SystemExit("the two routes differ")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
