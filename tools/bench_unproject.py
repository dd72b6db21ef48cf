"""Times the closest-point walk of a stereo / RGB-D frame (Tracking::UpdateLastFrame) at two sizes:

  (a) csrc/unproject.h's unp_walk_host, compiled with g++ -O3, on one host core: 256 frames x 2,000 keypoints, and one frame
  (b) slamit_unproject_closest: one frame, host pointers, staging and both copies included
  (c) slamit_unproject_closest_batch_dev alone, 256 frames resident
  (d) the resident motion-model chain slamit_project_batch_dev_stereo -> slamit_guided_search_stereo_batch_dev ->
      slamit_rotation_check_batch_dev WITHOUT and WITH (c) in front of it, on one stream

    python tools/bench_unproject.py [--reps 30] [--warmup 5] [--out profiles/r21_unproject.json]

Warm-up calls first, then the median of the repetitions; (c) and (d) are wall clock from the first launch to the end of a stream
synchronisation.  The device's statuses, order, counters and points must equal the host build's bit for bit (two NaNs equal), or the
tool fails.  Recorded, not gated."""
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
// the header's walk on one core, over the same records the C-ABI takes
#include <stdint.h>
#include <string.h>
#include "slamit.h"
#include "unproject.h"
extern "C" void cpu_unproject(int nprob, const slamit_unproject_problem* probs, slamit_unproject_result* res) {
    for (int p = 0; p < nprob; ++p) {
        const slamit_unproject_problem& P = probs[p];
        UnprojectFrame F;
        memcpy(&F, &P.frame, sizeof(F));
        int counts[6];
        unp_walk_host(F, P.n, (const unsigned char*)P.kps_un, sizeof(slamit_kp), 20, P.depth, P.tracked, res[p].status, res[p].order, res[p].pos,
                      res[p].normal, res[p].max_dist, res[p].min_dist, counts);
        memcpy(&res[p].counts, counts, sizeof(counts));
    }
}
'''

OUT = (("status", np.uint8, 1), ("order", np.int32, 1), ("pos", np.float32, 3), ("normal", np.float32, 3), ("max_dist", np.float32, 1), ("min_dist", np.float32, 1))


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
    m = len(probs)
    P, R = (api.UnprojectProblem * m)(), (api.UnprojectResult * m)()
    outs, keep = [], []
    for i, pr in enumerate(probs):
        n = int(pr["n"])
        C.memmove(C.byref(P[i].frame), api.unproject_frame_record(pr).ctypes.data, C.sizeof(api.UnprojectFrame))
        k = {"kps_un": np.ascontiguousarray(pr["kps_un"], api.KP_DTYPE), "depth": np.ascontiguousarray(pr["depth"], np.float32),
             "tracked": np.ascontiguousarray(pr["tracked"], np.uint8)}
        for key, arr in k.items():
            setattr(P[i], key, arr.ctypes.data)
        P[i].n = n
        o = {name: np.zeros((n, w) if w > 1 else n, dt) for name, dt, w in OUT}
        for name, arr in o.items():
            setattr(R[i], name, arr.ctypes.data)
        outs.append(o)
        keep.append(k)
    return P, R, outs, keep


def same(a, b):
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_unproject.json"))
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
    B, n = a.frames, a.keypoints
    # an RGB-D-like frame: 85 % of the keypoints have a depth, a third of those are close, depths quantised, 40 % carry a tracked point
    probs = [synth.synth_unproject(seed=3000 + k, n=n, n_candidates=int(0.85 * n), n_close=int(0.3 * n), tie_at_cut=True, octave_bad_frac=0.0) for k in range(B)]
    res = {"workload": "%d frames x %d keypoints (UpdateLastFrame)" % (B, n), "comparator": "csrc/unproject.h compiled with g++ -O3, one core", "reps": a.reps,
           "warmup": a.warmup}

    # (a) and (b)
    Pc, Rc, outs_c, keep_c = records(api, probs)
    cpu_ms, cpu_min = median_ms(lambda: port.cpu_unproject(B, Pc, Rc), 2, a.reps)
    cpu1_ms, cpu1_min = median_ms(lambda: port.cpu_unproject(1, Pc, Rc), 2, a.reps)
    P, R, outs, keep = records(api, probs)
    assert L.slamit_unproject_closest(0, P, R) == 0, L.slamit_last_error()
    one_ms, one_min = median_ms(lambda: L.slamit_unproject_closest(0, P, R), a.warmup, a.reps)
    assert L.slamit_unproject_closest_batch(0, B, P, R) == 0, L.slamit_last_error()
    ok = all(same(g[name], c[name]) for g, c in zip(outs, outs_c) for name, _, _ in OUT)
    ok = ok and all(bytes(R[i].counts) == bytes(Rc[i].counts) for i in range(B))
    res.update({"a_cpu_header_batch_ms_median": cpu_ms, "a_cpu_header_batch_ms_min": cpu_min, "a_cpu_header_one_frame_ms_median": cpu1_ms,
                "a_cpu_header_one_frame_ms_min": cpu1_min, "b_one_frame_host_pointers_ms_median": one_ms, "b_one_frame_host_pointers_ms_min": one_min,
                "created": int(sum(R[i].counts.n_created for i in range(B))), "visited": int(sum(R[i].counts.n_visited for i in range(B))),
                "device_equals_cpu_header_bit_for_bit": bool(ok)})
    if not ok:
        print(json.dumps(res))
        raise SystemExit("the device and the g++-built header differ")

    # (c) and (d): everything resident.  The tracked points sit near where their keypoints unproject; the current camera is the last
    # frame's moved a little; its keypoints lie near the projections of the host form's merged points.
    f32 = np.float32
    bf = f32(38.6)
    rs = np.random.RandomState(9)
    cams, hpos, hskip, hoct = [], [], [], []
    for pr, o in zip(probs, outs_c):
        d = pr["depth"]
        with np.errstate(invalid="ignore"):
            z = np.where(np.isfinite(d) & (d > 0.1), d, f32(5.0)).astype(f32)
        x = (pr["kps_un"]["x"] - pr["cx"]) * z * pr["invfx"]
        y = (pr["kps_un"]["y"] - pr["cy"]) * z * pr["invfy"]
        Rwc = pr["Rwc"].reshape(3, 3)
        pos = (np.stack([x, y, z], 1) @ Rwc.T + pr["Ow"] + rs.normal(0, 0.01, (n, 3))).astype(f32)
        made, tr = o["status"] == 3, pr["tracked"] != 0
        hpos.append(np.where(made[:, None], o["pos"], pos).astype(f32))
        hskip.append((~(made | tr)).astype(np.uint8))
        hoct.append(np.where(made | tr, pr["kps_un"]["octave"], 0).astype(np.int32))
        Rcw = Rwc.T.copy()
        tcw = (-(Rcw.astype(np.float64) @ pr["Ow"].astype(np.float64)) + rs.uniform(-0.05, 0.05, 3)).astype(f32)
        cams.append(dict(form="LAST_FRAME", direction=0, R=Rcw.reshape(9), t=tcw, O=(-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32), fx=pr["fx"],
                         fy=pr["fy"], cx=pr["cx"], cy=pr["cy"], min_x=f32(0), max_x=f32(640), min_y=f32(0), max_y=f32(480), log_scale_factor=f32(np.log(f32(1.2))),
                         th=f32(7.0), n_levels=int(pr["n_levels"]), scale_factors=pr["scale_factors"]))
    proj = api.project_batch([dict(c, n=n, pos=p, normal=None, max_dist=None, min_dist=None, octave=o, skip=s) for c, p, o, s in zip(cams, hpos, hoct, hskip)],
                             bf=[bf] * B)
    kp_cap, clutter = n + 304, 300
    t = dict(frames=np.concatenate([api.unproject_frame_record(pr) for pr in probs]).view(np.float32).reshape(B, -1),
             cameras=np.concatenate([api.project_camera_record(c) for c in cams]).view(np.float32).reshape(B, -1), n=np.full(B, n, np.int32),
             depth=np.stack([pr["depth"] for pr in probs]), tracked=np.stack([pr["tracked"] for pr in probs]),
             pos=np.stack([np.where((pr["tracked"] != 0)[None, :], p.T, f32(0)) for pr, p in zip(probs, hpos)]).astype(f32),
             octave=np.stack([np.where(pr["tracked"] != 0, pr["kps_un"]["octave"], 0) for pr in probs]).astype(np.int32),
             skip=np.stack([(pr["tracked"] == 0) for pr in probs]).astype(np.uint8), normal=np.zeros((B, 3, n), f32), max_dist=np.zeros((B, n), f32),
             min_dist=np.zeros((B, n), f32), bf=np.full(B, bf, f32), kn=np.zeros(B, np.int32), desc=np.zeros((B, kp_cap, 32), np.uint8),
             kp_taken=np.zeros((B, kp_cap), np.uint8), qdesc=rs.randint(0, 256, (B, n, 32)).astype(np.uint8), takes=np.ones((B, n), np.uint8),
             kp_ur=np.full((B, kp_cap), -1.0, f32), qangle=rs.uniform(0, 360, (B, n)).astype(f32))
    last = np.stack([np.ascontiguousarray(pr["kps_un"], api.KP_DTYPE) for pr in probs])
    cur = np.zeros((B, kp_cap), api.KP_DTYPE)
    for f, pj in enumerate(proj):
        okq = np.flatnonzero(pj["valid"])
        k = len(okq) + clutter
        cur["x"][f, :k] = np.concatenate([pj["uvr"][okq, 0] + rs.uniform(-1.5, 1.5, len(okq)), rs.uniform(0, 640, clutter)])
        cur["y"][f, :k] = np.concatenate([pj["uvr"][okq, 1] + rs.uniform(-1.5, 1.5, len(okq)), rs.uniform(0, 480, clutter)])
        cur["octave"][f, :k] = np.concatenate([pj["level_max"][okq], rs.randint(0, 8, clutter)])
        cur["angle"][f, :k] = np.concatenate([t["qangle"][f, okq] + rs.uniform(-5, 5, len(okq)), rs.uniform(0, 360, clutter)]) % 360
        t["desc"][f, :k] = np.concatenate([t["qdesc"][f, okq], rs.randint(0, 256, (clutter, 32))])
        t["kp_ur"][f, :k] = np.concatenate([pj["ur"][okq] + rs.uniform(-2, 2, len(okq)), rs.uniform(0, 640, clutter)])
        t["kn"][f] = k
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in t.items()}
    d_last = torch.from_numpy(last.view(np.float32).reshape(B, n, 7)).cuda()
    d_cur = torch.from_numpy(cur.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    i32 = torch.int32
    un = dict(frames=d["frames"], n=d["n"], kps_un=d_last, depth=d["depth"], tracked=d["tracked"], pos=d["pos"], octave=d["octave"], skip=d["skip"],
              normal=d["normal"], max_dist=d["max_dist"], min_dist=d["min_dist"], status=torch.zeros((B, n), dtype=torch.uint8, device="cuda"),
              order=torch.zeros((B, n), dtype=i32, device="cuda"), counts=torch.zeros((B, 6), dtype=i32, device="cuda"))
    pj = dict(cameras=d["cameras"], m=d["n"], pos=d["pos"], normal=d["normal"], max_dist=d["max_dist"], min_dist=d["min_dist"], octave=d["octave"], skip=d["skip"],
              bf=d["bf"], ur=torch.zeros((B, n), device="cuda"), uvr=torch.zeros((B, n, 3), device="cuda"), level_min=torch.zeros((B, n), dtype=i32, device="cuda"),
              level_max=torch.zeros((B, n), dtype=i32, device="cuda"), valid=torch.zeros((B, n), dtype=torch.uint8, device="cuda"))
    se = dict(n=d["kn"], kps_un=d_cur, desc=d["desc"], kp_taken=d["kp_taken"], m=d["n"], uvr=pj["uvr"], level_min=pj["level_min"], level_max=pj["level_max"],
              qdesc=d["qdesc"], valid=pj["valid"], takes=d["takes"], match_kp=torch.zeros((B, n), dtype=i32, device="cuda"),
              nmatches=torch.zeros(B, dtype=i32, device="cuda"), workspace=torch.zeros(api.ORBmatcher.guided_search_workspace(B, n), dtype=torch.uint8, device="cuda"),
              qangle=d["qangle"], kp_query=torch.zeros((B, kp_cap), dtype=i32, device="cuda"), bins=torch.zeros((B, 3), dtype=i32, device="cuda"))
    bounds = (0.0, 0.0, float(f32(64) / f32(640)), float(f32(48) / f32(480)))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def dev_only():
        api.unproject_closest_batch_dev(un, stream=s.cuda_stream)
        s.synchronize()

    def chain(with_unproject):
        if with_unproject:
            api.unproject_closest_batch_dev(un, stream=s.cuda_stream)
        api.project_batch_dev(pj, stream=s.cuda_stream)
        api.ORBmatcher.guided_search_batch_dev(se, bounds, 100, True, 0.8, stream=s.cuda_stream, stereo=dict(er_mode=1, kp_ur=d["kp_ur"], q_ur=pj["ur"]))
        api.ORBmatcher.rotation_check_batch_dev(se, stream=s.cuda_stream)
        s.synchronize()

    without_ms, without_min = median_ms(lambda: chain(False), a.warmup, a.reps)   # first: the arrays still hold the tracked points alone
    m_without = int(se["nmatches"].sum())
    dev_ms, dev_min = median_ms(dev_only, a.warmup, a.reps)                        # the merge is idempotent: the same entries get the same values
    ok = all(same(un[name][f].cpu().numpy(), outs_c[f][name]) for f in (0, B - 1) for name in ("status", "order"))
    made0 = outs_c[0]["status"] == 3
    ok = ok and same(d["pos"][0].cpu().numpy().T[made0].copy(), outs_c[0]["pos"][made0]) and un["counts"][0].cpu().numpy().tolist() == list(bytes_to_counts(Rc[0].counts))
    with_ms, with_min = median_ms(lambda: chain(True), a.warmup, a.reps)
    m_with = int(se["nmatches"].sum())
    res.update({"c_batch_dev_ms_median": dev_ms, "c_batch_dev_ms_min": dev_min, "d_chain_without_ms_median": without_ms, "d_chain_without_ms_min": without_min,
                "d_chain_with_ms_median": with_ms, "d_chain_with_ms_min": with_min, "matches_without": m_without, "matches_with": m_with,
                "speedup_batch_dev_vs_one_core": cpu_ms / dev_ms, "resident_equals_cpu_header_bit_for_bit": bool(ok)})
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the resident form and the g++-built header differ")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


def bytes_to_counts(c):
    return (c.n_candidates, c.n_close, c.n_visited, c.n_created, c.n_total, c.n_map)


if __name__ == "__main__":
    main()
