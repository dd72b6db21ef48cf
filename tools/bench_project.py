"""Times the projections in front of the guided search (csrc/project.h):

  (a) csrc/project.h itself, compiled with g++ -O2, on one host core             at 1 x 2,000 and 64 x 2,000 points
  (b) slamit_project_batch: host pointers, staging and both copies included       at the same two sizes (the six forms in turn)
  (c) the resident chain slamit_project_batch_dev -> slamit_guided_search_batch_dev -> slamit_rotation_check_batch_dev of the
      motion-model search (LAST_FRAME) for 256 frames x 1,000 points: with the device idle before every chain (a pause, then one
      chain and a stream synchronisation) and back to back (a run of chains, one synchronisation, divided by their number)

    python tools/bench_project.py [--reps 30] [--warmup 5] [--out profiles/r16_project.json]

Warm-up calls first, then the median of the repetitions.  The device's outputs must equal the host build's bit for bit, or the tool
fails.  Recorded, not gated."""
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
#include "project.h"
extern "C" void cpu_project(int nprob, const slamit_project_problem* probs, slamit_project_result* res) {
    const float zero3[3] = {0.f, 0.f, 0.f};
    for (int p = 0; p < nprob; ++p) {
        const slamit_project_problem& P = probs[p];
        ProjectCamera Cm;
        memcpy(&Cm, &P.camera, sizeof(Cm));
        int ok = 0;
        for (int i = 0; i < P.n; ++i) {
            ProjectOut o;
            const int st = project_point(Cm, P.pos + 3 * i, P.normal ? P.normal + 3 * i : zero3, P.max_dist ? P.max_dist[i] : 0.f, P.min_dist ? P.min_dist[i] : 0.f,
                                         P.octave ? P.octave[i] : 0, P.skip[i] != 0, o);
            res[p].status[i] = (uint8_t)st;
            res[p].proj[2 * i] = o.u; res[p].proj[2 * i + 1] = o.v; res[p].level[i] = o.level;
            int l0, l1;
            project_query(Cm, st, o, res[p].uvr + 3 * i, l0, l1, res[p].valid[i]);
            res[p].level_min[i] = l0; res[p].level_max[i] = l1;
            ok += st == 0;
        }
        res[p].n_valid = ok;
    }
}
'''

OUT = (("status", np.uint8, 1), ("proj", np.float32, 2), ("level", np.int32, 1), ("uvr", np.float32, 3), ("level_min", np.int32, 1), ("level_max", np.int32, 1),
       ("valid", np.uint8, 1))
IN = (("pos", np.float32), ("normal", np.float32), ("max_dist", np.float32), ("min_dist", np.float32), ("octave", np.int32), ("skip", np.uint8))


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
    P, R = (api.ProjectProblem * m)(), (api.ProjectResult * m)()
    outs, keep = [], []
    for i, pr in enumerate(probs):
        n = int(pr["n"])
        C.memmove(C.byref(P[i].camera), api.project_camera_record(pr).ctypes.data, C.sizeof(api.ProjectCamera))
        k = {key: np.ascontiguousarray(pr[key], dt) for key, dt in IN if pr[key] is not None}
        for key, arr in k.items():
            setattr(P[i], key, arr.ctypes.data)
        P[i].n = n
        o = {name: np.zeros((n, w) if w > 1 else n, dt) for name, dt, w in OUT}
        for name, arr in o.items():
            setattr(R[i], name, arr.ctypes.data)
        outs.append(o)
        keep.append(k)
    return P, R, outs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--chain-frames", type=int, default=256)
    ap.add_argument("--chain-points", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_project.json"))
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api, synth

    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    shutil.rmtree(tmp, ignore_errors=True)   # the library stays mapped
    L = api.lib()
    n = a.points
    res = {"comparator": "csrc/project.h compiled with g++ -O2, one core", "reps": a.reps, "warmup": a.warmup, "sizes": {}}

    # (a) and (b)
    for B in (1, 64):
        probs = [synth.synth_project(3000 + k, n, (2 + k) % 6, (3.0, 10.0, 4.0, 7.5, 7.0, 10.0)[k % 6]) for k in range(B)]
        Pc, Rc, outs_c, keep_c = records(api, probs)
        cpu_ms, cpu_min = median_ms(lambda: port.cpu_project(B, Pc, Rc), 2, a.reps)
        P, R, outs, keep = records(api, probs)
        assert L.slamit_project_batch(0, B, P, R) == 0, L.slamit_last_error()
        call_ms, call_min = median_ms(lambda: L.slamit_project_batch(0, B, P, R), a.warmup, a.reps)
        same = all(np.array_equal(g[name].view(np.uint8), c[name].view(np.uint8)) for g, c in zip(outs, outs_c) for name, _, _ in OUT)
        same = same and all(R[i].n_valid == Rc[i].n_valid for i in range(B))
        res["sizes"]["%d x %d points" % (B, n)] = {"a_cpu_header_ms_median": cpu_ms, "a_cpu_header_ms_min": cpu_min, "b_batch_host_pointers_ms_median": call_ms,
                                                   "b_batch_host_pointers_ms_min": call_min, "accepted": int(sum(R[i].n_valid for i in range(B))),
                                                   "device_equals_cpu_header_bit_for_bit": bool(same)}
        if not same:
            print(json.dumps(res))
            raise SystemExit("the device and the g++-built header differ")

    # (c): the motion-model chain, everything resident
    B, q_cap = a.chain_frames, a.chain_points
    probs = [synth.synth_project(4000 + k, q_cap, "LAST_FRAME", 7.0) for k in range(B)]
    Pc, Rc, outs_c, keep_c = records(api, probs)
    port.cpu_project(B, Pc, Rc)
    rs = np.random.RandomState(1)
    kp = []
    for o in outs_c:                                                    # a keypoint near each accepted point, at its octave, and clutter
        seen = np.flatnonzero(o["status"] == 0)
        xy = o["uvr"][seen, :2] + rs.uniform(-0.5, 0.5, (len(seen), 2)) * o["uvr"][seen, 2:3]
        xy = np.concatenate([xy, np.stack([rs.uniform(0, 640, 300), rs.uniform(0, 480, 300)], 1)]).astype(np.float32)
        kp.append((xy, np.concatenate([o["level"][seen], rs.randint(0, 8, 300)]).astype(np.int32), seen))
    kp_cap = max(len(k[0]) for k in kp)
    t = dict(cameras=np.concatenate([api.project_camera_record(pr) for pr in probs]).view(np.float32).reshape(B, -1), m=np.full(B, q_cap, np.int32),
             pos=np.stack([pr["pos"].T for pr in probs]), normal=np.zeros((B, 3, q_cap), np.float32), max_dist=np.zeros((B, q_cap), np.float32),
             min_dist=np.zeros((B, q_cap), np.float32), octave=np.stack([pr["octave"] for pr in probs]), skip=np.stack([pr["skip"] for pr in probs]),
             n=np.array([len(k[0]) for k in kp], np.int32), desc=np.zeros((B, kp_cap, 32), np.uint8), kp_taken=np.zeros((B, kp_cap), np.uint8),
             qdesc=rs.randint(0, 256, (B, q_cap, 32)).astype(np.uint8), takes=(rs.rand(B, q_cap) < 0.9).astype(np.uint8),
             qangle=rs.uniform(0, 360, (B, q_cap)).astype(np.float32))
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    for f, (xy, octave, seen) in enumerate(kp):
        kps["x"][f, :len(xy)], kps["y"][f, :len(xy)], kps["octave"][f, :len(xy)] = xy[:, 0], xy[:, 1], octave
        kps["angle"][f, :len(xy)] = rs.uniform(0, 360, len(xy))
        kps["angle"][f, :len(seen)] = np.mod(t["qangle"][f, seen] - 20.0 + rs.uniform(-8, 8, len(seen)), 360.0)
        t["desc"][f, :len(xy)] = rs.randint(0, 256, (len(xy), 32))
        t["desc"][f, :len(seen)] = t["qdesc"][f, seen]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, q_cap), dtype=torch.uint8, device="cuda")
    for name, dt, w in OUT[3:]:
        d[name] = torch.zeros((B, q_cap, w) if w > 1 else (B, q_cap), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
    d.update(match_kp=torch.zeros((B, q_cap), dtype=torch.int32, device="cuda"), nmatches=torch.zeros(B, dtype=torch.int32, device="cuda"),
             kp_query=torch.zeros((B, kp_cap), dtype=torch.int32, device="cuda"), bins=torch.zeros((B, 3), dtype=torch.int32, device="cuda"))
    pr0 = probs[0]
    bounds = (float(pr0["min_x"]), float(pr0["min_y"]), float(np.float32(64) / np.float32(pr0["max_x"] - pr0["min_x"])),
              float(np.float32(48) / np.float32(pr0["max_y"] - pr0["min_y"])))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def launch_chain():
        api.project_batch_dev(d, stream=s.cuda_stream)
        api.ORBmatcher.guided_search_batch_dev(d, bounds, 100, False, 0.9, stream=s.cuda_stream)
        api.ORBmatcher.rotation_check_batch_dev(d, stream=s.cuda_stream)

    def chain_idle():
        launch_chain()
        s.synchronize()

    def timed_idle():
        for _ in range(a.warmup):
            chain_idle()
        ts = []
        for _ in range(a.reps):
            time.sleep(0.02)                                            # the device is idle when the chain starts
            t0 = time.perf_counter()
            chain_idle()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    run = 20

    def chain_run():
        for _ in range(run):
            launch_chain()
        s.synchronize()

    idle_ms, idle_min = timed_idle()
    same_q = all(np.array_equal(d[name][f].cpu().numpy().view(np.uint8), outs_c[f][name].view(np.uint8)) for name, _, _ in OUT[3:] for f in (0, B - 1))
    matches_before = int(d["nmatches"].sum())
    b2b_ms, b2b_min = median_ms(chain_run, 2, max(3, a.reps // 3))
    res["chain"] = {"workload": "%d frames x %d points, LAST_FRAME" % (B, q_cap), "c_chain_idle_ms_median": idle_ms, "c_chain_idle_ms_min": idle_min,
                    "c_chain_back_to_back_ms_median": b2b_ms / run, "c_chain_back_to_back_ms_min": b2b_min / run, "chains_per_run": run,
                    "matches_after_the_rotation_check": matches_before, "device_queries_equal_cpu_header_bit_for_bit": bool(same_q)}
    print(json.dumps(res))
    if not same_q:
        raise SystemExit("the device and the g++-built header differ")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
