"""Times the host-pointer entry points (the calls a Tracking / LocalMapping thread makes with plain arrays: stage, copy up, launch,
copy down) through the Python binding, each at one fixed size, and prints one JSON line of median milliseconds per call.

    python tools/bench_host_calls.py [--calls 200] [--warmup 20]

With --compare the same measurement is made on two builds of the library in turn, `rounds` fresh processes each, alternating, and the
medians, their round-to-round spread and the verdict per call are written as one record:

    python tools/bench_host_calls.py --compare /path/to/parent/libslamit_hip.so --rounds 3 --out profiles/rNN_host_calls.json

A call holds when the head's median of round medians is no slower than the parent's by more than the parent's own spread (max - min of
its round medians).  The comparison stops at the first process that fails.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAM = [526.69, 540.36, 313.07, 238.39, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314]


def cases():
    """name -> a function of no arguments that makes one call"""
    from weiner_slamit_v2_amd import api, synth

    rs = np.random.RandomState(1)
    out = {}
    pose1, pose64 = synth.synth_pose(1000, 0.15, 3), [synth.synth_pose(300, 0.15, 100 + i) for i in range(64)]
    out["pose_1x1000"] = lambda: api.Optimizer.PoseOptimization(pose1)
    out["pose_64x300"] = lambda: api.Optimizer.PoseOptimization(pose64)
    sim1, sim64 = synth.synth_sim3(300, 0.2, 3), [synth.synth_sim3(300, 0.2, 200 + i, 0.03) for i in range(64)]
    out["sim3_1x300"] = lambda: api.Optimizer.OptimizeSim3(sim1)
    out["sim3_64x300"] = lambda: api.Optimizer.OptimizeSim3(sim64)
    frame, queries = synth.synth_search(1000, 300, 3, retarget=False)
    out["guided_search_1000kp_300q"] = lambda: api.ORBmatcher.guided_search(frame, queries)
    s1, s2, groups, epi = synth.synth_bow(1000, 1000, 200, 1, mode=0)
    out["bow_1000x1000_200groups"] = lambda: api.ORBmatcher.bow_search(s1, s2, groups, mode=0, th=50, th_inclusive=True, nnratio=0.6, epi=epi)
    xy = (rs.rand(1000, 2) * [640, 480]).astype(np.float32)
    out["undistort_1000"] = lambda: api.Frame.undistort_points(CAM, xy)
    kps = np.zeros(1000, api.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = xy[:, 0], xy[:, 1], rs.randint(0, 8, 1000)
    b = api.Frame.ComputeImageBounds(CAM, 640, 480)
    out["frame_finish_1000"] = lambda: api.Frame.finish(CAM, kps, b[0], b[2], b[4], b[5])
    q, t = rs.randint(0, 256, (1000, 32)).astype(np.uint8), rs.randint(0, 256, (1000, 32)).astype(np.uint8)
    out["best2_1000x1000"] = lambda: api.ORBmatcher.best2(q, t)
    out["hamming_matrix_256x256"] = lambda: api.ORBmatcher.distance_matrix(q[:256], t[:256])
    offsets = np.concatenate([[0], np.cumsum(rs.randint(2, 21, 200))]).astype(np.int32)
    desc = rs.randint(0, 256, (int(offsets[-1]), 32)).astype(np.uint8)
    out["distinctive_200pts"] = lambda: api.ORBmatcher.distinctive(desc, offsets)
    # the "batch of problems" calls, on the generators of their own tools/bench_*.py: one problem, and 64 in one call
    fru = lambda m, n: [synth.synth_frustum(2000 + k, n, (1.0, 3.0, 5.0)[k % 3]) for k in range(m)]
    prj = lambda m, n: [synth.synth_project(3000 + k, n, (2 + k) % 6, (3.0, 10.0, 4.0, 7.5, 7.0, 10.0)[k % 6]) for k in range(m)]
    tri = lambda m, n: [synth.synth_triangulation_stereo(n, 900 + k, 0.05 + 0.7 * (k % 20) / 19.0, 0.2, 0.7, depth=(1.5, 40.0)) for k in range(m)]
    rgbd = lambda m, n, w, h: [synth.synth_rgbd(seed=k, n=n, width=w, height=h, pad=8) for k in range(m)]
    unp = lambda m, n: [synth.synth_unproject(seed=3000 + k, n=n, n_candidates=int(0.85 * n), n_close=int(0.3 * n), tie_at_cut=True, octave_bad_frac=0.0)
                        for k in range(m)]

    def ransac(m, n, nh, gen, key, sample):
        probs = []
        for k in range(m):
            pr, rk = gen(n, 0.3, 500 + k, 0.5), np.random.RandomState(k)
            pr[key] = sample(n, nh, lambda lo, hi: int(rk.randint(lo, hi + 1)))
            probs.append(pr)
        return probs

    def refine_jobs(probs):   # Refine() sees the inliers of a good hypothesis: here the true matches of the scene
        return [dict(pr, subset=~pr["true"]["bad"]) for pr in probs]

    for m, n in ((1, 1000), (64, 300)):
        tag = "%dx%d" % (m, n)
        for name, fn, probs in (("frustum", api.frustum_batch, fru(m, n)), ("project", api.project_batch, prj(m, n)), ("triangulate_stereo", api.triangulate_batch, tri(m, n)),
                                ("rgbd_depth", api.rgbd_depth_batch, rgbd(m, n, 640 if m == 1 else 160, 480 if m == 1 else 120)),
                                ("unproject_closest", api.unproject_closest_batch, unp(m, n))):
            out["%s_%s" % (name, tag)] = lambda fn=fn, probs=probs: fn(probs)
        pnp = ransac(m, n, 35, synth.synth_pnp, "quads", api.PnPsolver.sample_quads)
        out["pnp_ransac_%sx35hyp" % tag] = lambda pnp=pnp: api.PnPsolver.ransac(pnp)
        out["pnp_refine_%s" % tag] = lambda jobs=refine_jobs(pnp): api.PnPsolver.refine(jobs)
        s3 = ransac(m, n, 300 if m == 1 else 35, synth.synth_sim3_ransac, "triples", api.Sim3Solver.sample_triples)
        out["sim3_ransac_%sx%dhyp" % (tag, 300 if m == 1 else 35)] = lambda s3=s3: api.Sim3Solver.evaluate(s3, want_bits=False)
    return out


def measure(calls, warmup):
    res = {}
    for name, fn in cases().items():
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = round(float(np.median(ts)), 4)
    return res


def compare(parent_lib, rounds, calls, warmup, out_path):
    runs = {"parent": [], "head": []}
    for r in range(rounds):
        for side in ("parent", "head"):
            env = dict(os.environ)
            if side == "parent":
                env["SLAMIT_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("SLAMIT_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(calls), "--warmup", str(warmup)], env=env,
                               stdout=subprocess.PIPE, timeout=300)
            if p.returncode != 0:
                sys.exit("bench_host_calls: the %s run of round %d ended with status %d; nothing more is started" % (side, r, p.returncode))
            runs[side].append(json.loads(p.stdout.decode().strip().splitlines()[-1])["median_ms"])
            print("round %d %s: %s" % (r, side, runs[side][-1]), flush=True)
    rec = {"metric": "host_calls", "calls": calls, "warmup": warmup, "rounds": rounds, "entry_points": {}}
    for name in runs["head"][0]:
        p, h = [x[name] for x in runs["parent"]], [x[name] for x in runs["head"]]
        spread = max(p) - min(p)
        rec["entry_points"][name] = {"parent_ms": p, "head_ms": h, "parent_median_ms": float(np.median(p)), "head_median_ms": float(np.median(h)),
                                     "parent_spread_ms": round(spread, 4), "head_spread_ms": round(max(h) - min(h), 4),
                                     "holds": bool(np.median(h) <= np.median(p) + spread)}
    rec["all_hold"] = all(e["holds"] for e in rec["entry_points"].values())
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"all_hold": rec["all_hold"], "out": out_path}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--compare", metavar="PARENT_LIB", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="host_calls.json")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare, a.rounds, a.calls, a.warmup, a.out)
    from weiner_slamit_v2_amd import api

    print(json.dumps({"metric": "host_calls", "lib": api.LIB_PATH, "calls": a.calls, "warmup": a.warmup, "median_ms": measure(a.calls, a.warmup)}))


if __name__ == "__main__":
    main()
