"""Times slamit_triangulate_stereo_batch: 20 and 160 keyframe pairs x 300 matched pairs of stereo keyframes in one call, against
tri_pair_stereo of csrc/triangulate.h itself compiled with g++ -O3 and run on one core -- the method of tools/bench_triangulate.py --
and the OLD monocular symbol of this tree against the parent commit's library, loaded side by side in one process.

    python tools/bench_triangulate_stereo.py [--parent-lib PATH] [--reps 50] [--warmup 10] [--rounds 9] [--out profiles/r19_triangulate_stereo.json]

Stereo: warm-up calls first, then the median of the repetitions (wall clock around the synchronous call, host staging and both
copies included).  The comparator's statuses and sources must equal the device's on every pair, or the tool fails.  Recorded, not
bounded.  Monocular (with --parent-lib): slamit_triangulate_batch of the two libraries alternates over `rounds` rounds (parent, head,
parent, ...), each round the median of `reps` calls of the 160-problem batch after 3 warm-up calls; the answers must be bit-equal,
or the tool fails.  `within_parent_spread`: this tree's median over the rounds lies within the parent's own min..max over the
rounds, widened on both sides by that same max - min."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CPU_PORT = r'''
// the kernel's per-pair text on one core, over the same records the C-ABI takes
#include <stdint.h>
#include "slamit.h"
#include "triangulate.h"
extern "C" void cpu_triangulate_stereo(int nprob, const slamit_triangulate_problem* probs, const slamit_triangulate_stereo_rec* const* stereo,
                                       slamit_triangulate_result* res, uint8_t* const* source) {
    for (int p = 0; p < nprob; ++p) {
        const slamit_triangulate_problem& P = probs[p];
        const slamit_triangulate_stereo_rec& T = *stereo[p];
        TriView c1, c2;
        for (int k = 0; k < 12; ++k) { c1.T[k] = P.Tcw1[k]; c2.T[k] = P.Tcw2[k]; }
        c1.fx = P.intr1[0]; c1.fy = P.intr1[1]; c1.cx = P.intr1[2]; c1.cy = P.intr1[3]; c1.invfx = P.intr1[4]; c1.invfy = P.intr1[5];
        c2.fx = P.intr2[0]; c2.fy = P.intr2[1]; c2.cx = P.intr2[2]; c2.cy = P.intr2[3]; c2.invfx = P.intr2[4]; c2.invfy = P.intr2[5];
        tri_centre(c1); tri_centre(c2);
        int acc = 0;
        for (int i = 0; i < P.n; ++i) {
            const int o1 = P.octave1[i], o2 = P.octave2[i];
            const TriStereoPair s = {T.ur1[i], T.ur2[i], T.depth1[i], T.depth2[i], {T.raw1_xy[2 * i], T.raw1_xy[2 * i + 1]}, {T.raw2_xy[2 * i], T.raw2_xy[2 * i + 1]}};
            int src;
            const int st = tri_pair_stereo(c1, c2, P.kp1_xy + 2 * i, P.kp2_xy + 2 * i, s, T.mb1, T.mb2, T.bf, P.level_sigma2_1[o1], P.level_sigma2_2[o2],
                                           P.scale_factors1[o1], P.scale_factors2[o2], P.ratio_factor, res[p].x3d + 3 * i, src);
            res[p].status[i] = (uint8_t)st;
            source[p][i] = (uint8_t)src;
            acc += st == 0;
        }
        res[p].n_accepted = acc;
    }
}
'''

STEREO_KEYS = ("ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy")


def stereo_records(api, probs):
    """The stereo records of a list of problem dicts and their source outputs: (T pointers, SRC pointers, sources, keep-alive)."""
    m = len(probs)
    T, SRC = (C.POINTER(api.TriangulateStereo) * m)(), (C.c_void_p * m)()
    srcs, keep = [], []
    for i, pr in enumerate(probs):
        t = api.TriangulateStereo()
        k = {key: np.ascontiguousarray(pr[key], np.float32) for key in STEREO_KEYS}
        for key, arr in k.items():
            setattr(t, key, arr.ctypes.data)
        t.mb1, t.mb2, t.bf = float(pr["mb1"]), float(pr["mb2"]), float(pr["bf"])
        T[i] = C.pointer(t)
        s = np.full(int(pr["n"]), 255, np.uint8)
        SRC[i] = s.ctypes.data
        srcs.append(s)
        keep.append((k, t))
    return T, SRC, srcs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_triangulate_stereo.json"))
    a = ap.parse_args()
    from bench_triangulate import median_ms, records
    from weiner_slamit_v2_amd import api, synth

    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "port.cc"), "w").write(CPU_PORT)
    so = os.path.join(tmp, "port.so")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "port.cc"), "-o", so])
    port = C.CDLL(so)
    res = {"workload": "N problems x 300 pairs of stereo keyframes (synth_triangulation_stereo), one slamit_triangulate_stereo_batch call",
           "comparator": "tri_pair_stereo of csrc/triangulate.h compiled with g++ -O3, one core", "reps": a.reps, "warmup": a.warmup, "cases": []}
    L = api.lib()
    for nprob in (20, 160):
        probs = [synth.synth_triangulation_stereo(300, 900 + k, 0.05 + 0.7 * (k % 20) / 19.0, 0.2, 0.7, depth=(1.5, 40.0)) for k in range(nprob)]
        bind_ms, _ = median_ms(lambda: api.triangulate_batch(probs), a.warmup, a.reps)
        P, R, outs, keep = records(api, probs)
        T, SRC, srcs, keep_t = stereo_records(api, probs)
        assert L.slamit_triangulate_stereo_batch(0, nprob, P, T, R, SRC) == 0, L.slamit_last_error()
        call_ms, call_min = median_ms(lambda: L.slamit_triangulate_stereo_batch(0, nprob, P, T, R, SRC), a.warmup, a.reps)
        Pc, Rc, outs_c, keep_c = records(api, probs)
        Tc, SRCc, srcs_c, keep_tc = stereo_records(api, probs)
        cpu_ms, cpu_min = median_ms(lambda: port.cpu_triangulate_stereo(nprob, Pc, Tc, Rc, SRCc), 2, a.reps)
        same = all(np.array_equal(g[0], c[0]) for g, c in zip(outs, outs_c)) and all(np.array_equal(g, c) for g, c in zip(srcs, srcs_c))
        same_x = all(np.array_equal(g[1].view(np.uint32), c[1].view(np.uint32)) for g, c in zip(outs, outs_c))
        src_all = np.concatenate(srcs)
        res["cases"].append({"problems": nprob, "pairs_per_call": 300 * nprob, "accepted": int(sum(R[i].n_accepted for i in range(nprob))),
                             "sources": np.bincount(src_all, minlength=4).tolist(),
                             "gpu_binding_ms_median": bind_ms, "gpu_c_call_ms_median": call_ms, "gpu_c_call_ms_min": call_min,
                             "cpu_header_ms_median": cpu_ms, "cpu_header_ms_min": cpu_min, "speedup_c_call_vs_cpu_header": cpu_ms / call_ms,
                             "statuses_and_sources_equal_cpu_header": bool(same), "points_bit_equal_cpu_header": bool(same_x),
                             "n_accepted_equal": all(R[i].n_accepted == Rc[i].n_accepted for i in range(nprob))})
        if not same:
            print(json.dumps(res))
            raise SystemExit("statuses or sources differ between the device and the g++-built header")
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.slamit_triangulate_batch.argtypes = [C.c_int, C.c_int, C.POINTER(api.TriangulateProblem), C.POINTER(api.TriangulateResult)]
        nprob = 160
        probs = [synth.synth_triangulation(300, 900 + k, 0.05 + 0.7 * (k % 20) / 19.0, 0.2, 0.7) for k in range(nprob)]
        Pp, Rp, outs_p, keep_p = records(api, probs)
        Ph, Rh, outs_h, keep_h = records(api, probs)
        variants = {"parent": lambda: parent.slamit_triangulate_batch(0, nprob, Pp, Rp), "head": lambda: L.slamit_triangulate_batch(0, nprob, Ph, Rh)}
        for name, fn in variants.items():
            if fn() != 0:
                raise SystemExit("bench_triangulate_stereo: %s failed" % name)
        if not all(np.array_equal(p[0], h[0]) and np.array_equal(p[1].view(np.uint32), h[1].view(np.uint32)) for p, h in zip(outs_p, outs_h)):
            raise SystemExit("bench_triangulate_stereo: the monocular answers of the two libraries differ")
        runs = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                runs[name].append(median_ms(fn, 3, a.reps)[0])
        mono = {"what": "slamit_triangulate_batch (the old symbol), 160 problems x 300 monocular pairs, ms per call; %d rounds alternating the two libraries, "
                        "each round the median of %d calls after 3 warm-up calls; answers bit-equal" % (a.rounds, a.reps)}
        for name, r in runs.items():
            mono[name] = {"median_ms": round(float(np.median(r)), 4), "min_ms": round(float(np.min(r)), 4), "max_ms": round(float(np.max(r)), 4),
                          "runs_ms": [round(float(x), 4) for x in r]}
        spread = mono["parent"]["max_ms"] - mono["parent"]["min_ms"]
        mono["parent_spread_ms"] = round(spread, 4)
        mono["within_parent_spread"] = bool(mono["parent"]["min_ms"] - spread <= mono["head"]["median_ms"] <= mono["parent"]["max_ms"] + spread)
        res["monocular_against_parent"] = mono
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if a.parent_lib and not res["monocular_against_parent"]["within_parent_spread"]:
        raise SystemExit("bench_triangulate_stereo: the monocular median lies outside the parent's widened min..max")


if __name__ == "__main__":
    main()
