"""The right-image column of the two projections whose search reads one (csrc/project.h, project_point_stereo):
csrc/project.h behind a small main of its own through g++, and a numpy restatement of ur = u - bf * invz with each form's invz.

    LAST_FRAME  ORBmatcher.cc:1369, :1413   invzc = 1.0 / x3Dc.at<float>(2): a double division rounded to float
    FUSE        ORBmatcher.cc:860, :874     invz = 1 / p3Dc.at<float>(2): a float division
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import project_ref as ref

STEREO_DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "project.h"
// <in> <out> <bf>: the blob of tests/project_ref.py's driver -> that driver's output, then ur[n] (float)
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const float bf = strtof(argv[3], NULL);
    int n;
    ProjectCamera C;
    if (fread(&n, 4, 1, f) != 1 || fread(&C, sizeof(C), 1, f) != 1 || n < 0) return 2;
    std::vector<float> pos(3 * (size_t)n), nrm(3 * (size_t)n), maxd(n), mind(n);
    std::vector<int> octave(n);
    std::vector<unsigned char> skip(n);
    size_t got = fread(pos.data(), 4, 3 * (size_t)n, f) + fread(nrm.data(), 4, 3 * (size_t)n, f) + fread(maxd.data(), 4, n, f) + fread(mind.data(), 4, n, f);
    got += fread(octave.data(), 4, n, f) + fread(skip.data(), 1, n, f);
    fclose(f);
    if (got != 10 * (size_t)n) return 2;
    std::vector<unsigned char> st(n), valid(n);
    std::vector<float> fl(3 * (size_t)n), uvr(3 * (size_t)n), ur(n);
    std::vector<int> level(n), l0(n), l1(n);
    for (int i = 0; i < n; ++i) {
        ProjectOut o;
        st[i] = (unsigned char)project_point_stereo(C, &pos[3 * (size_t)i], &nrm[3 * (size_t)i], maxd[i], mind[i], octave[i], skip[i] != 0, bf, o, ur[i]);
        fl[i] = o.u; fl[(size_t)n + i] = o.v; fl[2 * (size_t)n + i] = o.r;
        level[i] = o.level;
        project_query(C, st[i], o, &uvr[3 * (size_t)i], l0[i], l1[i], valid[i]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(st.data(), 1, n, o); fwrite(fl.data(), 4, 3 * (size_t)n, o); fwrite(level.data(), 4, n, o); fwrite(uvr.data(), 4, 3 * (size_t)n, o);
    fwrite(l0.data(), 4, n, o); fwrite(l1.data(), 4, n, o); fwrite(valid.data(), 1, n, o); fwrite(ur.data(), 4, n, o);
    fclose(o);
    return 0;
}
'''

BF = {ref.LAST_FRAME: 38.6, ref.FUSE: 41.25}   # mbf of the two test cameras (a 7.5 cm and an 8 cm baseline at fx about 517)


@functools.lru_cache(maxsize=None)
def stereo_exe():
    d = tempfile.mkdtemp(prefix="project_stereo_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "project_stereo_host.cc"), os.path.join(d, "project_stereo_host")
    open(src, "w").write(STEREO_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-I", ref.CSRC, src, "-o", exe])
    return exe


def host_points_stereo(pr, bf):
    """csrc/project.h's project_point_stereo through g++ -> project_ref.host_points' dict plus ur (n) float32"""
    exe = stereo_exe()
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(ref.problem_blob(pr))
    subprocess.check_call([exe, pin, pout, repr(float(np.float32(bf)))])
    raw = open(pout, "rb").read()
    n = int(pr["n"])
    out = ref.parse_host_output(raw[:len(raw) - 4 * n], n)
    out["ur"] = np.frombuffer(raw, np.float32, n, len(raw) - 4 * n).copy()
    return out


def ur_numpy(pr, bf, status):
    """u - bf * invz in float32, two roundings, for the points of status 0; zero otherwise.  Forms LAST_FRAME and FUSE.
    -> (ur, u): u is the restatement's own column, for the caller to hold against the header's."""
    lo, f64 = np.float32, np.float64
    form = int(pr["form"])
    assert form in (ref.LAST_FRAME, ref.FUSE)
    n = int(pr["n"])
    P = np.asarray(pr["pos"], lo).reshape(n, 3)
    R, t = np.asarray(pr["R"], lo).reshape(3, 3), np.asarray(pr["t"], lo)
    with np.errstate(all="ignore"):
        # cv::gemm's small-matrix branch: the dot in float, left to right, then (float)((double)t0 + (double)t)
        pc = [((((R[r, 0] * P[:, 0] + R[r, 1] * P[:, 1]) + R[r, 2] * P[:, 2]).astype(f64)) + f64(t[r])).astype(lo) for r in range(3)]
        if form == ref.LAST_FRAME:
            invz = (f64(1.0) / pc[2].astype(f64)).astype(lo)
            u = lo(pr["fx"]) * pc[0] * invz + lo(pr["cx"])
        else:
            invz = lo(1) / pc[2]
            u = lo(pr["fx"]) * (pc[0] * invz) + lo(pr["cx"])
        ur = u - lo(bf) * invz
    ok = np.asarray(status) == 0
    return np.where(ok, ur, lo(0)).astype(lo), np.where(ok, u, lo(0)).astype(lo)
