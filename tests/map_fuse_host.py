"""What the map-fuse tests share: the arrays a call must leave, laid out from the restatement's result (tests/map_fuse_ref.py) over the
caller's prefilled outputs; csrc/map_fuse.h built with g++ behind a small main that takes any number of jobs; the comparison, exact.
The layouts are tests/map_replace_host.py's with `outcome` per op and `n_fused` beside them."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import map_replace_host as mrh
from tests.map_fuse_ref import default_cap as ref_default_cap
from tests.map_replace_host import CSRC, INPLACE, records   # noqa: F401  (records: the ops as slamit_map_replace)
from tests.map_replace_ref import OBS_OVERFLOW, TABLE_OVERFLOW

FILL = dict(mrh.FILL, outcome=-11, n_fused=-12)
OUT_TYPES = mrh.OUT_TYPES + (("outcome", np.int32),)
OUT_KEYS = tuple(k for k, _ in OUT_TYPES) + ("n_touched", "n_fused", "n_obs_out", "status")


def default_cap(fx):
    return ref_default_cap(fx["t"], fx["ops"])


def fills(fx, cap):
    f = mrh.fills(fx, cap)
    f.update(outcome=np.full(len(fx["ops"]), FILL["outcome"], np.int32), n_fused=FILL["n_fused"])
    return f


def laid_out(fx, want, cap):
    """Every array of OUT_KEYS as the call must leave it with obs_cap_out = cap over outputs prefilled with FILL."""
    refused = bool(want["status"] & (OBS_OVERFLOW | TABLE_OVERFLOW))
    e = mrh.laid_out(fx, want, cap)
    e["outcome"], e["n_fused"] = np.full(len(fx["ops"]), FILL["outcome"], np.int32), FILL["n_fused"]
    if not refused:
        e["outcome"][:], e["n_fused"] = want["outcome"], want["n_fused"]
    return e


def assert_same(got, want, what=""):
    for k in OUT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s: %s" % (what, k, (np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8], a.reshape(-1)[:8], b.reshape(-1)[:8])
                                                                                   if a.shape == b.shape else (a.shape, b.shape))


def of_api(out):
    """api.map_fuse's result under the names of OUT_KEYS, the arrays in full."""
    got = {k: out["raw"][k] for k, _ in OUT_TYPES}
    got.update(n_touched=out["raw"]["n_touched"], n_fused=out["raw"]["n_fused"], n_obs_out=out["raw"]["n_obs_out"], status=out["status"])
    return got


HOST_DRIVER = r"""
// csrc/map_fuse.h's sequential statement over any number of jobs: per job a header, the tables and the list in, every output out.
// The refusals of slamit_map_fuse_apply are restated by the caller: a job that reaches this program is valid.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "map_fuse.h"

template <typename T> static std::vector<T> rd(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v((size_t)n + 1);   // never empty: data() is an address
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) exit(2);
    v.resize((size_t)n);               // a sanitizer sees the true end; the storage stays
    return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    int32_t h[4];   // n_kf n_mp n_ops obs_cap_out
    while (fread(h, 4, 4, f) == 4) {
        LmMap M = LmMap();
        MrIndex X = MrIndex();
        M.n_kf = h[0]; M.n_mp = h[1];
        std::vector<int32_t> obs_ptr = rd<int32_t>(f), obs_kf = rd<int32_t>(f), kf_mp_ptr = rd<int32_t>(f), kf_mp = rd<int32_t>(f);
        std::vector<uint8_t> mp_bad = rd<uint8_t>(f);
        std::vector<int32_t> obs_idx = rd<int32_t>(f);
        std::vector<uint8_t> obs_octave = rd<uint8_t>(f), obs_weight = rd<uint8_t>(f);
        std::vector<int32_t> mp_nobs = rd<int32_t>(f), mp_found = rd<int32_t>(f), mp_visible = rd<int32_t>(f), mp_replaced = rd<int32_t>(f);
        std::vector<MrOp> ops = rd<MrOp>(f);
        std::vector<int32_t> obs_ptr_out = rd<int32_t>(f), obs_kf_out = rd<int32_t>(f), obs_idx_out = rd<int32_t>(f);
        std::vector<uint8_t> obs_octave_out = rd<uint8_t>(f), obs_weight_out = rd<uint8_t>(f);
        std::vector<int32_t> moved = rd<int32_t>(f), erased = rd<int32_t>(f), touched = rd<int32_t>(f), outcome = rd<int32_t>(f);
        std::vector<int32_t> tail = rd<int32_t>(f);   // n_touched n_fused n_obs_out status
        if ((int)ops.size() != h[2] || (int)obs_kf_out.size() != h[3] || tail.size() != 4) return 3;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.data(); M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.data(); M.mp_bad = mp_bad.data();
        X.obs_idx = obs_idx.data(); X.obs_octave = obs_octave.data(); X.obs_weight = obs_weight.data();
        X.mp_bad = mp_bad.data(); X.mp_nobs = mp_nobs.data(); X.mp_found = mp_found.data(); X.mp_visible = mp_visible.data(); X.mp_replaced = mp_replaced.data();
        X.kf_mp = kf_mp.data();
        X.obs_ptr_out = obs_ptr_out.data(); X.obs_kf_out = obs_kf_out.data(); X.obs_idx_out = obs_idx_out.data();
        X.obs_octave_out = obs_octave_out.data(); X.obs_weight_out = obs_weight_out.data(); X.obs_cap_out = h[3];
        mf_apply_seq(M, X, h[2], ops.data(), outcome.data(), moved.data(), erased.data(), touched.data(), &tail[0], &tail[1], &tail[2], &tail[3]);
        wr(o, obs_ptr_out); wr(o, obs_kf_out); wr(o, obs_idx_out); wr(o, obs_octave_out); wr(o, obs_weight_out);
        wr(o, mp_bad); wr(o, mp_nobs); wr(o, mp_found); wr(o, mp_visible); wr(o, mp_replaced); wr(o, kf_mp); wr(o, moved); wr(o, erased); wr(o, touched);
        wr(o, outcome); wr(o, tail);
    }
    fclose(f);
    fclose(o);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False):
    d = tempfile.mkdtemp(prefix="map_fuse_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "map_fuse_host.cc"), os.path.join(d, "map_fuse_host")
    open(src, "w").write(HOST_DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I", CSRC, src, "-o", exe] + extra)   # without include/slamit.h
    return exe


def job_bytes(fx, cap):
    t, x = fx["t"], fx["x"]
    ed = records(fx["ops"])
    blob = np.array([t["n_kf"], t["n_mp"], len(ed), cap], np.int32).tobytes()
    for key, dt, src in (("obs_ptr", np.int32, t), ("obs_kf", np.int32, t), ("kf_mp_ptr", np.int32, t), ("kf_mp", np.int32, t), ("mp_bad", np.uint8, t),
                         ("obs_idx", np.int32, x), ("obs_octave", np.uint8, x), ("obs_weight", np.uint8, x), ("mp_nobs", np.int32, x), ("mp_found", np.int32, x),
                         ("mp_visible", np.int32, x), ("mp_replaced", np.int32, x)):
        blob += mrh._arr(src[key], dt)
    blob += np.int32(len(ed)).tobytes() + ed.tobytes()
    f = fills(fx, cap)
    for key, dt in OUT_TYPES[:5]:
        blob += mrh._arr(f[key], dt)
    for key in ("moved", "erased", "touched", "outcome"):
        blob += mrh._arr(f[key], np.int32)
    return blob + mrh._arr([f["n_touched"], f["n_fused"], f["n_obs_out"], -1], np.int32)


def host_run(jobs, sanitize=False):
    """jobs: (fixture, obs_cap_out) through csrc/map_fuse.h on the host, in one process -> per job the arrays of OUT_KEYS in full."""
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(b"".join(job_bytes(fx, cap) for fx, cap in jobs))
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    o, outs = 0, []
    for fx, cap in jobs:
        n_mp, n_kfmp, n = fx["t"]["n_mp"], len(fx["t"]["kf_mp"]), len(fx["ops"])
        counts = {"obs_ptr_out": n_mp + 1, "obs_kf_out": cap, "obs_idx_out": cap, "obs_octave_out": cap, "obs_weight_out": cap, "mp_bad": n_mp, "mp_nobs": n_mp,
                  "mp_found": n_mp, "mp_visible": n_mp, "mp_replaced": n_mp, "kf_mp": n_kfmp, "moved": n, "erased": n, "touched": n_mp, "outcome": n}
        out = {}
        for key, dt in OUT_TYPES:
            out[key] = np.frombuffer(raw, dt, counts[key], o).copy()
            o += out[key].nbytes
        out["n_touched"], out["n_fused"], out["n_obs_out"], out["status"] = (int(v) for v in np.frombuffer(raw, np.int32, 4, o))
        o += 16
        outs.append(out)
    assert o == len(raw)
    return outs
