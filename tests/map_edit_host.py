"""What the map-edit tests share: the arrays a call must leave, laid out from the restatement's result (tests/map_edit_ref.py) over the
caller's prefilled outputs; csrc/map_edit.h built with g++ behind a small main that takes any number of jobs; the comparison, exact."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests.helpers import ROOT
from tests.map_edit_ref import TABLE_OVERFLOW

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
EDIT_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("mp", "<i4"), ("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("weight", "u1"), ("pad", "u1", 2)])
# what the caller leaves in the outputs before the call
FILL = {"obs_ptr_out": -5, "obs_kf_out": -6, "obs_idx_out": -7, "obs_octave_out": 0xee, "obs_weight_out": 0xdd, "status_mp": -9, "touched": -8, "n_touched": -3}
OUT_TYPES = (("obs_ptr_out", np.int32), ("obs_kf_out", np.int32), ("obs_idx_out", np.int32), ("obs_octave_out", np.uint8), ("obs_weight_out", np.uint8),
             ("mp_bad", np.uint8), ("mp_nobs", np.int32), ("mp_ref_kf", np.int32), ("kf_mp", np.int32), ("status_mp", np.int32), ("touched", np.int32))
OUT_KEYS = tuple(k for k, _ in OUT_TYPES) + ("n_touched", "n_obs_out", "status")


def records(edits):
    out = np.zeros(len(edits), EDIT_DTYPE)
    for i, e in enumerate(edits):
        out[i] = tuple(int(v) for v in e) + ((0, 0),)
    return out


def default_cap(fx):
    return int(fx["t"]["obs_ptr"][-1]) + len(fx["edits"])


def laid_out(fx, want, cap):
    """Every array of OUT_KEYS as the call must leave it with obs_cap_out = cap over outputs prefilled with FILL: past the counts the
    fill stays, and with TABLE_OVERFLOW everything but n_obs_out and status keeps its bytes."""
    t, x, n_mp = fx["t"], fx["x"], fx["t"]["n_mp"]
    e = {"obs_ptr_out": np.full(n_mp + 1, FILL["obs_ptr_out"], np.int32), "status_mp": np.full(n_mp, FILL["status_mp"], np.int32),
         "touched": np.full(n_mp, FILL["touched"], np.int32), "n_touched": FILL["n_touched"], "n_obs_out": want["n_obs_out"], "status": want["status"]}
    for key, dt in OUT_TYPES[1:5]:
        e[key] = np.full(cap, FILL[key], dt)
    over = bool(want["status"] & TABLE_OVERFLOW)
    assert over == (want["n_obs_out"] > cap)
    for key, src in (("mp_bad", t), ("mp_nobs", x), ("mp_ref_kf", x), ("kf_mp", t)):
        e[key] = np.array(src[key] if over else want[key], dict(OUT_TYPES)[key]).reshape(-1)
    if not over:
        need = want["n_obs_out"]
        e["obs_ptr_out"][:] = want["obs_ptr"]
        for key in ("obs_kf", "obs_idx", "obs_octave", "obs_weight"):
            e[key + "_out"][:need] = want[key]
        e["status_mp"][:] = want["status_mp"]
        e["touched"][:want["n_touched"]] = want["touched"]
        e["n_touched"] = want["n_touched"]
    return e


def fills(fx, cap):
    n_mp = fx["t"]["n_mp"]
    f = {"obs_ptr_out": np.full(n_mp + 1, FILL["obs_ptr_out"], np.int32), "status_mp": np.full(n_mp, FILL["status_mp"], np.int32),
         "touched": np.full(n_mp, FILL["touched"], np.int32), "n_touched": FILL["n_touched"]}
    for key, dt in OUT_TYPES[1:5]:
        f[key] = np.full(cap, FILL[key], dt)
    return f


def assert_same(got, want, what=""):
    for k in OUT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s: %s" % (what, k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8] if a.shape == b.shape else (a.shape, b.shape))


def of_api(out):
    """api.map_edit's result under the names of OUT_KEYS, the arrays in full."""
    got = {k: out["raw"][k] for k, _ in OUT_TYPES}
    got.update(n_touched=out["n_touched"], n_obs_out=out["n_obs_out"], status=out["status"])
    return got


HOST_DRIVER = r"""
// csrc/map_edit.h's sequential statement over any number of jobs: per job a header, the tables and the list in, every output out.
// The refusals of slamit_map_edit_apply are restated by the caller: a job that reaches this program is valid.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "map_edit.h"

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
    int32_t h[4];   // n_kf n_mp n_edits obs_cap_out
    while (fread(h, 4, 4, f) == 4) {
        LmMap M = LmMap();
        MeIndex X = MeIndex();
        M.n_kf = h[0]; M.n_mp = h[1];
        std::vector<int32_t> obs_ptr = rd<int32_t>(f), obs_kf = rd<int32_t>(f), kf_mp_ptr = rd<int32_t>(f), kf_mp = rd<int32_t>(f);
        std::vector<uint8_t> mp_bad = rd<uint8_t>(f);
        std::vector<int32_t> obs_idx = rd<int32_t>(f);
        std::vector<uint8_t> obs_octave = rd<uint8_t>(f), obs_weight = rd<uint8_t>(f);
        std::vector<int32_t> mp_nobs = rd<int32_t>(f), mp_ref_kf = rd<int32_t>(f);
        std::vector<MeEdit> edits = rd<MeEdit>(f);
        std::vector<int32_t> obs_ptr_out = rd<int32_t>(f), obs_kf_out = rd<int32_t>(f), obs_idx_out = rd<int32_t>(f);
        std::vector<uint8_t> obs_octave_out = rd<uint8_t>(f), obs_weight_out = rd<uint8_t>(f);
        std::vector<int32_t> status_mp = rd<int32_t>(f), touched = rd<int32_t>(f), tail = rd<int32_t>(f);   // tail: n_touched n_obs_out status
        if ((int)edits.size() != h[2] || (int)obs_kf_out.size() != h[3] || tail.size() != 3) return 3;
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.data(); M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.data(); M.mp_bad = mp_bad.data();
        X.obs_idx = obs_idx.data(); X.obs_octave = obs_octave.data(); X.obs_weight = obs_weight.data();
        X.mp_bad = mp_bad.data(); X.mp_nobs = mp_nobs.data(); X.mp_ref_kf = mp_ref_kf.data(); X.kf_mp = kf_mp.data();
        X.obs_ptr_out = obs_ptr_out.data(); X.obs_kf_out = obs_kf_out.data(); X.obs_idx_out = obs_idx_out.data();
        X.obs_octave_out = obs_octave_out.data(); X.obs_weight_out = obs_weight_out.data(); X.obs_cap_out = h[3];
        std::vector<int32_t> bucket((size_t)h[2] + 1), start((size_t)h[1] + 2), stamp(kf_mp.size() + 1);
        me_apply_seq(M, X, h[2], edits.data(), status_mp.data(), touched.data(), &tail[0], &tail[1], &tail[2], bucket.data(), start.data(), stamp.data());
        wr(o, obs_ptr_out); wr(o, obs_kf_out); wr(o, obs_idx_out); wr(o, obs_octave_out); wr(o, obs_weight_out);
        wr(o, mp_bad); wr(o, mp_nobs); wr(o, mp_ref_kf); wr(o, kf_mp); wr(o, status_mp); wr(o, touched); wr(o, tail);
    }
    fclose(f);
    fclose(o);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False):
    d = tempfile.mkdtemp(prefix="map_edit_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "map_edit_host.cc"), os.path.join(d, "map_edit_host")
    open(src, "w").write(HOST_DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I", CSRC, src, "-o", exe] + extra)
    return exe


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return np.int32(len(a)).tobytes() + a.tobytes()


def job_bytes(fx, cap):
    t, x = fx["t"], fx["x"]
    ed = records(fx["edits"])
    blob = np.array([t["n_kf"], t["n_mp"], len(ed), cap], np.int32).tobytes()
    for key, dt, src in (("obs_ptr", np.int32, t), ("obs_kf", np.int32, t), ("kf_mp_ptr", np.int32, t), ("kf_mp", np.int32, t), ("mp_bad", np.uint8, t),
                         ("obs_idx", np.int32, x), ("obs_octave", np.uint8, x), ("obs_weight", np.uint8, x), ("mp_nobs", np.int32, x), ("mp_ref_kf", np.int32, x)):
        blob += _arr(src[key], dt)
    blob += np.int32(len(ed)).tobytes() + ed.tobytes()
    f = fills(fx, cap)
    for key, dt in OUT_TYPES[:5]:
        blob += _arr(f[key], dt)
    blob += _arr(f["status_mp"], np.int32) + _arr(f["touched"], np.int32) + _arr([f["n_touched"], -1, -1], np.int32)
    return blob


def host_run(jobs, sanitize=False):
    """jobs: (fixture, obs_cap_out) through csrc/map_edit.h on the host, in one process -> per job the arrays of OUT_KEYS in full."""
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(b"".join(job_bytes(fx, cap) for fx, cap in jobs))
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    o, outs = [0], []
    for fx, cap in jobs:
        n_mp, n_kfmp = fx["t"]["n_mp"], len(fx["t"]["kf_mp"])
        counts = {"obs_ptr_out": n_mp + 1, "obs_kf_out": cap, "obs_idx_out": cap, "obs_octave_out": cap, "obs_weight_out": cap, "mp_bad": n_mp, "mp_nobs": n_mp,
                  "mp_ref_kf": n_mp, "kf_mp": n_kfmp, "status_mp": n_mp, "touched": n_mp}
        out = {}
        for key, dt in OUT_TYPES:
            out[key] = np.frombuffer(raw, dt, counts[key], o[0]).copy()
            o[0] += out[key].nbytes
        out["n_touched"], out["n_obs_out"], out["status"] = (int(v) for v in np.frombuffer(raw, np.int32, 3, o[0]))
        o[0] += 12
        outs.append(out)
    assert o[0] == len(raw)
    return outs
