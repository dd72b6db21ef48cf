"""What the map-point upkeep tests share: the expected arrays of a call, from the restatement (tests/upkeep_ref.py) and the stated
departures; csrc/upkeep.h built with g++ behind a small main that takes any number of jobs; the comparison, bit for bit."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests.helpers import ROOT
from tests.upkeep_ref import MapPointCulling, objects

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
REF_NOT_OBSERVER, NO_REF, REF_NO_KP, OCTAVE, DESC_OVERFLOW, OBS_OVERFLOW, BAD_SLOT = 1, 2, 4, 8, 16, 32, 64
MAX_OBS, MAX_DESC = 512, 128
PLANES = ("mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc")
UP_OUTPUTS = ("status",) + PLANES
CULL_OUTPUTS = ("verdict", "kept", "n_kept", "status")
VERDICT_FILL, KEPT_FILL = 0xee, -77                       # what the caller leaves in the in / out arrays
MAP_TABLES = (("obs_ptr", np.int32), ("obs_kf", np.int32), ("mp_bad", np.uint8), ("kf_bad", np.uint8), ("kf_mp_ptr", np.int32), ("mp_pos", np.float32))
POINT_TABLES = (("obs_idx", np.int32), ("obs_octave", np.uint8), ("kf_octave", np.uint8), ("kf_center", np.float32), ("kf_desc", np.uint8),
                ("mp_ref_kf", np.int32), ("mp_nobs", np.int32), ("mp_found", np.int32), ("mp_visible", np.int32), ("mp_first_kf", np.int32),
                ("mp_normal", np.float32), ("mp_max_dist", np.float32), ("mp_min_dist", np.float32), ("mp_desc", np.uint8))


def up_expected(t, x, points, what):
    """The listed points through the restatement on fresh mock objects -> status per entry and the four planes of the whole map.  Where
    the reference reads out of bounds (no reference keyframe, one without keypoints, a level outside the table) the restatement raises and
    the point keeps its normal and distances; the ceilings leave what they name.  A slot outside the table is BAD_SLOT and nothing else."""
    kfs, mps = objects(t, x)
    status = []
    for p in points:
        if not 0 <= p < t["n_mp"]:
            status.append(BAD_SLOT)
            continue
        mp, st = mps[p], 0
        if mp.isBad() or not mp.mObservations:
            status.append(0)
            continue
        if len(mp.mObservations) > MAX_OBS:
            status.append(OBS_OVERFLOW)
            continue
        if what & 1:
            ref = mp.mpRefKF
            if ref is None:
                st |= NO_REF
            else:
                if ref not in mp.mObservations:
                    st |= REF_NOT_OBSERVER
                    if not ref.octave:
                        st |= REF_NO_KP
                if not st & REF_NO_KP and ref.octave[mp.mObservations.get(ref, 0)] >= x["n_levels"]:
                    st |= OCTAVE
            before = (list(mp.mNormalVector), mp.mfMaxDistance, mp.mfMinDistance)
            try:
                mp.UpdateNormalAndDepth()
                assert not st & (NO_REF | REF_NO_KP | OCTAVE) and mp.default_inserted == bool(st & REF_NOT_OBSERVER)
            except (AttributeError, IndexError):
                assert st & (NO_REF | REF_NO_KP | OCTAVE) and before == (list(mp.mNormalVector), mp.mfMaxDistance, mp.mfMinDistance)
        if what & 2:
            if sum(not kf.isBad() for kf in mp.mObservations) > MAX_DESC:
                st |= DESC_OVERFLOW
            else:
                mp.ComputeDistinctiveDescriptors()
        status.append(st)
    n_mp = t["n_mp"]
    return {"status": np.array(status, np.int32).reshape(-1),
            "mp_normal": np.array([m.mNormalVector for m in mps], np.float32).reshape(n_mp, 3),
            "mp_max_dist": np.array([m.mfMaxDistance for m in mps], np.float32).reshape(n_mp),
            "mp_min_dist": np.array([m.mfMinDistance for m in mps], np.float32).reshape(n_mp),
            "mp_desc": np.array([m.mDescriptor for m in mps], np.uint8).reshape(n_mp, 32)}


def cull_expected(t, x, recent, cur_id, monocular, cap=None):
    """MapPointCulling on a recent list through the restatement -> verdict / kept laid into prefilled arrays of `cap` entries, n_kept,
    status, and set_bad: the slots SetBadFlag would run on, in order."""
    _, mps = objects(t, x)
    lst = [mps[p] for p in recent]
    verdicts, set_bad = MapPointCulling(lst, cur_id, monocular)
    cap = len(recent) if cap is None else cap
    e = {"verdict": np.full(cap, VERDICT_FILL, np.uint8), "kept": np.full(cap, KEPT_FILL, np.int32), "n_kept": len(lst), "status": 0}
    e["verdict"][:len(verdicts)] = verdicts
    e["kept"][:len(lst)] = [m.slot for m in lst]
    e["set_bad"] = [m.slot for m in set_bad]
    return e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, keys, what=""):
    for k in keys:
        a, b = bits(np.asarray(got[k])), bits(np.asarray(want[k]))
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s: %s" % (what, k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8] if a.shape == b.shape else (a.shape, b.shape))


HOST_DRIVER = r"""
// csrc/upkeep.h's sequential statement over any number of jobs: per job a header, the tables and the lists in, the results out.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "upkeep.h"

template <typename T> static std::vector<T> rd(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v((size_t)n + 1);   // never empty: data() is an address
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) exit(2);
    return v;
}
template <typename T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    int32_t h[8];   // n_kf n_mp n_levels n_points what n_recent cur_id monocular
    while (fread(h, 4, 8, f) == 8) {
        LmMap M = LmMap();
        UpIndex X = UpIndex();
        M.n_kf = h[0]; M.n_mp = h[1]; X.n_levels = h[2];
        std::vector<float> sf = rd<float>(f);
        for (int i = 0; i < UNP_MAX_LEVELS; ++i) X.scale_factors[i] = sf[(size_t)i];
        std::vector<int32_t> obs_ptr = rd<int32_t>(f), obs_kf = rd<int32_t>(f);
        std::vector<uint8_t> mp_bad = rd<uint8_t>(f), kf_bad = rd<uint8_t>(f);
        std::vector<int32_t> kf_mp_ptr = rd<int32_t>(f);
        std::vector<float> mp_pos = rd<float>(f);
        std::vector<int32_t> obs_idx = rd<int32_t>(f);
        std::vector<uint8_t> obs_octave = rd<uint8_t>(f), kf_octave = rd<uint8_t>(f);
        std::vector<float> kf_center = rd<float>(f);
        std::vector<uint8_t> kf_desc = rd<uint8_t>(f);
        std::vector<int32_t> mp_ref_kf = rd<int32_t>(f), mp_nobs = rd<int32_t>(f), mp_found = rd<int32_t>(f), mp_visible = rd<int32_t>(f), mp_first_kf = rd<int32_t>(f);
        std::vector<float> mp_normal = rd<float>(f), mp_max_dist = rd<float>(f), mp_min_dist = rd<float>(f);
        std::vector<uint8_t> mp_desc = rd<uint8_t>(f);
        std::vector<int32_t> points = rd<int32_t>(f), recent = rd<int32_t>(f);
        std::vector<uint8_t> verdict = rd<uint8_t>(f);
        std::vector<int32_t> kept = rd<int32_t>(f);
        M.obs_ptr = obs_ptr.data(); M.obs_kf = obs_kf.data(); M.mp_bad = mp_bad.data(); M.kf_bad = kf_bad.data(); M.kf_mp_ptr = kf_mp_ptr.data();
        M.mp_pos = mp_pos.data();
        X.obs_idx = obs_idx.data(); X.obs_octave = obs_octave.data(); X.kf_octave = kf_octave.data(); X.kf_center = kf_center.data();
        X.kf_desc = kf_desc.data(); X.mp_ref_kf = mp_ref_kf.data(); X.mp_nobs = mp_nobs.data(); X.mp_found = mp_found.data();
        X.mp_visible = mp_visible.data(); X.mp_first_kf = mp_first_kf.data(); X.mp_normal = mp_normal.data(); X.mp_max_dist = mp_max_dist.data();
        X.mp_min_dist = mp_min_dist.data(); X.mp_desc = mp_desc.data();
        std::vector<int32_t> status((size_t)h[3] + 1);
        std::vector<uint32_t> keys(UP_MAX_OBS);
        std::vector<const uint8_t*> rows(UP_MAX_DESC);
        up_points_seq(M, X, h[3], points.data(), h[4], status.data(), keys.data(), rows.data());
        wr(o, status.data(), (size_t)h[3]);
        wr(o, mp_normal.data(), 3 * (size_t)M.n_mp); wr(o, mp_max_dist.data(), (size_t)M.n_mp); wr(o, mp_min_dist.data(), (size_t)M.n_mp);
        wr(o, mp_desc.data(), 32 * (size_t)M.n_mp);
        int32_t tail[2] = {-1, 0};
        up_culling_seq(M, X, h[6], h[7] != 0, h[5], recent.data(), verdict.data(), kept.data(), &tail[0], tail[1]);
        wr(o, verdict.data(), (size_t)h[5]); wr(o, kept.data(), (size_t)h[5]); wr(o, tail, 2);
    }
    fclose(f);
    fclose(o);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def host_exe():
    d = tempfile.mkdtemp(prefix="upkeep_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "upkeep_host.cc"), os.path.join(d, "upkeep_host")
    open(src, "w").write(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-Wall", "-I", CSRC, src, "-o", exe])
    return exe


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return np.int32(len(a)).tobytes() + a.tobytes()


def host_run(jobs):
    """jobs: dicts(t, x, points, what, recent, cur_id, monocular) through csrc/upkeep.h on the host, in one process -> per job the arrays of
    UP_OUTPUTS and CULL_OUTPUTS (verdict and kept prefilled as cull_expected prefills them)."""
    blob = b""
    for j in jobs:
        t, x = j["t"], j["x"]
        blob += np.array([t["n_kf"], t["n_mp"], x["n_levels"], len(j["points"]), j["what"], len(j["recent"]), j["cur_id"], int(j["monocular"])], np.int32).tobytes()
        blob += _arr(x["scale_factors"], np.float32)
        for key, dt in MAP_TABLES:
            blob += _arr(t[key], dt)
        for key, dt in POINT_TABLES:
            blob += _arr(x[key], dt)
        blob += _arr(j["points"], np.int32) + _arr(j["recent"], np.int32)
        blob += _arr(np.full(len(j["recent"]), VERDICT_FILL, np.uint8), np.uint8) + _arr(np.full(len(j["recent"]), KEPT_FILL, np.int32), np.int32)
    exe = host_exe()
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(blob)
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    o, outs = [0], []

    def take(dt, count, shape=None):
        a = np.frombuffer(raw, dt, count, o[0]).copy()
        o[0] += a.nbytes
        return a.reshape(shape) if shape else a
    for j in jobs:
        n_mp, n, r = j["t"]["n_mp"], len(j["points"]), len(j["recent"])
        out = {"status_up": take(np.int32, n), "mp_normal": take(np.float32, 3 * n_mp, (n_mp, 3)), "mp_max_dist": take(np.float32, n_mp),
               "mp_min_dist": take(np.float32, n_mp), "mp_desc": take(np.uint8, 32 * n_mp, (n_mp, 32)), "verdict": take(np.uint8, r), "kept": take(np.int32, r)}
        out["n_kept"], out["status"] = (int(v) for v in take(np.int32, 2))
        outs.append(out)
    assert o[0] == len(raw)
    return outs


def up_of(out):
    """The update part of a host_run result under the names of UP_OUTPUTS."""
    return dict(out, status=out["status_up"])


# ---- the resident forms' tensors ------------------------------------------------------------------------------------------------

def resident(fxs):
    """MapIndex and PointIndex of every map in fxs (the point record's planes ARE the map record's)."""
    from weiner_slamit_v2_amd import api

    maps = [api.MapIndex(fx["t"]) for fx in fxs]
    return maps, [api.PointIndex(fx["x"], mi) for fx, mi in zip(fxs, maps)]


def planes_of(pi, n_mp):
    return {"mp_normal": pi.t["mp_normal"].cpu().numpy().reshape(n_mp, 3), "mp_max_dist": pi.t["mp_max_dist"].cpu().numpy()[:n_mp],
            "mp_min_dist": pi.t["mp_min_dist"].cpu().numpy()[:n_mp], "mp_desc": pi.t["mp_desc"].cpu().numpy()[:32 * n_mp].reshape(n_mp, 32)}


def up_tensors(items, pad=3, item_map=None):
    """items: (map, points, what) per item -> the resident update call's tensors, status prefilled with -9."""
    import torch

    B = len(items)
    cap = max(len(p) for _, p, _ in items) + pad
    h = {"item_map": np.array([m for m, _, _ in items] if item_map is None else item_map, np.int32), "n": np.array([len(p) for _, p, _ in items], np.int32),
         "what": np.array([w for _, _, w in items], np.int32), "points": np.full((B, cap), -3, np.int32), "status": np.full((B, cap), -9, np.int32)}
    for i, (_, p, _) in enumerate(items):
        h["points"][i, :len(p)] = p
    return {k: torch.from_numpy(v).cuda() for k, v in h.items()}


def cull_tensors(lists, pad=3, list_map=None):
    """lists: (map, recent, cur_id, monocular) per list -> the resident culling call's tensors, verdict / kept prefilled."""
    import torch

    B = len(lists)
    cap = max(len(r) for _, r, _, _ in lists) + pad
    h = {"list_map": np.array([m for m, _, _, _ in lists] if list_map is None else list_map, np.int32), "cur_id": np.array([c for _, _, c, _ in lists], np.int32),
         "monocular": np.array([int(mo) for _, _, _, mo in lists], np.int32), "n": np.array([len(r) for _, r, _, _ in lists], np.int32),
         "recent": np.full((B, cap), -3, np.int32), "verdict": np.full((B, cap), VERDICT_FILL, np.uint8), "kept": np.full((B, cap), KEPT_FILL, np.int32),
         "n_kept": np.full(B, -9, np.int32), "status": np.full(B, -9, np.int32)}
    for i, (_, r, _, _) in enumerate(lists):
        h["recent"][i, :len(r)] = r
    return {k: torch.from_numpy(v).cuda() for k, v in h.items()}


def columns_for(t, seed, n_levels=8):
    """Point columns for any map whose observations are the inverse of its keyframe rows (the local-map fixtures): an observation's index
    is the point's first place in the keyframe's row, the reference keyframe the first stored observer."""
    rng = np.random.default_rng(seed)
    n_kf, n_mp, n_kp = t["n_kf"], t["n_mp"], len(t["kf_mp"])
    obs_idx = np.zeros(len(t["obs_kf"]), np.int32)
    for p in range(n_mp):
        for o in range(t["obs_ptr"][p], t["obs_ptr"][p + 1]):
            k = t["obs_kf"][o]
            obs_idx[o] = np.flatnonzero(t["kf_mp"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k + 1]] == p)[0]
    kf_octave = rng.integers(0, n_levels, n_kp).astype(np.uint8)
    has = t["obs_ptr"][1:] > t["obs_ptr"][:-1]
    sf = np.zeros(16, np.float32)
    sf[:n_levels] = np.float32(1.2) ** np.arange(n_levels)
    return {"n_levels": n_levels, "scale_factors": sf, "obs_idx": obs_idx, "obs_octave": kf_octave[t["kf_mp_ptr"][t["obs_kf"]] + obs_idx], "kf_octave": kf_octave,
            "kf_center": rng.uniform(-0.5, 0.5, (n_kf, 3)).astype(np.float32), "kf_desc": rng.integers(0, 256, (n_kp, 32)).astype(np.uint8),
            "mp_ref_kf": np.where(has, t["obs_kf"][np.minimum(t["obs_ptr"][:-1], max(len(t["obs_kf"]) - 1, 0))], -1).astype(np.int32),
            "mp_nobs": (t["obs_ptr"][1:] - t["obs_ptr"][:-1]).astype(np.int32), "mp_found": np.ones(n_mp, np.int32), "mp_visible": np.ones(n_mp, np.int32),
            "mp_first_kf": np.zeros(n_mp, np.int32), "mp_normal": t["mp_normal"], "mp_max_dist": t["mp_max_dist"], "mp_min_dist": t["mp_min_dist"],
            "mp_desc": rng.integers(0, 256, (n_mp, 32)).astype(np.uint8)}
