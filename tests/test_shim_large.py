"""GPU: the shim's Optimizer over windows past 85 keyframes (shim/Optimizer.h SolvePOD grows its handle through slamit_ba_create_ex:
keyframe tables by 2 n_kf, the reduced system by min(2 n_free, 341)).  LocalMapping.cc:84's LocalBundleAdjustment with a long tail of fixed
observers, and GlobalBundleAdjustemnt over a 150-keyframe map (tiled LDLt), against the CPU oracle at test_shim.py's float32 write-back
tolerances."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT
from tests.test_shim import EXE, _ba_blob, _build

pytestmark = pytest.mark.gpu

REF = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "ba_large_ref.json.gz")).read())["cases"]


def _run(tmp_path, prob, extra=()):
    blob, K, P = _ba_blob(prob)
    pin, pout = tmp_path / "p.bin", tmp_path / "o.bin"
    open(pin, "wb").write(blob)
    subprocess.check_call([EXE, "ba", str(pin), str(pout)] + list(extra), timeout=300)
    raw = open(pout, "rb").read()
    f = np.frombuffer(raw, np.float32, 12 * K + 3 * P)
    R, t, pts = f[:9 * K].reshape(K, 9), f[9 * K:12 * K].reshape(K, 3), f[12 * K:].reshape(P, 3)
    erased, updates = struct.unpack_from("<ii", raw, 4 * (12 * K + 3 * P))
    return R, t, pts, erased, updates


def _sub_window(prob, keep_pt):
    """The window restricted to the points in keep_pt (every observation of them), point indices renumbered."""
    new = -np.ones(len(prob["pt_xyz"]), np.int64)
    new[keep_pt] = np.arange(len(keep_pt))
    e = np.flatnonzero(new[prob["edge_pt"]] >= 0)
    q = dict(prob)
    q["pt_xyz"] = prob["pt_xyz"][keep_pt]
    for k in ("edge_kf", "edge_uv", "edge_inv_sigma2"):
        q[k] = prob[k][e]
    q["edge_pt"] = new[prob["edge_pt"][e]].astype(np.int32)
    return q


def test_shim_local_ba_with_150_fixed_observers(tmp_path):
    """fixed150 (20 free keyframes, keyframes 0 .. 149 fixed) through LocalBundleAdjustment: keyframe 0 (mnId 0, fixed by id) and the
    20 free ones are the local keyframes, their points the local map points, and every other observer of those a fixed camera
    (Optimizer.cc:456-546) -- 170 keyframes, more than slamit_ba_create takes."""
    from oracle import bindings as ob
    from weiner_slamit_v2_amd import synth

    _build()
    prob = synth.synth_map(**REF["fixed150"]["synth_map"])
    local_kf = (prob["kf_fixed"] == 0) | (np.arange(len(prob["kf_fixed"])) == 0)
    local_pt = np.unique(prob["edge_pt"][local_kf[prob["edge_kf"]]])
    sub = _sub_window(prob, local_pt)
    ref = ob.ba_solve(sub)
    R, t, pts, erased, updates = _run(tmp_path, prob)
    assert np.abs(R - ref["kf_pose"][:, :9]).max() < 2e-6
    assert np.abs(t - ref["kf_pose"][:, 9:]).max() < 1e-5 * max(np.abs(ref["kf_pose"][:, 9:]).max(), 1)
    assert np.abs(pts[local_pt] - ref["pt_xyz"]).max() < 1e-5 * np.abs(ref["pt_xyz"]).max()
    others = np.setdiff1d(np.arange(len(pts)), local_pt)
    assert np.array_equal(pts[others], prob["pt_xyz"][others].astype(np.float32))   # not in the window: untouched
    assert erased == int(ref["edge_outlier"].sum()) and updates == len(local_pt)


def test_shim_global_ba_over_150_keyframes(tmp_path):
    """global150 (149 free keyframes, keyframe 0 fixed: a reduced system of 894 rows, the tiled LDLt) through
    GlobalBundleAdjustemnt(pMap, 10, pbStopFlag, 0, true), the schedule of the fixture."""
    from oracle import bindings as ob
    from weiner_slamit_v2_amd import synth

    _build()
    c = REF["global150"]
    prob = synth.synth_map(**c["synth_map"])
    its, _, huber = c["schedule"]
    ref = ob.ba_solve(prob, its_robust=its, its_final=0, huber_delta=huber)
    R, t, pts, erased, updates = _run(tmp_path, prob, ["global", str(its), "0", "1"])
    assert np.abs(R - ref["kf_pose"][:, :9]).max() < 2e-6
    assert np.abs(t - ref["kf_pose"][:, 9:]).max() < 1e-5 * max(np.abs(ref["kf_pose"][:, 9:]).max(), 1)
    assert np.abs(pts - ref["pt_xyz"]).max() < 1e-5 * np.abs(ref["pt_xyz"]).max()
    assert erased == 0 and updates == len(pts)
