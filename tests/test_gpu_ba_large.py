"""GPU: bundle adjustment beyond 85 keyframes on one slamit_ba_create_ex handle (max_free_kf = 341): fixed keyframes off the reduced
system, and the tiled LDLt of reduced systems past k_ldlt_blocked's LDS panel (Npad > 512) and past BaWin's inline structure (Npad > 640),
against the CPU oracle (oracle/ba_oracle.cc, a dense solve)."""
import base64
import gzip
import json
import os

import numpy as np
import pytest

from oracle import bindings as ob
from tests.helpers import ROOT, load_ba_golden
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

# the windows, their schedules and the reference g2o's results (tools/gen_ba_large_golden.py): fixed150, stereo_fixed70, free90,
# sparse100 (a narrow band past 512 rows), global150, global300
REF = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "ba_large_ref.json.gz")).read())["cases"]
WINDOWS = {name: (c["synth_map"], tuple(c["schedule"])) for name, c in REF.items()}
LOCAL = tuple(REF["fixed150"]["schedule"])
GLOBAL = tuple(REF["global300"]["schedule"])
STATE_RTOL = 1e-5
SLAMIT_ERR_ARG, SLAMIT_ERR_CAPACITY = -1, -3


def _f64(s):
    return np.frombuffer(base64.b64decode(s), "<f8")


def _bits(s, n):
    return np.unpackbits(np.frombuffer(base64.b64decode(s), np.uint8))[:n].astype(np.uint8)


def _prob(name):
    return synth.synth_map(**WINDOWS[name][0])


def _solve(opt, prob, sched):
    return opt.LocalBundleAdjustment(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2])


def _oracle(prob, sched):
    return ob.ba_solve(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2])


def _gates(prob):
    return np.where(prob["edge_ur"] >= 0, 7.815, 5.991) if prob.get("edge_ur") is not None else 5.991


def _close(res, ref, tag, prob, rtol=STATE_RTOL):
    mixed = prob.get("edge_ur") is not None and (prob["edge_ur"] < 0).any()
    tol = 3 * rtol if mixed else rtol   # (mixed monocular / stereo windows: tests/test_gpu_ba.py::_close)
    err = np.abs(res["kf_pose"] - ref["kf_pose"]).max() / max(np.abs(ref["kf_pose"]).max(), 1.0)
    assert err <= tol, "%s pose rel err %g" % (tag, err)
    perr = np.abs(res["pt_xyz"] - ref["pt_xyz"]).max() / max(np.abs(ref["pt_xyz"]).max(), 1.0)
    assert perr <= tol, "%s point rel err %g" % (tag, perr)
    near = np.abs(ref["edge_chi2"] - _gates(prob)) <= 1e-6 * _gates(prob)
    for key in ("edge_stage1_outlier", "edge_outlier"):
        diff = res[key] != ref[key]
        assert not (diff & ~near).any(), "%s %s differs on %d edges" % (tag, key, int((diff & ~near).sum()))
    s, r = res["stats"], ref["stats"]
    assert s["n_its"] == r["n_its"], "%s iterations %s vs %s" % (tag, s["n_its"], r["n_its"])
    assert [list(t) for t in s["trials"]] == [list(t) for t in r["trials"]], tag


@pytest.mark.parametrize("name", sorted(REF))
def test_large_windows_vs_reference_g2o(big, name):
    """Every pose, the pinned sample of points, both outlier flag sets and the LM path against the reference's g2o (every point:
    test_large_windows_vs_oracle)."""
    c, prob = REF[name], _prob(name)
    sched = WINDOWS[name][1]
    res = _solve(big, prob, sched)
    mixed = prob.get("edge_ur") is not None and (prob["edge_ur"] < 0).any()
    tol = 3 * STATE_RTOL if mixed else STATE_RTOL
    pose = _f64(c["kf_pose"]).reshape(-1, 12)
    assert np.abs(res["kf_pose"] - pose).max() / max(np.abs(pose).max(), 1.0) <= tol, name
    idx = np.array(c["pt_index"])
    pts = _f64(c["pt_xyz"]).reshape(-1, 3)
    assert np.abs(res["pt_xyz"][idx] - pts).max() / max(np.abs(pts).max(), 1.0) <= tol, name
    ne = len(prob["edge_kf"])
    near = np.abs(res["edge_chi2"] - _gates(prob)) <= 1e-5 * _gates(prob)
    for key in ("edge_stage1_outlier", "edge_outlier"):
        diff = res[key] != _bits(c[key], ne)
        assert not (diff & ~near).any(), "%s %s differs on %d edges" % (name, key, int((diff & ~near).sum()))
    s = res["stats"]
    assert s["n_its"] == c["n_its"], name
    assert [list(t) for t in s["trials"]] == c["trials"], name
    for st in range(2):
        assert np.allclose(s["chi2"][st], _f64(c["chi2"][st]), rtol=1e-5 if mixed else 1e-6, atol=1e-9), name


@pytest.fixture(scope="module")
def big():
    return api.Optimizer(max_kf=342, max_pt=3200, max_edge=24000, max_batch=8, max_free_kf=341)


@pytest.fixture(scope="module")
def oracle_results():
    """The oracle's dense solves, once per module (global300: ~1.9 GFLOP per LM trial on the host)."""
    return {name: _oracle(_prob(name), WINDOWS[name][1]) for name in WINDOWS}


@pytest.mark.parametrize("name", sorted(REF))
def test_large_windows_vs_oracle(big, oracle_results, name):
    prob = _prob(name)
    _close(_solve(big, prob, WINDOWS[name][1]), oracle_results[name], name, prob)


def test_global300_solves_bit_identically_twice(big):
    prob = _prob("global300")
    a, b = (_solve(big, prob, GLOBAL) for _ in range(2))
    for key in ("kf_pose", "pt_xyz", "edge_chi2", "edge_outlier", "edge_stage1_outlier"):
        assert np.array_equal(a[key], b[key]), key
    assert a["stats"]["n_its"] == b["stats"]["n_its"]


def test_batch_of_large_and_small_windows(big):
    """The map windows and two existing goldens in one batch (one schedule per batch: the local one): each as its single-window solve."""
    probs = [_prob(n) for n in sorted(WINDOWS)]   # (every map window, sparse100 among them)
    probs += [load_ba_golden("%s/tests/golden/%s.npz" % (ROOT, g))[0] for g in ("ba_window8", "ba_fixed3")]
    outs = big.LocalBundleAdjustmentBatch(probs)
    for i, (p, o) in enumerate(zip(probs, outs)):
        one = big.LocalBundleAdjustment(p)
        scale = max(np.abs(one["kf_pose"]).max(), 1.0)
        assert np.abs(o["kf_pose"] - one["kf_pose"]).max() / scale <= 1e-9, i
        assert np.abs(o["pt_xyz"] - one["pt_xyz"]).max() / max(np.abs(one["pt_xyz"]).max(), 1.0) <= 1e-9, i
        assert o["stats"]["n_its"] == one["stats"]["n_its"] and o["stats"]["trials"] == one["stats"]["trials"], i
        assert np.array_equal(o["edge_outlier"], one["edge_outlier"]), i


def test_small_window_on_the_large_handle_is_bit_identical(big):
    """ba_window8 plans and solves on the max_free_kf = 341 handle exactly as on a 64-keyframe slamit_ba_create handle."""
    prob = load_ba_golden("%s/tests/golden/ba_window8.npz" % ROOT)[0]
    small = api.Optimizer(max_kf=64, max_pt=3200, max_edge=24000, max_batch=1)
    a, b = big.LocalBundleAdjustment(prob), small.LocalBundleAdjustment(prob)
    small.close()
    for key in ("kf_pose", "pt_xyz", "edge_chi2", "edge_outlier", "edge_stage1_outlier"):
        assert np.array_equal(a[key], b[key]), key
    assert a["stats"]["n_its"] == b["stats"]["n_its"] and a["stats"]["trials"] == b["stats"]["trials"]
    for st in range(2):
        assert np.array_equal(a["stats"]["chi2"][st], b["stats"]["chi2"][st]) and np.array_equal(a["stats"]["lambda"][st], b["stats"]["lambda"][st])
    assert a["stats"]["chi2_init"] == b["stats"]["chi2_init"]


def test_refusals():
    import ctypes as C

    L = api.lib()
    h = C.c_void_p()
    assert L.slamit_ba_create_ex(400, 342, 64, 64, 1, 0, C.byref(h)) == SLAMIT_ERR_ARG   # past SLAMIT_BA_MAX_FREE_KF
    assert "max_free_kf" in L.slamit_last_error().decode() and not h.value
    assert L.slamit_ba_create_ex(10, 11, 64, 64, 1, 0, C.byref(h)) == SLAMIT_ERR_ARG     # max_free_kf > max_kf
    assert L.slamit_ba_create_ex(400, 341, 64, 64, 1, 0, C.byref(h)) == 0                # the ceiling itself
    L.slamit_ba_destroy(h)
    o = api.Optimizer(max_kf=170, max_pt=2000, max_edge=12000, max_batch=1, max_free_kf=19)
    with pytest.raises(api.SlamitError, match=r"\(%d\).*free keyframes" % SLAMIT_ERR_CAPACITY):
        o.LocalBundleAdjustment(_prob("fixed150"))   # 20 free keyframes
    o.close()
    o = api.Optimizer(max_kf=170, max_pt=2000, max_edge=12000, max_batch=1, max_free_kf=20)
    res = o.LocalBundleAdjustment(_prob("fixed150"))   # the same window at its exact size
    o.close()
    assert res["stats"]["n_its"][0] > 0
