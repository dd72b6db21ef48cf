"""GPU: local / global BA, PoseOptimization and OptimizeSim3 on geometry the synthesizers alone never make (the fixtures and what they
must contain: tests/test_hard_geometry_fixtures.py) -- observations of points behind the camera, which only the depth half of the BA
gate flags and which the two single-block solvers must keep, and keyframes / points the gate leaves without an active edge, whose
all-zero block columns the banded, the blocked and the tiled LDLt have to walk through with dx = 0.

The goldens themselves also run through test_gpu_ba.py::test_vs_reference_g2o_golden, test_gpu_pose.py and test_gpu_sim3.py (they
glob tests/golden); every comparison here uses those modules' bounds."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import bindings as ob
from tests.helpers import (ROOT, b64_bits, b64_f64, large_hard_cases, large_hard_problem, load_ba_golden, load_pose_golden, load_sim3_golden,
                           sim3_close)
from tests.test_gpu_ba import _close as ba_close
from tests.test_gpu_pose import _close as pose_close
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

G = os.path.join(ROOT, "tests", "golden")
STATE_RTOL = 1e-5   # (tests/test_gpu_ba_large.py)


def _golden(name):
    prob, ref = load_ba_golden(os.path.join(G, name + ".npz"))
    return prob, ref, np.load(os.path.join(G, name + ".npz"))


@pytest.fixture(scope="module")
def opt():
    return api.Optimizer(max_kf=64, max_pt=2048, max_edge=110000, max_batch=4)


@pytest.fixture(scope="module")
def big():
    return api.Optimizer(max_kf=342, max_pt=3200, max_edge=24000, max_batch=8, max_free_kf=341)


def _without_edges(prob, ref):
    """Keyframes and points that the reference's gate left without an active edge."""
    alive = ref["edge_stage1_outlier"] == 0
    kf = np.bincount(prob["edge_kf"][alive], minlength=len(prob["kf_fixed"])) == 0
    pt = np.bincount(prob["edge_pt"][alive], minlength=len(prob["pt_xyz"])) == 0
    return np.flatnonzero(kf & (prob["kf_fixed"] == 0)), np.flatnonzero(pt)


@pytest.mark.parametrize("name", ["ba_starved_kf", "ba_starved_pts"])
def test_starved_vertices_keep_their_stage1_value_bit_for_bit(opt, name):
    """g2o drops a vertex without active edges from the second stage.  Here the keyframe keeps its column (diagonal block lambda I, zero
    right-hand side) and the point its 3 x 3 block: both must come out of the solve with dx = 0 exactly -- the state after the full
    schedule equals, bit for bit, the state of a solve that stops after the robust stage (the R -> q -> R round trip is the same in
    both), while every other free keyframe moves."""
    prob, ref, z = _golden(name)
    kfs, pts = _without_edges(prob, ref)
    assert set(z["starved_kf"]) <= set(kfs) and (name != "ba_starved_pts" or set(z["starved_pt0"]) <= set(pts))
    stage1 = opt.LocalBundleAdjustment(prob, its_final=0)
    full = opt.LocalBundleAdjustment(prob)
    assert np.array_equal(stage1["edge_stage1_outlier"], ref["edge_stage1_outlier"])
    assert np.array_equal(full["kf_pose"][kfs], stage1["kf_pose"][kfs])
    assert np.array_equal(full["pt_xyz"][pts], stage1["pt_xyz"][pts])
    others = np.setdiff1d(np.flatnonzero(prob["kf_fixed"] == 0), kfs)
    assert (full["kf_pose"][others] != stage1["kf_pose"][others]).any(1).all()
    if name == "ba_starved_pts":   # one active edge: still in the system, Hll of rank 2 before damping
        one = z["starved_pt1"]
        assert (full["pt_xyz"][one] != stage1["pt_xyz"][one]).any(1).all()
    # ... and the stage-1 state itself is the reference's
    scale = max(np.abs(z["ref_kf_pose_stage1"]).max(), 1.0)
    assert np.abs(stage1["kf_pose"] - z["ref_kf_pose_stage1"]).max() / scale <= STATE_RTOL
    assert np.abs(stage1["pt_xyz"] - z["ref_pt_xyz_stage1"]).max() / max(np.abs(z["ref_pt_xyz_stage1"]).max(), 1.0) <= STATE_RTOL
    ba_close(full, ref, name, prob=prob)


def _solve_in_child(name, env):
    """The fixture through a fresh process (a handle reads the switches when it is created) -> the result dict."""
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r)\n"
            "from weiner_slamit_v2_amd import api\n"
            "from tests.helpers import load_ba_golden\n"
            "prob, _ = load_ba_golden(sys.argv[1])\n"
            "o = api.Optimizer(max_kf=64, max_pt=2048, max_edge=110000, max_batch=1)\n"
            "a = o.LocalBundleAdjustment(prob, its_final=0)\n"
            "r = o.LocalBundleAdjustment(prob)\n"
            "np.savez(sys.argv[2], stage1_kf_pose=a['kf_pose'], stats=np.array(json.dumps(r['stats'])), **{k: r[k] for k in r if k != 'stats'})\n" % ROOT)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        subprocess.check_call([sys.executable, "-c", code, os.path.join(G, name + ".npz"), out], env=dict(os.environ, **env), cwd=ROOT, timeout=300)
        d = np.load(out)
        res = {k: d[k] for k in d.files if k != "stats"}
        res["stats"] = json.loads(str(d["stats"]))
    return res


def test_starved_keyframe_through_the_band_and_the_blocked_ldlt(opt):
    """ba_starved_kf plans onto the banded LDLt (tests/test_hard_geometry_fixtures.py); SLAMIT_BA_NO_BAND=1 sends it through
    k_ldlt_blocked.  Both against the reference's g2o, and the starved keyframe bit-identical to its stage-1 value in both."""
    prob, ref, z = _golden("ba_starved_kf")
    ba_close(opt.LocalBundleAdjustment(prob), ref, "starved_kf, band", prob=prob)
    res = _solve_in_child("ba_starved_kf", {"SLAMIT_BA_NO_BAND": "1"})
    ba_close(res, ref, "starved_kf, blocked", prob=prob)
    k = z["starved_kf"]
    assert np.array_equal(res["kf_pose"][k], res["stage1_kf_pose"][k])


def test_large_starved_window_through_the_tiled_ldlt(big):
    """starved100 (594 reduced rows: tiled; a starved keyframe mid-trajectory, mirrored observations of points seen in front by others)
    on a slamit_ba_create_ex handle against the reference's g2o: every pose, the pinned sample of points, both flag sets exactly
    (no edge of the fixture sits near the gate), the LM path."""
    c = large_hard_cases()["starved100"]
    prob = large_hard_problem(c)
    sched = c["schedule"]
    res = big.LocalBundleAdjustment(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2])
    pose = b64_f64(c["kf_pose"]).reshape(-1, 12)
    assert np.abs(res["kf_pose"] - pose).max() / max(np.abs(pose).max(), 1.0) <= STATE_RTOL
    idx, pts = np.array(c["pt_index"]), b64_f64(c["pt_xyz"]).reshape(-1, 3)
    assert np.abs(res["pt_xyz"][idx] - pts).max() / max(np.abs(pts).max(), 1.0) <= STATE_RTOL
    ne = len(prob["edge_kf"])
    assert not c["edge_chi2_near_gate"]
    for key in ("edge_stage1_outlier", "edge_outlier"):
        assert np.array_equal(res[key], b64_bits(c[key], ne)), key
    m = np.array(c["mirror_edges"])
    assert np.allclose(res["edge_chi2"][m], b64_f64(c["mirror_edge_chi2"]), rtol=1e-5, atol=1e-7)   # (test_gpu_ba.py::_close, monocular)
    s = res["stats"]
    assert s["n_its"] == c["n_its"] and [list(t) for t in s["trials"]] == c["trials"]
    for st in range(2):
        assert np.allclose(s["chi2"][st], b64_f64(c["chi2"][st]), rtol=1e-6, atol=1e-9)
    stage1 = big.LocalBundleAdjustment(prob, its_robust=sched[0], its_final=0, huber_delta=sched[2])
    pose1 = b64_f64(c["kf_pose_stage1"]).reshape(-1, 12)
    assert np.abs(stage1["kf_pose"] - pose1).max() / max(np.abs(pose1).max(), 1.0) <= STATE_RTOL
    kfs = [k for k, _ in c["hard"]["starve_kf"]]
    assert np.array_equal(res["kf_pose"][kfs], stage1["kf_pose"][kfs])
    others = np.setdiff1d(np.flatnonzero(prob["kf_fixed"] == 0), kfs)
    assert (res["kf_pose"][others] != stage1["kf_pose"][others]).any(1).all()
    ba_close(res, ob.ba_solve(prob, its_robust=sched[0], its_final=sched[1], huber_delta=sched[2]), "starved100 vs oracle", prob=prob)


def test_batch_of_hard_and_ordinary_windows(big):
    """Mirrored and starved windows next to ordinary ones in one batch -- the tiled window among banded ones: every slot as its
    single-window solve (the bound of test_gpu_ba_large.py::test_batch_of_large_and_small_windows) and as the reference's g2o."""
    names = ["ba_behind", "ba_fixed3", "ba_starved_kf", "ba_stereo_behind", "ba_small", "ba_starved_pts", "ba_stereo_mixed"]
    probs, refs = zip(*[load_ba_golden(os.path.join(G, n + ".npz")) for n in names])
    probs = list(probs) + [large_hard_problem(large_hard_cases()["starved100"])]
    outs = big.LocalBundleAdjustmentBatch(probs)
    for i, (p, o) in enumerate(zip(probs, outs)):
        one = big.LocalBundleAdjustment(p)
        scale = max(np.abs(one["kf_pose"]).max(), 1.0)
        assert np.abs(o["kf_pose"] - one["kf_pose"]).max() / scale <= 1e-9, i
        assert np.abs(o["pt_xyz"] - one["pt_xyz"]).max() / max(np.abs(one["pt_xyz"]).max(), 1.0) <= 1e-9, i
        assert o["stats"]["n_its"] == one["stats"]["n_its"] and o["stats"]["trials"] == one["stats"]["trials"], i
        assert np.array_equal(o["edge_outlier"], one["edge_outlier"]) and np.array_equal(o["edge_stage1_outlier"], one["edge_stage1_outlier"]), i
        if i < len(names):
            ba_close(o, refs[i], "batch:" + names[i], prob=p)


def only_mirrored_keyframe_window():
    """A window in which keyframe 5 sees nothing but mirrored points (each also behind keyframes 4 and 6): the gate flags all of its
    edges by depth alone, and the second stage runs without it.  -> (problem, keyframe, its edges)."""
    prob = synth.synth_ba(10, 200, 4, seed=91, n_fixed=1)
    keep = prob["edge_kf"] != 5
    for k in ("edge_kf", "edge_pt", "edge_uv", "edge_inv_sigma2"):
        prob[k] = prob[k][keep]
    assert np.bincount(prob["edge_pt"], minlength=200).min() >= 2
    prob, _, _ = synth.ba_mirror_points(prob, 24, 3, seed=191, first_kfs=(4,) * 24)
    return prob, 5, np.flatnonzero(prob["edge_kf"] == 5)


def test_keyframe_that_sees_only_mirrored_points(opt):
    prob, kf, edges = only_mirrored_keyframe_window()
    ref = ob.ba_solve(prob)
    # the premise, on the oracle (which meets the reference on the behind / starved goldens, tests/test_oracle_ba.py): small residuals,
    # flagged all the same, and the keyframe does not move after the gate
    assert len(edges) == 24 and ref["edge_stage1_outlier"][edges].all() and ref["edge_outlier"][edges].all()
    assert (ref["edge_chi2"][edges] <= 0.5 * 5.991).sum() >= 8
    assert not (np.abs(ref["edge_chi2"] - 5.991) <= 1e-6 * 5.991).any()
    assert np.array_equal(ref["kf_pose"][kf], ob.ba_solve(prob, its_final=0)["kf_pose"][kf]) and ref["stats"]["n_its"][1] >= 3
    res = opt.LocalBundleAdjustment(prob)
    ba_close(res, ref, "only mirrored", prob=prob)
    assert np.array_equal(res["kf_pose"][kf], opt.LocalBundleAdjustment(prob, its_final=0)["kf_pose"][kf])


def test_pose_batch_with_mirrored_correspondences():
    """PoseOptimization has no depth test: the *_behind frames in one launch with ordinary ones -- every frame equals its single solve
    bit for bit and the reference's g2o (mirrored correspondences with a small residual kept, the gross ones pruned)."""
    names = ["pose_behind", "pose_typical", "pose_stereo_behind", "pose_stereo_mixed", "pose_few", "pose_behind"]
    probs, refs = zip(*[load_pose_golden(os.path.join(G, n + ".npz")) for n in names])
    outs = api.Optimizer.PoseOptimization(list(probs))
    for n, p, r, o in zip(names, probs, refs, outs):
        one = api.Optimizer.PoseOptimization(p)
        assert np.array_equal(o["pose"], one["pose"]) and np.array_equal(o["outlier"], one["outlier"]) and o["n_its"] == one["n_its"], n
        pose_close(o, r, "batch:" + n)
    z = np.load(os.path.join(G, "pose_behind.npz"))
    assert (outs[0]["outlier"][z["mirror_small"]] == 0).sum() >= 8 and (outs[0]["outlier"][z["mirror_gross"]] != 0).sum() >= 8


def test_sim3_batch_with_mirrored_pairs():
    """OptimizeSim3 likewise: the mirrored pairs with a small residual stay inliers, the wrong associations among them are dropped."""
    names = ["sim3_behind", "sim3_typical", "sim3_behind_fixed_scale", "sim3_fixed_scale", "sim3_twelve", "sim3_behind"]
    probs, refs = zip(*[load_sim3_golden(os.path.join(G, n + ".npz")) for n in names])
    outs = api.Optimizer.OptimizeSim3(list(probs))
    for n, p, r, o in zip(names, probs, refs, outs):
        one = api.Optimizer.OptimizeSim3(p)
        assert np.array_equal(o["r12"], one["r12"]) and np.array_equal(o["t12"], one["t12"]) and o["s12"] == one["s12"], n
        assert np.array_equal(o["inlier"], one["inlier"]) and list(o["n_its"]) == list(one["n_its"]), n
        sim3_close(o, r, tol=1e-5)
        assert max(np.abs(o["r12"] - r["r12"].reshape(o["r12"].shape)).max(), abs(o["s12"] - r["s12"])) < 1e-6, n   # (test_gpu_sim3.py)
    z = np.load(os.path.join(G, "sim3_behind.npz"))
    assert (outs[0]["inlier"][z["mirror_small"]] == 1).sum() >= 8 and (outs[0]["inlier"][z["mirror_gross"]] == 0).sum() >= 8
