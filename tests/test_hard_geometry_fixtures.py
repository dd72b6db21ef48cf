"""CPU: what the hard-geometry fixtures must contain for the tests that use them to be able to fail.

tests/golden/{ba_*behind*, ba_starved_*, pose_*behind, sim3_behind*}.npz and ba_large_hard_ref.json.gz come from the reference's g2o on
inputs the synthesizers alone never make (weiner_slamit_v2_amd/synth.py: ba_mirror_points / ba_mirror_edges / ba_starve_kf /
ba_starve_pt / pose_mirror / sim3_mirror): observations of points BEHIND the camera with a small residual -- only the depth half of
local BA's gate (`chi2 > gate || !(z > 0)`, Optimizer.cc:672-743) flags them, and PoseOptimization / OptimizeSim3, which have no depth
test, must keep them --, and keyframes / points that the gate leaves without active edges.  These are conditions on the golden data
itself, not measurements of the code under test."""
import glob
import os

import numpy as np
import pytest

from tests.helpers import ROOT, load_ba_golden, load_pose_golden, load_sim3_golden

G = os.path.join(ROOT, "tests", "golden")
BEHIND = ("ba_behind", "ba_stereo_behind", "ba_behind_global")
STARVED = ("ba_starved_kf", "ba_starved_pts")


def ba_gates(prob):
    return np.where(prob["edge_ur"] >= 0, 7.815, 5.991) if prob.get("edge_ur") is not None else np.full(len(prob["edge_kf"]), 5.991)


def edge_depth(kf_pose, pt_xyz, edge_kf, edge_pt):
    """z of every edge's point in its keyframe's frame."""
    R = kf_pose[:, :9].reshape(-1, 3, 3)
    return np.einsum("ej,ej->e", R[edge_kf][:, 2, :], pt_xyz[edge_pt]) + kf_pose[edge_kf, 11]


def depth_flagged(prob, ref, key="edge_outlier"):
    """Edges the reference flagged although their chi2 is at most half the gate: flagged by depth alone."""
    return (ref[key] != 0) & (ref["edge_chi2"] <= 0.5 * ba_gates(prob))


def test_the_set_is_complete():
    have = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G, "*.npz"))}
    assert set(BEHIND + STARVED) | {"pose_behind", "pose_stereo_behind", "sim3_behind", "sim3_behind_fixed_scale"} <= have
    assert os.path.exists(os.path.join(G, "ba_large_hard_ref.json.gz"))


@pytest.mark.parametrize("name", BEHIND + STARVED)
def test_no_edge_sits_in_the_gate_band(name):
    """The comparisons exempt a flag when |ref_edge_chi2 - gate| <= 1e-6 gate: empty for these windows, so every flag is compared."""
    prob, ref = load_ba_golden(os.path.join(G, name + ".npz"))
    gate = ba_gates(prob)
    assert not (np.abs(ref["edge_chi2"] - gate) <= 1e-6 * gate).any()


@pytest.mark.parametrize("name", BEHIND)
def test_behind_windows_hold_edges_only_the_depth_test_flags(name):
    path = os.path.join(G, name + ".npz")
    prob, ref = load_ba_golden(path)
    low = depth_flagged(prob, ref)
    assert low.sum() >= 8
    fixed = prob["kf_fixed"][prob["edge_kf"]] != 0
    if name == "ba_behind_global":
        # (its_final = 0: no second stage follows the gate, which the harness and the library still evaluate -- as in ba_global_map,
        #  the stage-1 flags equal the final ones; BundleAdjustment itself only applies the final test)
        assert ref["schedule"][1] == 0 and ref["stats"]["n_its"][1] == 0 and np.array_equal(ref["edge_stage1_outlier"], ref["edge_outlier"])
    else:
        low1 = depth_flagged(prob, ref, "edge_stage1_outlier")
        assert low1.sum() >= 8
        if name == "ba_behind":
            assert prob["kf_fixed"].sum() >= 2 and (low1 & fixed).sum() >= 3 and (low1 & ~fixed).sum() >= 3
    if name == "ba_behind":
        assert (low & fixed).sum() >= 3 and (low & ~fixed).sum() >= 3
    if name == "ba_stereo_behind":
        stereo = prob["edge_ur"] >= 0
        assert (low & stereo).sum() >= 3 and (low & ~stereo).sum() >= 3
    # the depth, recomputed from the reference's final state: negative for exactly those edges among the ones with a low chi2, and
    # every edge with a negative depth is flagged, whatever its chi2
    z = edge_depth(ref["kf_pose"], ref["pt_xyz"], prob["edge_kf"], prob["edge_pt"])
    small = ref["edge_chi2"] <= 0.5 * ba_gates(prob)
    assert np.array_equal(z[small] < 0, low[small])
    assert ref["edge_outlier"][z < 0].all() and not (np.abs(z) < 0.5).any()
    # ... and they are the observations the generator mirrored
    mirrored = np.zeros(len(z), bool)
    mirrored[np.load(path)["mirror_edges"]] = True
    assert np.array_equal(z < 0, mirrored)


@pytest.mark.parametrize("name", STARVED)
def test_starved_windows_lose_whole_vertices_at_the_gate(name):
    path = os.path.join(G, name + ".npz")
    prob, ref = load_ba_golden(path)
    z = np.load(path)
    alive = ref["edge_stage1_outlier"] == 0
    kf_alive = np.bincount(prob["edge_kf"][alive], minlength=len(prob["kf_fixed"]))
    pt_alive = np.bincount(prob["edge_pt"][alive], minlength=len(prob["pt_xyz"]))
    kfs = z["starved_kf"]
    assert len(kfs) >= 1 and not prob["kf_fixed"][kfs].any() and (kf_alive[kfs] == 0).all()
    assert (np.bincount(prob["edge_kf"], minlength=len(kf_alive))[kfs] >= 20).all()        # (they had edges to lose)
    free = np.flatnonzero(prob["kf_fixed"] == 0)
    assert all(free.min() < k < free.max() for k in kfs)                                     # interior columns of the reduced system
    assert ref["stats"]["n_its"][1] >= 3                                                     # stage 2 really iterates without them
    for k in kfs:   # g2o drops a vertex without active edges from the second stage: bit for bit its stage-1 estimate
        assert np.array_equal(ref["kf_pose"][k], z["ref_kf_pose_stage1"][k])
    moved = np.flatnonzero((ref["kf_pose"] != z["ref_kf_pose_stage1"]).any(1))
    assert set(moved) == set(free) - set(kfs)                                                # ... and every other free keyframe moved
    if name == "ba_starved_pts":
        one, zero = z["starved_pt1"], z["starved_pt0"]
        assert len(one) >= 4 and len(zero) >= 4
        assert (pt_alive[one] == 1).all() and (pt_alive[zero] == 0).all()
        assert np.array_equal(ref["pt_xyz"][zero], z["ref_pt_xyz_stage1"][zero])
        assert (ref["pt_xyz"][one] != z["ref_pt_xyz_stage1"][one]).any(1).all()             # one edge: still in the system
    # points whose only other observers were starved keyframes count too: every point without an active edge stays put
    for p in np.flatnonzero(pt_alive == 0):
        assert np.array_equal(ref["pt_xyz"][p], z["ref_pt_xyz_stage1"][p])


@pytest.mark.parametrize("name", ("pose_behind", "pose_stereo_behind"))
def test_pose_fixtures_keep_and_prune_mirrored_correspondences(name):
    path = os.path.join(G, name + ".npz")
    prob, ref = load_pose_golden(path)
    z = np.load(path)
    R, t = ref["pose"][:9].reshape(3, 3), ref["pose"][9:]
    depth = prob["xw"] @ R[2] + t[2]
    small, gross = z["mirror_small"], z["mirror_gross"]
    assert np.array_equal(np.sort(np.flatnonzero(depth < 0)), np.sort(np.concatenate([small, gross])))
    assert ((ref["outlier"][small] == 0).sum() >= 8) and (ref["outlier"][gross] != 0).sum() >= 8
    assert (ref["outlier"][depth > 0] != 0).sum() >= 8          # ordinary outliers besides
    assert all(n > 0 for n in ref["n_its"])
    if name == "pose_stereo_behind":
        st = prob["ur"] >= 0
        assert ((ref["outlier"][small] == 0) & st[small]).sum() >= 3 and ((ref["outlier"][small] == 0) & ~st[small]).sum() >= 3


@pytest.mark.parametrize("name", ("sim3_behind", "sim3_behind_fixed_scale"))
def test_sim3_fixtures_keep_and_prune_mirrored_pairs(name):
    path = os.path.join(G, name + ".npz")
    prob, ref = load_sim3_golden(path)
    z = np.load(path)
    R, t, s = ref["r12"].reshape(3, 3), ref["t12"], ref["s12"]
    z1 = (s * (prob["p2"] @ R.T) + t)[:, 2]                    # p2 in camera 1 (EdgeSim3ProjectXYZ)
    z2 = (((prob["p1"] - t) @ R) / s)[:, 2]                    # p1 in camera 2 (EdgeInverseSim3ProjectXYZ)
    small, gross = z["mirror_small"], z["mirror_gross"]
    both = np.sort(np.concatenate([small, gross]))
    assert np.array_equal(np.flatnonzero(z1 < 0), both) and np.array_equal(np.flatnonzero(z2 < 0), both)
    assert (ref["inlier"][small] == 1).sum() >= 8 and (ref["inlier"][gross] == 0).sum() >= 8
    assert ((ref["inlier"] == 0) & (z1 > 0)).sum() >= 8       # ordinary outliers besides
    assert ref["n_its"][0] > 0 and ref["n_its"][1] > 0
    assert (ref["s12"] == 1.0) == (name == "sim3_behind_fixed_scale") == bool(prob["fix_scale"])


def test_large_starved_window_conditions():
    """starved100: past 512 reduced rows, a free keyframe mid-trajectory without a surviving edge, mirrored observations of points that
    other keyframes see in front -- flagged in both flag sets with a chi2 of at most half the gate."""
    from tests.helpers import b64_bits, b64_f64, large_hard_cases, large_hard_problem

    c = large_hard_cases()["starved100"]
    prob = large_hard_problem(c)
    ne, n_kf = len(prob["edge_kf"]), len(prob["kf_fixed"])
    assert 6 * int((prob["kf_fixed"] == 0).sum()) > 512
    out1, out = b64_bits(c["edge_stage1_outlier"], ne), b64_bits(c["edge_outlier"], ne)
    kfs = [k for k, _ in c["hard"]["starve_kf"]]
    alive = np.bincount(prob["edge_kf"][out1 == 0], minlength=n_kf)
    assert all(n_kf // 4 < k < 3 * n_kf // 4 and not prob["kf_fixed"][k] and alive[k] == 0 for k in kfs)
    assert (np.bincount(prob["edge_kf"], minlength=n_kf)[kfs] >= 20).all() and (np.delete(alive, kfs) >= 10).all()
    pose, pose1 = b64_f64(c["kf_pose"]).reshape(-1, 12), b64_f64(c["kf_pose_stage1"]).reshape(-1, 12)
    assert c["n_its"][1] >= 3
    moved = np.flatnonzero((pose != pose1).any(1))
    assert set(moved) == set(np.flatnonzero(prob["kf_fixed"] == 0)) - set(kfs)
    m = np.array(c["mirror_edges"])
    low = b64_f64(c["mirror_edge_chi2"]) <= 0.5 * 5.991
    assert low.sum() >= 8 and out[m].all() and out1[m].all()
    z = edge_depth(pose, prob["truth_pt"], prob["edge_kf"], prob["edge_pt"])    # (the true points: a mirrored point is metres behind)
    assert np.array_equal(np.flatnonzero(z < 0), m) and (z[m] < -1.0).all()
    assert (np.bincount(prob["edge_pt"][z > 0], minlength=len(prob["pt_xyz"]))[prob["edge_pt"][m]] >= 2).all()   # seen in front by two or more
    assert not c["edge_chi2_near_gate"]


def test_the_three_factorizations_are_covered(tmp_path):
    """csrc/ba_plan.cc sends ba_starved_kf to the banded LDLt, the same window with SLAMIT_BA_NO_BAND=1 to the blocked one and starved100
    to the tiled one (tests/test_gpu_hard_geometry.py runs the three): a starved column passes through every kind of reduced solve."""
    from tests.helpers import large_hard_cases, large_hard_problem
    from tests.test_ba_plan import build_plan_lib, limits, plan, CSRC

    BAND, BLOCKED, TILED = 0, 1, 2
    L = build_plan_lib(str(tmp_path), [os.path.join(CSRC, "ba_plan.cc")])
    prob, _ = load_ba_golden(os.path.join(G, "ba_starved_kf.npz"))
    o = plan(L, prob, limits())
    assert (o["solver"], o["nS"], o["Npad"]) == (BAND, 66, 128) and o["band"] <= 17
    assert plan(L, prob, limits(no_band=1))["solver"] == BLOCKED
    big = plan(L, large_hard_problem(large_hard_cases()["starved100"]), limits(max_kf=341))
    assert (big["solver"], big["nS"], big["Npad"]) == (TILED, 594, 640)
    col = big["col"][50]   # the starved keyframe's rows lie inside the system, away from both ends
    assert 64 <= 6 * col and 6 * col + 6 <= 594 - 64
