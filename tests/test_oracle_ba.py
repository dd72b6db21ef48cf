"""Pins the BA oracle (oracle/ba_oracle.cc) to the REFERENCE's own g2o.

tests/golden/ba_*.npz were produced by tools/gen_ba_golden.py from g2o + Eigen compiled out of
the reference sources (oracle/Makefile.ref).  The oracle is also compared on fresh synthesized problems with that
g2o's results on them (tests/golden/ref_g2o_cases.json.gz), and live where the build exists.
"""
import glob
import os

import numpy as np
import pytest

from oracle import bindings as ob
from tests.helpers import ROOT, load_ba_golden, ref_case
from weiner_slamit_v2_amd import synth

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ba_*.npz")))


def _compare(res, ref, tol=1e-9, counts=True, lam_rtol=1e-7):
    scale = max(np.abs(ref["kf_pose"]).max(), 1.0)
    assert np.abs(res["kf_pose"] - ref["kf_pose"]).max() <= tol * scale
    assert np.abs(res["pt_xyz"] - ref["pt_xyz"]).max() <= tol * max(np.abs(ref["pt_xyz"]).max(), 1.0)
    assert np.array_equal(res["edge_stage1_outlier"], ref["edge_stage1_outlier"])
    assert np.array_equal(res["edge_outlier"], ref["edge_outlier"])
    # (a point that moved by 1e-6 of its depth moves its residuals by ~1e-3 px: the chi2 bound follows the state bound)
    assert np.allclose(res["edge_chi2"], ref["edge_chi2"], rtol=max(1e-6, 1e3 * tol), atol=max(1e-9, 1e3 * tol))
    if counts:
        s, r = res["stats"], ref["stats"]
        assert s["n_its"] == r["n_its"] and s["trials"] == r["trials"]
        for st in range(2):
            assert np.allclose(s["chi2"][st], r["chi2"][st], rtol=max(1e-7, tol), atol=1e-12)
            assert np.allclose(s["lambda"][st], r["lambda"][st], rtol=lam_rtol)
        assert np.allclose(s["chi2_init"], r["chi2_init"], rtol=1e-7)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[3:-4] for p in GOLDEN])
def test_oracle_vs_golden(path):
    prob, ref = load_ba_golden(path)
    sched = ref.get("schedule", (5, 10, ob.HUBER_MONO))   # the global-BA fixtures carry (nIterations, 0, sqrt(5.99))
    # two keyframes with one fixed leave the scale barely constrained: the same LM path, but 1e-7 instead of 1e-9
    # (lambda's update takes rho from a cancelling difference of two large costs: control state, looser bound on the long
    #  single-stage runs)
    glob_ = "global" in path
    # windows that mix monocular and stereo observations amplify summation-order noise by ~5x per LM iteration (the reference's g2o
    # against itself with another elimination order does the same): same LM path and flags, poses to 1e-6, lambda as control state
    mixed = "stereo" in path and "stereo_all" not in path
    _compare(ob.ba_solve(prob, *sched), ref, tol=5e-6 if mixed else 1e-6 if "global_init" in path else 1e-8 if glob_ else 1e-9,
             lam_rtol=1e-3 if (glob_ or mixed) else 1e-7)


def test_golden_set_is_complete():
    names = {os.path.basename(p)[3:-4] for p in GOLDEN}
    assert {"tiny", "small", "fixed3", "rough", "rejects", "allout", "window8"} <= names
    _, ref = load_ba_golden(os.path.join(ROOT, "tests", "golden", "ba_rejects.npz"))
    assert max(ref["stats"]["trials"][0]) >= 3      # exercises the reject / lambda*=ni path
    _, ref = load_ba_golden(os.path.join(ROOT, "tests", "golden", "ba_allout.npz"))
    assert ref["stats"]["n_its"][1] == 0 and ref["edge_outlier"].all()
    _, ref = load_ba_golden(os.path.join(ROOT, "tests", "golden", "ba_window8.npz"))
    assert ref["stats"]["n_its"][1] < 10            # Raul's stop rule fired (levenberg.cpp:155-161)


# (keyframes, points, observations per point, seed, fixed keyframes); the reference g2o's results on these problems are stored
# in tests/golden/ref_g2o_cases.json.gz (tools/gen_ref_cases_golden.py)
REF_CASES = [(6, 80, 3, 21, 1), (9, 120, 5, 22, 2), (20, 400, 6, 23, 1), (15, 250, None, 24, 1),
             # windows at a handle's capacity, max_kf = 85 (tests/test_ba_capacity_plan.py): Npad 512 through the banded solve and
             # through the blocked one over 16 panels, and 40 fixed keyframes (they count toward max_kf, not toward the reduced system)
             (85, 1200, 3, 92, 1), (85, 900, 8, 94, 1), (85, 1000, 6, 95, 40)]


@pytest.mark.parametrize("k,p,o,seed,nfix", REF_CASES)
def test_vs_reference_g2o(k, p, o, seed, nfix):
    prob = synth.synth_ba(k, p, o, seed=seed, n_fixed=nfix)
    res = ob.ba_solve(prob)
    _compare(res, ref_case("ba%s" % ((k, p, o, seed, nfix),), prob))
    if ob.ba_ref_available():   # where the reference's g2o is built: also against it live
        _compare(res, ob.ba_ref_solve(prob))


def test_schedule_options_and_stop_flag():
    prob, _ = load_ba_golden(os.path.join(ROOT, "tests", "golden", "ba_small.npz"))
    full = ob.ba_solve(prob)
    # stop flag raised before the call: nothing moves (Optimizer.cc:655-657)
    stop = np.ones(1, np.uint8)
    r = ob.ba_solve(prob, stop=stop)
    assert np.allclose(r["pt_xyz"], prob["pt_xyz"]) and r["stats"]["n_its"] == [0, 0]
    # fewer iterations: a prefix of the full run
    r = ob.ba_solve(prob, its_robust=2, its_final=0)
    assert r["stats"]["n_its"] == [2, 0]
    assert np.allclose(r["stats"]["chi2"][0], full["stats"]["chi2"][0][:2])


def test_cost_decreases():
    prob = synth.synth_ba(10, 300, 5, seed=5, n_fixed=2)
    r = ob.ba_solve(prob)
    for st in range(2):
        c = [r["stats"]["chi2_init"][st]] + r["stats"]["chi2"][st]
        assert all(b <= a for a, b in zip(c, c[1:]))
    # inliers end near the noise floor (1 px, 2 dof per edge)
    inl = r["edge_outlier"] == 0
    assert r["edge_chi2"][inl].mean() < 2.5


# ---- Optimizer::OptimizeSim3: the oracle against golden vectors from the reference's own g2o ----------------------
SIM3_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sim3_*.npz")))


@pytest.mark.parametrize("path", SIM3_GOLDEN, ids=[os.path.basename(p)[5:-4] for p in SIM3_GOLDEN])
def test_sim3_oracle_matches_reference_g2o_golden(path):
    from tests.helpers import load_sim3_golden, sim3_close

    prob, ref = load_sim3_golden(path)
    sim3_close(ob.sim3_solve(prob), ref, tol=1e-6)


def test_sim3_golden_set_covers_the_branches():
    from tests.helpers import load_sim3_golden

    assert {os.path.basename(p)[5:-4] for p in SIM3_GOLDEN} >= {"typical", "many_outliers", "fixed_scale", "twelve", "under10", "rough"}
    _, ref = load_sim3_golden(os.path.join(ROOT, "tests", "golden", "sim3_under10.npz"))
    prob, _ = load_sim3_golden(os.path.join(ROOT, "tests", "golden", "sim3_under10.npz"))
    assert ref["n_inliers"] == 0 and ref["n_its"][1] == 0                  # fewer than 10 pairs left: returns 0 ...
    assert np.array_equal(ref["r12"].reshape(9), prob["r12"].reshape(9)) and ref["s12"] == prob["s12"]   # ... and g2oS12 untouched
    _, ref = load_sim3_golden(os.path.join(ROOT, "tests", "golden", "sim3_fixed_scale.npz"))
    assert ref["s12"] == 1.0                                                   # bFixScale: the scale never moves


SIM3_REF_SEEDS = range(20, 26)


def sim3_ref_problem(seed):
    return synth.synth_sim3(int(40 + 70 * (seed % 5)), 0.1 * (seed % 4), seed, 0.02 + 0.02 * (seed % 3), fix_scale=(seed % 5 == 0))


def test_sim3_oracle_matches_live_reference_g2o():
    """Fresh problems against the reference g2o's stored results on them, and live where its build exists."""
    from tests.helpers import sim3_close

    for seed in SIM3_REF_SEEDS:
        pr = sim3_ref_problem(seed)
        res = ob.sim3_solve(pr)
        sim3_close(res, ref_case("sim3(%d,)" % seed, pr), tol=1e-6)
        if ob.ba_ref_available():
            sim3_close(res, ob.sim3_ref_solve(pr), tol=1e-6)


def test_oracle_vs_large_hard_golden():
    """starved100 (tests/golden/ba_large_hard_ref.json.gz): a map-sized window with a starved keyframe and mirrored observations of points
    that other keyframes see in front -- every pose, the sampled points, both flag sets, the LM path, the state between the stages."""
    from tests.helpers import b64_bits, b64_f64, large_hard_cases, large_hard_problem

    c = large_hard_cases()["starved100"]
    prob = large_hard_problem(c)
    sched = c["schedule"]
    res = ob.ba_solve(prob, *sched)
    pose, idx = b64_f64(c["kf_pose"]).reshape(-1, 12), np.array(c["pt_index"])
    assert np.abs(res["kf_pose"] - pose).max() <= 1e-9 * max(np.abs(pose).max(), 1.0)
    assert np.abs(res["pt_xyz"][idx] - b64_f64(c["pt_xyz"]).reshape(-1, 3)).max() <= 1e-9 * max(np.abs(res["pt_xyz"]).max(), 1.0)
    for key in ("edge_stage1_outlier", "edge_outlier"):
        assert np.array_equal(res[key], b64_bits(c[key], len(prob["edge_kf"]))), key
    s = res["stats"]
    assert s["n_its"] == c["n_its"] and [list(t) for t in s["trials"]] == c["trials"]
    for st in range(2):
        assert np.allclose(s["chi2"][st], b64_f64(c["chi2"][st]), rtol=1e-7, atol=1e-12)
        assert np.allclose(s["lambda"][st], b64_f64(c["lambda"][st]), rtol=1e-7)
    pose1 = b64_f64(c["kf_pose_stage1"]).reshape(-1, 12)
    one = ob.ba_solve(prob, sched[0], 0, sched[2])
    assert np.abs(one["kf_pose"] - pose1).max() <= 1e-9 * max(np.abs(pose1).max(), 1.0)
    kfs = [k for k, _ in c["hard"]["starve_kf"]]
    assert np.array_equal(res["kf_pose"][kfs], one["kf_pose"][kfs])   # the starved keyframe: its stage-1 estimate, bit for bit


@pytest.mark.parametrize("name", ["starved_kf", "starved_pts"])
def test_oracle_keeps_starved_vertices_bit_for_bit(name):
    """What g2o does by dropping a vertex without active edges (ref_kf_pose == ref_kf_pose_stage1 there, tests/test_hard_geometry_fixtures.py)
    the oracle does too: the full schedule leaves them exactly where the robust stage put them."""
    path = os.path.join(ROOT, "tests", "golden", "ba_%s.npz" % name)
    prob, ref = load_ba_golden(path)
    z = np.load(path)
    full, one = ob.ba_solve(prob), ob.ba_solve(prob, its_final=0)
    alive = ref["edge_stage1_outlier"] == 0
    pts = np.flatnonzero(np.bincount(prob["edge_pt"][alive], minlength=len(prob["pt_xyz"])) == 0)
    assert len(z["starved_kf"]) and np.array_equal(full["kf_pose"][z["starved_kf"]], one["kf_pose"][z["starved_kf"]])
    assert np.array_equal(full["pt_xyz"][pts], one["pt_xyz"][pts]) and (name != "starved_pts" or len(pts) >= 6)
    assert np.abs(one["kf_pose"] - z["ref_kf_pose_stage1"]).max() <= 1e-9 * max(np.abs(z["ref_kf_pose_stage1"]).max(), 1.0)
    assert np.abs(one["pt_xyz"] - z["ref_pt_xyz_stage1"]).max() <= 1e-9 * max(np.abs(z["ref_pt_xyz_stage1"]).max(), 1.0)
