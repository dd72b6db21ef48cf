"""Pins the PoseOptimization oracle (oracle/ba_oracle.cc:pose_oracle_solve) to the reference's g2o:
golden vectors from tools/gen_pose_golden.py, and fresh synthesized problems against that g2o's stored results on them
(live as well where oracle/_ref exists)."""
import glob
import os

import numpy as np
import pytest

from oracle import bindings as ob
from tests.helpers import ROOT, load_pose_golden, ref_case
from weiner_slamit_v2_amd import synth

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pose_*.npz")))


def compare_pose(res, ref, tol=1e-9):
    assert np.abs(res["pose"] - ref["pose"]).max() <= tol * max(np.abs(ref["pose"]).max(), 1.0)
    assert np.array_equal(res["outlier"], ref["outlier"]) and res["n_inliers"] == ref["n_inliers"]
    assert res["n_its"] == ref["n_its"]
    assert np.allclose(res["chi2"], ref["chi2"], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[5:-4] for p in GOLDEN])
def test_oracle_vs_golden(path):
    prob, ref = load_pose_golden(path)
    compare_pose(ob.pose_solve(prob), ref)


def test_golden_covers_the_edge_cases():
    names = {os.path.basename(p)[5:-4] for p in GOLDEN}
    assert {"typical", "dense1000", "few", "under10", "under3", "hard"} <= names
    _, r = load_pose_golden(os.path.join(ROOT, "tests", "golden", "pose_under10.npz"))
    assert r["n_its"][1:] == [0, 0, 0]
    p, r = load_pose_golden(os.path.join(ROOT, "tests", "golden", "pose_under3.npz"))
    assert r["n_inliers"] == 0 and np.array_equal(r["pose"], p["pose"])


# (observations, outlier fraction, seed, pose perturbation); the reference g2o's results on these problems are stored in
# tests/golden/ref_g2o_cases.json.gz (tools/gen_ref_cases_golden.py)
REF_CASES = [(250, 0.2, 31, 0.03), (900, 0.4, 32, 0.08), (12, 0.0, 33, 0.02)]


@pytest.mark.parametrize("n,of,seed,pert", REF_CASES)
def test_vs_reference_g2o(n, of, seed, pert):
    prob = synth.synth_pose(n, of, seed, pert)
    res = ob.pose_solve(prob)
    compare_pose(res, ref_case("pose%s" % ((n, of, seed, pert),), prob))
    if ob.ba_ref_available():   # where the reference's g2o is built: also against it live
        compare_pose(res, ob.pose_ref_solve(prob))


def test_recovers_the_pose_and_the_outliers():
    prob = synth.synth_pose(500, 0.2, 41, 0.03)
    r = ob.pose_solve(prob)
    assert np.abs(r["pose"] - prob["truth_pose"]).max() < 0.02
    # gross outliers (>= 8 px) are all flagged; few inliers are lost to the chi2 gate
    assert r["outlier"][prob["truth_outlier"]].mean() > 0.97
    assert r["outlier"][~prob["truth_outlier"]].mean() < 0.10
