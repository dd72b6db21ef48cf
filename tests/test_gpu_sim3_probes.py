"""The Sim3 algebra of essential.hip (eg_exp, eg_log, eg_abc, eg_lu_solve3) and Quaterniond(R) (se3_device.h's R_to_quat) on the device,
branch by branch, through api.essential_graph alone: the probe problems of synth.synth_sim3_probes against
tests/golden/sim3probe_<family>.npz (the reference's own g2o) with the checks of tests/sim3_probe_checks.py, which
tests/test_sim3_probes_ref.py shows to reject every listed mutation at the bounds used here (10 x the CPU constants).

Per family: max_its = 0 is the round trip through Quaterniond(R) in all four branches, bit for bit the restatement's (eg_init, eg_recover,
and eg_points on reference keyframes that look backwards about x and about y); max_its = 1 is the golden's step.  `gn` also lands on its
closed form.  Then the failed trial (a pivot that is exactly zero) and a free keyframe without an edge.

MEASURED on an MI355X, worst relative difference to the golden over sim3_r, sim3_t, sim3_s, pose and points against the bound
(10 x PROBE_WORST), and chi2_init's relative difference against 1e-9:
    gn 5.1e-07 / 6e-06, 1.2e-16    damped 7.1e-07 / 8e-06, 2.9e-16    fixscale 4.1e-07 / 4e-06, 3.6e-16
    noturn 7.4e-07 / 7e-06, 0      edges 7.3e-08 / 8e-07, 0           twoedge 7.7e-07 / 7e-06, 1.4e-16
so the device is as far from the reference's g2o as the numpy restatement is (within a factor 1.2 everywhere), and a tenth of each bound.
`gn` against its closed form: 3.8e-07 against 5e-06, chi2 123.783 -> 5.6e-12.  Every family takes one trial, as the golden does.  The zero
pivot: n_its 1, trials [10], every rho -inf, lambda 0, every trial_chi2 DBL_MAX, the state untouched.  No device bug was found.
"""
import os

import numpy as np
import pytest

from tests import essential_ref as er
from tests import sim3_probe_checks as pc
from tests.helpers import ROOT
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def round_trip(g):
    """what max_its = 0 returns: every Sim3 through Quaterniond(R) and back, the points mapped by it"""
    return er.recover(g, er.from_rts(g["scw_r"], g["scw_t"], g["scw_s"]))


@pytest.fixture(scope="module")
def runs():
    out = {}
    for family in pc.FAMILIES:
        g = pc.golden(family)
        out[family] = (g, api.essential_graph(dict(g, max_its=0)), api.essential_graph(g))
    return out


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_max_its_zero_is_the_round_trip_in_every_branch(runs, family):
    g, r0, _ = runs[family]
    want = round_trip(g)
    kinds = pc.r2q_branch(g["scw_r"].reshape(-1, 3, 3))
    assert min(int((kinds == k).sum()) for k in range(4)) >= 8
    assert r0["n_its"] == 0 and r0["n_trials"] == 0
    for k in ("sim3_r", "pose", "points"):
        assert np.array_equal(bits(r0[k]), bits(want[k])), k
    assert np.array_equal(bits(r0["sim3_t"]), bits(g["scw_t"])) and np.array_equal(bits(r0["sim3_s"]), bits(g["scw_s"]))
    assert np.array_equal(r0["touched"], g["ref_touched"])
    ref_kinds = kinds[g["pt_ref"][g["pt_bad"] == 0]]
    assert (ref_kinds == 0).sum() >= 8 and (ref_kinds == 1).sum() >= 8   # eg_points on keyframes of case 0 and of case 1
    assert pc.rel(r0["sim3_r"], g["scw_r"]) < 1e-6                       # and the round trip is one: float-rounded rotations are orthonormal to 1e-7


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_one_iteration_is_the_goldens(runs, family):
    g, _, r = runs[family]
    worst = pc.differences(g, r)
    print(family, "worst relative differences", {k: "%.3g" % v for k, v in worst.items()}, "bound %.3g" % (10 * pc.PROBE_WORST[family]),
          "chi2_init %.3g relative" % (abs(r["chi2_init"] - g["ref_chi2_init"]) / g["ref_chi2_init"]), "trials", r["trials"].tolist(), "rho", r["trial_rho"].tolist())
    pc.check(family, g, r, scale=10.0)
    assert r["n_free"] == 48 and pc.rel(r["lam"], g["ref_lam"]) < 1e-6
    # the points are the restated map on the device's OWN corrected Sim3s, bit for bit; the bad point keeps its position
    pts, touched = er.map_points(g, r["sim3_r"], r["sim3_t"], r["sim3_s"])
    assert np.array_equal(bits(pts), bits(r["points"])) and np.array_equal(touched, r["touched"])
    bad = g["pt_bad"].astype(bool)
    assert bad.sum() == 1 and np.array_equal(bits(r["points"][bad]), bits(g["pt_pos"][bad]))
    # a fixed keyframe keeps its Sim3, and every free one has moved
    f = g["fixed"].astype(bool)
    assert np.array_equal(bits(r["sim3_t"][f]), bits(g["scw_t"][f])) and np.array_equal(bits(r["sim3_s"][f]), bits(g["scw_s"][f]))
    assert pc.rel(g["scw_t"], r["sim3_t"]) > 1e-2                      # ... and the step is no rounding matter
    if int(g["fix_scale"]):
        assert np.array_equal(bits(r["sim3_s"]), bits(g["scw_s"]))     # exp(0) = 1: no scale moved by a bit


def test_gn_lands_on_its_closed_form(runs):
    g, _, r = runs["gn"]
    d = pc.closed_form_differences(g, r)
    print("gn: device against the closed form %.3g, bound %.3g; chi2 %.6g -> %.3g" % (d, 10 * pc.GN_CLOSED_WORST, r["chi2_init"], r["chi2"][-1]))
    assert d <= 10 * pc.GN_CLOSED_WORST
    assert r["chi2"][-1] < 1e-9 * r["chi2_init"]
    f = g["fixed"].astype(bool)
    assert np.array_equal(bits(r["sim3_t"][f]), bits(g["scw_t"][f])) and np.array_equal(bits(r["sim3_s"][f]), bits(g["scw_s"][f]))


def test_a_free_keyframe_without_an_edge_comes_out_as_its_round_trip(runs):
    """The host form takes such a keyframe: its block of H is lambda I and its b is 0, so x = 0 and exp(0) leaves it alone."""
    g, _, r = runs["gn"]
    n = int(g["n_kf"])
    h = dict(g, n_kf=n + 1, fixed=np.append(g["fixed"], 0).astype(np.uint8), bad=np.append(g["bad"], 0).astype(np.uint8))
    for k in ("scw_r", "snc_r", "scw_t", "snc_t"):
        h[k] = np.concatenate([g[k], g[k][5:6]])
    for k in ("scw_s", "snc_s"):
        h[k] = np.append(g[k], 1.25)
    h["pt_ref"] = g["pt_ref"].copy()
    h["pt_ref"][0] = n   # ... and it is a point's reference keyframe
    q = api.essential_graph(h)
    want = round_trip(h)
    assert q["n_free"] == 49 and q["n_its"] == 1 and q["trials"].tolist() == [1] and q["trial_rho"][0] > 0
    for k in ("sim3_r", "sim3_t", "sim3_s", "pose"):
        assert np.array_equal(bits(q[k][n]), bits(want[k][n])), k
    assert np.array_equal(bits(q["points"][0]), bits(want["points"][0]))
    # the others do not notice: the system is block diagonal
    assert max(pc.rel(q[k][:n], r[k]) for k in ("sim3_r", "sim3_t", "sim3_s", "pose")) <= 10 * pc.PROBE_WORST["gn"]
    assert pc.closed_form_differences(g, {k: q[k][:n] for k in ("sim3_r", "sim3_t", "sim3_s")}) <= 10 * pc.GN_CLOSED_WORST


def test_a_zero_pivot_fails_every_trial_and_leaves_the_state():
    """lambda_init = 0 is taken literally (include/slamit.h).  Under fix_scale column 6 of every Jacobian is exactly zero, so with
    lambda = 0 the pivot of index 6 is exactly 0: the trial counts as DBL_MAX, lambda (0 x ni) stays 0, ten trials fail, the iteration
    ends the run, and the state is the max_its = 0 state bit for bit.  The restatement does the same (its trial_chi2 records the cost at
    the step not taken where the device records DBL_MAX, so that field is not compared)."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "eg_ring12_fixscale.npz")))
    g.update(lambda_init=0.0, max_its=3)
    r, r0 = api.essential_graph(g), api.essential_graph(dict(g, max_its=0))
    with np.errstate(all="ignore"):
        w = er.optimize(g)
    print("zero pivot: device n_its", r["n_its"], "trials", r["trials"].tolist(), "rho", r["trial_rho"].tolist(), "lambda", r["lam"].tolist(), "restatement", w["n_its"], w["trials"].tolist())
    assert w["n_its"] == 1 and w["trials"].tolist() == [10] and np.all(w["trial_rho"] < 0) and w["lam"].tolist() == [0.0]
    assert r["n_its"] == 1 and r["trials"].tolist() == [10] and r["n_trials"] == 10
    assert np.all(r["trial_rho"] < 0) and np.all(np.isneginf(r["trial_rho"]))
    assert np.all(r["trial_chi2"] == DBL_MAX) and r["chi2"].tolist() == [DBL_MAX]
    assert r["lam"].tolist() == [0.0]
    for k in ("sim3_r", "sim3_t", "sim3_s", "pose", "points"):
        assert np.array_equal(bits(r[k]), bits(r0[k])), k
        assert np.array_equal(bits(r[k]), bits(w[k])), k
    assert np.array_equal(r["touched"], r0["touched"]) and r["chi2_init"] > 0
