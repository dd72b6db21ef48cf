"""The checks of the Sim3 probes (synth.synth_sim3_probes, tests/golden/sim3probe_<family>.npz from the reference's own g2o), as
functions of (golden, result): tests/test_sim3_probes_ref.py runs them on the numpy restatement's result (tests/essential_ref.py) at
1 x the constants below, tests/test_gpu_sim3_probes.py on the device's at 10 x.

What each family isolates (48 disjoint pairs, one fixed and one free keyframe and one edge each, so the system is block diagonal and
chi2_init is a sum over one branch; one iteration, which every golden ends on an accepted first trial; 336 unknowns, 11 panels):
    gn        lambda 1e-16: the step is the error itself and the free keyframe lands on Snc_j Snc_i^-1 Scw_i, a closed form without exp,
              log, Jacobian or solve.  Cancels whatever exp and log share (the A, B, C of eg_abc), hence:
    damped    the same pairs at lambda 1: the step -(J^T J + I)^-1 J^T e moves with every component of log and of J.  (sigma, theta) large.
    fixscale  sigma exactly 0 with theta large (A01, B01), coordinate 6 held; every other pair has the free keyframe as vertex 0.
    noturn    theta 0 / 3e-6 / 9e-6 with sigma large (A10, B10) or exactly 0 (A00, B00: W = I, pure translation).
    edges     both sides of theta = 1e-5 (exp's test), of d = 1 - 1e-5 (log's test: theta = 4.47e-3) and of |sigma| = 1e-5.
    twoedge   noturn's pairs (sigma large throughout) with a second edge per free keyframe, from a second fixed keyframe, that turns by
              0.3 .. 1.5 rad.  A single edge holds A10 in its cost only as A^2 theta^2 with theta < 4.47e-3: a factor 1 + 1e-4 on A10
              moves a single-edge step by 1e-7 at most, below any bound the 1e-9 differences allow.  Here the first edge's
              J^T J (which holds A10 |t| to first order) divides the second edge's gradient, and the same factor moves the step by 2e-5.

PROBE_WORST[family]: the largest relative difference (to the array's largest magnitude) between the restatement and the golden over
sim3_r, sim3_t, sim3_s, pose and points, as measured on the CPU, rounded up to one digit; GN_CLOSED_WORST: the same between the restatement's
free Sim3s of `gn` and the closed form.  Both are what g2o's 1e-9 central differences leave of a double.
tests/test_sim3_probes_ref.test_the_constants_are_the_measurement pins them; every one is below 1e-6, so 10 x stays within the 1e-5 of
tests/test_gpu_essential.py."""
import os

import numpy as np

from tests import essential_ref as er
from tests.helpers import ROOT

FAMILIES = ("gn", "damped", "fixscale", "noturn", "edges", "twoedge")
KEYS = ("sim3_r", "sim3_t", "sim3_s", "pose", "points")
PROBE_WORST = {"gn": 6e-07, "damped": 8e-07, "fixscale": 4e-07, "noturn": 7e-07, "edges": 8e-08, "twoedge": 7e-07}   # measured: 5.1e-7, 7.3e-7, 3.7e-7, 6.3e-7, 7.3e-8, 6.4e-7
GN_CLOSED_WORST = 5e-07                                                                          # measured: 4.2e-7
CHI2_INIT_TOL = 1e-9   # tests/test_gpu_essential.py's bound on chi2_init


def round_up(x):
    """x rounded up to one significant digit"""
    e = int(np.floor(np.log10(x)))
    return float("%de%d" % (int(np.ceil(x / 10.0 ** e)), e))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def golden(family):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "sim3probe_%s.npz" % family)))


def differences(g, r):
    return {k: rel(r[k], g["ref_" + k]) for k in KEYS}


def check(family, g, r, scale=1.0):
    """`r` is the golden's run: the same iterations, trials and accept signs, chi2_init to 1e-9, the state within scale x the
    family's measured worst.  Raises AssertionError with the figure that missed; returns the worst difference."""
    assert r["n_its"] == int(g["ref_n_its"]) == 1, "n_its %d" % r["n_its"]
    assert np.asarray(r["trials"]).tolist() == g["ref_trials"].tolist(), "trials %s" % np.asarray(r["trials"]).tolist()
    assert (np.asarray(r["trial_rho"]) > 0).tolist() == (g["ref_trial_rho"] > 0).tolist(), "accept signs"
    c = abs(r["chi2_init"] - g["ref_chi2_init"]) / g["ref_chi2_init"]
    assert c <= CHI2_INIT_TOL, "chi2_init differs by %.3g relative" % c
    assert np.array_equal(r["touched"], g["ref_touched"]), "touched"
    worst = differences(g, r)
    # (every key on its own: a NaN fails it)
    assert all(v <= scale * PROBE_WORST[family] for v in worst.values()), "state differs by %s, bound %.3g" % ({k: "%.3g" % v for k, v in worst.items()}, scale * PROBE_WORST[family])
    return max(worst.values())


def closed_form(g):
    """Where the free keyframe of every pair of `gn` lands: Snc_j Snc_i^-1 Scw_i, as (r [P, 9], t, s)."""
    est = er.from_rts(g["scw_r"], g["scw_t"], g["scw_s"])
    q, t, s = er.sim3_mul(er.measurements(g), er._take(est, np.asarray(g["edge_v0"], np.int64)))
    return er.q2R(q).reshape(-1, 9), t, s


def closed_form_differences(g, r):
    j = np.asarray(g["edge_v1"], np.int64)
    want = closed_form(g)
    return max(rel(r[k][j], w) for k, w in zip(("sim3_r", "sim3_t", "sim3_s"), want))


# ---- the census: what the unperturbed log calls of a run of the restatement reach ---------------------------------------------------
def r2q_branch(R):
    """per matrix: 3 where the trace is positive, else the index of the largest diagonal element as Eigen picks it"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    i = np.where(R[:, 1, 1] > R[:, 0, 0], 1, 0)
    i = np.where(R[:, 2, 2] > np.where(i == 1, R[:, 1, 1], R[:, 0, 0]), 2, i)
    return np.where(tr > 0, 3, i)


def lu_swaps(W):
    """(first, second): does Matrix3d::lu() swap rows at the first / the second pivot of W"""
    W = np.array(W, np.float64)
    p = int(np.argmax(np.abs(W[:, 0])))
    W[[0, p]] = W[[p, 0]]
    for i in (1, 2):
        W[i] -= W[i, 0] / W[0, 0] * W[0]
    return p != 0, bool(abs(W[2, 1]) > abs(W[1, 1]))


def traced_optimize(prob):
    """er.optimize(prob) and the arguments of its unperturbed log calls (start of the iteration, every trial): a list of (q, t, s)"""
    calls = []
    orig = er.edge_errors

    def recording(meas, est, v0, v1):
        a = er.sim3_mul(er.sim3_mul(meas, er._take(est, v0)), er.sim3_inv(er._take(est, v1)))
        calls.append(a)
        return er.sim3_log(a)

    er.edge_errors = recording
    try:
        r = er.optimize(prob)
    finally:
        er.edge_errors = orig
    return r, calls


def census(prob, calls):
    """Counts over the unperturbed log calls of one run; theta is measured from the argument itself (atan2 of the skew part and d), so
    that the sides of exp's 1e-5 show even where log takes its small-angle branch.  The pivot conditions come from W as log builds it."""
    c = dict(big_big=0, nosigma_big=0, big_small=0, small_small_t=0, theta_exp=[0, 0], theta_log=[0, 0], sigma_eps=[0, 0], swap1=0, swap2=0)
    for q, t, s in calls:
        sigma = np.log(s)
        R = er.q2R(q)
        d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
        dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        theta = np.arctan2(0.5 * np.sqrt((dR * dR).sum(-1)), d)
        small = d > 1 - 0.00001
        ssig = np.abs(sigma) < 0.00001
        c["big_big"] += int(((np.abs(sigma) >= 0.2) & (theta >= 0.3)).sum())
        c["nosigma_big"] += int((ssig & (theta >= 0.3)).sum())
        c["big_small"] += int(((np.abs(sigma) >= 0.2) & small).sum())
        c["small_small_t"] += int((ssig & small & (np.sqrt((t * t).sum(-1)) >= 1)).sum())
        for key, below in (("theta_exp", theta < 0.00001), ("theta_log", small), ("sigma_eps", ssig)):
            c[key][0] += int(below.sum())
            c[key][1] += int((~below).sum())
        e = er.sim3_log((q, t, s))
        A, B, C = er._abc(sigma, s, np.where(small, 0.0, np.arccos(np.minimum(d, 1.0))), small)
        O = er.skew(e[:, :3])
        W = A[:, None, None] * O + B[:, None, None] * (O @ O) + C[:, None, None] * np.eye(3)
        for w in W:
            a, b = lu_swaps(w)
            c["swap1"] += int(a)
            c["swap2"] += int(b)
    kinds = r2q_branch(np.concatenate([np.asarray(prob["scw_r"]).reshape(-1, 9), np.asarray(prob["snc_r"]).reshape(-1, 9)]).reshape(-1, 3, 3))
    n = len(np.asarray(prob["scw_s"]))
    c["r2q"] = [int((kinds[:n] == k).sum()) for k in range(4)]   # keyframes (their Scw) per branch: x, y, z, positive trace
    return c
