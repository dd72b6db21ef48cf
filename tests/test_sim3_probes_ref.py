"""The Sim3 probes on the CPU (no GPU): the numpy restatement (tests/essential_ref.py) against tests/golden/sim3probe_<family>.npz,
which hold what the reference's own g2o computes on synth.synth_sim3_probes (tools/gen_essential_golden.py, PROBES).

  * the census: what the unperturbed log calls of each family reach, so that the fixture cannot quietly stop reaching a branch;
  * the restatement reproduces every golden (tests/sim3_probe_checks.check at 1 x PROBE_WORST), and the constants are the measurement;
  * `gn` lands on its closed form;
  * the probes bite: every mutation of MUTATIONS, applied to the restatement, is rejected by the shared checker AT THE DEVICE'S BOUNDS
    (10 x the constants) on at least one family.

What the eight eg_* goldens see of the same mutations (run once by hand on the CPU: the assertions of tests/test_essential_ref.py, with
the chi2 bounds tests/test_gpu_essential.py uses, on the mutated restatement).  They MISS: the sign of w in Quaterniond(R) case 0 and
case 1 (no golden reaches either case), and A01, B01, A10, A11, B11 (at their angles a factor 1 + 1e-4 stays inside 1e-5).  They CATCH:
B10 (eg_panels75 alone: one accept flips; sim3.h's B10 lacks the series' "- 1" and is of the order 1 / sigma^3, so it is no small term),
either small-angle test replaced by the other (n_its differs on six and on seven goldens, for the same reason: B10 against B11), and
coordinate 6 not zeroed under fix_scale (eg_ring12_fixscale: the trials differ).

A10 is what the sixth family, `twoedge`, is there for: no problem of single-edge pairs shows it (tests/sim3_probe_checks.py)."""
import numpy as np
import pytest

from tests import essential_ref as er
from tests import sim3_probe_checks as pc
from weiner_slamit_v2_amd import synth


@pytest.fixture(scope="module")
def runs():
    out = {}
    for family in pc.FAMILIES:
        g = pc.golden(family)
        r, calls = pc.traced_optimize(g)
        out[family] = (g, r, pc.census(g, calls))
    return out


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_the_golden_is_the_synthesised_problem(family):
    g, p = pc.golden(family), synth.synth_sim3_probes(family)
    assert synth.SIM3_PROBE_FAMILIES == pc.FAMILIES
    for k, v in p.items():
        assert np.array_equal(np.asarray(g[k]), np.asarray(v)), k
    two = family == "twoedge"
    assert int(g["n_kf"]) == (144 if two else 96) and len(g["edge_v0"]) == (96 if two else 48) and int(g["max_its"]) == 1
    assert 7 * int((g["fixed"] == 0).sum()) == 336   # 11 panels
    assert int(g["ref_n_its"]) == 1 and g["ref_trial_rho"][-1] > 0 and np.all(np.abs(g["ref_trial_rho"]) > 1e-6)   # what the generator asserted
    n = int(g["n_kf"])
    assert g["pt_bad"].sum() == 1 and len(g["pt_ref"]) == n + 1 and np.array_equal(g["pt_ref"][:n], np.arange(n))


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_census(runs, family):
    c = runs[family][2]
    print(family, c)
    assert min(c["r2q"]) >= 8                                        # each branch of Quaterniond(R): x, y, z, positive trace
    if family in ("gn", "damped"):
        assert c["big_big"] >= 16                                    # sigma and theta large: A11, B11
    if family == "fixscale":
        assert c["nosigma_big"] >= 16                                # A01, B01
    if family == "noturn":
        assert c["big_small"] >= 16 and c["small_small_t"] >= 8      # A10, B10; A00, B00 with a translation to carry
    if family == "twoedge":
        assert c["big_small"] >= 16 and c["big_big"] >= 16           # per free keyframe one edge of each
    if family == "edges":
        assert min(c["theta_exp"]) >= 2 and min(c["theta_log"]) >= 2 and min(c["sigma_eps"]) >= 2
    if family == "damped":
        assert c["swap1"] >= 8 and c["swap2"] >= 4                   # W.lu(): a row swap at the first pivot, at the second


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_restatement_reproduces_the_reference(runs, family):
    g, r, _ = runs[family]
    worst = pc.differences(g, r)
    print(family, "worst relative differences", {k: "%.3g" % v for k, v in worst.items()}, "chi2_init %.17g / %.17g" % (r["chi2_init"], g["ref_chi2_init"]))
    pc.check(family, g, r)
    assert pc.rel(r["lam"], g["ref_lam"]) < 1e-6


def test_the_constants_are_the_measurement(runs):
    for family in pc.FAMILIES:
        g, r, _ = runs[family]
        assert pc.round_up(max(pc.differences(g, r).values())) == pc.PROBE_WORST[family], family
        assert pc.PROBE_WORST[family] <= 1e-6   # else the family is too ill conditioned to probe with
    g, r, _ = runs["gn"]
    assert pc.round_up(pc.closed_form_differences(g, r)) == pc.GN_CLOSED_WORST


def test_gn_lands_on_its_closed_form(runs):
    """One free vertex per edge and lambda 1e-16: f(t e) = (1 - t) e along e, so the Gauss-Newton step is e itself and the free
    keyframe lands on Snc_j Snc_i^-1 Scw_i: the same float64 algebra with no exp, log, Jacobian or solve in it."""
    g, r, _ = runs["gn"]
    d = pc.closed_form_differences(g, r)
    print("gn: restatement against the closed form %.3g, golden against it %.3g, chi2 left %.3g" % (d, pc.closed_form_differences(g, {k: g["ref_" + k] for k in pc.KEYS}), r["chi2"][-1]))
    assert d <= pc.GN_CLOSED_WORST
    assert r["chi2"][-1] < 1e-9 * r["chi2_init"]
    moved = pc.rel(g["scw_t"], r["sim3_t"])
    assert moved > 0.1   # ... and the step itself is no rounding matter


# ---- the probes bite ---------------------------------------------------------------------------------------------------------------------
def _r2q_w_sign(case):
    orig = er.R2q

    def R2q(R):
        out = orig(R)
        k = pc.r2q_branch(R).reshape(out.shape[:-1])
        out[k == case, 3] *= -1
        return out
    return dict(R2q=R2q)


def _abc_scaled(name):
    """name: A or B, then 0 / 1 for sigma small / not, then 0 / 1 for theta small / not, as tests/essential_ref._abc names them"""
    orig = er._abc

    def _abc(sigma, s, theta, small_theta):
        A, B, C = orig(sigma, s, theta, small_theta)
        small_sigma = np.abs(sigma) < 0.00001
        sel = (small_sigma if name[1] == "0" else ~small_sigma) & (small_theta if name[2] == "0" else ~small_theta)
        f = np.where(sel, 1 + 1e-4, 1.0)
        return (A * f, B, C) if name[0] == "A" else (A, B * f, C)
    return dict(_abc=_abc)


def _oplus_keeps_coordinate_6():
    return dict(sim3_oplus=lambda a, u, fix_scale: er.sim3_mul(er.sim3_exp(np.array(u, np.float64)), a))


MUTATIONS = {
    "R2q case 0: sign of w": lambda: _r2q_w_sign(0),
    "R2q case 1: sign of w": lambda: _r2q_w_sign(1),
    "A01 x (1 + 1e-4)": lambda: _abc_scaled("A01"),
    "B01 x (1 + 1e-4)": lambda: _abc_scaled("B01"),
    "A10 x (1 + 1e-4)": lambda: _abc_scaled("A10"),
    "B10 x (1 + 1e-4)": lambda: _abc_scaled("B10"),
    "A11 x (1 + 1e-4)": lambda: _abc_scaled("A11"),
    "B11 x (1 + 1e-4)": lambda: _abc_scaled("B11"),
    "log's small-angle test replaced by exp's": lambda: dict(log_small=lambda d, theta: theta < 0.00001),
    "exp's small-angle test replaced by log's": lambda: dict(exp_small=lambda theta: np.cos(theta) > 1 - 0.00001),
    "coordinate 6 not zeroed under fix_scale": _oplus_keeps_coordinate_6,
}


def rejections(check_one, problems):
    """{name of the problem: the checker's complaint} for the problems on which check_one(name, golden, mutated result) raises"""
    out = {}
    for name, g in problems.items():
        try:
            with np.errstate(all="ignore"):
                check_one(name, g, er.optimize(g))
        except (AssertionError, np.linalg.LinAlgError) as e:
            out[name] = str(e)[:160]
    return out


def test_the_restatement_as_it_is_passes_at_the_devices_bounds():
    assert not rejections(lambda f, g, r: pc.check(f, g, r, scale=10.0), {family: pc.golden(family) for family in pc.FAMILIES})


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_probes_bite(monkeypatch, mutation):
    problems = {family: pc.golden(family) for family in pc.FAMILIES}
    for k, v in MUTATIONS[mutation]().items():
        monkeypatch.setattr(er, k, v)
    rejected = rejections(lambda f, g, r: pc.check(f, g, r, scale=10.0), problems)
    print(mutation, "->", rejected)
    assert rejected, "no family sees: " + mutation
