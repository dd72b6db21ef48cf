"""The numpy restatement of Optimizer::OptimizeEssentialGraph (tests/essential_ref.py) against tests/golden/eg_*.npz, which hold what the
reference's own g2o computes (tools/gen_essential_golden.py): the same n_its, the same trials per iteration, the same accept / reject
sequence, and the estimates close to the reference's.  No GPU.

CHI2_WORST is the largest relative difference between the restatement's and the reference's per-trial chi2 over all goldens as
measured here on the CPU, to four decimals: 0.1511 (eg_panels75; eg_five 0.1229, eg_mixed40 0.0199, eg_rough30 1.2e-3, the others below
1e-4).  The large ones are the trials of an iteration that ends in ten rejects: Gauss-Newton steps from an all but converged state, whose
cost is the amplified rounding of g2o's 1e-9 central differences and of the solve.  CHI2_ACCEPTED_WORST is the same over the ACCEPTED
trials only: 0.0184 (eg_panels75, whose one accepted step lands on a cost 25 times below the start; eg_rough30 3.2e-4, the others
below 1e-5).  test_the_constants_are_the_measurement pins both to what is measured; tests/test_gpu_essential.py holds the device's
chi2 trace to 10 x each."""
import glob
import os

import numpy as np
import pytest

from tests import essential_ref as er
from tests.helpers import ROOT

GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "eg_*.npz")))
NAMES = ["eg_five", "eg_mixed40", "eg_panels75", "eg_ring12", "eg_ring12_fixscale", "eg_rough30", "eg_six", "eg_tiny4"]
CHI2_WORST = 0.1511
CHI2_ACCEPTED_WORST = 0.0184


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_every_case_of_the_table_is_there():
    assert [os.path.basename(f)[:-4] for f in GOLDENS] == NAMES
    for f in GOLDENS:
        g = np.load(f)
        assert np.all(np.abs(g["ref_trial_rho"]) > 1e-6)   # what the generator asserted


def chi2_differences(g, r):
    """worst relative difference of the per-trial chi2 to the reference's: over all trials, over the accepted ones"""
    acc = g["ref_trial_rho"] > 0
    d = np.abs(r["trial_chi2"] - g["ref_trial_chi2"]) / np.abs(g["ref_trial_chi2"])
    return float(d.max()), float(d[acc].max())


@pytest.fixture(scope="module")
def runs():
    return {os.path.basename(f)[:-4]: (dict(np.load(f)), er.optimize(dict(np.load(f)))) for f in GOLDENS}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(runs, name):
    g, r = runs[name]
    assert r["n_its"] == int(g["ref_n_its"])
    assert r["trials"].tolist() == g["ref_trials"].tolist()
    assert (r["trial_rho"] > 0).tolist() == (g["ref_trial_rho"] > 0).tolist()
    worst = max(rel(r[k], g["ref_" + k]) for k in ("sim3_r", "sim3_t", "sim3_s", "pose", "points"))
    print(name, "worst relative difference %.3g" % worst)
    assert worst < 1e-5
    assert np.array_equal(r["touched"], g["ref_touched"])
    d, da = chi2_differences(g, r)
    print(name, "chi2: worst %.4g, accepted trials %.4g" % (d, da))
    assert round(d, 4) <= CHI2_WORST and round(da, 4) <= CHI2_ACCEPTED_WORST
    assert rel(r["lam"], g["ref_lam"]) < 1e-6


def test_the_constants_are_the_measurement(runs):
    worst = [chi2_differences(*runs[name]) for name in NAMES]
    assert round(max(w[0] for w in worst), 4) == CHI2_WORST and round(max(w[1] for w in worst), 4) == CHI2_ACCEPTED_WORST
