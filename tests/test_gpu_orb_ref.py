"""The HIP extractor against tests/golden/orb_ref_*.npz: outputs of the reference's own ORBextractor.cc under a monotone allocator
(oracle/orb_ref_harness.cc, tools/gen_orb_ref_golden.py).  Reads the committed files only, neither the harness nor the reference."""
import numpy as np
import pytest

from tests import orb_ref_fixtures as fx
from tests.test_gpu_orb import _assert_same
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(fx.EXTRACT_CASES))
def test_hip_equals_the_reference_golden(name):
    img, golden = fx.load_extract_golden(name)
    nf, sf, nl, ini, mn = fx.extract_params(name)
    ext = api.ORBextractor(nf, sf, nl, ini, mn)
    kg, dg = ext(img)
    _assert_same(kg, dg, golden["kps"], golden["desc"], name)
    for l in range(nl):
        assert np.array_equal(ext.level(0, l), golden["levels"][l]), "%s pyramid level %d differs" % (name, l)
    t = golden["tables"]
    assert np.array_equal(ext.GetScaleFactors(), t["scale"])
    assert np.array_equal(ext.GetInverseScaleFactors(), t["inv_scale"])
    assert np.array_equal(ext.GetScaleSigmaSquares(), t["sigma2"])
    assert np.array_equal(ext.GetInverseScaleSigmaSquares(), t["inv_sigma2"])
    assert np.array_equal(ext.features_per_level(), t["per_level"])
