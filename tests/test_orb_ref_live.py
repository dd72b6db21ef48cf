"""The reference's own ORBextractor.cc, compiled where it lies and run under a monotone allocator (oracle/orb_ref_harness.cc), against the
restatement oracle/orb_oracle.cc and against the committed goldens, bit for bit, on every fixture of tests/orb_ref_fixtures.py.  The six
OpenCV primitives are orb_oracle.cc's on both sides (they stay unpinned); everything the reference wrote itself runs as it wrote it.
Runs where oracle/Makefile.ref built the harness, i.e. where the reference's sources are."""
import numpy as np
import pytest

from oracle import bindings as ob
from tests import orb_ref_fixtures as fx

pytestmark = pytest.mark.skipif(not ob.orb_ref_available(),
                                reason="oracle/_ref/orb_ref_harness is built only where the reference's sources are (oracle/Makefile.ref)")


@pytest.fixture(scope="module")
def octree_golden():
    return fx.load_octree_golden()


@pytest.mark.parametrize("case", fx.OCTREE_CASES, ids=[c["name"] for c in fx.OCTREE_CASES])
def test_octree_reference_equals_oracle_and_golden(case, octree_golden):
    """DistributeOctTree called directly: same keys in the same list order."""
    b = case["borders"]
    got = ob.orb_ref_octree(case["keys"], b[0], b[1], b[2], b[3], case["n"], case["level"])
    assert np.array_equal(got, fx.octree_oracle(case)), "the reference differs from the oracle"
    assert np.array_equal(got, octree_golden[case["name"]]), "stale golden: tools/gen_orb_ref_golden.py"


@pytest.mark.parametrize("name", list(fx.EXTRACT_CASES))
def test_extract_reference_equals_oracle_and_golden(name):
    """operator() from the top: keypoints, angle bits, descriptors, padded pyramid planes, the per-level lists as they leave
    ComputeKeyPointsOctTree, constructor tables."""
    img, golden = fx.load_extract_golden(name)
    nf, sf, nl, ini, mn = fx.extract_params(name)
    got = ob.orb_ref_extract(img, nf, sf, nl, ini, mn)
    fx.assert_same_extract(got, fx.oracle_extract(name, img), name + " reference vs oracle")
    fx.assert_same_extract(got, golden, name + " reference vs golden (stale? tools/gen_orb_ref_golden.py)")
