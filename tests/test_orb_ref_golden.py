"""The restatement oracle/orb_oracle.cc against tests/golden/orb_ref_*.npz: outputs of the reference's own ORBextractor.cc recorded from
oracle/orb_ref_harness.cc (the reference under a monotone allocator; tools/gen_orb_ref_golden.py).  Runs anywhere: committed files only.
Also re-asserts what the fixtures are there for, from the oracle alone -- above all that the octree's tie rule DECIDES results, without
which equality with the reference would say nothing about that rule."""
import os

import numpy as np
import pytest

from oracle import bindings as ob
from tests import orb_ref_fixtures as fx


@pytest.fixture(scope="module")
def octree_golden():
    return fx.load_octree_golden()


def test_octree_fixture_premises():
    """Each of the three exits of DistributeOctTree's loop is taken by three cases or more, and in ten or more the result changes when
    the tie key is reversed."""
    exits, decisive = fx.octree_premises()
    fx.assert_octree_premises(exits, decisive)
    regions = {c["name"].split("-")[0] for c in fx.OCTREE_CASES if c["name"] in decisive}
    assert len(regions) >= 3, "decisive ties in %s only" % sorted(regions)
    for w, h in fx.REGIONS.values():
        assert round(float(np.float32(w) / np.float32(h))) >= 1   # round(w / h) == 0: the reference divides by zero (:558-560)
    assert [round(w / h) for w, h in fx.REGIONS.values()] == [1, 2, 1, 2]


@pytest.mark.parametrize("case", fx.OCTREE_CASES, ids=[c["name"] for c in fx.OCTREE_CASES])
def test_octree_oracle_equals_golden(case, octree_golden):
    assert np.array_equal(fx.octree_oracle(case), octree_golden[case["name"]])


@pytest.mark.parametrize("name", list(fx.EXTRACT_CASES))
def test_extract_oracle_equals_golden(name):
    img, golden = fx.load_extract_golden(name)
    o = fx.oracle_extract(name, img)
    fx.extract_premises(name, o)
    fx.assert_same_extract(o, golden, name + " oracle vs golden")


def test_golden_files_are_small_and_hold_data_only():
    names = [f for f in os.listdir(fx.GOLDEN) if f.startswith("orb_ref_")]
    want = {"orb_ref_octree.npz"} | {"orb_ref_%s.npz" % n for n in fx.EXTRACT_CASES}
    assert want <= set(names)
    for f in names:
        assert os.path.getsize(os.path.join(fx.GOLDEN, f)) < fx.MAX_FILE_BYTES, f
        with np.load(os.path.join(fx.GOLDEN, f), allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
