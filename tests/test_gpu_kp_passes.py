"""GPU parity of the orientation and descriptor passes where their launch shape matters: a level has the workgroups its own kp_cap
needs (KpBlockTab, both grid forms), and the descriptor's patch rows at every alignment.  Keypoints and descriptors bit for bit
against the CPU oracle, as tests/test_gpu_orb.py."""
import numpy as np
import pytest

from oracle import bindings as ob
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu


def _assert_same(kg, dg, ko, do, tag=""):
    assert len(kg) == len(ko), "%s keypoint count %d vs oracle %d" % (tag, len(kg), len(ko))
    for f in ("octave", "x", "y", "response", "size", "class_id"):
        assert np.array_equal(kg[f], ko[f]), "%s field %s differs" % (tag, f)
    assert np.array_equal(kg["angle"].view(np.uint32), ko["angle"].view(np.uint32)), "%s angle bits differ" % tag
    assert np.array_equal(dg, do), "%s descriptors differ" % tag


def _kp_caps(ext, roots=1):
    """OrbLevel::kp_cap of every level: max(quota, 4 * octree roots) + 4"""
    return [max(int(q), 4 * roots) + 4 for q in ext.features_per_level()]


def _single_and_batch(w, h, nf, nl, nbatch, caps, seeds):
    kinds = [synth.synth_frame(w, h, s) for s in seeds]
    orc = ob.OrbOracle(nf, 1.2, nl, 20, 7)
    want = [orc.extract(f) for f in kinds]
    one = api.ORBextractor(nf, 1.2, nl, 20, 7)
    assert _kp_caps(one) == caps
    for i, f in enumerate(kinds):
        kg, dg = one(f)
        _assert_same(kg, dg, want[i][0], want[i][1], "%dx%d single[%d]" % (w, h, i))
    ext = api.ORBextractor(nf, 1.2, nl, 20, 7, max_batch=nbatch)
    ks, ds = ext.extract_batch(np.stack([kinds[i % len(kinds)] for i in range(nbatch)]))
    for i in range(nbatch):
        _assert_same(ks[i], ds[i], want[i % len(kinds)][0], want[i % len(kinds)][1], "%dx%d batch%d[%d]" % (w, h, nbatch, i))
    return want


def test_caps_that_are_no_multiple_of_a_workgroup():
    """317x251, 500 features, 4 levels: no level's capacity is a multiple of 16.  One frame takes the (workgroups, frames) grid, 17
    frames the XCD-dealt grid with seven padding frame slots."""
    want = _single_and_batch(317, 251, 500, 4, 17, [165, 138, 116, 97], (11, 12, 13))
    assert all(len(k) > 300 for k, _ in want)


def test_levels_smaller_than_one_workgroup():
    """640x480, 60 features, 8 levels: level 0 holds 16 + 1 slots (two descriptor workgroups, the second with one slot that the
    octree's 13 keypoints never reach), every other level less than one workgroup of either pass.  One frame, and 16 frames: the
    smallest call on the XCD-dealt grid."""
    want = _single_and_batch(640, 480, 60, 8, 16, [17, 15, 13, 12, 10, 9, 8, 8], (44, 45, 46))
    assert all(len(k) >= 60 for k, _ in want)


def _sparse_frame():
    sparse = np.full((480, 640), 100, np.uint8)   # (test_gpu_orb.py::test_edge_images: top levels below their quota)
    rs = np.random.RandomState(4)
    for _ in range(60):
        x, y = rs.randint(30, 600), rs.randint(30, 440)
        sparse[y:y + 9, x:x + 9] = 220
    return sparse


def test_mixed_batch_of_19_equals_single_frames_and_oracle():
    """Rich, flat (no keypoint on any level) and sparse (top levels below quota) frames in one call of 19: the in-kernel count test
    ends the workgroups a level's capacity provides and its keypoints do not fill."""
    kinds = [synth.synth_frame(640, 480, 50), synth.flat_frame(640, 480), _sparse_frame()]
    orc = ob.OrbOracle(1000)
    want = [orc.extract(f) for f in kinds]
    assert len(want[1][0]) == 0
    top = want[2][0]["octave"]
    assert len(want[2][0]) > 0 and (top == 7).sum() < (want[0][0]["octave"] == 7).sum()
    one = api.ORBextractor(1000, 1.2, 8, 20, 7)
    alone = [one(f) for f in kinds]
    ext = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=19)
    order = [(i * 7 + i // 3) % 3 for i in range(19)]   # not periodic in eight: an XCD meets every kind
    assert sorted(set(order)) == [0, 1, 2]
    ks, ds = ext.extract_batch(np.stack([kinds[j] for j in order]))
    for i, j in enumerate(order):
        assert np.array_equal(ks[i], alone[j][0]) and np.array_equal(ds[i], alone[j][1]), (i, j)
        _assert_same(ks[i], ds[i], want[j][0], want[j][1], "mixed[%d]" % i)


def test_patch_rows_at_every_alignment_and_both_image_edges():
    """A patch row is staged from the 4-byte boundary at or below its first column: 37 columns and 0 .. 3 of alignment, 40 of the
    row pitch's bytes.  Level-0 keypoints of every residue (x - 18) & 3, and in the first (19) and last (w - 20) column FAST can
    report: the positions that a narrower pitch would get wrong first."""
    img = synth.synth_frame(640, 480, 2)
    orc = ob.OrbOracle(1000)
    ko, do = orc.extract(img)
    x0 = ko["x"][ko["octave"] == 0].astype(np.int64)
    assert sorted(set(((x0 - 18) & 3).tolist())) == [0, 1, 2, 3]
    assert x0.min() == 19 and x0.max() == 640 - 20
    kg, dg = api.ORBextractor(1000, 1.2, 8, 20, 7)(img)
    _assert_same(kg, dg, ko, do, "alignment")
