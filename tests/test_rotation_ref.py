"""tests/rotation_ref.py, the sequential restatement of the rotation-consistency check (ORBmatcher.cc:1430-1471, :1605-1646), against
cases worked out by hand.  The device kernel is held to the same cases and to this restatement in tests/test_gpu_project.py."""
import numpy as np
import pytest

from tests import rotation_ref as rot


@pytest.mark.parametrize("name", sorted(rot.hand_cases()))
def test_hand_cases(name):
    case, owners, nmatches, bins = rot.hand_cases()[name]
    owner, nm, ind = rot.rotation_check(**case)
    assert ind == bins and nm == nmatches
    for k, q in owners.items():
        assert owner[k] == q, (k, owner[k], q)


def test_a_shared_keypoint_with_one_entry_in_a_rejected_bin():
    case, _, _, _ = rot.hand_cases()["shared_keypoint_one_entry_rejected"]
    assert (case["match_kp"] == 5).sum() == 2 and case["match_kp"][21] == 5
    owner, nm, ind = rot.rotation_check(**case)
    assert owner[5] == -1 and nm == 21 and (owner >= 0).sum() == 20      # 22 matches, 21 keypoints, one cleared, one entry subtracted


def test_first_index_on_ties_and_the_ten_percent_rule_in_float():
    assert rot.three_maxima([0, 4, 4, 4, 4]) == (1, 2, 3)
    assert rot.three_maxima([0, 3, 5, 5, 1]) == (2, 3, 1)
    assert rot.three_maxima([10, 1, 1]) == (0, 1, 2)                     # 1 < 0.1f * 10 = 1.0f is false
    assert 0.1 * 10 == 1.0 and float(np.float32(0.1)) * 10 > 1.0         # in double over the float constant the same bins would fall
    assert rot.three_maxima([20, 1, 1]) == (0, -1, -1)
    assert rot.three_maxima([20, 2, 1]) == (0, 1, -1)
    assert rot.three_maxima([0] * 30) == (-1, -1, -1)


def test_bins():
    assert rot.bin_of(33.0, 3.0) == 1 and rot.bin_of(3.0, 33.0) == 11 and rot.bin_of(359.0, 3.0) == 12 and rot.bin_of(2.0, 358.0) == 0
    assert rot.bin_of(360.0, 0.0) == 12 and rot.bin_of(15.0, 0.0) in (0, 1) and rot.bin_of(np.nan, 0.0) is None
    assert rot.HISTO_LENGTH == 30
