"""slamit_unproject_closest at its ceiling: SLAMIT_STEREO_MAX_KP = 8,191 keypoints, all of them candidates -- 8,192 keys of 8 bytes
in LDS, the 1,024-thread workgroup, 91 stages of the sorting network -- and one more keypoint refused before a launch.  The input is
checked against csrc/unproject.h on the CPU in tests/test_unproject_ref.py."""
import numpy as np
import pytest

from tests import unproject_ref as ur
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


def test_at_the_ceiling():
    pr = ur.ceiling_fixture()
    assert int(pr["n"]) == api.STEREO_MAX_KP == 8191
    ref = ur.walk(pr)
    assert ref["n_candidates"] == 8191 and ref["n_visited"] == ref["n_close"] + 1 > 5000
    ur.assert_same(api.unproject_closest(pr), ref, "ceiling")


def test_all_mode_at_the_ceiling():
    pr = dict(ur.ceiling_fixture(), mode=1, ctor=1)
    ref = ur.walk(pr)
    assert ref["n_visited"] == 8191
    ur.assert_same(api.unproject_closest(pr), ref, "ceiling, mode ALL")


def test_one_more_is_refused():
    pr = ur.ceiling_fixture()
    n = 8192
    big = dict(pr, n=n, kps_un=np.concatenate([pr["kps_un"], pr["kps_un"][:1]]), depth=np.concatenate([pr["depth"], pr["depth"][:1]]),
               tracked=np.concatenate([pr["tracked"], pr["tracked"][:1]]))
    with pytest.raises(api.SlamitError, match="SLAMIT_STEREO_MAX_KP") as e:
        api.unproject_closest(big)
    assert "(-3)" in str(e.value)
