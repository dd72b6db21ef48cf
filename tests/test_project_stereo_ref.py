"""project_point_stereo of csrc/project.h on the CPU: ur bit-equal to a numpy restatement on synth_project problems of the two
forms that have a reader of it, zero for every rejected point, every other output that of project_point; and the mains that
tests/project_ref.py builds around project_point still compile against the header."""
import numpy as np
import pytest

from tests import project_ref as ref
from tests import project_stereo_ref as sref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("k", [k for k, f in enumerate(ref.FIXTURES) if f[0] in (ref.LAST_FRAME, ref.FUSE)])
def test_ur_is_the_restatement(k):
    pr = ref.fixture(k)
    bf = sref.BF[int(pr["form"])]
    h = sref.host_points_stereo(pr, bf)
    plain = ref.host_fixture(k)                       # the existing main, built from the same header
    for key in ("status", "level", "level_min", "level_max", "valid"):
        assert np.array_equal(h[key], plain[key]), key
    for key in ("u", "v", "r", "uvr"):
        assert np.array_equal(bits(h[key]), bits(plain[key])), key
    ur, u = sref.ur_numpy(pr, bf, h["status"])
    ok = h["status"] == 0
    assert ok.sum() >= 30 and (~ok).sum() >= 30
    assert np.array_equal(bits(u[ok]), bits(h["u"][ok]))
    assert np.array_equal(bits(ur), bits(h["ur"]))
    assert np.all(bits(h["ur"][~ok]) == 0)            # +0.0f, not merely zero
    # a disparity: the right-image column lies left of u by bf / z
    assert np.all(h["ur"][ok] < h["u"][ok])


def test_bf_zero_gives_u():
    pr = ref.fixture(ref.first_fixture(ref.FUSE))
    h = sref.host_points_stereo(pr, 0.0)
    ok = h["status"] == 0
    assert np.array_equal(bits(h["ur"][ok]), bits(h["u"][ok])) and np.all(bits(h["ur"][~ok]) == 0)


def test_the_existing_mains_still_build():
    exe = ref.host_exe()
    pr = ref.head(ref.fixture(ref.first_fixture(ref.SIM3_PAIR)), 65)
    assert len(ref.host_points(pr)["status"]) == 65 and exe
