"""The checker of the stereo SearchForTriangulation on the CPU (tests/bow_stereo_ref.py): without stereo keypoints it is the
oracle's mode 1 exactly; on a scene whose epipole lies inside image 2 the stereo flags change matches through the skipped epipole
test, and only_stereo removes every monocular query and candidate."""
import functools

import numpy as np
import pytest

from oracle import bindings as ob
from tests import bow_stereo_ref as ref
from weiner_slamit_v2_amd import synth


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    return synth.synth_bow_stereo(seed=seed)


@functools.lru_cache(maxsize=None)
def expected(seed, only):
    """The restatement on scene(seed): only = None is the monocular reading, else only_stereo."""
    s1, s2, g, epi = scene(seed)
    st = None if only is None else dict(ur1=s1["ur"], ur2=s2["ur"], only_stereo=only)
    return ref.search_for_triangulation(s1, s2, g, epi, th=50, stereo=st)


@pytest.mark.parametrize("seed", [1, 2, 4, 5])
def test_without_stereo_it_equals_the_oracle(seed):
    s1, s2, g, epi = synth.synth_bow(700, 650, 50, seed, mode=1)
    o = ob.bow_search(s1, s2, g, mode=1, th=50, epi=epi)
    for st in (None, dict(ur1=np.full(700, -1.0, np.float32), ur2=np.full(650, np.nan, np.float32), only_stereo=False)):
        r = ref.search_for_triangulation(s1, s2, g, epi, th=50, stereo=st)
        assert np.array_equal(r[0], o[0]) and np.array_equal(r[1], o[1]) and r[2] == o[2] > 0


def test_the_stereo_scene_without_flags_equals_the_oracle():
    s1, s2, g, epi = scene(0)
    o = ob.bow_search(s1, s2, g, mode=1, th=50, epi=epi)
    r = expected(0, None)
    assert np.array_equal(r[0], o[0]) and np.array_equal(r[1], o[1]) and r[2] == o[2] > 100
    sizes = (g["c_ptr"][1:] - g["c_ptr"][:-1]).tolist()
    assert sizes[:5] == [1, 63, 64, 65, 130] and 280 <= len(s1["desc"]) <= 320
    assert 0 < epi["ex"] < 640 and 0 < epi["ey"] < 480                     # the epipole lies inside image 2


def test_stereo_flags_change_matches_through_the_skipped_epipole_test():
    s1, s2, g, epi = scene(0)
    m0, m1 = expected(0, None), expected(0, False)
    changed = np.flatnonzero(m0[0] != m1[0])
    print("monocular %d matches, stereo %d, %d queries differ" % (m0[2], m1[2], len(changed)))
    assert len(changed) >= 10
    # every change is a candidate inside the epipole's disc that only a stereo pair may take
    for q in changed:
        c = m1[0][q]
        assert c >= 0 and (s1["ur"][q] >= 0 or s2["ur"][c] >= 0)
        dx, dy = np.float32(epi["ex"]) - s2["kp_xy"][c, 0], np.float32(epi["ey"]) - s2["kp_xy"][c, 1]
        assert dx * dx + dy * dy < 100 * epi["scale_factor"][s2["kp_octave"][c]]
    # a NaN ur is monocular, 0.0f is stereo (:709, :732)
    assert np.isnan(s1["ur"]).sum() == 1 and np.isnan(s2["ur"]).sum() == 1 and (s1["ur"] == 0).sum() == 1 and (s2["ur"] == 0).sum() == 1


def test_only_stereo_removes_every_monocular_query_and_candidate():
    s1, s2, g, epi = scene(0)
    m1, m2 = expected(0, False), expected(0, True)
    with np.errstate(invalid="ignore"):
        mono1, mono2 = ~(s1["ur"] >= 0), ~(s2["ur"] >= 0)
    assert np.all(m2[0][mono1] == -1) and np.all(m2[1][mono1] == 256)
    taken = m2[0][m2[0] >= 0]
    assert len(taken) == m2[2] > 20 and not mono2[taken].any()
    assert (m1[0][mono1] >= 0).sum() > 10 and mono2[m1[0][m1[0] >= 0]].sum() > 10   # both kinds were there to remove
