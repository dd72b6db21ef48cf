"""slamit_bow_search_stereo on the device against tests/bow_stereo_ref.py (ORBmatcher.cc:695-793 on stereo keyframes): identical
match12, dist12 and count on a scene whose epipole lies inside image 2, with candidate groups of 1, 63, 64, 65 and 130; a NULL
record is slamit_bow_search; the argument errors."""
import ctypes as C

import numpy as np
import pytest

from tests.test_bow_stereo_ref import expected, scene
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


def device(s1, s2, g, epi, stereo):
    return api.ORBmatcher.bow_search(s1, s2, g, mode=1, th=50, epi=epi, stereo=stereo)


@pytest.mark.parametrize("only", [False, True])
def test_the_device_equals_the_restatement(only):
    s1, s2, g, epi = scene(0)
    sizes = (g["c_ptr"][1:] - g["c_ptr"][:-1]).tolist()
    assert sizes[:5] == [1, 63, 64, 65, 130] and len(s1["desc"]) == 300
    want = expected(0, only)
    got = device(s1, s2, g, epi, dict(ur1=s1["ur"], ur2=s2["ur"], only_stereo=only))
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:8]
    assert got[2] == want[2] == int((want[0] >= 0).sum()) > 20
    if not only:
        assert int((want[0] != expected(0, None)[0]).sum()) >= 10      # what a device without the stereo branch would return


def test_a_second_scene():
    s1, s2, g, epi = scene(1)
    want = expected(1, False)
    got = device(s1, s2, g, epi, dict(ur1=s1["ur"], ur2=s2["ur"], only_stereo=False))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_a_null_record_and_all_monocular_flags_equal_slamit_bow_search():
    s1, s2, g, epi = scene(0)
    want = expected(0, None)
    old = device(s1, s2, g, epi, None)
    assert np.array_equal(old[0], want[0]) and np.array_equal(old[1], want[1]) and old[2] == want[2]
    none = device(s1, s2, g, epi, dict(ur1=np.full(len(s1["ur"]), -1.0, np.float32), ur2=np.full(len(s2["ur"]), np.nan, np.float32), only_stereo=False))
    assert np.array_equal(none[0], old[0]) and np.array_equal(none[1], old[1]) and none[2] == old[2]
    m, d, nm = raw_call(s1, s2, g, epi, None)
    assert np.array_equal(m, old[0]) and np.array_equal(d, old[1]) and nm == old[2]


def raw_call(s1, s2, g, epi, st, mode=1, expect=0):
    """slamit_bow_search_stereo straight through the C-ABI with the record st (or NULL)."""
    d1, d2 = np.ascontiguousarray(s1["desc"], np.uint8), np.ascontiguousarray(s2["desc"], np.uint8)
    v1, v2 = np.ascontiguousarray(s1["valid"], np.uint8), np.ascontiguousarray(s2["valid"], np.uint8)
    qp, qi, cp, ci = (np.ascontiguousarray(g[k], np.int32) for k in ("q_ptr", "q_idx", "c_ptr", "c_idx"))
    gg = api.BowGroups(len(qp) - 1, qp.ctypes.data, qi.ctypes.data, cp.ctypes.data, ci.ctypes.data)
    k1, k2, o2 = np.ascontiguousarray(s1["kp_xy"], np.float32), np.ascontiguousarray(s2["kp_xy"], np.float32), np.ascontiguousarray(s2["kp_octave"], np.int32)
    rule = api.BowRule()
    rule.mode, rule.th, rule.th_inclusive, rule.nnratio = mode, 50, 1, 0.6
    rule.F12 = (C.c_float * 9)(*[float(v) for v in epi["F12"]])
    rule.ex, rule.ey = float(epi["ex"]), float(epi["ey"])
    rule.kp1_xy, rule.kp2_xy, rule.kp2_octave = k1.ctypes.data, k2.ctypes.data, o2.ctypes.data
    rule.scale_factor = (C.c_float * 16)(*(list(epi["scale_factor"]) + [1.0] * 8))
    rule.level_sigma2 = (C.c_float * 16)(*(list(epi["level_sigma2"]) + [1.0] * 8))
    m, d = np.full(len(d1), 77, np.int32), np.full(len(d1), 88, np.int32)
    nm = C.c_int32(-3)
    rc = api.lib().slamit_bow_search_stereo(0, d1.ctypes.data, len(d1), v1.ctypes.data, d2.ctypes.data, len(d2), v2.ctypes.data, C.byref(gg), C.byref(rule),
                                            C.byref(st) if st is not None else None, m.ctypes.data, d.ctypes.data, C.byref(nm))
    assert rc == expect, (rc, api.lib().slamit_last_error())
    return m, d, nm.value


def test_argument_errors_launch_nothing():
    s1, s2, g, epi = scene(0)
    u1, u2 = np.ascontiguousarray(s1["ur"]), np.ascontiguousarray(s2["ur"])
    # SearchByBoW has no stereo branch
    m, d, nm = raw_call(s1, s2, g, epi, api.BowStereo(u1.ctypes.data, u2.ctypes.data, 0), mode=0, expect=-1)
    assert b"needs mode 1" in api.lib().slamit_last_error() and np.all(m == 77) and np.all(d == 88) and nm == -3
    for st in (api.BowStereo(None, u2.ctypes.data, 0), api.BowStereo(u1.ctypes.data, None, 1)):
        m, d, nm = raw_call(s1, s2, g, epi, st, expect=-1)
        assert b"null ur1 / ur2" in api.lib().slamit_last_error() and np.all(m == 77) and np.all(d == 88) and nm == -3
    with pytest.raises(api.SlamitError, match="n1 / n2 entries"):
        device(s1, s2, g, epi, dict(ur1=u1[:5], ur2=u2, only_stereo=False))
    m, d, nm = raw_call(s1, s2, g, epi, api.BowStereo(u1.ctypes.data, u2.ctypes.data, 0))      # the same call, whole
    assert nm == expected(0, False)[2]
