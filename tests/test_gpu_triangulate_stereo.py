"""slamit_triangulate_stereo on the device against tests/triangulate_stereo_ref.py: statuses and sources equal
ref32j's on every decided pair, triangulated points within 4 Y of the all-double variant, unprojected points equal to ref32's bit
for bit; the wavefront and workgroup edges, ragged batches that mix stereo and monocular problems, the monocular equivalence of
the new entry points and their argument errors.

Bounds: Y = 5.62e-8 from the CPU variants alone, 4 Y = 2.25e-7 for the device; measured on one MI355X: 6.46e-8, the
g++-built header's figure, with no status or source different from ref32j's.  test_every_fixture_in_one_ragged_batch
prints the device's largest e before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_ref as mono
from tests import triangulate_stereo_ref as ref
from tests.test_triangulate_stereo_ref import check_against
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


def check(a, out, n=None):
    worst = check_against(a, out["status"], out["source"], out["x3d"], n)
    assert out["n_accepted"] == int((out["status"] == 0).sum())
    n = len(out["status"])
    assert abs(out["n_accepted"] - int((a["r32j"]["status"][:n] == 0).sum())) <= int((~a["decided"][:n]).sum())
    return worst


def same(one, b):
    return (np.array_equal(one["status"], b["status"]) and np.array_equal(one["source"], b["source"]) and one["n_accepted"] == b["n_accepted"]
            and np.array_equal(one["x3d"].view(np.uint32), b["x3d"].view(np.uint32)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_wavefront_and_workgroup_edges(n):
    pr, a = ref.head(ref.fixture(ref.MIXED), n), ref.admissibility(ref.MIXED)
    check(a, api.triangulate(pr), n)


def test_every_fixture_in_one_ragged_batch():
    """All fixtures, an n = 0 problem and a problem without a stereo record in one launch: each equals its single run bit for bit."""
    ks = list(range(len(ref.FIXTURES)))
    probs = [ref.fixture(k) for k in ks] + [ref.head(ref.fixture(0), 0), mono.fixture(8)]
    assert [int(p["n"]) for p in probs[-2:]] == [0, 300] and "ur1" not in probs[-1]
    outs = api.triangulate_batch(probs)
    worst, seen_st, seen_src = 0.0, set(), set()
    for k in ks:
        a = ref.admissibility(k)
        print("fixture %d: device differs from ref32j on %d undecided pairs of %d" % (k, int((outs[k]["status"] != a["r32j"]["status"]).sum()), len(outs[k]["status"])))
        worst = max(worst, check(a, outs[k]))
        seen_st |= set(int(s) for s in outs[k]["status"])
        seen_src |= set(int(s) for s in outs[k]["source"])
    print("device e max %.3e, Y %.3e, bound %.3e" % (worst, ref.yardstick(), 4 * ref.yardstick()))
    assert seen_st == {0, 1, 3, 4, 5, 6, 8} and seen_src == {0, 1, 2, 3}
    assert outs[-2]["n_accepted"] == 0 and outs[-2]["status"].shape == (0,)
    for pr, b in zip(probs, outs):
        assert same(api.triangulate(pr), b)
    # the problem without a stereo record is the monocular one, in the stereo launch too
    old = old_entry_point(mono.fixture(8))
    assert np.array_equal(old["status"], outs[-1]["status"]) and np.array_equal(old["x3d"].view(np.uint32), outs[-1]["x3d"].view(np.uint32))
    assert np.array_equal(outs[-1]["source"], np.where((old["status"] == 1) | (old["status"] == 2), 0, 1))


def records(pr):
    """The C records of one problem -> (P, T or None, keep)."""
    keep = {k: np.ascontiguousarray(pr[k], np.int32 if k[:3] == "oct" else np.float32)
            for k in ("kp1_xy", "kp2_xy", "octave1", "octave2", "scale_factors1", "level_sigma2_1", "scale_factors2", "level_sigma2_2")}
    P = api.TriangulateProblem()
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    P.n, P.n_levels, P.ratio_factor = int(pr["n"]), int(pr["n_levels"]), float(pr["ratio_factor"])
    P.Tcw1, P.Tcw2 = (C.c_float * 12)(*pr["Tcw1"]), (C.c_float * 12)(*pr["Tcw2"])
    P.intr1, P.intr2 = (C.c_float * 6)(*pr["intr1"]), (C.c_float * 6)(*pr["intr2"])
    T = None
    if "ur1" in pr:
        T = api.TriangulateStereo()
        for k in ref.STEREO_KEYS:
            keep[k] = np.ascontiguousarray(pr[k], np.float32)
            setattr(T, k, keep[k].ctypes.data)
        T.mb1, T.mb2, T.bf = float(pr["mb1"]), float(pr["mb2"]), float(pr["bf"])
    return P, T, keep


def old_entry_point(pr):
    """slamit_triangulate itself, not the binding (which goes through the stereo entry point)."""
    P, _, keep = records(pr)
    n = int(pr["n"])
    out = {"status": np.zeros(n, np.uint8), "x3d": np.zeros((n, 3), np.float32)}
    R = api.TriangulateResult(out["status"].ctypes.data, out["x3d"].ctypes.data, 0)
    assert api.lib().slamit_triangulate(0, C.byref(P), C.byref(R)) == 0
    out["n_accepted"] = int(R.n_accepted)
    return out


def test_monocular_equivalence():
    """The stereo entry point with NULL, and with all-negative ur, equals slamit_triangulate bit for bit."""
    pr = mono.fixture(8)
    old = old_entry_point(pr)
    assert old["n_accepted"] > 100
    P, _, keep = records(pr)
    n = int(pr["n"])
    status, x3d, source = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.full(n, 77, np.uint8)
    R = api.TriangulateResult(status.ctypes.data, x3d.ctypes.data, 0)
    assert api.lib().slamit_triangulate_stereo(0, C.byref(P), None, C.byref(R), source.ctypes.data) == 0
    assert np.array_equal(status, old["status"]) and np.array_equal(x3d.view(np.uint32), old["x3d"].view(np.uint32)) and R.n_accepted == old["n_accepted"]
    assert np.array_equal(source, np.where((status == 1) | (status == 2), 0, 1))
    assert api.lib().slamit_triangulate_stereo(0, C.byref(P), None, C.byref(R), None) == 0      # source is optional
    neg = api.triangulate(ref.with_mono_stereo(pr))                                                # every ur = -1, through the stereo kernel
    assert np.array_equal(neg["status"], old["status"]) and np.array_equal(neg["x3d"].view(np.uint32), old["x3d"].view(np.uint32))
    assert neg["n_accepted"] == old["n_accepted"] and np.array_equal(neg["source"], source)
    plain = api.triangulate(pr)
    assert np.array_equal(plain["status"], old["status"]) and np.array_equal(plain["x3d"].view(np.uint32), old["x3d"].view(np.uint32))


def test_hand_made_single_pairs_in_one_batch():
    cases = ref.hand_cases()
    probs = [c[0] for c in cases.values()]
    outs = api.triangulate_batch(probs)
    for (name, (pr, want_st, want_src)), out in zip(cases.items(), outs):
        a = ref.analyse(pr)
        assert a["decided"][0], name
        assert out["status"][0] == a["r32j"]["status"][0] and out["source"][0] == a["r32j"]["source"][0], (name, out["status"], out["source"])
        assert out["source"][0] == want_src and (want_st is None or out["status"][0] == want_st), name
        assert out["n_accepted"] == int(out["status"][0] == 0)
        if out["status"][0] in (1, 2, 9):
            assert np.all(out["x3d"] == 0), name
        if out["source"][0] >= 2:
            assert np.array_equal(out["x3d"][0].view(np.uint32), a["r32"]["x3d"][0].view(np.uint32)), name
    assert 9 in [int(o["status"][0]) for o in outs]


def test_argument_errors_launch_nothing():
    pr = ref.head(ref.fixture(ref.MIXED), 8)
    with pytest.raises(api.SlamitError, match="needs all of"):
        api.triangulate({k: v for k, v in pr.items() if k != "depth2"})
    with pytest.raises(api.SlamitError, match="raw1_xy has"):
        api.triangulate(dict(pr, raw1_xy=pr["raw1_xy"][:5]))
    P, T, keep = records(pr)
    status, x3d, source = np.full(8, 99, np.uint8), np.full((8, 3), 7.0, np.float32), np.full(8, 55, np.uint8)
    R = api.TriangulateResult(status.ctypes.data, x3d.ctypes.data, -5)
    for key in ref.STEREO_KEYS:
        setattr(T, key, None)
        assert api.lib().slamit_triangulate_stereo(0, C.byref(P), C.byref(T), C.byref(R), source.ctypes.data) == -1, key
        assert b"null array in a stereo record" in api.lib().slamit_last_error()
        assert np.all(status == 99) and np.all(x3d == 7.0) and np.all(source == 55) and R.n_accepted == -5
        setattr(T, key, keep[key].ctypes.data)
    P.kp2_xy = None                                                       # the old refusals hold on the new entry point
    assert api.lib().slamit_triangulate_stereo(0, C.byref(P), C.byref(T), C.byref(R), source.ctypes.data) == -1
    assert b"null array" in api.lib().slamit_last_error() and np.all(status == 99) and np.all(source == 55)
    P.kp2_xy = keep["kp2_xy"].ctypes.data
    P.n = 0                                                               # n == 0 reads nothing: null arrays in the record are fine
    T.ur1 = None
    assert api.lib().slamit_triangulate_stereo(0, C.byref(P), C.byref(T), C.byref(R), source.ctypes.data) == 0
    assert R.n_accepted == 0 and np.all(status == 99) and np.all(source == 55)
    P.n, T.ur1 = 8, keep["ur1"].ctypes.data
    assert api.lib().slamit_triangulate_stereo(0, C.byref(P), C.byref(T), C.byref(R), source.ctypes.data) == 0   # the same records, whole again
    a = ref.admissibility(ref.MIXED)
    assert np.array_equal(status[a["decided"][:8]], a["r32j"]["status"][:8][a["decided"][:8]]) and R.n_accepted == int((status == 0).sum())
    assert np.all(source <= 3)
