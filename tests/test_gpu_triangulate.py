"""slamit_triangulate on the device against tests/triangulate_ref.py: statuses equal ref32j's on every decided pair,
points within 4 Y of the all-double variant, the wavefront and workgroup edges, ragged batches and the argument errors.

Bounds: Y = 5.94e-8 from the CPU variants alone, 4 Y = 2.38e-7 for the device; the g++-built header reaches 5.79e-8.
test_every_fixture_in_one_batch prints the device's largest e before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_ref as ref
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

MIXED = 8   # the fixture with points behind the camera and octave jumps among the usual outcomes: codes 0, 3, 5, 6, 8


def check(pr, a, out, n=None):
    """Device result `out` of problem pr against the analysis a (sliced to the first n pairs)."""
    n = int(pr["n"]) if n is None else n
    st, x = out["status"], out["x3d"]
    assert st.shape == (n,) and x.shape == (n, 3)
    d = a["decided"][:n]
    want = a["r32j"]["status"][:n]
    assert np.array_equal(st[d], want[d]), np.flatnonzero(d & (st != want))
    assert out["n_accepted"] == int((st == 0).sum())
    assert abs(out["n_accepted"] - int((want == 0).sum())) <= int((~d).sum())
    acc = (st == 0) & a["all_accept"][:n]
    e = ref.point_error({"A": a["r64"]["A"][:n], "x3d": a["r64"]["x3d"][:n]}, x)
    assert np.all(e[acc] <= 4 * ref.yardstick()), (e[acc].max(), 4 * ref.yardstick())
    assert np.all(x[(st == 1) | (st == 2)] == 0)
    return float(e[acc].max()) if acc.any() else 0.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_wavefront_and_workgroup_edges(n):
    pr, a = ref.head(ref.fixture(MIXED), n), ref.admissibility(MIXED)
    check(pr, a, api.triangulate(pr), n)


def test_no_pairs_and_no_problems():
    pr = ref.head(ref.fixture(MIXED), 0)
    out = api.triangulate(pr)
    assert out["n_accepted"] == 0 and out["status"].shape == (0,) and out["x3d"].shape == (0, 3)
    assert api.triangulate_batch([]) == []
    assert api.lib().slamit_triangulate_batch(0, 0, None, None) == 0


def test_a_ragged_batch_equals_its_problems_run_singly():
    full = ref.fixture(MIXED)
    probs = [full, ref.head(full, 0), ref.fixture(11)]
    assert [int(p["n"]) for p in probs] == [300, 0, 65]
    batch = api.triangulate_batch(probs)
    for pr, b in zip(probs, batch):
        one = api.triangulate(pr)
        assert np.array_equal(one["status"], b["status"]) and np.array_equal(one["x3d"].view(np.uint32), b["x3d"].view(np.uint32))
        assert one["n_accepted"] == b["n_accepted"]
    assert batch[0]["n_accepted"] > 100 and batch[2]["n_accepted"] > 20


def test_every_fixture_in_one_batch():
    ks = range(len(ref.FIXTURES))
    outs = api.triangulate_batch([ref.fixture(k) for k in ks])
    worst, seen = 0.0, set()
    for k, out in zip(ks, outs):
        a = ref.admissibility(k)
        print("fixture %d: device differs from ref32j on %d undecided pairs of %d" % (k, int((out["status"] != a["r32j"]["status"]).sum()), len(out["status"])))
        worst = max(worst, check(ref.fixture(k), a, out))
        seen |= set(int(s) for s in out["status"])
    print("device e max %.3e, Y %.3e, bound %.3e" % (worst, ref.yardstick(), 4 * ref.yardstick()))
    assert seen == {0, 1, 3, 4, 5, 6, 8}


def hand_made(X, t2=(-0.5, 0.0, 0.0), o1=0, o2=0, d1=(0.0, 0.0)):
    """One pair: keyframe 1 at the origin, keyframe 2 with translation t2 (no rotation), the exact projections of X, keypoint 1
    moved by d1 pixels."""
    f32 = np.float32
    K = np.array([500.0, 500.0, 320.0, 240.0, 1 / 500.0, 1 / 500.0], f32)
    T1 = np.eye(4)[:3].astype(f32)
    T2 = T1.copy()
    T2[:, 3] = t2
    X = np.asarray(X, np.float64)
    X2 = X + np.asarray(t2, np.float64)
    sf = f32(1.2) ** np.arange(8, dtype=f32)
    kp1 = np.array([[500 * X[0] / X[2] + 320 + d1[0], 500 * X[1] / X[2] + 240 + d1[1]]], f32)
    kp2 = np.array([[500 * X2[0] / X2[2] + 320, 500 * X2[1] / X2[2] + 240]], f32)
    return dict(n=1, Tcw1=T1.reshape(12), Tcw2=T2.reshape(12), intr1=K, intr2=K, kp1_xy=kp1, kp2_xy=kp2, octave1=np.array([o1], np.int32),
                octave2=np.array([o2], np.int32), n_levels=8, scale_factors1=sf, level_sigma2_1=sf * sf, scale_factors2=sf, level_sigma2_2=sf * sf,
                ratio_factor=f32(1.5) * f32(1.2))


HAND = {
    0: dict(X=(0.2, 0.1, 4.0)),
    1: dict(X=(0.2, 0.1, 400.0)),                                     # rays all but parallel
    3: dict(X=(0.2, 0.1, -4.0)),                                      # behind both
    4: dict(X=(0.3, 0.2, 3.0), t2=(0.0, 0.0, -5.0)),                  # keyframe 2 five units ahead: the point lies between the two
    5: dict(X=(0.2, 0.1, 4.0), d1=(0.0, 10.0)),                       # 10 px across the epipolar line: about 5 px lands in each image
    6: dict(X=(0.2, 0.1, 4.0), d1=(0.0, 10.0), o1=7),                 # the same, with keyframe 1's gate at octave 7 (76.9 px^2)
    8: dict(X=(0.2, 0.1, 4.0), o1=5),                                 # ratioOctave 2.49 against ratioDist 1 and ratioFactor 1.8
}


def test_one_hand_made_problem_per_reachable_code():
    probs = [hand_made(**HAND[c]) for c in sorted(HAND)]
    outs = api.triangulate_batch(probs)
    for c, pr, out in zip(sorted(HAND), probs, outs):
        a = ref.analyse(pr)
        assert a["decided"][0] and a["r32j"]["status"][0] == c, (c, a["r32j"]["status"])
        assert out["status"][0] == c and out["n_accepted"] == (1 if c == 0 else 0), (c, out["status"])
    assert np.abs(outs[0]["x3d"][0] - np.array([0.2, 0.1, 4.0])).max() < 1e-3


def test_argument_errors_launch_nothing():
    pr = ref.head(ref.fixture(MIXED), 8)
    for bad in (8, -1, 1 << 20):
        o = pr["octave2"].copy()
        o[5] = bad
        with pytest.raises(api.SlamitError, match=r"octave outside \[0, n_levels\)") as e:
            api.triangulate(dict(pr, octave2=o))
        assert "(-1)" in str(e.value)                                # SLAMIT_ERR_ARG
    big = api.TRIANGULATE_MAX_N + 1
    with pytest.raises(api.SlamitError, match="SLAMIT_TRIANGULATE_MAX_N"):
        api.triangulate(dict(pr, n=big, kp1_xy=np.ones((big, 2), np.float32), kp2_xy=np.ones((big, 2), np.float32),
                             octave1=np.zeros(big, np.int32), octave2=np.zeros(big, np.int32)))
    with pytest.raises(api.SlamitError, match="n_levels"):
        api.triangulate(dict(pr, n_levels=17, **{k: np.ones(17, np.float32) for k in ("scale_factors1", "level_sigma2_1", "scale_factors2", "level_sigma2_2")}))
    with pytest.raises(api.SlamitError, match="same length"):
        api.triangulate(dict(pr, octave1=pr["octave1"][:5]))
    # a null array with n > 0, straight through the C-ABI: SLAMIT_ERR_ARG, a message, and the outputs untouched
    P, R = api.TriangulateProblem(), api.TriangulateResult()
    keep = {k: np.ascontiguousarray(pr[k]) for k in ("kp1_xy", "kp2_xy", "octave1", "octave2", "scale_factors1", "level_sigma2_1", "scale_factors2", "level_sigma2_2")}
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    P.n, P.n_levels, P.ratio_factor = 8, 8, 1.8
    P.Tcw1, P.Tcw2 = (C.c_float * 12)(*pr["Tcw1"]), (C.c_float * 12)(*pr["Tcw2"])
    P.intr1, P.intr2 = (C.c_float * 6)(*pr["intr1"]), (C.c_float * 6)(*pr["intr2"])
    status, x3d = np.full(8, 99, np.uint8), np.full((8, 3), 7.0, np.float32)
    R.status, R.x3d, R.n_accepted = status.ctypes.data, x3d.ctypes.data, -5
    P.kp2_xy = None
    assert api.lib().slamit_triangulate(0, C.byref(P), C.byref(R)) == -1
    assert b"null array" in api.lib().slamit_last_error()
    assert np.all(status == 99) and np.all(x3d == 7.0) and R.n_accepted == -5
    P.kp2_xy = keep["kp2_xy"].ctypes.data
    assert api.lib().slamit_triangulate(0, C.byref(P), C.byref(R)) == 0          # the same record, whole again
    assert np.all(status <= 8) and R.n_accepted == int((status == 0).sum())
