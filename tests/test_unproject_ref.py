"""csrc/unproject.h on the host against the numpy restatement of the reference's loops (tests/unproject_ref.py), bit for bit, and the
admissibility of the fixtures the GPU tests run on.  No GPU."""
import numpy as np
import pytest

from tests import unproject_ref as ur


def _all_problems():
    out = [(name, ur.fixture(name), ur.ref_fixture(name)) for name in ur.FIXTURES]
    out += [("shape%d" % k, ur.shape_fixture(k), ur.ref_shape(k)) for k in range(len(ur.SHAPES))]
    return out


def _sorted_depths(pr):
    d = np.asarray(pr["depth"], np.float32)
    with np.errstate(invalid="ignore"):
        return sorted((float(z), i) for i, z in enumerate(d) if z > 0)


@pytest.mark.parametrize("name", sorted(ur.FIXTURES))
def test_header_equals_restatement_on_fixtures(name):
    ur.assert_same(ur.host_walk(ur.fixture(name)), ur.ref_fixture(name), name)


def test_header_equals_restatement_on_shapes():
    for k in range(len(ur.SHAPES)):
        ur.assert_same(ur.host_walk(ur.shape_fixture(k)), ur.ref_shape(k), "shape %d %r" % (k, ur.SHAPES[k]))


def test_header_equals_restatement_at_the_ceiling():
    """The input of tests/test_gpu_unproject_ceiling.py: 8,191 keypoints, all of them candidates."""
    pr = ur.ceiling_fixture()
    ref = ur.walk(pr)
    assert pr["n"] == 8191 == ref["n_candidates"] and ref["n_created"] > 1000
    ur.assert_same(ur.host_walk(pr), ref, "ceiling")


@pytest.mark.parametrize("name", sorted(ur.RGBD_CASES))
def test_header_equals_restatement_rgbd(name):
    pr, ref = ur.rgbd_fixture(name), ur.ref_rgbd(name)
    ur.assert_same_rgbd(ur.host_rgbd(pr), ref, name)
    assert set(ref["status"].tolist()) == {0, 1, 2}
    h, w = pr["plane"].shape
    cols, rows = pr["kps"]["x"][:3].astype(np.int64), pr["kps"]["y"][:3].astype(np.int64)
    assert cols[0] == w - 1 and rows[1] == h - 1 and (cols[2], rows[2]) == (w - 1, h - 1)      # last column, last row, both
    assert ref["status"][3] == 0 and pr["plane"][0, 0] == 0                                     # a zero depth
    assert ref["status"][4] == 0                                                                 # (-0.5, -0.99) truncates to pixel (0, 0)
    assert pr["storage"].shape[1] == w + ur.RGBD_CASES[name]["pad"]


def test_closed_form_equals_the_literal_loop():
    for name, pr, ref in _all_problems():
        th, mp = float(pr["th_depth"]), int(pr["min_points"])
        depths = [z for z, _ in _sorted_depths(pr)]
        m, c = len(depths), sum(1 for z in depths if not z > th)
        assert (m, c) == (ref["n_candidates"], ref["n_close"]), name
        if int(pr["mode"]) == 1:
            assert ref["n_visited"] == m
            continue
        assert ur.literal_visits(depths, th, mp) == ur.closed_form(m, c, mp) == ref["n_visited"], name
    rs = np.random.RandomState(5)
    for _ in range(3000):
        m, mp = int(rs.randint(0, 40)), int(rs.randint(0, 30))
        depths = sorted(rs.choice([0.5, 1.0, 2.0, 2.0, 3.0, 4.0, 4.0, 9.0, float("inf")], m).tolist())
        th = float(rs.choice([0.1, 1.0, 2.0, 3.5, 9.0, 1e9]))
        assert ur.literal_visits(depths, th, mp) == ur.closed_form(m, sum(1 for z in depths if not z > th), mp)


def test_fixtures_are_admissible():
    probs = _all_problems()
    seen = set()
    for name, pr, ref in probs:
        seen |= set(ref["status"].tolist())
        assert pr["n"] <= 2048, name
        made = ref["status"] == 3
        pc = ref["pos"][made] - np.asarray(pr["Ow"], np.float32)[None, :]
        assert not np.any(pc == 0), "%s: a zero component of Pos - Ow would let the sign of zero decide" % name
        assert np.array_equal(np.flatnonzero(ref["order"] >= 0), np.arange(ref["n_visited"])), name
    assert seen == {0, 1, 2, 3, 4}
    assert set(ur.ref_fixture(ur.MIXED)["status"][:65].tolist()) == {0, 1, 2, 3, 4}
    fewer = {ref["n_close"] < int(pr["min_points"]) for name, pr, ref in probs if int(pr["mode"]) == 0 and ref["n_candidates"] > 0}
    assert fewer == {True, False}
    # a tie in depth across the last visited position p = max(c, min_points): equal depths at p (visited) and p + 1 (not visited),
    # and in one fixture with c < min_points also at p - 1
    straddle = below = False
    for name, pr, ref in probs:
        if int(pr["mode"]) == 1:
            continue
        s = _sorted_depths(pr)
        p = max(ref["n_close"], int(pr["min_points"]))
        if p + 1 < len(s) and s[p][0] == s[p + 1][0]:
            assert ref["n_visited"] == p + 1 and ref["status"][s[p][1]] in (2, 3, 4) and ref["status"][s[p + 1][1]] == 1, name
            straddle = True
            below = below or (p >= 1 and s[p - 1][0] == s[p][0])
    assert straddle and below
    depths = np.concatenate([np.asarray(pr["depth"], np.float32) for _, pr, _ in probs])
    assert any(np.any(np.asarray(pr["depth"], np.float32) == np.float32(pr["th_depth"])) for _, pr, _ in probs)
    bits = depths.view(np.uint32)
    assert np.any(depths == -1) and np.any(bits == 0) and np.any(np.isposinf(depths)) and np.any(np.isnan(depths))
    assert np.any((bits > 0) & (bits < 0x00800000)), "a denormal depth"
    # +inf and the denormal are candidates, the NaN is none; at least one +inf keypoint is visited
    inf_visited = False
    for name, pr, ref in probs:
        d = np.asarray(pr["depth"], np.float32)
        b = d.view(np.uint32)
        assert np.all(ref["status"][np.isnan(d)] == 0) and np.all(ref["status"][(b > 0) & (b < 0x00800000)] != 0), name
        assert np.all(ref["status"][np.isposinf(d)] != 0), name
        inf_visited = inf_visited or bool(np.any(ref["status"][np.isposinf(d)] >= 2))
    assert inf_visited


def test_the_two_constructors_differ_in_the_sign_of_zero_only():
    """ctor KEYFRAME is ctor FRAME on every fixture point (no zero component occurs there); on a constructed point whose
    quotient underflows to -0 the two differ in that component's sign bit and in nothing else."""
    pr = dict(ur.fixture("mixed"))
    a = ur.host_walk(pr)
    b = ur.host_walk(dict(pr, ctor=1))
    ur.assert_same(a, b, "ctor")
    one = dict(pr, n=1, Rwc=np.eye(3, dtype=np.float32).reshape(9), Ow=np.array([0.0, 1.0, 2.0], np.float32), cx=np.float32(10.0),
               depth=np.array([2.0], np.float32), tracked=np.zeros(1, np.uint8), min_points=0)
    kp = pr["kps_un"][:1].copy()
    kp["x"], kp["y"], kp["octave"] = 9.5, 300.0, 0
    one["kps_un"] = kp
    one["invfx"] = np.float32(1e-45)   # the least denormal: x = (-0.5 * 2) * invfx is minus one unit, and times 1 / norm < 0.5 it rounds to -0
    fa, fb = ur.host_walk(dict(one, ctor=0)), ur.host_walk(dict(one, ctor=1))
    ur.assert_same(fa, ur.walk(dict(one, ctor=0)), "ctor 0")
    ur.assert_same(fb, ur.walk(dict(one, ctor=1)), "ctor 1")
    assert fa["status"][0] == fb["status"][0] == 3
    assert fa["normal"].view(np.uint32)[0, 0] == 0x80000000 and fb["normal"].view(np.uint32)[0, 0] == 0
    assert np.array_equal(fa["normal"][0, 1:], fb["normal"][0, 1:]) and ur.same_bits(fa["pos"], fb["pos"])
