"""slamit_pnp_ransac_batch / slamit_pnp_refine_batch on the GPU against the numpy restatement (tests/pnp_ref.py): the device's
CheckInliers bits against the restated CheckInliers on the device's own pose (exact, every hypothesis), poses and counts against
variant A on the admitted hypotheses, Refine(), the whole solver through api.PnPsolver, batch == single, the wavefront edges, the
legal degenerates, the errors and the ceilings.  What makes these checks meaningful is asserted on the CPU (tests/test_pnp_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import pnp_ref as ref
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

ALL = list(ref.FIXTURES)
_dev = {}


def dev_hyp(name):
    """The device's hypotheses of a fixture, evaluated once."""
    if name not in _dev:
        _dev[name] = api.PnPsolver.ransac(dict(ref.fixture(name), quads=ref.admissibility(name)["quads"]))
    return _dev[name]


def check_own_bits(pr, g):
    """bits and counts == the restated CheckInliers on the device's own double pose, for every hypothesis."""
    n = len(pr["max_err"])
    flags, _ = ref.check_inliers(g["pose"], pr["p3d"], pr["p2d"], pr["max_err"], pr["intr"])
    assert np.array_equal(ref.unpack_bits(g["inlier_bits"], n), flags)
    assert np.array_equal(g["inlier_bits"], ref.pack_bits(flags))            # the bits past n are zero
    assert np.array_equal(g["n_inliers"], flags.sum(1))


@pytest.mark.parametrize("name", ALL)
def test_hypotheses(name):
    pr, a = ref.fixture(name), ref.admissibility(name)
    g = dev_hyp(name)
    check_own_bits(pr, g)
    ad, sA = a["admitted"], a["A"]["solver"]
    assert a["not_admitted_frac"] <= 0.02
    ok, gap = ref.within(g["pose"][ad], sA.pose[ad])
    print("fixture %s: n %d hyp %d, admitted %d, largest pose gap to A %.3g" % (name, pr["n"], len(ad), int(ad.sum()), gap))
    assert ok, gap
    assert np.array_equal(g["n_inliers"][ad], sA.counts[ad])
    assert np.all((g["n_inliers"] >= 0) & (g["n_inliers"] <= pr["n"]))


@pytest.mark.parametrize("name", ALL)
def test_refine(name):
    pr, cases = ref.fixture(name), ref.refine_cases(name)
    assert cases
    res = api.PnPsolver.refine([dict(pr, subset=s) for s, _ in cases])
    for (sub, (pose, count, flags)), r in zip(cases, res):
        ok, gap = ref.within(r["pose"], pose)
        print("fixture %s: subset of %d, largest refine pose gap to A %.3g" % (name, int(sub.sum()), gap))
        assert ok, gap
        assert np.array_equal(ref.unpack_bits(r["inlier_bits"], pr["n"]), flags) and r["n_inliers"] == count
        own, _ = ref.check_inliers(r["pose"], pr["p3d"], pr["p2d"], pr["max_err"], pr["intr"])
        assert np.array_equal(r["inlier_bits"], ref.pack_bits(own[0]))


@pytest.mark.parametrize("name", ALL)
def test_end_to_end_through_the_solver(name):
    """The same accepted hypothesis, inlier set and bNoMore trace as the restatement, iterate(5) by iterate(5)."""
    pr, a = ref.fixture(name), ref.admissibility(name)
    want, trace = a["A"]["result"], a["A"]["trace"]
    rand_int, _ = ref.scripted_rand(pr["seed"])
    s = api.PnPsolver(pr, rand_int)
    s.SetRansacParameters(*pr["params"])
    sA = a["A"]["solver"]
    assert (s.mRansacMinInliers, s.mRansacMaxIts) == (sA.minInliers, sA.maxIts)
    got = []
    for _ in range(4):
        T, no_more, vb, nin = s.iterate(5)
        got.append(bool(no_more))
        if T is not None or no_more:
            break
    assert np.array_equal(s.quads[:len(a["quads"])], a["quads"])
    assert got == trace and s.kind == want["kind"] and nin == want["nInliers"]
    assert np.array_equal(vb, want["flags"])
    if want["kind"]:
        assert s.accepted == want["h"]
        assert T.dtype == np.float32 and np.array_equal(T[3], [0, 0, 0, 1])
        ok, gap = ref.within(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]), want["pose"], ref.TOL + 2.0 ** -23)   # the float32 rounding on top
        assert ok, gap
    else:
        assert T is None
    assert set(sA.refined) <= set(s.refined)   # every Refine() of the reference's loop was in the one refine call


def test_the_special_fixtures_are_what_they_are_named():
    a = ref.admissibility("refine_fails_first")
    assert len(a["A"]["records"]) >= 2 and a["A"]["result"]["kind"] == "refined" and a["A"]["result"]["h"] != a["A"]["records"][0]
    assert ref.admissibility("never")["A"]["result"]["kind"] == "best"


@pytest.mark.parametrize("names", [["n150"], ALL[:5], ALL])
def test_batch_equals_single_bit_for_bit(names):
    probs = [dict(ref.fixture(k), quads=ref.admissibility(k)["quads"]) for k in names]
    batch = api.PnPsolver.ransac(probs)
    for k, b in zip(names, batch):
        s = dev_hyp(k)
        for key in ("pose", "n_inliers", "inlier_bits"):
            assert np.array_equal(b[key].view(np.uint32), s[key].view(np.uint32)), (k, key)
    nobits = api.PnPsolver.ransac(probs, want_bits=False)                     # inlier_bits is nullable
    for a, b in zip(nobits, batch):
        assert np.array_equal(a["n_inliers"], b["n_inliers"]) and np.array_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64))
    jobs = [dict(ref.fixture(k), subset=s) for k in names for s, _ in ref.refine_cases(k)]
    rb = api.PnPsolver.refine(jobs)
    for j, b in zip(jobs, rb):
        s = api.PnPsolver.refine(j)
        assert np.array_equal(b["pose"].view(np.uint64), s["pose"].view(np.uint64)) and b["n_inliers"] == s["n_inliers"]
        assert np.array_equal(b["inlier_bits"], s["inlier_bits"])


@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("nh", [1, 5])
def test_wavefront_edges(n, nh):
    v = ref.variants_on(("head", "n150", n, nh))
    g = api.PnPsolver.ransac(dict(v["pr"], quads=v["quads"]))
    check_own_bits(v["pr"], g)
    ad = v["admitted"]
    assert ad.any()
    ok, gap = ref.within(g["pose"][ad], v["pose"][ad])
    assert ok, gap
    assert np.array_equal(g["n_inliers"][ad], v["counts"][ad])


def test_legal_degenerates():
    pr = ref.fixture("n150")
    n = pr["n"]
    quads = np.array([[3, 3, 7, 9], [5, 5, 5, 5], [1, 2, 1, 2], [0, 1, 2, 3]], np.int32)
    g = api.PnPsolver.ransac(dict(pr, quads=quads))
    check_own_bits(pr, g)
    assert np.all((g["n_inliers"] >= 0) & (g["n_inliers"] <= n))
    flat = synth.synth_pnp(90, 0.1, 50, 0.5)
    flat["p3d"] = flat["p3d"].copy()
    flat["p3d"][:, 2] = 1.5                                                   # a planar scene
    rand_int, _ = ref.scripted_rand(550)
    g = api.PnPsolver.ransac(dict(flat, quads=ref.sample_quads(90, 6, rand_int)))
    check_own_bits(flat, g)
    assert np.all((g["n_inliers"] >= 0) & (g["n_inliers"] <= 90))
    r = api.PnPsolver.refine([dict(flat, subset=np.ones(90, bool)), dict(pr, subset=np.arange(n) < 4), dict(pr, subset=np.arange(n) < 5)])
    for x, m in zip(r, (90, n, n)):
        assert 0 <= x["n_inliers"] <= m
    # a subset of four takes the four-point path: the hypothesis on the same four points, bit for bit
    h = api.PnPsolver.ransac(dict(pr, quads=np.array([[0, 1, 2, 3]], np.int32)))
    assert np.array_equal(h["inlier_bits"][0], r[1]["inlier_bits"]) and h["n_inliers"][0] == r[1]["n_inliers"]
    ok, gap = ref.within(r[1]["pose"], h["pose"][0], 1e-12)                   # the sums over four points in another order
    assert ok or not np.isfinite(h["pose"]).all(), gap


def test_empty_problems_write_nothing():
    L = api.lib()
    pr = ref.fixture("n12")
    p3d, p2d, err = (np.ascontiguousarray(pr[k], np.float32) for k in ("p3d", "p2d", "max_err"))
    quads = np.zeros((3, 4), np.int32)
    for n, nh in ((0, 3), (12, 0)):
        P, R = (api.PnpProblem * 1)(), (api.PnpResult * 1)()
        pose, cnt, bits = np.full((3, 12), 7.0), np.full(3, 7, np.int32), np.full((3, 1), 7, np.uint32)
        P[0].n, P[0].n_hyp, P[0].p3d, P[0].p2d, P[0].max_err, P[0].quads = n, nh, p3d.ctypes.data, p2d.ctypes.data, err.ctypes.data, quads.ctypes.data
        P[0].intr = (C.c_double * 4)(*pr["intr"])
        R[0].pose, R[0].n_inliers, R[0].inlier_bits = pose.ctypes.data, cnt.ctypes.data, bits.ctypes.data
        assert L.slamit_pnp_ransac_batch(0, 1, P, R) == 0
        assert (pose == 7.0).all() and (cnt == 7).all() and (bits == 7).all()
    assert L.slamit_pnp_ransac_batch(0, 0, None, None) == 0 and L.slamit_pnp_refine_batch(0, 0, None, None) == 0
    P, R = (api.PnpRefineProblem * 1)(), (api.PnpRefineResult * 1)()
    R[0].n_inliers = 7
    assert L.slamit_pnp_refine_batch(0, 1, P, R) == 0 and R[0].n_inliers == 7   # n == 0


def test_errors_come_before_any_launch():
    pr = ref.fixture("n40")
    with pytest.raises(api.SlamitError, match=r"outside \[0, n\)"):
        api.PnPsolver.ransac(dict(pr, quads=np.array([[0, 1, 2, 40]], np.int32)))
    with pytest.raises(api.SlamitError, match=r"outside \[0, n\)"):
        api.PnPsolver.ransac(dict(pr, quads=np.array([[0, -1, 2, 3]], np.int32)))
    with pytest.raises(api.SlamitError, match="SLAMIT_PNP_MAX_HYP"):
        api.PnPsolver.ransac(dict(pr, quads=np.zeros((api.PNP_MAX_HYP + 1, 4), np.int32)))
    big = api.PNP_MAX_N + 1
    over = dict(p3d=np.ones((big, 3), np.float32), p2d=np.ones((big, 2), np.float32), max_err=np.ones(big, np.float32), intr=pr["intr"])
    with pytest.raises(api.SlamitError, match="SLAMIT_PNP_MAX_N"):
        api.PnPsolver.ransac(dict(over, quads=np.zeros((1, 4), np.int32)))
    with pytest.raises(api.SlamitError, match="SLAMIT_PNP_MAX_N"):
        api.PnPsolver.refine(dict(over, subset=np.ones(big, bool)))
    with pytest.raises(api.SlamitError, match="fewer than four"):
        api.PnPsolver.refine(dict(pr, subset=np.arange(40) < 3))
    with pytest.raises(api.SlamitError, match="minSet"):
        api.PnPsolver(pr).SetRansacParameters(0.99, 10, 300, 5, 0.5, 5.991)


@pytest.mark.parametrize("which", ["ceiling_n", "ceiling_hyp"])
def test_at_the_ceilings(which):
    v = ref.variants_on((which,))
    pr = v["pr"]
    assert (len(pr["max_err"]), len(v["quads"])) == ((api.PNP_MAX_N, 1) if which == "ceiling_n" else (16, api.PNP_MAX_HYP))
    g = api.PnPsolver.ransac(dict(pr, quads=v["quads"]))
    check_own_bits(pr, g)
    ad = v["admitted"][v["unique"]]
    assert ad.any()
    ok, gap = ref.within(g["pose"][ad], v["pose"][v["unique"]][ad])
    assert ok, gap
    assert np.array_equal(g["n_inliers"][ad], v["counts"][v["unique"]][ad])
    if which == "ceiling_n":
        sub = v["flags"][0] if v["counts"][0] >= 6 else np.ones(api.PNP_MAX_N, bool)
        r = api.PnPsolver.refine(dict(pr, subset=sub))
        pose, count, flags = ref.refine(pr, sub, "A")
        ok, gap = ref.within(r["pose"], pose)
        assert ok, gap
        own, _ = ref.check_inliers(r["pose"], pr["p3d"], pr["p2d"], pr["max_err"], pr["intr"])
        assert np.array_equal(r["inlier_bits"], ref.pack_bits(own[0]))
