"""slamit_init_hyp_batch / slamit_init_reconstruct_batch on the device against tests/initializer_ref.py and the
g++-built csrc/two_view.h.

Own bits: score, count and inlier bits of EVERY hypothesis equal the restated CheckHomography / CheckFundamental evaluated on the
device's own matrix, bit for bit; any other summation order of the float score fails this.  Models of admitted hypotheses are held
to variant A within 4 x the host header's measured gap (ref.HOST_GAP, never above 1e-5 x max(1, |entry|)).  The motion pass equals
the g++-built header run on the device's own chosen matrix and mask, bit for bit.  Measured on an MI355X: the device's models,
motions and points equal the host build's bit for bit on every fixture, so the device gap to A is the host gap."""
import functools

import numpy as np
import pytest

from tests import initializer_ref as ref
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    """Float arrays equal bit for bit; a NaN equals a NaN (its payload is the hardware's choice)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def problem(name):
    pr = ref.fixture(name)
    return {k: pr[k] for k in ("keys1", "keys2", "matches", "sigma", "sets", "K")}


@functools.lru_cache(maxsize=None)
def dev_hyp(name):
    return api.init_hypotheses(problem(name))


def bound(a, what):
    return np.minimum(4 * ref.HOST_GAP[what], 1e-5) * np.maximum(1, np.abs(a))


def own_bits(pr, hyp):
    m12 = ref.m12_of(pr)
    n = len(m12)
    for kind in (ref.H, ref.F):
        for h in range(hyp["model"].shape[1]):
            score, inl = ref.check(kind, hyp["model"][kind, h], m12, pr["sigma"])
            assert same(hyp["score"][kind, h], score), (kind, h, hyp["score"][kind, h], score)
            assert np.array_equal(ref.unpack_bits(hyp["inlier_bits"][kind, h], n), inl), (kind, h)
            assert hyp["n_inliers"][kind, h] == int(inl.sum())
            assert not np.unpackbits(hyp["inlier_bits"][kind, h].view(np.uint8), bitorder="little")[n:].any()   # nothing past n


@pytest.mark.parametrize("name", ref.NAMES)
def test_scores_and_inlier_bits_are_the_restated_check_on_the_devices_own_matrix(name):
    own_bits(ref.fixture(name), dev_hyp(name))


@pytest.mark.parametrize("name", ref.NAMES)
def test_models_of_admitted_hypotheses_against_variant_a(name):
    dev, a, adm = dev_hyp(name)["model"], ref.initialize(name, "A")["models"], ref.admitted(name)
    assert adm.mean() >= 0.98
    gap = np.abs(dev.astype(np.float64) - a.astype(np.float64))
    print("%s: device model gap to A on admitted hypotheses %.3g" % (name, gap[adm].max()))
    assert np.all(gap[adm] <= bound(a, "model")[adm])
    host = ref.host_initialize(name)[0]
    assert same(dev, host["model"]) and same(dev_hyp(name)["score"], host["score"])


def motion_case(pr, kind, model, subset_bits):
    """Device and header on one chosen matrix and mask."""
    q = dict(pr, kind=kind, model=model, subset_bits=subset_bits)
    return api.init_reconstruct(q), ref.host_run(pr, 1, kind=kind, model=model, subset_bits=subset_bits)


def same_motion_pass(dev, host):
    nm = len(dev["n_good"])
    assert dev["decomposable"] == host["decomposable"]
    assert np.array_equal(dev["status"], host["status"][:nm]), np.argwhere(dev["status"] != host["status"][:nm])[:5]
    assert same(dev["points"], host["points"][:nm])
    assert np.array_equal(dev["n_good"], host["n_good"][:nm]) and np.array_equal(dev["good_bits"], host["good_bits"][:nm])
    assert same(dev["cos_sel"], host["cos_sel"][:nm])
    assert same(dev["R"], host["R"][:nm]) and same(dev["t"], host["t"][:nm])


@pytest.mark.parametrize("name", ref.NAMES)
def test_motion_pass_equals_the_header_on_the_devices_own_matrix_and_mask(name):
    pr, hyp = problem(name), dev_hyp(name)
    sel = api.init_select(hyp)
    for kind, b in ((ref.H, sel["best_h"]), (ref.F, sel["best_f"])):   # both models, whichever Initialize would choose
        if b < 0:
            continue
        dev, host = motion_case(pr, kind, hyp["model"][kind, b], hyp["inlier_bits"][kind, b])
        assert len(dev["n_good"]) == (8 if kind == ref.H else 4)
        same_motion_pass(dev, host)


def test_a_homography_with_equal_singular_values_is_reported_not_decomposable():
    pr = problem("n65")
    n = len(pr["matches"])
    sub = ref.pack_bits(np.ones(n, bool))
    dev, host = motion_case(pr, ref.H, np.eye(3, dtype=f32), sub)       # d1 / d2 = 1 < 1.00001: ReconstructH's early return
    same_motion_pass(dev, host)
    assert dev["decomposable"] == 0 and not dev["n_good"].any() and np.all(dev["status"] == ref.RT_NOT_INLIER)
    assert not dev["points"].any() and not dev["good_bits"].any() and not dev["R"].any()
    assert api.init_select({"score": np.zeros((2, 1), f32), "N": n}, dev)["motion"] == -1


@pytest.mark.parametrize("count", [50, 51, 52])
def test_parallax_index_at_exactly_50_51_52_accepted_cosines(count):
    c = ref.parallax_case(count)
    dev, host = motion_case(problem("general"), c["kind"], c["model"], ref.pack_bits(c["subset"]))
    same_motion_pass(dev, host)
    assert dev["n_good"][c["motion"]] == count
    acc = np.sort(dev_cosines(c, dev))
    assert bits(dev["cos_sel"][c["motion"]]) == bits(acc[min(50, count - 1)])


def dev_cosines(c, dev):
    """cosParallax of the matches the device accepted for the case's motion, recomputed from its own R, t and points."""
    mo = c["motion"]
    rt = ref.check_rt(dev["R"][mo], dev["t"][mo], ref.m12_of(ref.fixture("general")), c["subset"], 1.0)
    x = dev["points"][mo][dev["status"][mo] == 0]
    R, t = dev["R"][mo].reshape(3, 3), dev["t"][mo]
    O2 = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])
    n2 = x - O2
    d1 = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=1)).astype(f32)
    d2 = np.sqrt(np.sum(n2.astype(np.float64) ** 2, axis=1)).astype(f32)
    assert rt["n_good"] == len(x)
    return (np.sum(x.astype(np.float64) * n2.astype(np.float64), axis=1) / (d1 * d2).astype(np.float64)).astype(f32)


@pytest.mark.parametrize("name", ref.NAMES)
def test_initializer_end_to_end_against_variant_a(name):
    pr, a = ref.fixture(name), ref.initialize(name, "A")
    ini = api.Initializer(pr["keys1"], pr["K"], pr["sigma"], len(pr["sets"]))
    ok, R21, t21, vP3D, vbT = ini.Initialize(pr["keys2"], pr["vMatches12"], sets=pr["sets"])
    assert (ok, ini.last["kind"], ini.last["motion"]) == (a["ok"], a["kind"], a["motion"])
    assert pr["expect"][1] == ok and pr["expect"][0] in (None, ini.last["kind"])
    assert np.array_equal(vbT, a["vbTriangulated"])
    if ok:
        Ra, ta = a["R"][a["motion"]], a["t"][a["motion"]]
        assert np.all(np.abs(R21 - Ra) <= bound(Ra, "pose")) and np.all(np.abs(t21 - ta) <= bound(ta, "pose"))
        assert np.array_equal(np.any(vP3D != 0, axis=1), np.any(a["vP3D"] != 0, axis=1))
        assert np.all(np.abs(vP3D - a["vP3D"]) <= bound(a["vP3D"], "points"))
        assert vbT.sum() > 50
    else:
        assert not vbT.any() and not vP3D.any() and not R21.any()


def test_batch_equals_single_bit_for_bit():
    names = ("n63", "general", "eight", "n65", "planar")
    hyps = api.init_hypotheses([problem(n) for n in names])
    recos_in = []
    for n, hy in zip(names, hyps):
        one = dev_hyp(n)
        for k in ("model", "score"):
            assert same(hy[k], one[k]), (n, k)
        assert np.array_equal(hy["n_inliers"], one["n_inliers"]) and np.array_equal(hy["inlier_bits"], one["inlier_bits"])
        kind = ref.H if n == "planar" else ref.F
        b = int(np.argmax(hy["score"][kind]))
        recos_in.append(dict(problem(n), kind=kind, model=hy["model"][kind, b], subset_bits=hy["inlier_bits"][kind, b]))
    for q, rb in zip(recos_in, api.init_reconstruct(recos_in)):
        one = api.init_reconstruct(q)
        for k in ("status", "n_good", "good_bits"):
            assert np.array_equal(one[k], rb[k]), k
        for k in ("points", "cos_sel", "R", "t"):
            assert same(one[k], rb[k]), k
        assert one["decomposable"] == rb["decomposable"]


def test_empty_problems_write_nothing():
    L = api.lib()
    assert L.slamit_init_hyp_batch(0, 0, None, None) == 0 and L.slamit_init_reconstruct_batch(0, 0, None, None) == 0
    assert api.init_hypotheses([]) == [] and api.init_reconstruct([]) == []
    pr = problem("n63")
    P, R = (api.InitProblem * 2)(), (api.InitResult * 2)()
    keep = []
    outs = []
    for i, nh in enumerate((0, 3)):
        k1, k2 = np.ascontiguousarray(pr["keys1"], f32), np.ascontiguousarray(pr["keys2"], f32)
        m, s = np.ascontiguousarray(pr["matches"], np.int32), np.ascontiguousarray(pr["sets"][:nh], np.int32)
        P[i].n1, P[i].n2, P[i].n, P[i].n_hyp, P[i].sigma = len(k1), len(k2), len(m), nh, 1.0
        P[i].keys1, P[i].keys2, P[i].matches, P[i].sets = k1.ctypes.data, k2.ctypes.data, m.ctypes.data, s.ctypes.data
        o = [np.full((2, 3, 9), 7, f32), np.full((2, 3), 7, f32), np.full((2, 3), 7, np.int32), np.full((2, 3, 2), 7, np.uint32)]
        R[i].model, R[i].score, R[i].n_inliers, R[i].inlier_bits = (a.ctypes.data for a in o)
        keep.append((k1, k2, m, s))
        outs.append(o)
    assert L.slamit_init_hyp_batch(0, 2, P, R) == 0
    assert all(np.all(a == 7) for a in outs[0])                       # n_hyp == 0: untouched
    assert np.array_equal(bits(outs[1][1]), bits(dev_hyp("n63")["score"][:, :3]))


def test_argument_errors_launch_nothing():
    pr = problem("n63")
    with pytest.raises(api.SlamitError, match="fewer than eight") as e:
        api.init_hypotheses(dict(pr, matches=pr["matches"][:7], sets=np.arange(8).reshape(1, 8) % 7))
    assert "(-1)" in str(e.value)                                      # SLAMIT_ERR_ARG
    with pytest.raises(api.SlamitError, match="outside"):
        api.init_hypotheses(dict(pr, sets=np.array([[0, 1, 2, 3, 4, 5, 6, 63]])))
    with pytest.raises(api.SlamitError, match="repeats"):
        api.init_hypotheses(dict(pr, sets=np.array([[0, 1, 2, 3, 4, 5, 6, 3]])))
    bad = pr["matches"].copy()
    bad[5, 1] = len(pr["keys2"])
    with pytest.raises(api.SlamitError, match="match index"):
        api.init_hypotheses(dict(pr, matches=bad))
    with pytest.raises(api.SlamitError, match="SLAMIT_INIT_MAX_HYP"):
        api.init_hypotheses(dict(pr, sets=np.tile(np.arange(8), (api.INIT_MAX_HYP + 1, 1))))
    big = np.zeros((api.INIT_MAX_N + 1, 2), np.int32)
    with pytest.raises(api.SlamitError, match="SLAMIT_INIT_MAX_N"):
        api.init_hypotheses(dict(pr, matches=big))
    hy = dev_hyp("n63")
    q = dict(pr, kind=ref.F, model=hy["model"][1, 0], subset_bits=hy["inlier_bits"][1, 0])
    with pytest.raises(api.SlamitError, match="match index"):
        api.init_reconstruct(dict(q, matches=bad))
    with pytest.raises(api.SlamitError, match="kind"):
        api.init_reconstruct(dict(q, kind=2))
    with pytest.raises(api.SlamitError, match="SLAMIT_INIT_MAX_N"):
        api.init_reconstruct(dict(q, matches=big, subset_bits=np.zeros((len(big) + 31) // 32, np.uint32)))
    P, R = (api.InitProblem * 1)(), (api.InitResult * 1)()
    P[0].n, P[0].n_hyp, P[0].n1, P[0].n2 = 8, 1, 8, 8
    assert api.lib().slamit_init_hyp_batch(0, 1, P, R) == -1 and b"null array" in api.lib().slamit_last_error()


def ceiling_problem(n, n_hyp, seed):
    rs = np.random.RandomState(seed)
    base = ref.fixture("general")
    k1 = np.stack([rs.uniform(20, 620, n), rs.uniform(20, 460, n)], axis=1).astype(f32)
    k2 = (k1 + rs.normal(0, 3, (n, 2))).astype(f32)
    m = np.stack([np.arange(n), rs.permutation(n)], axis=1).astype(np.int32)
    k2 = k2[np.argsort(m[:, 1])]                                       # match i joins k1[i] to its displaced copy
    return {"keys1": k1, "keys2": k2, "matches": m, "sigma": 1.0, "sets": ref.sample_sets(rs, n, n_hyp), "K": base["K"]}


@pytest.mark.parametrize("n,n_hyp", [(api.INIT_MAX_N, 2), (16, api.INIT_MAX_HYP)])
def test_one_problem_at_each_ceiling(n, n_hyp):
    pr = ceiling_problem(n, n_hyp, 5)
    hyp = api.init_hypotheses(pr)
    if n_hyp > 8:
        hyp_few = {k: v[:, ::128] for k, v in hyp.items()}
        own_bits(pr, hyp_few)
    else:
        own_bits(pr, hyp)
    b = int(np.argmax(hyp["n_inliers"][0]))
    dev, host = motion_case(pr, ref.H, hyp["model"][0, b], hyp["inlier_bits"][0, b])
    same_motion_pass(dev, host)
    sub = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)                 # every match, and bits past n that must be ignored
    dev, host = motion_case(pr, ref.F, hyp["model"][1, 0], sub)
    same_motion_pass(dev, host)
