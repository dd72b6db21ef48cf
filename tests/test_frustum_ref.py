"""The checker of the device frustum test on the CPU (tests/frustum_ref.py): the committed fixtures are admissible by the reference's
restatement alone, and the text the kernel compiles (csrc/frustum.h), built with g++ for the host, equals variant "32" bit for bit.

Measured on the committed fixtures: 0 undecided points of 9,485; the two variants agree on every status; every code
0..7 occurs (in fixture 0 alone, and among its first 65 points); the header's own log is within 0.5 ulp of the double log on 100,006
floats (half between e^-80 and e^80, half in 0.5..2) and differs from numpy's float32 log, by 4 ulp at most, on 18 % of them."""
import numpy as np
import pytest

from tests import frustum_ref as ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixtures_are_admissible():
    """What keeps the GPU test honest, by the reference alone: no undecided point, the variants agree on every status, every status
    code occurs, both branches of viewCos > 0.998 occur among the points in view, th = 1, 3 and 5 are all used, no fixture is large."""
    seen, narrow, ths, total = set(), set(), set(), 0
    assert 8 <= len(ref.FIXTURES) <= 12
    for k, (seed, n, th) in enumerate(ref.FIXTURES):
        a = ref.admissibility(k)
        r32, r64 = a["r32"], a["r64"]
        print("fixture %d: n %d, th %g, undecided %d, codes %s" % (k, n, th, a["undecided"], np.bincount(r32["status"], minlength=8).tolist()))
        assert n <= 2048 and len(r32["status"]) == n
        assert a["undecided"] == 0, k
        assert np.array_equal(r32["status"], r64["status"]), k
        seen |= set(int(s) for s in r32["status"])
        narrow |= set(bool(b) for b in r32["cmp"]["narrow"][r32["status"] == 0])
        ths.add(float(th))
        total += n
    print("points: %d" % total)
    assert seen == set(range(8)), seen
    assert narrow == {True, False}
    assert ths == {1.0, 3.0, 5.0}
    mixed = ref.evaluate(ref.head(ref.fixture(ref.MIXED), 65), "32")["status"]
    assert set(int(s) for s in mixed) == set(range(8))           # the GPU test's wavefront-edge heads see every code from n = 65 on


@pytest.mark.parametrize("k", range(len(ref.FIXTURES)))
def test_the_header_on_the_host_equals_ref32(k):
    """The text the kernel compiles, run on the CPU: u, v, uR, viewCos, r equal variant "32" bit for bit on every point; status and level
    on every decided point (which is every point of a fixture)."""
    a, h = ref.admissibility(k), ref.host_fixture(k)
    r32, d = a["r32"], a["decided"]
    for f in ref.FLOATS:
        assert np.array_equal(bits(h[f]), bits(r32[f])), (k, f, np.flatnonzero(bits(h[f]) != bits(r32[f]))[:5])
    assert np.array_equal(h["status"][d], r32["status"][d]) and np.array_equal(h["level"][d], r32["level"][d])
    uvr, l0, l1, valid = ref.queries_of(r32)
    assert np.array_equal(bits(h["uvr"]), bits(uvr)) and np.array_equal(h["level_min"], l0) and np.array_equal(h["level_max"], l1)
    assert np.array_equal(h["valid"], valid)
    # level 7 is the departure: it keeps its projection, cosine and raw level, and is no query
    s7 = h["status"] == 7
    assert np.all((h["level"][s7] < 0) | (h["level"][s7] >= 8)) and not h["valid"][s7].any() and np.all(h["r"][s7] == 0)
    s0 = h["status"] == 0
    assert np.all((h["level"][s0] >= 0) & (h["level"][s0] < 8)) and np.all(h["r"][s0] > 0)


def test_the_boundary_fixture():
    """Ratios exactly on 1.2^k and distances exactly on the 0.8 and 1.2 gates: the last bit of a log decides, so only the set of
    levels {k, k + 1} and the set of statuses are asserted, for the header and for both variants."""
    pr, allowed = ref.boundary_fixture()
    a, h = ref.analyse(pr), ref.host_points(pr)
    for name, out in (("header", h), ("ref32", a["r32"]), ("ref64", a["r64"])):
        for i, (st, lv) in enumerate(allowed):
            assert int(out["status"][i]) in st, (name, i, int(out["status"][i]), st)
            if lv is not None and int(out["status"][i]) in (0, 7):
                assert int(out["level"][i]) in lv, (name, i, int(out["level"][i]), lv)
    assert not a["decided"][:10].all()                            # and the analysis knows that these are not decided
    assert [int(s) for s in h["status"][10:]] == [7, 5, int(h["status"][12]), 5]   # ON a gate passes it, one float beyond does not


HAND = {
    0: dict(P=(0.2, 0.1, 4.0), max_dist=8.0, min_dist=1.0),
    1: dict(P=(0.2, 0.1, 4.0), max_dist=8.0, min_dist=1.0, skip=1),
    2: dict(P=(0.2, 0.1, -4.0), max_dist=8.0, min_dist=1.0),
    3: dict(P=(10.0, 0.1, 4.0), max_dist=16.0, min_dist=1.0),
    4: dict(P=(0.2, -10.0, 4.0), max_dist=16.0, min_dist=1.0),
    5: dict(P=(0.0, 0.0, 4.0), max_dist=1.0, min_dist=0.2),                                  # 4 > 1.2 * 1
    6: dict(P=(0.0, 0.0, 4.0), Pn=(1, 0, 0), max_dist=8.0, min_dist=1.0),                    # seen at a right angle
    7: dict(P=(0.0, 0.0, 4.0), max_dist=4.0 * 1.2 ** 8.1, min_dist=4.0 * 1.2 ** 1.1),        # inside both gates, level 9
}


def test_one_hand_made_point_per_status_code():
    pr = ref.points_problem([HAND[c] for c in sorted(HAND)])
    a, h = ref.analyse(pr), ref.host_points(pr)
    assert a["decided"].all()
    assert h["status"].tolist() == sorted(HAND) == a["r32"]["status"].tolist() == a["r64"]["status"].tolist()
    assert h["level"][0] == 4 and h["level"][7] == 9                                         # ceil(log 2 / log 1.2) = ceil(3.8)
    assert abs(h["u"][0] - (517.3 * 0.05 + 318.6)) < 1e-3 and abs(h["v"][0] - (516.5 * 0.025 + 255.3)) < 1e-3
    assert abs(h["uR"][0] - (h["u"][0] - 38.6 / 4.0)) < 1e-3
    assert h["r"][0] == np.float32(2.5) * pr["scale_factors"][4]                              # viewCos = 4 / |P| = 0.9984 > 0.998: the narrow window
    assert np.all(h["u"][1:3] == 0) and np.all(h["viewCos"][1:6] == 0) and h["viewCos"][6] == 0 and h["viewCos"][7] == 1


def test_the_documented_corner_cases():
    """PcZ == +0: invz = +inf, u = +inf, code 3.  The camera centre itself with min_dist <= 0: u and v are NaN and pass the bounds,
    dist = 0 passes the gate, viewCos = 0 / 0 passes the angle, the ratio is +inf: code 7 with no level, before any conversion."""
    pr = ref.points_problem([dict(P=(1.0, 0.0, 0.0), max_dist=8.0, min_dist=1.0), dict(P=(0.0, 0.0, 0.0), max_dist=8.0, min_dist=0.0),
                             dict(P=(0.0, 0.0, 0.0), max_dist=8.0, min_dist=-1.0), dict(P=(0.0, 0.0, 4.0), max_dist=0.0, min_dist=0.0)])
    h, r32 = ref.host_points(pr), ref.evaluate(pr, "32")
    assert h["status"].tolist() == [3, 7, 7, 5] == r32["status"].tolist()
    assert np.isposinf(h["u"][0]) and np.isnan(h["u"][1]) and np.isnan(h["v"][1]) and np.isnan(h["viewCos"][1])
    assert h["level"][1] == ref.LEVEL_NONE == h["level"][2] == r32["level"][1]
    assert not h["valid"].any() and np.all(h["uvr"] == 0)


def test_the_headers_own_log():
    """fru_logf against the double log: correctly rounded to half an ulp and a hair; exact at 1; the same bits as numpy's float32 log
    on most floats and within 4 ulp of it on the rest (4 ulp of a log below 16 log 1.2 move q by less than 4 * 2^-24 * 16 = 4 * 2^-20), which
    is what the margin of `decided` covers."""
    rs = np.random.RandomState(5)
    x = np.concatenate([np.exp(rs.uniform(-80, 80, 50000)), rs.uniform(0.5, 2.0, 50000), [1.0, 2.0, 0.5, 1.2, 1e-45, 3.4e38]]).astype(np.float32)
    y = ref.host_log(x)
    want = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - want) / ulp
    print("fru_logf: max error %.6f ulp; differs from numpy's float32 log on %d of %d" % (err.max(), int((y != np.log(x)).sum()), len(x)))
    assert err.max() <= 0.5 + 1e-6
    assert y[100000] == 0.0 and y[100001] == np.float32(np.log(2.0))
    assert np.all(np.abs(y - np.log(x)) <= 4 * np.spacing(np.maximum(np.abs(y), np.abs(np.log(x)))))   # numpy's is a vector routine good to a few ulp
