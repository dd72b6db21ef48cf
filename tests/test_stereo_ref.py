"""Frame::ComputeStereoMatches on the CPU: csrc/stereo.h, built with g++, against the numpy restatement of the reference's text
(tests/stereo_ref.py), bit for bit on u_right, depth, every integer and every status; and the admissibility of the fixtures the GPU
tests run (no GPU here)."""
import numpy as np
import pytest

from tests import stereo_ref as ref

MIXED_SEEDS = (0, 2, 4)
REACHABLE = {0, 1, 2, 3, 4, 6, 7, 8}   # every status an image can produce: tests/stereo_ref.py proves that 5 is not one


@pytest.mark.parametrize("seed", ref.EXTRACTOR_SEEDS)
def test_extractor_driven_fixture_is_admissible_and_the_header_equals_the_restatement(seed, oracle_built):
    fr = ref.extractor_frame(seed)
    assert fr["nlevels"] == 8 and fr["left"][0].shape == (240, 320) and 400 <= len(fr["kl"]) <= 524 and 400 <= len(fr["kr"]) <= 524
    r = ref.restate(fr)
    c = ref.status_counts(r)
    print("extractor fixture %d: %d left keypoints, statuses %s, median SAD %d" % (seed, len(fr["kl"]), c.tolist(), r["median"]))
    assert c[0] >= 0.3 * len(fr["kl"]), "a fixture with fewer matches tests little"
    assert c[7] >= 1, "the median filter must remove something"
    assert c[8] == 0, "the extractor's own keypoints never meet a departure"
    assert r["n_matched"] == c[0]
    matched = r["status"] == 0
    assert (r["u_right"][matched] >= 0).all() and (r["depth"][matched] > 0).all() and (r["u_right"][~matched] == -1).all() and (r["depth"][~matched] == -1).all()
    ref.assert_same(ref.host_frame(fr), r, "extractor %d" % seed)


def test_hand_made_fixtures_reach_every_status_an_image_can_produce():
    seen = set()
    for seed in MIXED_SEEDS:
        fr = ref.mixed(seed)
        assert [p.shape for p in fr["left"]] == [(64, 96), (53, 80), (44, 67)] and len(fr["kl"]) == 130
        r = ref.mixed_ref(seed)
        seen |= set(int(s) for s in r["status"])
        ref.assert_same(ref.host_frame(fr), r, "mixed %d" % seed)
    assert seen == REACHABLE


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_prefixes_of_a_hand_made_fixture(n):
    fr = ref.head(ref.mixed(2), n)
    ref.assert_same(ref.host_frame(fr), ref.restate(fr), "head %d" % n)


def test_status_5_and_the_nan_on_the_subpixel_step():
    """What no image reaches (tests/stereo_ref.py): deltaR outside [-1, 1] is status 5, +-inf included; a NaN deltaR passes that test
    and fails the disparity test, status 6."""
    flat = [5] * 11
    recs = [([9, 9, 9, 9, 3, 2, 1, 9, 9, 9, 9], 0, 1.0, 30.0, 40.0, 40.0, 40.0),      # d1 + d3 - 2 d2 = 0, d1 > d3: +inf
            ([9, 9, 9, 9, 1, 2, 3, 9, 9, 9, 9], 0, 1.0, 30.0, 40.0, 40.0, 40.0),      # -inf
            (flat, 0, 1.0, 30.0, 40.0, 40.0, 40.0),                                    # 0 / 0
            ([9, 9, 9, 9, 10, 5, 1, 9, 9, 9, 9], 0, 1.0, 30.0, 40.0, 40.0, 40.0),     # 9 / (2 * 1) = 4.5
            ([9, 9, 9, 9, 1, 5, 10, 9, 9, 9, 9], 0, 1.0, 30.0, 40.0, 40.0, 40.0),     # -4.5
            ([9, 9, 9, 9, 4, 5, 8, 9, 9, 9, 9], 0, 1.0, 30.0, 40.0, 40.0, 40.0),      # -4 / (2 * 2) = -1: inside
            ([9, 9, 9, 9, 7, 2, 3, 9, 9, 9, 9], 0, 1.2, 30.0, 40.0, 40.0, 40.0),      # an ordinary one
            ([9, 9, 9, 9, 7, 2, 3, 9, 9, 9, 9], 0, 1.0, 50.0, 40.0, 40.0, 40.0),      # negative disparity
            (flat, -5, 1.0, 30.0, 40.0, 40.0, 40.0), (flat, 5, 1.0, 30.0, 40.0, 40.0, 40.0), (flat, -4, 1.0, 30.0, 40.0, 40.0, 40.0)]
    want = [ref.subpixel(*r) for r in recs]
    assert [w[0] for w in want] == [5, 5, 6, 5, 5, 0, 0, 6, 4, 4, 6]
    got = ref.host_subpixel(recs)
    for g, w in zip(got, want):
        assert g[0] == w[0] and ref.bits(g[1]) == ref.bits(w[1]) and ref.bits(g[2]) == ref.bits(w[2]), (g, w)


CASES = ref.cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_hand_made_case(k):
    name, fr, expect = CASES[k]
    assert [p.shape for p in fr["left"]] == [(64, 96), (53, 80), (44, 67)]
    r = ref.restate(fr)
    for key, vals in expect.items():                       # the case exercises what its name says
        assert len(vals) == len(fr["kl"])
        for i, want in enumerate(vals):
            if want is None:
                continue
            if key in ("u_right", "depth"):
                assert ref.bits(r[key][i]) == ref.bits(want), (name, key, i, r[key][i], want)
            else:
                assert r[key][i] == want, (name, key, i, r[key][i], want)
    ref.assert_same(ref.host_frame(fr), r, name)


def test_the_case_list_names_every_property():
    names = {c[0] for c in CASES}
    assert {"tie", "th_high", "band_ends", "octave_gate", "gate_ends", "right_window", "edge_shifts", "flat", "disparity_zero", "disparity_at_maxd",
            "disparity_below_maxd", "sad_at_thdist", "one_entry_zero_sad", "empty_list", "no_left", "no_right", "right_bands"} <= names
    assert sum(n.startswith("dep_") for n in names) == 11
    m, T = ref._thdist_pair()
    assert np.float32(1.5) * np.float32(1.4) * np.float32(m) == np.float32(T) and T - 1 > m


def test_the_optimised_host_build_equals_the_test_build():
    """tools/bench_stereo.py times the -O3 build: the same bits."""
    fr = ref.mixed(4)
    ref.assert_same(ref.host_frame(fr, "-O3"), ref.mixed_ref(4), "-O3")
