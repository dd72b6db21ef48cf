"""UpdateLocalMap without a GPU: the restatement (tests/local_map_ref.py) on the fixtures, with the lists of the odd places written
out by hand; and csrc/local_map.h, built with g++, against the restatement on every fixture."""
import numpy as np
import pytest

from tests.local_map_fixtures import NAMES, fixture
from tests.local_map_host import OUTPUTS, assert_same, expected, host_run

FRAMES = [(name, i) for name in NAMES for i in range(len(fixture(name)["frames"]))]


def lists(name, i=0):
    r = expected(name, i)["lists"]
    return list(r["local_kf"]), r["ref_kf"], list(r["local_mp"]), list(r["skip"])


def test_plain_case_is_a_real_local_map():
    r = expected("plain")["lists"]
    assert (r["votes"] > 0).sum() >= 5 and r["n_local_kf"] > (r["votes"] > 0).sum() - 3 and r["n_local_mp"] > 100
    assert (r["frame_mp"] == -1).sum() > (fixture("plain")["frames"][0]["frame_mp"] == -1).sum()     # a bad point was thrown out
    assert 0 < r["skip"].sum() < r["n_local_mp"] and len(set(r["local_mp"])) == r["n_local_mp"]
    assert r["votes"][r["ref_kf"]] == r["votes"][[k for k in range(12) if not fixture("plain")["maps"][0]["kf_bad"][k]]].max()


def test_no_observer_leaves_the_lists():
    kf, ref, mp, skip = lists("no_observer")
    assert (kf, ref) == ([3, 1], 1) and not expected("no_observer")["votes"].any()
    assert mp == [6, 7, 2, 3, 4] and skip == [0] * 5


def test_all_voted_bad_empties_the_list_and_keeps_the_reference():
    kf, ref, mp, skip = lists("all_voted_bad")
    assert list(expected("all_voted_bad")["votes"]) == [2, 2, 0]
    assert (kf, ref, mp, skip) == ([], 2, [], [])
    assert list(expected("all_voted_bad")["local_kf"][:1]) == [2]          # the array keeps what it held: only the count says empty


def test_tie_goes_to_the_lowest_slot():
    kf, ref, mp, skip = lists("tie")
    assert list(expected("tie")["votes"]) == [1, 2, 0, 2]
    assert (kf, ref, mp, skip) == ([0, 1, 3], 1, [0, 1, 2, 3, 4], [1] * 5)


def test_over_80_voted_are_all_kept_without_expansion():
    kf, ref, mp, _ = lists("over_80_voted")
    assert kf == list(range(90)) and ref == 0
    assert mp == [0] + list(range(1, 91))


def test_exactly_80_voted_expand_once():
    kf, ref, _, _ = lists("exactly_80_voted")
    assert kf == list(range(80)) + [80, 81] and ref == 0                   # 82, keyframe 1's neighbour, is never reached


def test_unmarked_parent_ends_the_walk():
    kf, ref, mp, skip = lists("parent_ends_walk")
    assert (kf, ref) == ([1, 2, 3, 0], 1)                                   # 4, keyframe 2's neighbour, is not added
    assert mp == [0, 1, 2, 3, 9] and skip == [1, 0, 0, 0, 0]


def test_bad_parent_is_pushed_untested():
    kf, ref, mp, skip = lists("bad_parent_pushed")
    assert (kf, ref) == ([1, 3, 0], 1)
    assert mp == [0, 1, 8, 5, 6] and skip == [1, 1, 0, 0, 0]


def test_shared_point_appears_once_at_its_first_position():
    kf, ref, mp, skip = lists("shared_by_five")
    assert (kf, ref) == ([0, 1, 2, 3, 4], 0)
    assert mp == [0, 7, 1, 2, 3, 5, 4] and skip == [1, 0, 1, 1, 0, 1, 1]


def test_skip_flags():
    assert lists("skip_own_point")[2:] == ([0, 1, 2, 3], [1, 0, 1, 0])
    assert lists("skip_frame_seen")[2:] == ([0, 1, 2, 3], [0, 0, 1, 1])


def test_overflow_and_sizes_of_the_large_fixtures():
    e = expected("q_cap_overflow")
    assert e["n_local_mp"] > 64 and e["status"] == 4 and e["m"] == 64 and np.array_equal(e["local_mp"], e["lists"]["local_mp"][:64])
    t = fixture("long_keyframe")["maps"][0]
    assert t["n_kf"] == 300 and np.diff(t["kf_mp_ptr"]).max() == 2000 and 150 in expected("long_keyframe")["lists"]["local_kf"]
    assert fixture("hbm_histogram")["maps"][0]["n_kf"] > 4096 and expected("hbm_histogram")["status"] == 0
    assert 80 < expected("hbm_histogram")["n_local_kf"] <= 512
    fx = fixture("three_frames_two_maps")
    assert [f["map"] for f in fx["frames"]] == [0, 1, 0] and all(expected("three_frames_two_maps", i)["n_local_mp"] > 50 for i in range(3))


def test_the_ceiling_fixture_sits_at_every_ceiling():
    fx, e = fixture("ceilings"), expected("ceilings")
    t = fx["maps"][0]
    assert t["n_kf"] == fx["kf_cap"] == 65535 and len(fx["frames"][0]["frame_mp"]) == 30000 and np.diff(t["kf_mp_ptr"]).max() == 65536
    assert e["n_local_kf"] == 65535 and np.array_equal(e["local_kf"], np.arange(65535)) and e["ref_kf"] == 0 and e["votes"].min() == 1 == e["votes"].max()
    assert e["n_local_mp"] == fx["q_cap"] == 65536 and e["status"] == 0
    assert list(e["local_mp"][:3]) == [0, 65535, 1] and e["local_mp"][-1] == 65534 and list(e["skip"][:3]) == [1, 0, 0]


@pytest.mark.parametrize("name,i", FRAMES)
def test_the_header_on_the_host_equals_the_restatement(name, i):
    """csrc/local_map.h through g++: votes, the cleaned frame_mp, the keyframe list, its size, the reference keyframe, the points, their
    number, the skip bytes and the gathered planes, with everything past a count left as the caller filled it."""
    assert_same(host_run(name, i), expected(name, i), OUTPUTS, "%s[%d]" % (name, i))
