"""UpdateConnections and KeyFrameCulling without a GPU: the restatement (tests/covis_ref.py) on the fixtures, with the expected lists
of the odd places written out by hand; csrc/covis.h, built with g++, against the restatement on every fixture; and the header's
`n > 0.9 * m` against Python's."""
import numpy as np
import pytest

from tests.covis_fixtures import CULL_NAMES, UC_NAMES, fixture
from tests.covis_host import CULL_OUTPUTS, PARENT_FILL, UC_OUTPUTS, assert_same, cull_expected, host_run, uc_expected, verdict_table


def row(e, key, j):
    n = e["cw_n" if key.startswith("cw") else "ord_n"][j]
    return list(zip(e[key + "_kf"][j][:n].tolist(), e[key + "_w"][j][:n].tolist()))


def unchanged(name, e, but=()):
    x = fixture("uc", name)["x"]
    for j in range(len(x["cw_n"])):
        if j not in but:
            for key in ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best"):
                assert np.array_equal(e[key][j], x[key][j]), (name, key, j)


def test_plain_case_lists_above_threshold_and_keeps_the_whole_counter():
    e = uc_expected("plain")
    c = e["counts"]
    assert (c >= 15).sum() >= 3 and ((c > 0) & (c < 15)).sum() >= 2 and c[6] == 0
    assert row(e, "cw", 6) == [(j, int(c[j])) for j in np.flatnonzero(c)]
    assert row(e, "ord", 6) == sorted([(j, int(c[j])) for j in np.flatnonzero(c >= 15)], key=lambda p: (-p[1], -p[0]))
    for j in np.flatnonzero(c >= 15):                                   # inserted into every listed neighbour, whose row is re-sorted whole
        assert (6, int(c[j])) in row(e, "cw", j) and sorted(row(e, "ord", j)) == sorted(row(e, "cw", j))
    unchanged("plain", e, but=[6] + list(np.flatnonzero(c >= 15)))     # the below-threshold ones do not hear of it


def test_no_observer_changes_nothing():
    e = uc_expected("no_observer")
    assert (e["status"], e["n_counted"], e["n_listed"], e["parent"]) == (1, 0, 0, PARENT_FILL) and not e["counts"].any()
    unchanged("no_observer", e)
    assert row(e, "cw", 2) == [(3, 9)]


def test_nobody_reaches_the_threshold_the_lowest_slot_of_the_maximum():
    e = uc_expected("tie_below")
    assert list(e["counts"]) == [0, 3, 0, 7, 7, 2] and row(e, "ord", 2) == [(3, 7)] and row(e, "cw", 2) == [(1, 3), (3, 7), (4, 7), (5, 2)]
    assert row(e, "cw", 3) == [(2, 7)] and row(e, "cw", 4) == [] and list(e["kf_best"][2]) == [3] + [-1] * 9


def test_fifteen_is_listed_fourteen_is_not():
    e = uc_expected("fifteen_fourteen")
    assert list(e["counts"]) == [0, 14, 0, 15, 14] and row(e, "ord", 0) == [(3, 15)] and row(e, "cw", 1) == [] and row(e, "cw", 3) == [(0, 15)]


def test_equal_weights_the_higher_slot_first():
    e = uc_expected("equal_weights")
    assert row(e, "ord", 3) == [(5, 25), (6, 20), (2, 20), (0, 20), (7, 16)] and list(e["kf_best"][3]) == [5, 6, 2, 0, 7, -1, -1, -1, -1, -1]
    assert row(e, "cw", 3) == [(0, 20), (1, 4), (2, 20), (5, 25), (6, 20), (7, 16)]


def test_a_bad_observer_counts_and_bad_or_null_points_do_not():
    e = uc_expected("bad_observer")
    assert fixture("uc", "bad_observer")["t"]["kf_bad"][2] == 1 and row(e, "ord", 1) == [(2, 18), (0, 16)] and row(e, "cw", 2) == [(1, 18)]
    e = uc_expected("skips")
    assert list(e["counts"]) == [15, 10, 0, 0, 0] and row(e, "ord", 2) == [(0, 15)]


def test_a_neighbour_that_holds_the_weight_is_left_alone():
    e = uc_expected("neighbour_holds_same")
    unchanged("neighbour_holds_same", e, but=[1, 2])
    assert row(e, "ord", 4) == [(0, 30), (1, 17), (5, 15)] and list(e["kf_best"][4][:4]) == [0, 1, 5, 2]   # still without (3, 4)
    assert row(e, "ord", 2) == [(1, 16)]


def test_a_neighbour_with_another_weight_is_resorted_from_its_whole_row():
    e = uc_expected("neighbour_other_weight")
    assert row(e, "cw", 4) == [(0, 30), (1, 17), (3, 4), (5, 17), (6, 2)]
    assert row(e, "ord", 4) == [(0, 30), (5, 17), (1, 17), (3, 4), (6, 2)] and list(e["kf_best"][4][:6]) == [0, 5, 1, 3, 6, -1]


def test_old_entries_of_k_are_dropped_and_the_bytes_behind_stay():
    e = uc_expected("old_entries_dropped")
    x = fixture("uc", "old_entries_dropped")["x"]
    assert x["cw_n"][5] == 5 and row(e, "cw", 5) == [(0, 16), (7, 3)] and row(e, "ord", 5) == [(0, 16)]
    assert np.array_equal(e["cw_kf"][5][2:], x["cw_kf"][5][2:]) and list(e["cw_kf"][5][2:5]) == [3, 4, 6]      # past the count: as they were
    assert row(e, "cw", 1) == [(5, 40)]                                 # the reference does not tell the dropped neighbours
    assert row(e, "cw", 7) == []


def test_parent_on_first_connection():
    assert uc_expected("first_origin")["parent"] == -1 and uc_expected("first_other")["parent"] == 4
    assert uc_expected("plain")["parent"] == -1                          # not a first connection


def test_row_overflows():
    e = uc_expected("k_row_overflow")
    assert (e["status"], e["n_counted"], e["n_listed"], e["parent"]) == (2, 17, 0, PARENT_FILL) and (e["counts"] > 0).sum() == 17
    unchanged("k_row_overflow", e)
    e = uc_expected("neighbour_row_overflow")
    assert e["status"] == 2 and row(e, "ord", 0) == [(4, 21), (3, 20)] and row(e, "cw", 4) == [(0, 21)]
    unchanged("neighbour_row_overflow", e, but=[0, 4])
    assert e["cw_n"][3] == 16 and 0 not in e["cw_kf"][3]


def test_the_large_fixtures_sit_where_they_should():
    assert fixture("uc", "lds_edge")["t"]["n_kf"] == 4096 and fixture("uc", "hbm_counts")["t"]["n_kf"] > 4096
    assert row(uc_expected("hbm_counts"), "ord", 7) == [(64, 33), (4099, 19), (4098, 15)] and uc_expected("hbm_counts")["parent"] == 64
    t = fixture("uc", "large")["t"]
    assert t["kf_mp_ptr"][22] - t["kf_mp_ptr"][21] == 2000 and 30 < uc_expected("large")["n_listed"] <= 39


def trace(name):
    return cull_expected(name)["trace"]


def test_culling_thresholds():
    assert trace("ninety_percent") == [(1, 10, 9, 0), (2, 10, 10, 1)]
    assert trace("three_observations") == [(1, 10, 9, 0)]
    assert trace("octaves") == [(1, 10, 10, 1), (2, 10, 0, 0)]
    assert trace("self_among_observers") == [(1, 10, 0, 0)]
    assert trace("depth_gate") == [(1, 9, 9, 1), (2, 10, 9, 0)]
    assert trace("no_points") == [(1, 0, 0, 0), (2, 3, 3, 1)]
    assert all(v == 0 for _, _, _, v in trace("no_cull") + trace("no_cull_stereo")) and len(trace("no_cull")) > 5


def test_culling_cascade():
    assert trace("cascade_keeps") == [(1, 15, 15, 1), (2, 10, 0, 0)]                       # alone, 2 would be 10 of 10
    e = cull_expected("cascade_culls")
    assert e["trace"] == [(1, 32, 30, 1), (2, 9, 9, 1), (3, 10, 9, 0)]                    # alone, 2 would be 9 of 11
    assert (e["mp_turned_bad"] == 1).sum() == 2
    e = cull_expected("stereo_weights")
    assert e["trace"] == [(1, 66, 61, 1), (2, 10, 9, 0)] and (e["mp_turned_bad"] == 1).sum() == 5
    assert trace("origin") == [(1, 0, 0, 3), (2, 10, 10, 1)]
    assert trace("not_erase") == [(1, 15, 15, 2), (2, 10, 10, 1)]                          # 1 stays an observer
    assert sum(v == 1 for _, _, _, v in trace("long_cascade")) >= 3 and any(v == 0 for _, _, _, v in trace("long_cascade"))


@pytest.mark.parametrize("name", UC_NAMES)
def test_update_connections_header_on_the_host_equals_the_restatement(name):
    assert_same(host_run("uc", name), uc_expected(name), UC_OUTPUTS, name)


@pytest.mark.parametrize("name", CULL_NAMES)
def test_keyframe_culling_header_on_the_host_equals_the_restatement(name):
    assert_same(host_run("cull", name), cull_expected(name), CULL_OUTPUTS, name)


def test_the_ninety_percent_compare_is_pythons():
    got = verdict_table()
    want = np.array([[int(n > 0.9 * m) for n in (m * 9 // 10, m * 9 // 10 + 1)] for m in range(1, 2001)], np.uint8)
    assert np.array_equal(got, want) and want[9].tolist() == [0, 1] and want[:, 1].all() and not want[:, 0].any()
