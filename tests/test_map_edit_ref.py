"""csrc/map_edit.h, built with g++, against the literal sequential restatement (tests/map_edit_ref.py) on every fixture, and the
fixtures against what they claim to contain (no GPU).  Every comparison is exact."""
import collections

import numpy as np

from tests.map_edit_fixtures import SCAN_BLOCK, all_fixtures, by_name, expected
from tests.map_edit_host import assert_same, default_cap, host_run, laid_out
from tests.map_edit_ref import ADD_OBS, EDIT_OVERFLOW, ERASE_OBS, MATCH, MAX_OBS, MAX_PER_POINT, OBS_OVERFLOW, REF_END, SET_BAD, TABLE_OVERFLOW, apply


def test_the_header_equals_the_restatement_on_every_fixture():
    fxs = all_fixtures()
    jobs = [(fx, default_cap(fx)) for fx in fxs]
    for (fx, cap), got in zip(jobs, host_run(jobs)):
        assert_same(got, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_the_table_capacity_is_all_or_nothing():
    """At the need the table is written; one below it nothing is, and n_obs_out says what is needed."""
    fxs = [fx for fx in all_fixtures() if expected(fx["name"])["n_obs_out"] > 0 and fx["t"]["n_mp"] < 1000]
    jobs = [(fx, expected(fx["name"])["n_obs_out"] + d) for fx in fxs for d in (0, -1)]
    for (fx, cap), got in zip(jobs, host_run(jobs)):
        want = expected(fx["name"], cap - expected(fx["name"])["n_obs_out"])
        assert bool(want["status"] & TABLE_OVERFLOW) == (cap < want["n_obs_out"])
        assert_same(got, laid_out(fx, want, cap), "%s cap %d" % (fx["name"], cap))


def test_the_fixtures_hold_what_they_claim():
    ev = collections.Counter(e for fx in all_fixtures() for e in expected(fx["name"])["events"])
    single = collections.Counter(expected("single")["events"])
    # single-point behaviour, all of it in the hand-written list
    for name in ("add_present", "erase_absent", "erase_ref_remaining", "erase_ref_end", "cascade_3_2", "erase_leaves_3", "cascade_4_2", "set_bad_on_bad", "add_on_bad"):
        assert single[name] >= 1, name
    fx, want = by_name("single"), expected("single")
    t, x, E = fx["t"], fx["x"], fx["edits"]
    assert want["status_mp"][3] == REF_END and want["mp_ref_kf"][3] == -1 and want["mp_ref_kf"][2] == 2 and want["mp_ref_kf"][15] == 1
    assert x["obs_weight"][t["obs_ptr"][5]] == 2 and x["mp_nobs"][5] == 4 and want["mp_bad"][5] == 1              # the stereo cascade
    assert [e[0] for e in E if e[2] == 7] == [ADD_OBS, ERASE_OBS, ADD_OBS] and len({e[3] for e in E if e[2] == 7}) == 1   # add -> erase -> add
    row7 = want["obs_kf"][want["obs_ptr"][7]:want["obs_ptr"][8]].tolist()
    assert row7 == [0, 1, 2, 3, 5] and want["obs_idx"][want["obs_ptr"][8] - 1] == [e for e in E if e[2] == 7][-1][4]
    kinds8 = [(i, e[0]) for i, e in enumerate(E) if e[2] == 8]
    assert [k for _, k in kinds8] == [SET_BAD, ADD_OBS] and want["mp_bad"][8] == 1 and want["obs_ptr"][9] - want["obs_ptr"][8] == 1   # the add onto a bad point took
    # cross-point order on kf_mp: the later write of two points onto one (kf, idx) stands
    at = lambda k, i: int(t["kf_mp_ptr"][k]) + i
    pos = lambda pred: next(i for i, e in enumerate(E) if pred(e))
    i9 = E[pos(lambda e: e[2] == 10 and e[0] == ADD_OBS)][4]
    assert pos(lambda e: e[2] == 9 and e[0] == ERASE_OBS and e[1] & MATCH) < pos(lambda e: e[2] == 10 and e[0] == ADD_OBS and e[1] & MATCH)
    assert t["kf_mp"][at(3, i9)] == 9 and want["kf_mp"][at(3, i9)] == 10                                          # erase, then add
    i11 = E[pos(lambda e: e[2] == 12 and e[0] == ADD_OBS)][4]
    assert pos(lambda e: e[2] == 12 and e[0] == ADD_OBS and e[1] & MATCH) < pos(lambda e: e[2] == 11 and e[0] == ERASE_OBS and e[1] & MATCH)
    assert t["kf_mp"][at(4, i11)] == 11 and want["kf_mp"][at(4, i11)] == -1                                       # add, then erase
    i13 = E[pos(lambda e: e[2] == 14 and e[0] == ADD_OBS)][4]
    assert pos(lambda e: e[2] == 13 and e[0] == ERASE_OBS and e[3] == 5) < pos(lambda e: e[2] == 14 and e[0] == ADD_OBS and e[1] & MATCH)
    assert t["kf_mp"][at(7, i13)] == 13 and want["kf_mp"][at(7, i13)] == 14 and want["mp_bad"][13] == 1            # the cascade's write, then the add
    # limits
    fx, want = by_name("limits"), expected("limits")
    t, E = fx["t"], fx["edits"]
    rows = np.diff(t["obs_ptr"]).tolist()
    assert rows[:10] == [0, 1, 63, 64, 65, 511, 512, 512, 513, 513] and MAX_OBS == 512
    assert np.diff(want["obs_ptr"]).tolist()[:10] == [1, 0, 64, 65, 64, 512, 512, 512, 513, 513]
    assert want["status_mp"][6] == OBS_OVERFLOW and want["status_mp"][7] == 0 and want["status_mp"][8] == OBS_OVERFLOW and want["status_mp"][9] == 0
    add6 = next(e for e in E if e[2] == 6 and e[0] == ADD_OBS)
    assert add6[1] & MATCH and want["kf_mp"][int(t["kf_mp_ptr"][add6[3]]) + add6[4]] == -1                        # an overflowing point writes nothing
    per_point = collections.Counter(e[2] for e in E)
    assert (per_point[10], per_point[11], per_point[12]) == (1, MAX_PER_POINT, MAX_PER_POINT + 1)
    assert want["status_mp"][11] == 0 and want["status_mp"][12] == EDIT_OVERFLOW and want["obs_ptr"][12] - want["obs_ptr"][11] == 40
    sl = slice(int(t["kf_mp_ptr"][200]), int(t["kf_mp_ptr"][265]))                                               # the keyframes point 12's adds name
    assert np.array_equal(want["kf_mp"][sl], t["kf_mp"][sl]) and any(e[2] == 12 and e[1] & MATCH for e in E)      # nor does one with too many edits
    # list and map shapes
    nothing, empty = by_name("nothing"), by_name("empty")
    for fx in (nothing, empty):
        want = expected(fx["name"])
        assert want["n_touched"] == 0 and np.array_equal(want["obs_kf"], fx["t"]["obs_kf"]) and np.array_equal(want["kf_mp"], fx["t"]["kf_mp"])
    assert len(nothing["edits"]) > 40 and len(empty["edits"]) == 0
    sizes = sorted(fx["t"]["n_mp"] for fx in all_fixtures() if fx["name"].startswith("scan"))
    assert sizes == [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_BLOCK * SCAN_BLOCK + 1]
    for fx in all_fixtures():
        if fx["name"] in ("single", "limits", "shuffled") or fx["name"].startswith("scan"):
            pts = [e[2] for e in fx["edits"]]
            assert pts != sorted(pts), fx["name"]                                                                 # list order is not point order
            again = [p for i, p in enumerate(pts) if p in pts[:i] and pts[i - 1] != p]
            assert again, fx["name"]                                                                              # a point comes back after others
    for name in ("erase_ref_remaining", "add_present", "erase_absent"):
        assert ev[name] > single[name]                                                                            # the random lists reach them too


def test_the_restatement_is_sequential():
    """The same list in another order gives another map: what is compared against is order-sensitive."""
    fx = by_name("single")
    a, b = expected("single"), apply(fx["t"], fx["x"], fx["edits"][::-1])
    assert not np.array_equal(a["kf_mp"], b["kf_mp"])
