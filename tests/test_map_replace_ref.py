"""csrc/map_replace.h on the host (g++, no GPU) against the literal sequential restatement (tests/map_replace_ref.py) on every fixture,
exact; that the fixtures hold what they claim; the all-or-nothing ceilings; the header under the address and undefined-behaviour
sanitizers behind a stand-alone main; mr_check_replaced_entry against three lines of numpy."""
import numpy as np
import pytest

from tests.map_replace_fixtures import all_fixtures, by_name, expected
from tests.map_replace_host import assert_same, default_cap, host_check_replaced, host_run, laid_out
from tests.map_replace_ref import OBS_OVERFLOW, OP_OVERFLOW, TABLE_OVERFLOW, check_replaced

NAMES = [fx["name"] for fx in all_fixtures()]
CAPPED = ("single", "chains", "add_order", "indep", "ops65")   # obs_cap_out at the need and one below


def jobs_of_all():
    jobs = [(fx, default_cap(fx) + 3) for fx in all_fixtures()]
    for name in CAPPED:
        need = expected(name)["n_obs_out"]
        jobs += [(by_name(name), need), (by_name(name), need - 1)]
    return jobs


def want_of(fx, cap):
    full = expected(fx["name"])
    if "n_obs_out" not in full:
        return full
    return expected(fx["name"], cap - full["n_obs_out"])


def test_the_fixtures_hold_what_they_claim():
    ev = lambda name: expected(name)["events"]
    assert {"replace_self", "replace_all_move", "replace_some_die", "replace_all_die", "replace_of_replaced", "replace_onto_bad", "replace_onto_empty",
            "replace_nothing"} <= set(ev("single"))
    w, fx = expected("single"), by_name("single")
    assert w["mp_found"][1] == -2 ** 31 + 4 and w["mp_found"][9] == 2 ** 31 - 1                       # both wraps
    assert w["mp_replaced"][5] == 7 and w["mp_found"][7] == fx["x"]["mp_found"][7] + fx["x"]["mp_found"][5]   # replaced twice: the counters again
    assert w["mp_found"][6] == fx["x"]["mp_found"][6] + fx["x"]["mp_found"][5] and w["mp_replaced"][14] == 15 and w["mp_replaced"][4] == -1
    assert w["obs_kf"][w["obs_ptr"][13]:w["obs_ptr"][14]].tolist() == [0, 1, 3, 7]                    # received in ascending slot
    assert w["mp_nobs"][13] == 1 + 4 and w["mp_bad"][12] == 1 and w["mp_nobs"][12] == fx["x"]["mp_nobs"][12]   # a stereo entry moved; S keeps nObs
    c, fc = expected("chains"), by_name("chains")
    f = fc["x"]["mp_found"]
    assert c["mp_found"][2] == f[0] + f[1] + f[2] and c["mp_found"][4] == f[3] + f[4] and c["mp_found"][5] == f[4] + f[5]   # the sums are carried along
    assert c["mp_replaced"][[0, 1, 3, 4, 6, 7]].tolist() == [1, 2, 4, 5, 7, 6] and np.diff(c["obs_ptr"])[[6, 7]].tolist() == [3, 0]   # the cycle ends in the bad 6
    assert c["mp_bad"][[6, 7]].tolist() == [1, 1]
    assert expected("deep")["n_touched"] == 300 and len(by_name("deep")["ops"]) == 300
    assert expected("fan20")["moved"].sum() == 39 and expected("fan20")["erased"].sum() == 1
    assert expected("fan64")["status"] == 0 and expected("fan65")["status"] == OP_OVERFLOW and len(by_name("fan65")["ops"]) == 65
    assert np.diff(expected("row512")["obs_ptr"]).max() == 512 and expected("row513")["status"] == OBS_OVERFLOW
    assert expected("row513_in")["status"] == OBS_OVERFLOW and np.diff(by_name("row513_in")["t"]["obs_ptr"]).max() == 513
    assert expected("row512_add")["status"] == OBS_OVERFLOW
    a = expected("add_order")
    assert a["moved"].tolist() == [1, 2, 1, 0, 0, 1] and a["erased"].tolist() == [0, 0, 1, 0, 0, 0] and "add_present" in a["events"]
    s, fs = expected("shared"), by_name("shared")
    at = lambda p: int(fs["t"]["kf_mp_ptr"][0] + fs["x"]["obs_idx"][fs["t"]["obs_ptr"][p]])
    assert at(0) == at(1) and at(4) == at(5) and s["kf_mp"][at(0)] == 3 and s["kf_mp"][at(4)] == -1   # the later write of the two stays
    assert [len(by_name(n)["ops"]) for n in ("ops0", "ops1", "ops63", "ops64", "ops65", "ops1025")] == [0, 1, 63, 64, 65, 1025]
    assert [by_name(n)["t"]["n_mp"] for n in ("ops1", "ops63", "ops64", "ops1025")] == [255, 256, 257, 65537]
    named = {}
    for op in by_name("indep")["ops"]:
        for p in (op[1], op[2]) if op[0] == 1 else (op[1],):
            named[p] = named.get(p, 0) + 1
    assert max(named.values()) == 1 and len(by_name("indep")["ops"]) == 400
    for name in ("ops63", "ops1025"):
        assert {"replace_of_replaced", "add_on_bad", "add_present", "replace_some_die"} <= set(ev(name))


@pytest.fixture(scope="module")
def host_results():
    jobs = jobs_of_all()
    return jobs, host_run(jobs)


@pytest.mark.parametrize("name", NAMES)
def test_the_host_statement_equals_the_restatement(host_results, name):
    jobs, outs = host_results
    seen = 0
    for (fx, cap), got in zip(jobs, outs):
        if fx["name"] == name:
            assert_same(got, laid_out(fx, want_of(fx, cap), cap), "%s cap %d" % (name, cap))
            seen += 1
    assert seen == (3 if name in CAPPED else 1)


def test_every_ceiling_is_all_or_nothing(host_results):
    jobs, outs = host_results
    seen = set()
    for (fx, cap), got in zip(jobs, outs):
        if got["status"] & (OP_OVERFLOW | OBS_OVERFLOW | TABLE_OVERFLOW):
            seen.add(got["status"])
            e = laid_out(fx, {"status": got["status"], "n_obs_out": got["n_obs_out"]}, cap)   # every array byte for byte as it was
            assert_same(got, e, fx["name"])
            assert np.array_equal(got["kf_mp"], fx["t"]["kf_mp"]) and np.array_equal(got["mp_replaced"], fx["x"]["mp_replaced"])
    assert seen == {OP_OVERFLOW, OBS_OVERFLOW, TABLE_OVERFLOW}


def test_the_host_statement_at_the_ceiling_of_ops():
    from tests.map_replace_fixtures import ceiling_fixtures
    from tests.map_replace_ref import MAX_OPS, apply

    jobs = [(fx, default_cap(fx)) for fx in ceiling_fixtures()]
    for (fx, cap), got in zip(jobs, host_run(jobs)):
        want = apply(fx["t"], fx["x"], fx["ops"])
        assert len(fx["ops"]) == MAX_OPS and want["status"] == 0
        assert_same(got, laid_out(fx, want, cap), fx["name"])


def test_replace_never_needs_more_than_the_adds():
    """obs_cap_out = the old table + the ADD_OBS ops always suffices: Replace moves or drops, it never creates."""
    for fx in all_fixtures():
        w = expected(fx["name"])
        if "n_obs_out" in w:
            assert w["n_obs_out"] <= default_cap(fx) and not w["status"] & TABLE_OVERFLOW


def test_the_header_is_clean_under_the_sanitizers():
    jobs = jobs_of_all()
    outs = host_run(jobs, sanitize=True)
    for (fx, cap), got in zip(jobs, outs):
        assert_same(got, laid_out(fx, want_of(fx, cap), cap), fx["name"])
    lst, st = host_check_replaced(5, [-1, 3, -1, -1, 0], [1, -1, 4, 9], sanitize=True)
    assert lst.tolist() == [3, -1, 0, 9] and st == 8


def test_check_replaced_is_three_lines_of_numpy():
    rng = np.random.default_rng(31)
    n_mp = 300
    rep = np.where(rng.random(n_mp) < 0.3, rng.integers(0, n_mp, n_mp), -1).astype(np.int32)
    rep[7], rep[rep[7] if rep[7] >= 0 else 0] = 9, 11                                       # a chain of two: ONE hop is followed
    rep[9] = 11
    frame = np.where(rng.random(1000) < 0.2, -1, rng.integers(0, n_mp, 1000)).astype(np.int32)
    frame[:3] = [7, 9, -1]
    got, st = host_check_replaced(n_mp, rep, frame)
    assert st == 0 and np.array_equal(got, check_replaced(rep, frame)) and got[0] == 9 and got[1] == 11 and np.any(got != frame)
    outside = frame.copy()
    outside[[5, 6]] = [n_mp, -2]
    got, st = host_check_replaced(n_mp, rep, outside)
    want = check_replaced(rep, np.where((outside < -1) | (outside >= n_mp), -1, outside))
    want[[5, 6]] = [n_mp, -2]                                                              # left alone, with the bit
    assert st == 8 and np.array_equal(got, want)
    got, st = host_check_replaced(0, [], [])
    assert st == 0 and len(got) == 0
