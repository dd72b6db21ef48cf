"""csrc/map_fuse.h on the host (g++, no GPU) against the literal sequential restatement (tests/map_fuse_ref.py) on every fixture, exact,
every prefix of three lists included; that the fixtures hold what they claim; the capacity at the need and one below it; the header
under the address and undefined-behaviour sanitizers behind a stand-alone main."""
import numpy as np

from tests.map_fuse_fixtures import all_fixtures, by_name, expected
from tests.map_fuse_host import assert_same, default_cap, host_run, laid_out
from tests.map_fuse_ref import ADD_OBS, ADDED, FUSE, OBS_OVERFLOW, OUT_NAMES, P_REPLACED, Q_REPLACED, TABLE_OVERFLOW, apply

CAPPED = ("outcomes", "mixed", "neighbours", "ops65", "ops1025")   # obs_cap_out at the need and one below
PREFIXES = ("flipped", "mixed", "neighbours")


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
    """From the reference walk: every fixture reaches the outcome, the event and the status it is named for."""
    seen = set()
    for fx in all_fixtures():
        w = expected(fx["name"])
        assert w["status"] == fx["status"], fx["name"]
        for i, o in fx["claims"].items():
            assert w["outcome"][i] == o, (fx["name"], i, OUT_NAMES[w["outcome"][i]], OUT_NAMES[o])
        for e in fx["events"]:
            assert e in w["events"], (fx["name"], e)
        seen.update(w.get("outcome", np.zeros(0, np.int32)).tolist())
        for i, o in fx.get("alone", {}).items():                         # the op on the untouched map goes the other way
            assert apply(fx["t"], fx["x"], [fx["ops"][i]])["outcome"][0] == o, (fx["name"], i)
        if fx["claims"]:
            assert fx["t"]["n_kf"] <= 8 and fx["t"]["n_mp"] <= 14 or fx["name"] in ("chain", "row512_add", "row512_rep"), fx["name"]
    assert seen == set(range(8))
    assert {len(fx["ops"]) for fx in all_fixtures()} >= {0, 1, 63, 64, 65, 1025} and {fx["t"]["n_mp"] for fx in all_fixtures()} >= {255, 256, 257}
    for n in (63, 64, 65, 1025):
        ops = by_name("ops%d" % n)["ops"]
        assert sum(1 for op in ops if op[0] == FUSE and op[3] < 0) > n // 8   # -1 ops sprinkled in
    ch, w = by_name("chain"), expected("chain")
    i0, at, rec = ch["ops"][0][3], int(ch["t"]["kf_mp_ptr"][0]) + ch["ops"][0][3], 0
    assert len(ch["ops"]) == 300 and all(op[2] == 0 and op[3] == i0 for op in ch["ops"]) and ch["t"]["kf_mp"][at] == 0
    for j, op in enumerate(ch["ops"]):                                       # every op's occupant is the receiver of the op before
        assert w["outcome"][j] == (P_REPLACED if j % 2 else Q_REPLACED)
        if j % 2:
            assert w["mp_replaced"][op[1]] == rec                            # the newcomer went into the occupant
        else:
            assert w["mp_replaced"][rec] == op[1]                            # the occupant gave way: the keypoint was rewritten
            rec = op[1]
    assert w["kf_mp"][at] == rec == 299 and len(set(w["mp_replaced"][w["mp_replaced"] >= 0].tolist())) == 150
    assert expected("row512_add")["obs_ptr"][1] == 512 and expected("row512_rep")["obs_ptr"][2] - expected("row512_rep")["obs_ptr"][1] == 512
    nb = by_name("neighbours")
    assert len(nb["bases"]) == 4 and [nb["ops"][b][2] for b in nb["bases"]] == [1, 2, 3, 0] and len(nb["ops"]) > nb["bases"][-1] > nb["bases"][1] > 0
    assert {op[0] for op in by_name("mixed")["ops"]} == {1, 2, 3}
    sh = by_name("shared")                                                  # two points on one (k, idx)
    i = sh["ops"][0][3]
    assert sum(1 for p in (0, 1) for o in range(sh["t"]["obs_ptr"][p], sh["t"]["obs_ptr"][p + 1]) if sh["t"]["obs_kf"][o] == 4 and sh["x"]["obs_idx"][o] == i) == 2


def test_the_header_equals_the_restatement_on_every_fixture():
    jobs = jobs_of_all()
    outs = host_run(jobs)
    for (fx, cap), got in zip(jobs, outs):
        assert_same(got, laid_out(fx, want_of(fx, cap), cap), "%s cap %d" % (fx["name"], cap))


def test_every_prefix_of_three_lists():
    """The state after k ops is the sequential walk's, and outcome / moved / erased of op k are what it did there."""
    jobs, wants = [], []
    for name in PREFIXES:
        fx = by_name(name)
        for k in range(len(fx["ops"]) + 1):
            pre = dict(fx, ops=fx["ops"][:k])
            jobs.append((pre, default_cap(pre)))
            wants.append(apply(fx["t"], fx["x"], pre["ops"]))
            if k:
                full = expected(name)
                assert all(wants[-1][key][k - 1] == full[key][k - 1] for key in ("outcome", "moved", "erased"))
    for (pre, cap), got, want in zip(jobs, host_run(jobs), wants):
        assert_same(got, laid_out(pre, want, cap), "%s[:%d]" % (pre["name"], len(pre["ops"])))


def test_capacity_at_the_need_and_one_below():
    for name in CAPPED:
        need = expected(name)["n_obs_out"]
        assert not expected(name, 0)["status"] & TABLE_OVERFLOW and expected(name, -1)["status"] & TABLE_OVERFLOW and expected(name, -1)["n_obs_out"] == need


def test_the_old_table_plus_the_adds_and_fuses_always_suffices():
    """An observation is created by ADD_OBS and by a FUSE that adds, by nothing else."""
    for fx in all_fixtures():
        w = expected(fx["name"])
        if w["status"] & OBS_OVERFLOW:
            continue
        old = int(fx["t"]["obs_ptr"][-1])
        assert w["n_obs_out"] <= default_cap(fx) == old + sum(1 for op in fx["ops"] if op[0] in (ADD_OBS, FUSE)) and not w["status"] & TABLE_OVERFLOW
        assert w["n_obs_out"] <= old + int(np.sum(w["outcome"] == ADDED)) + sum(1 for op in fx["ops"] if op[0] == ADD_OBS)
        assert w["n_fused"] == int(np.sum(w["outcome"] >= ADDED))


def test_the_header_is_clean_under_the_sanitizers():
    jobs = jobs_of_all()
    outs = host_run(jobs, sanitize=True)
    for (fx, cap), got in zip(jobs, outs):
        assert_same(got, laid_out(fx, want_of(fx, cap), cap), fx["name"])
