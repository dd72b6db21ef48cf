"""Map-point upkeep without a GPU: the fixtures hold what they claim; the restatement (tests/upkeep_ref.py) on them, with the odd places
written out by hand; csrc/upkeep.h, built with g++, against the restatement on every fixture and on random small maps, bit for bit."""
import numpy as np
import pytest

from tests.upkeep_fixtures import CULL_LENGTHS, CUR_ID, EMPTY_KF, FIRST_BAD_KF, MAX_DESC, MAX_OBS, N_LEVELS, cull_map, random_map, small_map, up_map
from tests.upkeep_host import (BAD_SLOT, CULL_OUTPUTS, DESC_OVERFLOW, NO_REF, OBS_OVERFLOW, OCTAVE, REF_NO_KP, REF_NOT_OBSERVER, UP_OUTPUTS, assert_same,
                               bits, cull_expected, host_run, up_expected, up_of)
from tests.upkeep_ref import DescriptorDistance, MapPoint, MapPointCulling, cv_norm, mat_div, mat_sub, objects


def obs_of(fx, name):
    t, p = fx["t"], fx["cases"][name]
    return t["obs_kf"][t["obs_ptr"][p]:t["obs_ptr"][p + 1]].tolist()


def test_the_fixtures_hold_what_they_claim():
    fx = up_map()
    t, x, cases = fx["t"], fx["x"], fx["cases"]
    assert [len(obs_of(fx, "n%d" % n)) for n in (1, 63, 64, 65, 128, 129)] == [1, 63, 64, 65, 128, 129] and len(obs_of(fx, "n2_descending")) == 2
    assert len(obs_of(fx, "ceiling")) == len(obs_of(fx, "ceiling_many_good")) == MAX_OBS and len(obs_of(fx, "above_ceiling")) == MAX_OBS + 1
    good = lambda name: sum(not t["kf_bad"][k] for k in obs_of(fx, name))
    assert good("n128") == MAX_DESC and good("n129") == MAX_DESC + 1 and 0 < good("ceiling") <= MAX_DESC < good("ceiling_many_good")
    assert obs_of(fx, "n2_descending") == [7, 3] and obs_of(fx, "n64") == list(range(63, -1, -1))                       # stored in descending slot
    for name in ("shuffled", "n65", "ceiling", "tie3"):                                                               # neither order
        o = obs_of(fx, name)
        assert o != sorted(o) and o != sorted(o)[::-1], name
    assert t["kf_bad"][250] and 250 in obs_of(fx, "bad_observer") and good("bad_observer") == 3 and good("all_observers_bad") == 0
    assert t["mp_bad"][cases["bad_point"]] and obs_of(fx, "no_observations") == [] and not t["kf_bad"][:FIRST_BAD_KF].any()
    assert x["mp_ref_kf"][cases["ref_not_observer"]] not in obs_of(fx, "ref_not_observer") and x["mp_ref_kf"][cases["ref_none"]] == -1
    assert x["mp_ref_kf"][cases["ref_without_keypoints"]] == EMPTY_KF and t["kf_mp_ptr"][EMPTY_KF + 1] == t["kf_mp_ptr"][EMPTY_KF]
    kfs, mps = objects(t, x)
    mp = mps[cases["octave_n_levels"]]
    assert mp.mpRefKF.octave[mp.mObservations[mp.mpRefKF]] == N_LEVELS == x["n_levels"]
    assert np.array_equal(x["obs_octave"], x["kf_octave"][t["kf_mp_ptr"][t["obs_kf"]] + x["obs_idx"]])                  # the two columns agree
    assert (t["kf_mp"][t["kf_mp_ptr"][:-2]] == -1).all()                                                              # keypoint 0 is nobody's observation
    # the ties really tie, on different bytes
    for name, n in (("n2_descending", 2), ("tie3", 3)):
        mp = mps[cases[name]]
        rows = [kf.mDescriptors[i] for kf, i in sorted(mp.mObservations.items(), key=lambda kv: kv[0].addr)]
        medians = [sorted(DescriptorDistance(a, b) for b in rows)[int(0.5 * (n - 1))] for a in rows]
        assert len(rows) == n and len(set(medians)) == 1 and len({r.tobytes() for r in rows}) == n, name
    # the product that underflows to -0, and what 0.0f + (-0) makes of it
    mp = mps[cases["minus_zero"]]
    normali = mat_sub(mp.mWorldPos, kfs[6].GetCameraCenter())
    c = mat_div(normali, cv_norm(normali))
    assert normali[0] < 0 and bits(np.array(c, np.float32))[0] == 0x80000000
    e = up_expected(t, x, fx["lists"]["all"], 3)
    assert bits(e["mp_normal"][cases["minus_zero"]])[0] == 0 and e["mp_normal"][cases["minus_zero"]][1] == 1.0
    assert fx["lists"]["twice"].count(cases["n65"]) == 3 and fx["lists"]["empty"] == []
    # every status bit a table can produce, each where it belongs
    st = dict(zip(fx["lists"]["all"], e["status"].tolist()))
    want = {"ref_not_observer": REF_NOT_OBSERVER, "ref_none": NO_REF, "ref_without_keypoints": REF_NOT_OBSERVER | REF_NO_KP, "octave_n_levels": OCTAVE,
            "n129": DESC_OVERFLOW, "ceiling_many_good": DESC_OVERFLOW, "above_ceiling": OBS_OVERFLOW}
    assert {name: st[p] for name, p in cases.items()} == {name: want.get(name, 0) for name in cases}
    assert up_expected(t, x, [t["n_mp"], -1, 0], 3)["status"].tolist() == [BAD_SLOT, BAD_SLOT, 0]
    cm = cull_map()
    assert sorted(cm["lists"]) == sorted(CULL_LENGTHS) == [0, 1, 63, 64, 65, 1000] and all(len(set(v.tolist())) == n for n, v in cm["lists"].items())
    for mono in (False, True):
        e = cull_expected(cm["t"], cm["x"], cm["lists"][1000], CUR_ID, mono)
        assert sorted(set(e["verdict"].tolist())) == [0, 1, 2, 3, 4] and 0 < e["n_kept"] < 1000
    seen = {c for c in cm["combos"]}
    assert {(0, 0), (3, 0), (1, 4)} <= {c[1] for c in seen} and {1, 2, 3} <= {c[2] for c in seen} and {2, 3, 4} <= {c[3] for c in seen}


def test_the_restatement_on_the_odd_places():
    fx = up_map()
    t, x, cases = fx["t"], fx["x"], fx["cases"]
    e = up_expected(t, x, fx["lists"]["all"], 3)
    same = lambda name, keys: all(np.array_equal(bits(e[k][cases[name]]), bits(x[k][cases[name]])) for k in keys)
    normal = ("mp_normal", "mp_max_dist", "mp_min_dist")
    for name in ("bad_point", "no_observations", "above_ceiling"):
        assert same(name, normal + ("mp_desc",)), name
    for name in ("ref_none", "ref_without_keypoints", "octave_n_levels"):                     # the normal stays, the descriptor is a separate walk
        assert same(name, normal) and not same(name, ("mp_desc",)), name
    for name in ("n129", "ceiling_many_good", "all_observers_bad"):                           # the other way round
        assert same(name, ("mp_desc",)) and not same(name, normal), name
    kfs, mps = objects(t, x)
    desc = lambda name, k: kfs[k].mDescriptors[mps[cases[name]].mObservations[kfs[k]]]
    assert np.array_equal(e["mp_desc"][cases["n2_descending"]], desc("n2_descending", 3))    # the first in SLOT order, stored second
    assert np.array_equal(e["mp_desc"][cases["tie3"]], desc("tie3", 2))
    assert np.array_equal(e["mp_desc"][cases["n1"]], desc("n1", 5))
    assert any(np.array_equal(e["mp_desc"][cases["bad_observer"]], desc("bad_observer", k)) for k in (1, 2, 4))     # never the bad observer's row
    # the reference keyframe that does not observe the point: the octave of ITS keypoint 0
    p = cases["ref_not_observer"]
    level = x["kf_octave"][t["kf_mp_ptr"][9]]
    PC = mat_sub(t["mp_pos"][p], x["kf_center"][9])
    assert bits(e["mp_max_dist"][p]) == bits(np.float32(np.float32(cv_norm(PC)) * x["scale_factors"][level]))
    # the order matters: the same observers summed in stored order give other bits somewhere
    differs = 0
    for name in ("n63", "n65", "n128", "ceiling"):
        p = cases[name]
        s = [np.float32(0)] * 3
        for k in obs_of(fx, name):
            d = mat_sub(t["mp_pos"][p], x["kf_center"][k])
            s = [np.float32(a + b) for a, b in zip(s, mat_div(d, cv_norm(d)))]
        differs += not np.array_equal(bits(np.array(mat_div(s, len(obs_of(fx, name))), np.float32)), bits(e["mp_normal"][p]))
    assert differs >= 1


def test_culling_verdicts_by_hand():
    class P:
        def __init__(self, bad, found, visible, first, nobs):
            self.bad, self.mnFound, self.mnVisible, self.mnFirstKFid, self.nobs = bad, found, visible, first, nobs
        isBad = lambda self: self.bad
        Observations = lambda self: self.nobs
        GetFoundRatio = MapPoint.GetFoundRatio
    v = lambda mono, *a: MapPointCulling([P(*a)], 10, mono)[0][0]
    assert v(True, True, 0, 1, 0, 0) == 1                                       # bad first, whatever else holds
    assert v(True, False, 0, 0, 10, 9) == 0 and v(True, False, 3, 0, 10, 9) == 0   # NaN and inf are not below a quarter
    assert v(True, False, 1, 4, 10, 9) == 0 and v(True, False, 1, 5, 10, 9) == 2   # exactly a quarter is not below
    assert v(True, False, 5, 5, 9, 2) == 0                                      # id difference 1
    assert v(True, False, 5, 5, 8, 2) == 3 and v(True, False, 5, 5, 8, 3) == 0    # difference 2: th = 2 monocular
    assert v(False, False, 5, 5, 8, 3) == 3 and v(False, False, 5, 5, 8, 4) == 0   # th = 3 otherwise
    assert v(True, False, 5, 5, 7, 3) == 4 and v(False, False, 5, 5, 7, 3) == 3 and v(False, False, 5, 5, 7, 4) == 4
    assert v(True, False, 5, 5, 12, 1) == 0                                     # a first keyframe after the current one


def jobs_of_fixtures():
    fx, sm, cm = up_map(), small_map(), cull_map()
    jobs = []
    for what in (1, 2, 3):
        for name in ("all", "twice", "reversed", "empty"):
            jobs.append(dict(t=fx["t"], x=fx["x"], points=fx["lists"][name], what=what, recent=[], cur_id=0, monocular=True))
    jobs.append(dict(t=fx["t"], x=fx["x"], points=[fx["t"]["n_mp"], -1, 0, 2 ** 31 - 1], what=3, recent=[], cur_id=0, monocular=True))
    jobs.append(dict(t=sm["t"], x=sm["x"], points=sm["lists"]["all"], what=3, recent=[0, 1, 2, 3], cur_id=1, monocular=False))
    for n in CULL_LENGTHS:
        for mono in (True, False):
            jobs.append(dict(t=cm["t"], x=cm["x"], points=[], what=1, recent=cm["lists"][n], cur_id=CUR_ID, monocular=mono))
    return jobs


def check(jobs):
    for i, (j, out) in enumerate(zip(jobs, host_run(jobs))):
        assert_same(up_of(out), up_expected(j["t"], j["x"], j["points"], j["what"]), UP_OUTPUTS, "job %d" % i)
        assert_same(out, cull_expected(j["t"], j["x"], j["recent"], j["cur_id"], j["monocular"]), CULL_OUTPUTS, "job %d" % i)


def test_header_on_the_host_equals_the_restatement_on_every_fixture():
    check(jobs_of_fixtures())


def test_header_on_the_host_skips_an_entry_outside_the_table():
    cm = cull_map()
    recent = [3, cm["t"]["n_mp"], 5, -1, 7]
    out = host_run([dict(t=cm["t"], x=cm["x"], points=[], what=1, recent=recent, cur_id=CUR_ID, monocular=True)])[0]
    e = cull_expected(cm["t"], cm["x"], [3, 5, 7], CUR_ID, True)
    assert out["status"] == BAD_SLOT and out["verdict"][[1, 3]].tolist() == [0xee, 0xee] and out["verdict"][[0, 2, 4]].tolist() == e["verdict"].tolist()
    assert out["n_kept"] == e["n_kept"] and out["kept"][:e["n_kept"]].tolist() == e["kept"][:e["n_kept"]].tolist()


@pytest.mark.parametrize("seed", range(4))
def test_header_on_the_host_equals_the_restatement_on_random_small_maps(seed):
    rng = np.random.default_rng(77 + seed)
    check([random_map(rng) for _ in range(600)])
