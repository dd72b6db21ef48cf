"""The restatement of map growth (tests/map_grow_ref.py) at the odd places, by hand; csrc/map_grow.h built with g++ against it on every
fixture, plainly and under -fsanitize=address,undefined in the same stand-alone program; and the two ways round: the end state the
restatement walked to equals map_edit_ref applied to (the tables the grow call leaves, the edits it emits), table for table."""
import numpy as np
import pytest

from tests import map_edit_ref
from tests import map_grow_ref as ref
from tests.map_grow_fixtures import all_fixtures, bad_fixtures, by_name
from tests.map_grow_host import assert_same, default_caps, host_run, laid_out

NAMES = [fx["name"] for fx in all_fixtures()]
NEEDS = ("kf_cap", "mp_cap", "kfmp_cap", "edit_cap", "recent_cap")
BITS = (ref.KF_OVERFLOW, ref.MP_OVERFLOW, ref.KFMP_OVERFLOW, ref.EDIT_OVERFLOW, ref.RECENT_OVERFLOW)


def edits_of(w):
    return [(p, k, i, wt) for _, _, p, k, i, _, wt in w["edits"]]


def test_a_new_keyframe_and_one_without_keypoints():
    w = ref.apply(by_name("kf_only"))
    assert w["op_status"] == [2, 3] and w["edits"] == [] and w["recent"] == [4, 1] and w["n_new"] == 0 and w["status"] == 0
    assert w["kfs"][2].mvpMapPoints == [0, -1, 3, 3, 6] and w["kfs"][3].mvpMapPoints == [] and len(w["kfs"]) == 4


def test_the_initial_map():
    w = ref.apply(by_name("two_new_kfs"))
    assert w["op_status"] == [0, 1, 0, 1, 2, 3, 4, 5] and w["n_new"] == 6 and w["recent"] == []
    assert edits_of(w)[:4] == [(0, 0, 1, 1), (0, 1, 7, 1), (1, 0, 2, 1), (1, 1, 6, 1)] and len(w["edits"]) == 12
    assert all(mp.mpRefKF == 1 and mp.nObs == 2 and list(mp.mObservations) == [0, 1] for mp in w["mps"])
    assert w["kfs"][0].mvpMapPoints == [-1, 0, 1, 2, 3, 4, 5, -1, -1] and w["kfs"][1].mvpMapPoints == [-1, -1, 5, 4, 3, 2, 1, 0]
    c = ref.center_of([1, 0, 0, 2, 0, 1, 0, 3, 0, 0, 1, 4])
    assert [float(v) for v in c] == [-2.0, -3.0, -4.0]


def test_associate_skips_nulls_and_bad_points_and_emits_in_keypoint_order():
    w = ref.apply(by_name("associate_plain"))
    assert w["op_status"] == [3, 3] and [(p, k, i) for p, k, i, _ in edits_of(w)] == [(4, 3, 1), (0, 3, 4), (8, 3, 5), (7, 3, 6)] and w["recent"] == [3]
    fr = by_name("associate_plain")["frames"][0]
    assert [wt for _, _, _, wt in edits_of(w)] == [2 if fr["uright"][i] >= 0 else 1 for i in (1, 4, 5, 6)]
    assert w["kfs"][3].mvpMapPoints[2] == 2 and w["mps"][2].mbBad                     # the bad point stays in the row


def test_a_point_at_two_keypoints_adds_once():
    w = ref.apply(by_name("associate_duplicate"))
    assert [(p, k, i) for p, k, i, _ in edits_of(w)] == [(5, 3, 0), (1, 3, 2)] and w["recent"] == [5, 1, 5]


def test_stereo_points_made_before_the_association_go_to_the_recent_list():
    w = ref.apply(by_name("associate_after_stereo_points"))
    assert w["op_status"] == [2, 8, 9, 2] and w["kfs"][2].mvpMapPoints == [3, -1, 8, 6, 9, 0]
    assert edits_of(w) == [(8, 2, 2, 2), (9, 2, 4, 2)] + [(p, 2, i, e[3]) for (p, i), e in zip(((3, 0), (6, 3), (0, 5)), edits_of(w)[2:])] and w["recent"] == [8, 9]


def test_a_keyframe_the_table_already_lists_as_observer():
    fx = by_name("associate_existing_observer")
    w = ref.apply(fx)
    row = fx["t"]["kf_mp"][fx["t"]["kf_mp_ptr"][1]:fx["t"]["kf_mp_ptr"][2]].tolist()
    old = [p for p in row if p >= 0 and 1 in fx["t"]["obs_kf"][fx["t"]["obs_ptr"][p]:fx["t"]["obs_ptr"][p + 1]].tolist()]
    assert w["recent"] == old and len(old) >= 3 and len(w["edits"]) == 2 and sorted(p for p, _, _, _ in edits_of(w)) == sorted(set(row) - set(old) - {-1})


def test_rejected_candidates_leave_compact_slots_and_an_inert_tail():
    fx = by_name("pairs_mixed_status")
    w = ref.apply(fx)
    assert w["op_status"] == [10, ref.OP_REJECTED, 11, ref.OP_REJECTED, 12] and w["n_new"] == 3 and w["P"] == 5 and w["recent"] == [2, 10, 11, 12] and len(w["edits"]) == 6
    e, _ = laid_out(fx, default_caps(fx))
    assert e["mp_bad"][10:15].tolist() == [0, 0, 0, 1, 1] and e["mp_ref_kf"][10:15].tolist() == [2, 2, 2, -1, -1] and e["obs_ptr"][10:16].tolist() == [e["obs_ptr"][10]] * 6
    assert np.array_equal(e["mp_pos"][30:39].reshape(3, 3), fx["cand_x3d"][[0, 2, 4]]) and not e["mp_pos"][39:45].any() and e["mp_found"][10:15].tolist() == [1, 1, 1, 0, 0]


def test_two_points_at_one_keypoint():
    w = ref.apply(by_name("same_keypoint_twice"))
    assert w["op_status"] == [5, 6, 7] and w["kfs"][1].mvpMapPoints[3] == 6 and w["kfs"][0].mvpMapPoints[2] == 5 and w["kfs"][0].mvpMapPoints[5] == 6
    assert w["mps"][5].mObservations == {1: 3, 0: 2} and w["mps"][6].mObservations == {0: 5, 1: 3}
    assert len(w["edits"]) == 6 and w["mps"][7].mObservations == {0: 1} and w["mps"][7].nObs == 1     # the second AddObservation of one keyframe does nothing


def test_ops_that_cannot_be_applied_are_skipped():
    a, b = bad_fixtures()
    w = ref.apply(a)
    assert w["op_status"] == [ref.OP_BAD, ref.OP_BAD, 3, ref.OP_BAD, 3] and w["status"] == ref.BAD_SLOT and len(w["kfs"]) == 4
    caps = default_caps(b)
    w = ref.apply(b, caps)
    st = w["op_status"]
    assert st[:4] == [ref.OP_BAD] * 4 and st[4] == 1 and st[5:22] == [ref.OP_BAD] * 17 and st[22:] == [ref.OP_REJECTED, 9, 3, 3] and w["status"] == ref.BAD_SLOT
    assert w["kfs"][3].mvpMapPoints == [-1, -1, 2, -1, -1, 8, 7] and w["n_new"] == 1 and w["P"] == 15


@pytest.mark.parametrize("name", NAMES + ["wrong_slot", "bad_slots"])
def test_the_edits_applied_to_what_grow_leaves_give_the_literal_end_state(name):
    """Both ways round: map_edit_ref over (the tables as laid out after the call, the emitted edits) == the tables built from scratch
    out of the objects the restatement ended with."""
    fx = ([fx for fx in all_fixtures() + bad_fixtures() if fx["name"] == name])[0]
    caps = default_caps(fx)
    e, w = laid_out(fx, caps)
    n_kf, n_mp = len(w["kfs"]), fx["t"]["n_mp"] + w["P"]
    t = {"n_kf": n_kf, "n_mp": n_mp, "obs_ptr": e["obs_ptr"][:n_mp + 1], "obs_kf": fx["t"]["obs_kf"], "kf_mp_ptr": e["kf_mp_ptr"][:n_kf + 1],
         "kf_mp": e["kf_mp"][:e["kf_mp_ptr"][n_kf]], "mp_bad": e["mp_bad"][:n_mp]}
    x = {"obs_idx": fx["t"]["obs_idx"], "obs_octave": fx["t"]["obs_octave"], "obs_weight": fx["t"]["obs_weight"], "mp_nobs": e["mp_nobs"][:n_mp], "mp_ref_kf": e["mp_ref_kf"][:n_mp]}
    if name == "bad_slots":                                                # map_edit_ref is shown valid tables
        t["kf_mp"] = np.where(t["kf_mp"] >= n_mp, -1, t["kf_mp"])
    got = map_edit_ref.apply(t, x, w["edits"], obs_cap_out=1 << 20)
    mps = w["mps"] + [None] * (n_mp - len(w["mps"]))
    assert got["status"] == 0 and got["obs_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(m.mObservations) if m else 0 for m in mps])]).tolist()
    assert got["obs_kf"].tolist() == [k for m in mps if m for k in m.mObservations] and got["obs_idx"].tolist() == [i for m in mps if m for i in m.mObservations.values()]
    assert got["mp_nobs"].tolist() == [m.nObs if m else 0 for m in mps] and got["mp_bad"].tolist() == [int(m.mbBad) if m else 1 for m in mps]
    assert got["mp_ref_kf"].tolist() == [m.mpRefKF if m else -1 for m in mps]
    rows = [v for kf in w["kfs"] for v in kf.mvpMapPoints]
    assert got["kf_mp"].tolist() == (np.where(np.array(rows) >= n_mp, -1, rows).tolist() if name == "bad_slots" else rows)
    assert sorted(set(got["touched"].tolist())) == sorted({ed[2] for ed in w["edits"]} - {m.slot for m in w["mps"] if not m.mObservations})
    for p, k, i, _ in edits_of(w):                                         # every emitted edit is one map_edit.h takes
        assert 0 <= p < n_mp and 0 <= k < n_kf and 0 <= i < t["kf_mp_ptr"][k + 1] - t["kf_mp_ptr"][k]


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_header_equals_the_restatement_on_every_fixture(sanitize):
    jobs = [(fx, default_caps(fx)) for fx in all_fixtures() + bad_fixtures()]
    jobs += [(fx, default_caps(fx, pad=0)) for fx in all_fixtures()]       # every capacity at its need
    for (fx, caps), got in zip(jobs, host_run(jobs, sanitize)):
        assert_same(got, laid_out(fx, caps)[0], fx["name"])


def test_each_capacity_one_below_its_need_writes_nothing_but_the_needs():
    jobs = []
    for name in ("wave_edges", "associate_after_stereo_points", "pairs_mixed_status"):
        fx = by_name(name)
        for key in NEEDS:
            caps = default_caps(fx, pad=0)
            holds = {"kf_cap": fx["t"]["n_kf"], "mp_cap": fx["t"]["n_mp"], "kfmp_cap": len(fx["t"]["kf_mp"]), "edit_cap": 0, "recent_cap": len(fx["recent"])}
            if caps[key] > holds[key]:                                     # a capacity never lies below what the tables hold
                caps[key] -= 1
                jobs.append((fx, caps, key))
    assert len(jobs) == 13 and {j[2] for j in jobs} == set(NEEDS)
    for (fx, caps, key), got in zip(jobs, host_run([j[:2] for j in jobs])):
        e, _ = laid_out(fx, caps)
        assert e["status"] == BITS[NEEDS.index(key)] and e["need"] == [default_caps(fx, pad=0)[k] for k in NEEDS], (fx["name"], key)
        assert_same(got, e, "%s %s" % (fx["name"], key))


def test_the_header_at_its_ceilings():
    from tests.map_grow_fixtures import ceiling_fixtures

    jobs = [(fx, default_caps(fx, pad=0, cap_pad=0)) for fx in ceiling_fixtures()]
    assert jobs[0][1]["cap"] == 65536
    outs = host_run(jobs)
    for (fx, caps), got in zip(jobs, outs):
        assert got["status"] == 0
        assert_same(got, laid_out(fx, caps)[0], fx["name"])
    assert outs[0]["n_new"] > 10000 and outs[1]["kf_mp_ptr"][-1] == 6 + 3 * 15


def test_the_same_input_twice_gives_the_same_bytes():
    jobs = [(fx, default_caps(fx)) for fx in all_fixtures()]
    a, b = host_run(jobs), host_run(jobs)
    for x, y, (fx, _) in zip(a, b, jobs):
        assert_same(x, y, fx["name"])
