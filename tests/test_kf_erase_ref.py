"""KeyFrame::SetBadFlag over the tables, on the CPU: the odd places of the restatement written out by hand, the g++-built header's
sequential form against the restatement on every fixture and at both gates, and the fixtures themselves."""
import numpy as np
import pytest

from tests import kf_erase_fixtures as fxs
from tests import kf_erase_host as host
from tests import kf_erase_ref as ref


def want_of(name):
    return ref.apply(fxs.by_name(name))


def test_a_leaf_leaves_its_neighbours_sorted_and_its_parent():
    w = want_of("leaf")
    assert w["op_status"] == [0] and w["kf_bad"] == [0, 0, 0, 1] and w["kf_parent"] == [-1, 0, 0, 1]
    assert w["children"] == [[1, 2], [], [], []]
    assert w["rows"] == {0: ([(1, 30), (2, 16)], [(1, 30), (2, 16)]), 1: ([(0, 30)], [(0, 30)]), 3: ([], [])}
    assert w["edits"] == [(6, 3), (7, 3)]


def test_the_early_exits_change_nothing_else():
    for name, status, tbe in (("origin", ref.ORIGIN, [0, 0, 0]), ("not_erase", ref.NOT_ERASE, [0, 1, 0]), ("no_parent", ref.NO_PARENT, [0, 0, 0])):
        fx, w = fxs.by_name(name), want_of(name)
        assert w["op_status"] == [status] and w["kf_to_be_erased"] == tbe and w["rows"] == {} and w["edits"] == [] and w["kf_bad"] == [0, 0, 0]
        assert w["kf_parent"] == fx["t"]["kf_parent"].tolist()


def test_asymmetric_links_stay_as_the_reference_leaves_them():
    w = want_of("asymmetric")
    assert set(w["rows"]) == {0, 1}            # 3's row lacks 1: byte for byte; 2 is not in 1's row: its stale entry stays
    assert w["rows"][0] == ([], [])


def test_a_thresholded_row_grows_and_equal_weights_descend_by_slot():
    assert want_of("thresholded")["rows"][2] == ([(0, 16), (3, 4)], [(0, 16), (3, 4)])
    assert want_of("equal_weights")["rows"][2][1] == [(4, 16), (3, 16), (0, 16)]
    assert want_of("one_to_zero")["rows"][1] == ([], [])


def test_the_spanning_tree_walk_as_written():
    assert want_of("child_to_parent")["kf_parent"] == [-1, 0, 0, 0] and want_of("child_to_parent")["children"] == [[2, 3], [], [], []]
    assert want_of("via_sibling")["kf_parent"] == [-1, 0, 0, 2, 0] and want_of("via_sibling")["children"] == [[2, 4], [], [3], [], []]
    assert want_of("equal_children")["kf_parent"] == [-1, 0, 0, 2, 0]
    assert want_of("equal_candidates")["kf_parent"] == [-1, 0, 0, 0, 0]
    assert want_of("ord_w_disagrees")["kf_parent"] == [-1, 0, 3, 0]
    assert want_of("ord_not_in_cw")["kf_parent"] == [-1, 0, 0, 0] and want_of("ord_not_in_cw")["children"] == [[2, 3], [], [], []]   # picked: it LEFT 1's row
    w = want_of("bad_child")
    assert w["kf_parent"] == [-1, 0, 0, 0] and w["children"] == [[2, 3], [2], [], []]                 # 3 was picked and left; 2 fell back and stays
    w = want_of("unlinked_child")
    assert w["kf_parent"] == [-1, 0, 0, 0] and w["children"] == [[2, 3], [2], [], []] and w["kf_bad"] == [0, 1, 0, 0]


def test_lists_run_in_list_order():
    assert want_of("twice")["op_status"] == [0, 0] and len(want_of("twice")["edits"]) == 4
    assert want_of("parent_heals")["op_status"] == [ref.NO_PARENT, 0, 0] and want_of("parent_heals")["edits"] == [(4, 2), (5, 2)]
    w = want_of("parent_present")
    assert w["children"][0] == [1, 4, 5] and w["children"][1] == [2, 4] and w["kf_parent"][4] == 0
    fx, w = fxs.by_name("empty"), want_of("empty")
    assert w["children"] == [[1, 5], [2, 4], [3], [], [], []] and w["rows"] == {}
    assert want_of("nulls")["edits"] == [(3, 2), (1, 2), (4, 1), (2, 1)]
    assert want_of("held_twice")["edits"] == [(5, 1), (2, 1), (5, 1)] and want_of("all_null")["edits"] == []


def test_the_fixtures_hold_what_they_claim():
    names = [fx["name"] for fx in fxs.all_fixtures()]
    assert len(set(names)) == len(names) and all(fx["what"] for fx in fxs.all_fixtures())
    for n in (0, 1, 63, 64, 65):
        fx = fxs.by_name("children_%d" % n)
        assert fx["t"]["kf_child_ptr"][2] - fx["t"]["kf_child_ptr"][1] == n
        w = ref.apply(fx)
        assert len(w["children"][1]) == n // 2 and sorted(w["children"][0]) == w["children"][0]      # the odd ones fell back and stay
    assert [fxs.by_name("n_kf_%d" % n)["t"]["n_kf"] for n in (1, 64, 65, 257)] == [1, 64, 65, 257]
    fx = fxs.by_name("row_cap")
    assert fx["x"]["cw_n"][1] == fx["x"]["row_cap"]
    fx = fxs.by_name("thresholded")
    assert fx["x"]["ord_n"][2] < fx["x"]["cw_n"][2]
    fx = fxs.by_name("ord_w_disagrees")
    assert fx["x"]["ord_w"][2][0] != fx["x"]["cw_w"][2][0]
    fx = fxs.by_name("ord_not_in_cw")
    assert 0 in fx["x"]["ord_kf"][2][:fx["x"]["ord_n"][2]] and 0 not in fx["x"]["cw_kf"][2][:fx["x"]["cw_n"][2]]
    fx = fxs.seeded()
    assert fx["t"]["n_kf"] == 40 and 10 <= len(fx["ops"]) <= 14
    w = ref.apply(fx)
    assert sum(1 for s in w["op_status"] if s == 0) >= 6 and ref.NOT_ERASE in w["op_status"] and len(w["rows"]) > 10
    assert any(x["ord_n"] < x["cw_n"] for x in [dict(ord_n=int(a), cw_n=int(b)) for a, b in zip(fx["x"]["ord_n"], fx["x"]["cw_n"])])   # thresholded rows, as UpdateConnections leaves them
    for f in fxs.all_fixtures():                  # every children row ascends, as the host form demands
        t = f["t"]
        for k in range(t["n_kf"]):
            row = t["kf_child"][t["kf_child_ptr"][k]:t["kf_child_ptr"][k + 1]].tolist()
            assert row == sorted(set(row))


def jobs_of(fx):
    cc, ec = host.default_caps(fx)
    want = ref.apply(fx)
    need, n_edits = sum(len(r) for r in want["children"]), len(want["edits"])
    jobs = [(fx, cc, ec), (fx, need, n_edits)]                        # roomy; both caps at the need
    if need > 0:
        jobs.append((fx, need - 1, ec))
    if n_edits > 0:
        jobs.append((fx, cc, n_edits - 1))
    return want, jobs


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_header_equals_the_restatement_on_every_fixture(sanitize):
    """csrc/kf_erase.h's sequential form, built by g++ as a stand-alone program (once more under the address and undefined-behaviour
    sanitizers), against the restatement: every array in full, what lies past every count included, at roomy caps, at the need, and
    one below each gate."""
    jobs, wants = [], []
    for fx in fxs.all_fixtures():
        want, js = jobs_of(fx)
        jobs += js
        wants += [want] * len(js)
    gated = 0
    for (fx, cc, ec), want, got in zip(jobs, wants, host.host_run(jobs, sanitize=sanitize)):
        e = host.laid_out(fx, want, cc, ec)
        gated += e["status"] != 0
        host.assert_same(got, e, "%s child_cap %d edit_cap %d" % (fx["name"], cc, ec))
    assert gated > 20


def test_the_header_at_its_ceilings():
    """1,024 children and 1,024 ops equal the restatement; one child more and the op is skipped whole."""
    cfx = list(fxs.ceiling_fixtures())
    jobs = [(fx,) + host.default_caps(fx) for fx in cfx]
    outs = host.host_run(jobs)
    for i in (0, 2):
        host.assert_same(outs[i], host.laid_out(cfx[i], ref.apply(cfx[i]), jobs[i][1], jobs[i][2]), cfx[i]["name"])
    assert outs[1]["status"] == ref.ROW_OVERFLOW and outs[1]["op_status"].tolist() == [ref.ROW_OVERFLOW] and outs[1]["n_edits_out"] == 0
    for key, _ in host.INPLACE:
        assert np.array_equal(outs[1][key], np.asarray(host.source(cfx[1], key)).reshape(-1)), key
    assert outs[1]["child_out"][:outs[1]["n_child_out"]].tolist() == cfx[1]["t"]["kf_child"].tolist()
