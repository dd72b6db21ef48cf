"""slamit_kf_erase_apply and slamit_kf_erase_batch_dev on the GPU against the literal restatement (tests/kf_erase_ref.py) on every
fixture: every output prefilled, every array and graph row compared in full, what lies past every count included; several maps with
lists of different lengths in one call; both gates; the same bytes from the same input twice; slots outside their tables."""
import copy

import numpy as np
import pytest

from tests import kf_erase_ref as ref
from tests.kf_erase_fixtures import all_fixtures, by_name, ceiling_fixtures
from tests.kf_erase_host import EDIT_DTYPE, INPLACE, OUT_KEYS, assert_same, default_caps, fills, host_run, laid_out, of_api, records, resident_run, source

pytestmark = pytest.mark.gpu
NAMES = [fx["name"] for fx in all_fixtures()]


def filled(fx, cc, ec):
    f = fills(fx, cc, ec)
    f["edits"] = f["edits"].view(EDIT_DTYPE)
    return f


@pytest.mark.parametrize("name", NAMES)
def test_the_host_form_equals_the_restatement(name):
    from weiner_slamit_v2_amd import api

    fx = by_name(name)
    cc, ec = (c + 3 for c in default_caps(fx))
    out = api.kf_erase(dict(fx["t"]), fx["x"], records(fx["ops"]), child_cap_out=cc, edit_cap=ec, fill=filled(fx, cc, ec))
    want = ref.apply(fx)
    assert_same(of_api(out), laid_out(fx, want, cc, ec), name)
    # what api.kf_erase hands back is a map: the children table as api.MapIndex takes it
    assert out["kf_child_ptr"].tolist() == np.cumsum([0] + [len(r) for r in want["children"]]).tolist()
    assert out["kf_child"].tolist() == [c for r in want["children"] for c in r] and len(out["edits"]) == len(want["edits"])
    rec, keep = api._map_index_host(dict(fx["t"], **{k: out[k] for k in ("kf_child_ptr", "kf_child", "kf_bad", "kf_parent")}))
    assert rec.n_kf == fx["t"]["n_kf"] and len(keep["kf_child"]) == out["n_child_out"]


@pytest.mark.parametrize("part", range(5))
def test_the_resident_form_equals_the_restatement(part):
    """One call over eight maps with lists of different lengths (among them none); every fixture is in one of the five calls."""
    every = all_fixtures()
    assert len(every) <= 40
    fxs = list(every[part::5])
    assert len({len(fx["ops"]) for fx in fxs}) > 1
    ec = max(default_caps(fx)[1] for fx in fxs) + 3
    caps = [(default_caps(fx)[0] + 3, ec) for fx in fxs]
    outs, _, _ = resident_run(fxs, caps)
    for fx, (cc, _), got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, ref.apply(fx), cc, ec), fx["name"])


def test_both_gates_write_nothing_but_the_need():
    """child_cap_out and edit_cap at the need and one below, in both forms; the map that meets a gate keeps every byte while its
    neighbours in the same call are written."""
    from weiner_slamit_v2_amd import api

    for name in ("via_sibling", "unlinked_child", "nulls", "seeded"):
        fx, want = by_name(name), ref.apply(by_name(name))
        need, n_edits = sum(len(r) for r in want["children"]), len(want["edits"])
        for cc, ec, status in ((need, n_edits, 0), (need - 1, n_edits, ref.CHILD_OVERFLOW), (need, n_edits - 1, ref.EDIT_OVERFLOW),
                               (need - 1, n_edits - 1, ref.CHILD_OVERFLOW | ref.EDIT_OVERFLOW)):
            if cc < 0 or ec < 0:                                           # nulls ends with an empty children table
                continue
            out = api.kf_erase(dict(fx["t"]), fx["x"], records(fx["ops"]), child_cap_out=cc, edit_cap=ec, fill=filled(fx, cc, ec))
            e = laid_out(fx, want, cc, ec)
            assert e["status"] == status and out["n_child_out"] == need and out["n_edits_out"] == n_edits
            assert_same(of_api(out), e, "%s %d %d" % (name, cc, ec))
    fxs = [by_name(n) for n in ("leaf", "via_sibling", "then_child", "unlinked_child", "nulls", "children_65")]
    wants = [ref.apply(fx) for fx in fxs]
    ec = max(len(w["edits"]) for w in wants)                               # nulls: 4 + ... every map fits; then one below the largest
    caps = [(sum(len(r) for r in w["children"]), ec) for w in wants]
    caps[1] = (caps[1][0] - 1, ec)
    caps[3] = (caps[3][0] - 1, ec)
    outs, _, _ = resident_run(fxs, caps)
    for fx, w, (cc, _), got in zip(fxs, wants, caps, outs):
        assert_same(got, laid_out(fx, w, cc, ec), fx["name"])
    assert [o["status"] for o in outs] == [0, ref.CHILD_OVERFLOW, 0, ref.CHILD_OVERFLOW, 0, 0]
    for i in (1, 3):
        for key, _ in INPLACE:
            assert np.array_equal(outs[i][key], np.asarray(source(fxs[i], key)).reshape(-1)), (fxs[i]["name"], key)
    ec -= 1                                                                # the batch's edit_cap one below the largest list
    outs, _, _ = resident_run(fxs, [(c, ec) for c, _ in caps])
    for fx, w, (cc, _), got in zip(fxs, wants, caps, outs):
        assert_same(got, laid_out(fx, w, cc, ec), fx["name"])
    assert sum(1 for o in outs if o["status"] & ref.EDIT_OVERFLOW) >= 1 and sum(1 for o in outs if o["status"] == 0) >= 2


def test_the_same_call_twice_gives_the_same_bytes():
    fxs = [by_name(n) for n in ("seeded", "children_65", "n_kf_257", "then_parent", "equal_weights")]
    ec = max(default_caps(fx)[1] for fx in fxs)
    caps = [(default_caps(fx)[0], ec) for fx in fxs]
    a, _, _ = resident_run(fxs, caps)
    b, _, _ = resident_run(fxs, caps)
    for fx, x, y in zip(fxs, a, b):
        for key in OUT_KEYS:
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), (fx["name"], key)


def test_slots_outside_their_tables_are_skipped_in_the_device_form():
    """The device cannot be shown its tables first.  An op whose keyframe or parent lies outside the table, a keyframe whose stored parent
    does, a neighbour or a child outside it: skipped, never dereferenced, SLAMIT_KF_ERASE_BAD_SLOT; everything else is applied.  What the
    call leaves equals csrc/kf_erase.h's sequential form, which states the same rules (its host driver refuses nothing)."""
    base = by_name("then_child")
    n_kf = base["t"]["n_kf"]
    a = copy.deepcopy(base)
    a["name"] = "bad_ops"
    a["ops"] = [(ref.SET_BAD, n_kf, -1), (ref.SET_BAD, -1, -1), (ref.SET_PARENT, 3, n_kf + 7), (ref.SET_PARENT, -2, 0), (7, 1, 0), (ref.SET_BAD, 1, -1), (ref.SET_PARENT, 5, 4)]
    b = copy.deepcopy(base)
    b["name"] = "bad_tables"
    b["x"]["cw_kf"][1, 1] = n_kf + 3            # a neighbour of 1 outside the table
    b["x"]["cw_kf"][2, 0] = -9                  # and one of 2
    b["x"]["ord_kf"][3, 0] = 1 << 20            # an ord entry of child 3 of 2: no candidate
    b["t"]["kf_child"][b["t"]["kf_child_ptr"][1]] = 9999   # a child of 1 outside the table
    b["t"]["kf_parent"][4] = n_kf               # a stored parent outside the table
    b["ops"] = [(ref.SET_BAD, 4, -1), (ref.SET_BAD, 1, -1), (ref.SET_BAD, 2, -1)]
    fxs = [a, b, base]
    ec = max(default_caps(base)[1], 12) + 2
    caps = [(default_caps(base)[0] + 8, ec)] * 3
    want = host_run([(fx, cc, e) for fx, (cc, e) in zip(fxs, caps)])
    outs, _, _ = resident_run(fxs, caps)
    for fx, w, got in zip(fxs, want, outs):
        assert_same(got, w, fx["name"])
    assert outs[0]["status"] == ref.BAD_SLOT and outs[0]["op_status"].tolist() == [ref.BAD_SLOT] * 5 + [0, 0]
    assert outs[1]["status"] == ref.BAD_SLOT and outs[1]["op_status"].tolist() == [ref.BAD_SLOT, 0, 0] and outs[1]["kf_bad"].tolist() == [0, 1, 1, 0, 0, 0]
    assert outs[2]["status"] == 0


def test_the_ceilings_at_and_one_past():
    """SLAMIT_KF_ERASE_MAX_CHILD children of one SET_BAD keyframe (applied), one more (the op is skipped whole, ROW_OVERFLOW in its and the
    call's status, nothing else changes) and SLAMIT_KF_ERASE_MAX_OPS ops in one list, three maps in one call."""
    from weiner_slamit_v2_amd import api

    fxs = list(ceiling_fixtures())
    assert len(fxs[2]["ops"]) == api.KF_ERASE_MAX_OPS and [fx["t"]["kf_child_ptr"][2] - fx["t"]["kf_child_ptr"][1] for fx in fxs[:2]] == [api.KF_ERASE_MAX_CHILD, api.KF_ERASE_MAX_CHILD + 1]
    ec = max(default_caps(fx)[1] for fx in fxs)
    caps = [(default_caps(fx)[0], ec) for fx in fxs]
    outs, _, _ = resident_run(fxs, caps, pad=0)
    header = host_run([(fx, cc, e) for fx, (cc, e) in zip(fxs, caps)])
    for i, (fx, (cc, _), got) in enumerate(zip(fxs, caps, outs)):
        assert_same(got, header[i], fx["name"])
        if i != 1:                                                         # the restatement knows no ceiling
            assert_same(got, laid_out(fx, ref.apply(fx), cc, ec), fx["name"])
    assert [o["status"] for o in outs] == [0, ref.ROW_OVERFLOW, 0] and outs[1]["op_status"].tolist() == [ref.ROW_OVERFLOW] and outs[1]["n_edits_out"] == 0
    for key, _ in INPLACE:
        assert np.array_equal(outs[1][key], np.asarray(source(fxs[1], key)).reshape(-1)), key
    assert outs[0]["kf_bad"][1] == 1 and int((outs[0]["kf_parent"][2:] == 0).sum()) == api.KF_ERASE_MAX_CHILD and sum(outs[2]["kf_bad"]) == 16
