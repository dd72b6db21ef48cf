"""slamit_map_grow_batch_dev on the GPU against the literal restatement (tests/map_grow_ref.py) on every fixture: the tables at their
capacities and every output prefilled, every array compared in full, what lies past every count included; eight maps with lists of
different lengths in one call, one of them empty; each capacity at its need and one below with the neighbours written; the same bytes
from the same input twice; ids outside their tables."""
import copy

import numpy as np
import pytest

from tests import map_grow_ref as ref
from tests.map_grow_fixtures import all_fixtures, bad_fixtures, by_name
from tests.map_grow_host import INDEX, api_run, assert_same, default_caps, host_run, inputs, laid_out, resident_run

pytestmark = pytest.mark.gpu
NEEDS = ("kf_cap", "mp_cap", "kfmp_cap", "edit_cap", "recent_cap")
BITS = (ref.KF_OVERFLOW, ref.MP_OVERFLOW, ref.KFMP_OVERFLOW, ref.EDIT_OVERFLOW, ref.RECENT_OVERFLOW)
SHARED = ("cap", "cand_cap", "edit_cap", "recent_cap")


def shared_caps(fxs, pad=2):
    """Per map its own table capacities; the batch's four are the largest any map needs."""
    caps = [default_caps(fx, pad=pad) for fx in fxs]
    for key in SHARED:
        top = max(c[key] for c in caps)
        for c in caps:
            c[key] = top
    return caps


def empty_list(fx):
    fx = copy.deepcopy(fx)
    fx["name"], fx["ops"] = fx["name"] + "_no_ops", []
    return fx


@pytest.mark.parametrize("name", [fx["name"] for fx in all_fixtures()])
def test_the_host_form_equals_the_restatement(name):
    fx = by_name(name)
    caps = default_caps(fx)
    got, out = api_run(fx, caps)
    assert_same(got, laid_out(fx, caps)[0], name)
    # what api.map_grow hands back is a map: the grown tables cut to the counts the records now hold
    w = ref.apply(fx)
    assert out["status"] == 0 and out["n_kf"] == len(w["kfs"]) and out["n_mp"] == fx["t"]["n_mp"] + w["P"] and len(out["edits"]) == len(w["edits"])
    assert len(out["kf_mp"]) == out["kf_mp_ptr"][-1] == sum(len(k.mvpMapPoints) for k in w["kfs"]) and len(out["obs_ptr"]) == out["n_mp"] + 1 and out["recent"].tolist() == w["recent"]


def test_the_host_form_meets_the_gate_and_refuses_what_the_resident_form_skips():
    from weiner_slamit_v2_amd import api

    fx = by_name("wave_edges")
    for key in NEEDS:
        caps = default_caps(fx, pad=0)
        caps[key] -= 1
        got, out = api_run(fx, caps)
        e, _ = laid_out(fx, caps)
        assert e["status"] == BITS[NEEDS.index(key)] == out["status"] and out["n_kf"] == fx["t"]["n_kf"] and out["n_mp"] == fx["t"]["n_mp"]
        assert_same(got, e, key)
    a, b = bad_fixtures()
    for fx, word in ((a, "a NEW_KF op does not name the next free slot"), (b, "kf_mp holds a point slot")):
        with pytest.raises(api.SlamitError) as err:
            api_run(fx, default_caps(fx))
        assert "(-1)" in str(err.value) and word in str(err.value)


@pytest.mark.parametrize("part", range(2))
def test_the_resident_form_equals_the_restatement(part):
    """One call over eight (seven) maps with lists of different lengths, one of them empty; every fixture is in one of the two calls."""
    every = all_fixtures() + bad_fixtures()
    assert len(every) == 13
    fxs = every[part::2] + [empty_list(every[part])]
    assert len(fxs) <= 8 and len({len(fx["ops"]) for fx in fxs}) > 3 and sum(len(fx["frames"]) for fx in fxs) <= 16
    caps = shared_caps(fxs)
    outs, _ = resident_run(fxs, caps)
    for fx, c, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, c)[0], fx["name"])
    assert outs[-1]["status"] == 0 and outs[-1]["n_new"] == 0 and outs[-1]["n_edits_out"] == 0


def test_every_capacity_at_its_need():
    fxs = [by_name(n) for n in ("kf_only", "two_new_kfs", "associate_duplicate", "pairs_mixed_status", "wave_edges")]
    caps = shared_caps(fxs, pad=0)
    outs, _ = resident_run(fxs, caps, pad=0)
    for fx, c, got in zip(fxs, caps, outs):
        assert got["status"] == 0
        assert_same(got, laid_out(fx, c)[0], fx["name"])


@pytest.mark.parametrize("key", NEEDS)
def test_a_capacity_one_below_its_need_writes_nothing_but_the_needs(key):
    """The map that meets the gate keeps every byte but its needs and its status; its neighbours in the same call are written."""
    fxs = [by_name("associate_plain"), by_name("wave_edges"), by_name("kf_only")]
    caps = shared_caps(fxs, pad=0)                                          # wave_edges has the largest need of everything: the batch's are its own
    caps[1][key] -= 1
    if key in SHARED:
        for c in caps:
            c[key] = caps[1][key]
    outs, _ = resident_run(fxs, caps)
    for fx, c, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, c)[0], fx["name"])
    assert [o["status"] for o in outs] == [0, BITS[NEEDS.index(key)], 0]
    assert outs[1]["need"] == [default_caps(fxs[1], pad=0)[k] for k in NEEDS]
    a = inputs(fxs[1], caps[1])
    for k, _, _ in INDEX:                                                   # byte for byte what it was given
        assert np.array_equal(outs[1][k], a[k]), k


def test_a_list_longer_than_its_capacity_is_refused():
    fxs = [by_name("pairs_mixed_status"), by_name("kf_only")]
    caps = shared_caps(fxs, pad=0)
    for c in caps:
        c["cap"] = 4                                                        # the first list has five ops
    outs, _ = resident_run(fxs, caps)
    assert outs[0]["status"] == ref.OPS_OVERFLOW and outs[1]["status"] == 0 and outs[0]["n_new"] == -11
    a = inputs(fxs[0], caps[0])
    for k, _, _ in INDEX:
        assert np.array_equal(outs[0][k], a[k]), k
    assert_same(outs[1], laid_out(fxs[1], caps[1])[0], "kf_only")


def test_the_ceilings_are_reached():
    """SLAMIT_GROW_MAX_OPS ops in one list and SLAMIT_GROW_MAX_FRAMES frame records in one call."""
    from weiner_slamit_v2_amd import api

    from tests.map_grow_fixtures import ceiling_fixtures

    fxs = ceiling_fixtures()
    assert len(fxs[0]["ops"]) == api.GROW_MAX_OPS and sum(len(fx["frames"]) for fx in fxs) == api.GROW_MAX_FRAMES
    caps = shared_caps(fxs, pad=0)
    for c in caps:
        c["cap"] = api.GROW_MAX_OPS
    outs, _ = resident_run(fxs, caps)
    for fx, c, got in zip(fxs, caps, outs):
        assert got["status"] == 0
        assert_same(got, laid_out(fx, c)[0], fx["name"])
    assert outs[0]["n_new"] > 10000 and outs[1]["kf_mp_ptr"][-1] == 6 + 3 * 15


def test_the_same_call_twice_gives_the_same_bytes():
    fxs = [by_name(n) for n in ("wave_edges", "chunk_edges", "same_keypoint_twice", "observers_65")]
    caps = shared_caps(fxs)
    a, _ = resident_run(fxs, caps)
    b, _ = resident_run(fxs, caps)
    for fx, x, y in zip(fxs, a, b):
        assert_same(x, y, fx["name"])


def test_ids_outside_their_tables_are_skipped_as_the_header_states():
    """The device cannot be shown its tables first: what the call leaves equals csrc/map_grow.h's sequential form, which states the same rules."""
    fxs = bad_fixtures() + [by_name("associate_plain")]
    caps = shared_caps(fxs)
    want = host_run(list(zip(fxs, caps)))
    outs, _ = resident_run(fxs, caps)
    for fx, w, got in zip(fxs, want, outs):
        assert_same(got, w, fx["name"])
    assert [o["status"] for o in outs] == [ref.BAD_SLOT, ref.BAD_SLOT, 0]
