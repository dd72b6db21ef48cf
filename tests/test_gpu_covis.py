"""slamit_update_connections, slamit_keyframe_culling and their resident forms on the device against the restatement
(tests/covis_ref.py) on every fixture.

Integer work and compares only: everything is equal EXACTLY -- the counts, every cw, ord and kf_best row of the whole map (not only
the touched ones, and with the sentinels past every count), the parent, the statuses, the verdicts, n_mps, n_redundant and
mp_turned_bad."""
import numpy as np
import pytest

from tests.covis_fixtures import CULL_NAMES, GRAPH, UC_NAMES, fixture
from tests.covis_host import (BAD_SLOT, CULL_OUTPUTS, NMPS_FILL, NRED_FILL, PARENT_FILL, TURNED_FILL, UC_OUTPUTS, VERDICT_FILL, assert_same, cull_expected,
                              cull_prefilled, cull_tensors, graph_of, resident, uc_expected, uc_tensors)
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

GROUPS = lambda names: [names[i:i + api.LOCAL_MAP_MAX_MAPS] for i in range(0, len(names), api.LOCAL_MAP_MAX_MAPS)]


@pytest.mark.parametrize("name", UC_NAMES)
def test_update_connections_host_form_equals_the_restatement(name):
    fx = fixture("uc", name)
    before = {key: fx["x"][key].copy() for key in GRAPH}
    out = api.update_connections(fx["t"], fx["x"], fx["uc"]["k"], first_connection=fx["uc"]["first"], parent=PARENT_FILL)
    assert_same(out, uc_expected(name), UC_OUTPUTS, name)
    assert all(np.array_equal(before[key], fx["x"][key]) for key in GRAPH)               # the caller's arrays are not written


@pytest.mark.parametrize("name", CULL_NAMES)
def test_keyframe_culling_host_form_equals_the_restatement(name):
    fx = fixture("cull", name)
    out = api.keyframe_culling(fx["t"], fx["x"], fx["cull"]["c"], fx["cull"]["monocular"], **cull_prefilled(fx))
    assert_same(out, cull_expected(name), CULL_OUTPUTS, name)


def uc_result(d, i, ci, fx):
    K, cap = fx["t"]["n_kf"], fx["x"]["row_cap"]
    counts = d["counts"][i].cpu().numpy()
    assert not counts[K:].any()                                                           # the rest of a counts row is cleared
    out = graph_of(ci, K, cap)
    out.update(counts=counts[:K], **{key: int(d[key][i]) for key in ("n_counted", "n_listed", "parent", "status")})
    return out


@pytest.mark.parametrize("names", GROUPS(UC_NAMES), ids=lambda g: g[0])
def test_update_connections_device_form_equals_the_restatement(names):
    """Up to eight maps a call, one keyframe of each; the items listed against the maps' order."""
    import torch

    fxs = [fixture("uc", n) for n in names]
    maps, covis = resident(fxs)
    order = list(range(len(fxs)))[::-1]
    d = uc_tensors([fxs[m] for m in order])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.update_connections_batch_dev(maps, covis, order, d, stream=s.cuda_stream)
    s.synchronize()
    for i, m in enumerate(order):
        out = uc_result(d, i, covis[m], fxs[m])
        assert_same(out, uc_expected(names[m]), UC_OUTPUTS, names[m])
        # the graph's kf_best is the map record's: the local map reads the refreshed rows with no copy
        assert covis[m].rec.kf_best == maps[m].rec.kf_best and np.array_equal(maps[m].t["kf_best"].cpu().numpy().reshape(-1, 10), out["kf_best"])


def test_a_second_update_of_the_same_keyframe_changes_nothing():
    """Every listed neighbour now holds (k, w): nothing of them changes, and k's rows are rewritten as they are.  No state but the graph."""
    import torch

    names = ["plain", "neighbour_other_weight", "equal_weights", "large"]
    fxs = [fixture("uc", n) for n in names]
    maps, covis = resident(fxs)
    d = uc_tensors(fxs)
    api.update_connections_batch_dev(maps, covis, range(len(fxs)), d)
    torch.cuda.synchronize()
    first = [graph_of(ci, fx["t"]["n_kf"], fx["x"]["row_cap"]) for ci, fx in zip(covis, fxs)]
    kept = {k: v.clone() for k, v in d.items()}
    api.update_connections_batch_dev(maps, covis, range(len(fxs)), d)
    torch.cuda.synchronize()
    for i, (ci, fx) in enumerate(zip(covis, fxs)):
        assert_same(graph_of(ci, fx["t"]["n_kf"], fx["x"]["row_cap"]), first[i], GRAPH, names[i])
    for k in ("counts", "n_counted", "n_listed", "status"):
        assert torch.equal(kept[k], d[k]), k
    # parent: first_connection is the caller's flag and was not cleared, so it is the same front again
    assert torch.equal(kept["parent"], d["parent"])


def cull_result(d, i, fx):
    cap, n_mp = fx["x"]["row_cap"], fx["t"]["n_mp"]
    g = lambda key: d[key][i].cpu().numpy()
    assert np.all(g("verdict")[cap:] == VERDICT_FILL) and np.all(g("n_mps")[cap:] == NMPS_FILL) and np.all(g("n_redundant")[cap:] == NRED_FILL)
    assert np.all(g("mp_turned_bad")[n_mp:] == TURNED_FILL)
    return {"verdict": g("verdict")[:cap], "n_mps": g("n_mps")[:cap], "n_redundant": g("n_redundant")[:cap], "mp_turned_bad": g("mp_turned_bad")[:n_mp],
            "n_cand": int(g("n_cand")), "status": int(g("status"))}


@pytest.mark.parametrize("names", GROUPS(CULL_NAMES), ids=lambda g: g[0])
def test_keyframe_culling_device_form_equals_the_restatement(names):
    import torch

    fxs = [fixture("cull", n) for n in names]
    maps, covis = resident(fxs)
    d = cull_tensors(fxs)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.keyframe_culling_batch_dev(maps, covis, d, stream=s.cuda_stream)
    s.synchronize()
    for i, name in enumerate(names):
        assert_same(cull_result(d, i, fxs[i]), cull_expected(name), CULL_OUTPUTS, name)


def test_culling_problems_may_share_a_map():
    """Nothing is modified, so two current keyframes of one map are two problems of one call; each sees the tables as they are."""
    import torch

    fx = fixture("cull", "long_cascade")
    other = dict(fx, cull=dict(fx["cull"], c=5))
    maps, covis = resident([fx])
    d = cull_tensors([fx, other, fx], prob_map=[0, 0, 0])
    api.keyframe_culling_batch_dev(maps, covis, d)
    torch.cuda.synchronize()
    want = cull_expected("long_cascade")
    assert_same(cull_result(d, 0, fx), want, CULL_OUTPUTS)
    assert_same(cull_result(d, 2, fx), want, CULL_OUTPUTS)
    from tests.covis_ref import KeyFrameCulling, objects
    kfs, mps = objects(fx["t"], fx["x"])
    trace = KeyFrameCulling(kfs[5], True)
    got = cull_result(d, 1, fx)
    assert got["n_cand"] == len(trace) and got["status"] == 0
    assert [(int(got["n_mps"][i]), int(got["n_redundant"][i]), got["verdict"][i] == 1) for i in range(len(trace))] == [(nm, nr, bool(c)) for _, nm, nr, c in trace]
    assert np.array_equal(np.flatnonzero(got["mp_turned_bad"] == 1), [mp.slot for mp in mps if mp.turned_bad])


def without_observation(t, x, o):
    """The tables with entry o of the observation columns taken out."""
    p = int(np.searchsorted(t["obs_ptr"], o, side="right")) - 1
    ptr = t["obs_ptr"].copy()
    ptr[p + 1:] -= 1
    cut = lambda a: np.delete(a, o)
    return (dict(t, obs_ptr=ptr, obs_kf=cut(t["obs_kf"])),
            dict(x, obs_octave=cut(x["obs_octave"]), obs_weight=cut(x["obs_weight"]), obs_idx=cut(x["obs_idx"])))


def test_update_connections_skips_and_reports_slots_outside_their_tables():
    """The device cannot be shown its tables first.  An observer outside the map is skipped and sets the bit: here it takes keyframe 3
    from 15 to 14, so nobody reaches the threshold any more.  A keyframe k outside its map does nothing at all."""
    import torch
    from tests.covis_ref import objects

    fx = fixture("uc", "fifteen_fourteen")
    t, x = fx["t"], fx["x"]
    o = int(np.flatnonzero(t["obs_kf"] == 3)[0])
    bad_t = dict(t, obs_kf=t["obs_kf"].copy())
    bad_t["obs_kf"][o] = t["n_kf"] + 2
    clean_t, clean_x = without_observation(t, x, o)
    kfs, _ = objects(clean_t, clean_x)
    counter = kfs[0].UpdateConnections()
    assert sorted((kf.addr, n) for kf, n in counter.items()) == [(1, 14), (3, 14), (4, 14)] and [kf.addr for kf in kfs[0].ord_kf] == [1]
    bad_fx, lost_fx = dict(fx, t=bad_t), dict(fx, uc=dict(fx["uc"], k=t["n_kf"]))
    maps, covis = resident([bad_fx, lost_fx])
    d = uc_tensors([bad_fx, lost_fx])
    api.update_connections_batch_dev(maps, covis, [0, 1], d)
    torch.cuda.synchronize()
    out = uc_result(d, 0, covis[0], bad_fx)
    assert (out["status"], out["n_counted"], out["n_listed"], out["parent"]) == (BAD_SLOT, 3, 1, -1) and list(out["counts"]) == [0, 14, 0, 14, 14]
    assert list(out["ord_kf"][0][:1]) == [1] and list(out["ord_w"][0][:1]) == [14] and list(out["cw_kf"][1][:1]) == [0] and out["cw_n"][3] == 0
    out = uc_result(d, 1, covis[1], lost_fx)
    assert (out["status"], out["n_counted"], out["n_listed"], out["parent"]) == (BAD_SLOT, 0, 0, PARENT_FILL) and not out["counts"].any()
    assert_same(out, x, GRAPH)


def test_keyframe_culling_skips_and_reports_slots_outside_their_tables():
    """A candidate outside the map is kept with no counts and reported; a problem naming a map the batch does not have, a current
    keyframe outside its map, or a stereo problem on a map without depth columns has no candidates and the bit."""
    import torch

    fx = fixture("cull", "ninety_percent")
    x = fx["x"]
    bad_x = dict(x, ord_kf=x["ord_kf"].copy(), ord_n=x["ord_n"].copy())
    bad_x["ord_kf"][0, :3], bad_x["ord_n"][0] = [1, 99, 2], 3
    a, b = dict(fx, x=bad_x), dict(fx, cull=dict(fx["cull"], c=-4))
    no_depth = dict(fx, x=dict(x, kf_depth=None, kf_th_depth=None), cull=dict(fx["cull"], monocular=False))
    maps, covis = resident([a, no_depth])
    d = cull_tensors([a, b, fx, no_depth], prob_map=[0, 0, 7, 1])
    api.keyframe_culling_batch_dev(maps, covis, d)
    torch.cuda.synchronize()
    out = cull_result(d, 0, a)
    assert (out["n_cand"], out["status"]) == (3, BAD_SLOT)
    assert list(out["verdict"][:3]) == [0, 0, 1] and list(out["n_mps"][:3]) == [10, 0, 10] and list(out["n_redundant"][:3]) == [9, 0, 10]
    pre = cull_prefilled(fx)
    for i, f in ((1, b), (2, fx), (3, no_depth)):
        out = cull_result(d, i, f)
        assert (out["n_cand"], out["status"]) == (0, BAD_SLOT), i
        assert_same(out, pre, ("verdict", "n_mps", "n_redundant", "mp_turned_bad"), str(i))
