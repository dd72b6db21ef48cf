"""Map-point upkeep on the GPU: the host forms and the resident forms of slamit_update_points and slamit_map_point_culling equal the
restatement (tests/upkeep_ref.py) on every fixture, bit for bit; in / out arrays keep what lies past their counts; a batch over several
maps with a different `what` per item; slots outside their tables; one case at each ceiling."""
import functools

import numpy as np
import pytest

from tests.upkeep_fixtures import CULL_LENGTHS, CUR_ID, cull_map, small_map, up_map
from tests.upkeep_host import (BAD_SLOT, CULL_OUTPUTS, KEPT_FILL, PLANES, UP_OUTPUTS, VERDICT_FILL, assert_same, cull_expected, cull_tensors, planes_of,
                               resident, up_expected, up_tensors)
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected(name, what):
    fx = up_map()
    return up_expected(fx["t"], fx["x"], fx["lists"][name], what)


@pytest.mark.parametrize("what", [1, 2, 3])
@pytest.mark.parametrize("name", ["all", "twice", "reversed", "empty"])
def test_update_points_host_form_equals_the_restatement(name, what):
    fx = up_map()
    before = {k: fx["x"][k].copy() for k in PLANES}
    got = api.update_points(fx["t"], fx["x"], fx["lists"][name], what)
    assert_same(got, expected(name, what), UP_OUTPUTS, "%s what=%d" % (name, what))
    assert all(np.array_equal(before[k], fx["x"][k]) for k in PLANES)                       # the caller's arrays are not modified
    if name == "all" and what == 3:
        assert {0, 1, 2, 5, 8, 16, 32} <= set(got["status"].tolist())                        # every status bit a table can produce


def test_update_points_host_form_on_the_small_map():
    fx = small_map()
    for what in (1, 2, 3):
        assert_same(api.update_points(fx["t"], fx["x"], fx["lists"]["all"], what), up_expected(fx["t"], fx["x"], fx["lists"]["all"], what), UP_OUTPUTS)


@pytest.mark.parametrize("mono", [True, False])
@pytest.mark.parametrize("n", CULL_LENGTHS)
def test_map_point_culling_host_form_equals_the_restatement(n, mono):
    cm = cull_map()
    recent = cm["lists"][n]
    got = api.map_point_culling(cm["t"], cm["x"], CUR_ID, mono, recent, verdict=np.full(n, VERDICT_FILL, np.uint8), kept=np.full(n, KEPT_FILL, np.int32))
    assert_same(got, cull_expected(cm["t"], cm["x"], recent, CUR_ID, mono), CULL_OUTPUTS, "n=%d" % n)


def test_update_points_resident_batch_over_maps_with_a_what_per_item():
    import torch

    fxs = [up_map(), small_map()]
    um, sm = fxs
    items = [(0, um["lists"]["all"], 3), (1, sm["lists"]["all"], 1), (0, um["lists"]["twice"], 2), (1, [1, 3], 2), (0, [], 3),
             (0, [0, um["t"]["n_mp"], -1, 2 ** 31 - 1, 4], 1), (1, [0, 1], 3)]
    item_map = [m for m, _, _ in items]
    item_map[-1] = 2                                                                        # a map outside the batch's
    maps, pts = resident(fxs)
    d = up_tensors(items, item_map=item_map)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        api.update_points_batch_dev(maps, pts, d, stream=st.cuda_stream)
    st.synchronize()
    status = d["status"].cpu().numpy()
    # every item writes what the restatement writes, and items that share a point write the same bytes: apply them one after the other
    xs = [dict(fx["x"]) for fx in fxs]
    for i, (m, points, what) in enumerate(items):
        if item_map[i] == 2:
            want = np.full(len(points), BAD_SLOT, np.int32)
        else:
            e = up_expected(fxs[m]["t"], xs[m], points, what)
            xs[m].update({k: e[k] for k in PLANES})
            want = e["status"]
        assert np.array_equal(status[i, :len(points)], want) and (status[i, len(points):] == -9).all(), i
    for m, fx in enumerate(fxs):
        assert_same(planes_of(pts[m], fx["t"]["n_mp"]), xs[m], PLANES, "map %d" % m)
    assert pts[0].t["mp_normal"].data_ptr() == maps[0].t["mp_normal"].data_ptr()            # the planes the local map gathers


def test_map_point_culling_resident_batch():
    import torch

    fxs = [cull_map(), small_map()]
    cm, sm = fxs
    lists = [(0, cm["lists"][n], CUR_ID, mono) for n in CULL_LENGTHS for mono in (True, False)]
    lists += [(1, [3, 2, 1, 0], 2, False), (0, [5, cm["t"]["n_mp"], 9, -1, 11], CUR_ID, True), (1, [0, 1], 2, True)]
    list_map = [m for m, _, _, _ in lists]
    list_map[-1] = -1
    maps, pts = resident(fxs)
    d = cull_tensors(lists, list_map=list_map)
    cap = d["recent"].shape[1]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        api.map_point_culling_batch_dev(maps, pts, d, stream=st.cuda_stream)
    st.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    for i, (m, recent, cur, mono) in enumerate(lists):
        got = {"verdict": h["verdict"][i], "kept": h["kept"][i], "n_kept": int(h["n_kept"][i]), "status": int(h["status"][i])}
        if list_map[i] == -1:
            e = dict(cull_expected(fxs[m]["t"], fxs[m]["x"], [], cur, mono, cap), status=BAD_SLOT)
        else:
            inside = [p for p in recent if 0 <= p < fxs[m]["t"]["n_mp"]]
            e = cull_expected(fxs[m]["t"], fxs[m]["x"], inside, cur, mono, cap)
            if len(inside) != len(recent):                                                  # the entries outside keep their byte and are dropped
                v = np.full(cap, VERDICT_FILL, np.uint8)
                v[[j for j, p in enumerate(recent) if 0 <= p < fxs[m]["t"]["n_mp"]]] = e["verdict"][:len(inside)]
                e = dict(e, verdict=v, status=BAD_SLOT)
        assert_same(got, e, CULL_OUTPUTS, "list %d" % i)


def test_the_list_ceilings():
    """SLAMIT_UPKEEP_MAX_POINTS listed points and SLAMIT_UPKEEP_MAX_RECENT recent entries, host and resident; one more is refused.  (The
    ceiling on observers and the one past it are the fixtures `ceiling` and `above_ceiling`.)"""
    import torch

    sm, cm = small_map(), cull_map()
    n = api.UPKEEP_MAX_POINTS
    points = np.resize(np.array(sm["lists"]["all"], np.int32), n)
    e = up_expected(sm["t"], sm["x"], sm["lists"]["all"], 3)
    want = np.resize(e["status"], n)
    got = api.update_points(sm["t"], sm["x"], points, 3)
    assert np.array_equal(got["status"], want)
    assert_same(got, e, PLANES)
    maps, pts = resident([sm])
    d = up_tensors([(0, points, 3)], pad=0)
    api.update_points_batch_dev(maps, pts, d)
    torch.cuda.synchronize()
    assert np.array_equal(d["status"].cpu().numpy()[0], want)
    assert_same(planes_of(pts[0], sm["t"]["n_mp"]), e, PLANES)
    with pytest.raises(api.SlamitError, match="SLAMIT_UPKEEP_MAX_POINTS"):
        api.update_points(sm["t"], sm["x"], np.resize(points, n + 1), 3)
    with pytest.raises(api.SlamitError, match="SLAMIT_UPKEEP_MAX_POINTS"):
        api.update_points_batch_dev(maps, pts, up_tensors([(0, points, 3)], pad=1))
    # culling: every point's verdict once through the restatement, laid over the long list
    n = api.UPKEEP_MAX_RECENT
    n_mp = cm["t"]["n_mp"]
    per_point = cull_expected(cm["t"], cm["x"], list(range(n_mp)), CUR_ID, False)["verdict"]
    recent = np.resize(np.random.default_rng(5).permutation(n_mp).astype(np.int32), n)
    verdict = per_point[recent]
    kept = recent[verdict == 0]
    got = api.map_point_culling(cm["t"], cm["x"], CUR_ID, False, recent, kept=np.full(n, KEPT_FILL, np.int32))
    assert np.array_equal(got["verdict"], verdict) and got["n_kept"] == len(kept) and np.array_equal(got["kept"][:len(kept)], kept)
    assert (got["kept"][len(kept):] == KEPT_FILL).all() and got["status"] == 0
    cmaps, cpts = resident([cm])
    d = cull_tensors([(0, recent, CUR_ID, False)], pad=0)
    api.map_point_culling_batch_dev(cmaps, cpts, d)
    torch.cuda.synchronize()
    assert np.array_equal(d["verdict"].cpu().numpy()[0], verdict) and int(d["n_kept"][0]) == len(kept)
    assert np.array_equal(d["kept"].cpu().numpy()[0, :len(kept)], kept) and (d["kept"].cpu().numpy()[0, len(kept):] == KEPT_FILL).all()
    with pytest.raises(api.SlamitError, match="SLAMIT_UPKEEP_MAX_RECENT"):
        api.map_point_culling(cm["t"], cm["x"], CUR_ID, False, np.resize(recent, n + 1))
    with pytest.raises(api.SlamitError, match="SLAMIT_UPKEEP_MAX_RECENT"):
        api.map_point_culling_batch_dev(cmaps, cpts, cull_tensors([(0, recent, CUR_ID, False)], pad=1))
