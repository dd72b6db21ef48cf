"""Loop correction feeding map-point upkeep, resident: slamit_essential_graph_dev writes the corrected positions INTO the map's own mp_pos
plane and leaves `touched` / `n_touched`; slamit_update_points_batch_dev follows on the same stream with those two as its point list and
count (UpdateNormalAndDepth, Optimizer.cc:1042), no host visit between them.  The planes must be those of the host sequence --
api.essential_graph, then api.update_points over its `touched` on a map holding its points -- bit for bit, and must differ from the stale
ones: the update read the positions the optimisation wrote."""
import numpy as np
import pytest

from tests.essential_host import OUT_KEYS, dev_tensors
from tests.test_gpu_essential import golden
from tests.upkeep_fixtures import up_map
from tests.upkeep_host import PLANES, bits, planes_of, resident
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

NORMAL = 1   # SLAMIT_UPKEEP_NORMAL


def test_corrected_points_feed_update_normal_and_depth_on_one_stream():
    import torch

    fx = up_map()
    t, x = fx["t"], fx["x"]
    n_mp = int(t["n_mp"])
    # the loop closure of eg_mixed40 over THIS map's points: every point hangs on one of the graph's good keyframes
    g = golden("eg_mixed40")
    good_kf = np.flatnonzero(g["bad"] == 0)
    g["pt_pos"] = np.ascontiguousarray(t["mp_pos"], np.float32).reshape(n_mp, 3).copy()
    g["pt_bad"] = np.ascontiguousarray(t["mp_bad"], np.uint8).copy()
    g["pt_ref"] = good_kf[np.arange(n_mp) % len(good_kf)].astype(np.int32)
    assert g["pt_bad"].any() and not g["pt_bad"].all()

    # ---- the host sequence ----
    r = api.essential_graph(g)
    moved = dict(t, mp_pos=r["points"].reshape(np.shape(t["mp_pos"])))
    want = api.update_points(moved, x, r["touched"], NORMAL)
    stale = api.update_points(t, x, r["touched"], NORMAL)
    assert len(r["touched"]) == int((g["pt_bad"] == 0).sum()) and np.abs(r["points"] - g["pt_pos"]).max() > 1e-3

    # ---- resident: one stream, the map's plane is the optimisation's output ----
    maps, pts = resident([fx])
    d, nf = dev_tensors(g)
    d["points"] = maps[0].t["mp_pos"]                                                       # corrected in place (pt_pos is a copy)
    assert d["points"].numel() == 3 * n_mp and d["pt_pos"].data_ptr() != d["points"].data_ptr()
    u = dict(item_map=torch.zeros(1, dtype=torch.int32, device="cuda"), what=torch.full((1,), NORMAL, dtype=torch.int32, device="cuda"),
             n=d["n_touched"], points=d["touched"].view(1, n_mp), status=torch.full((1, n_mp), -9, dtype=torch.int32, device="cuda"))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        api.essential_graph_dev(d, nf, int(g["fix_scale"]), int(g["max_its"]), float(g["lambda_init"]), stream=st.cuda_stream)
        api.update_points_batch_dev(maps, pts, u, stream=st.cuda_stream)
    st.synchronize()
    k = len(r["touched"])
    assert int(d["n_touched"].cpu()[0]) == k and np.array_equal(d["touched"].cpu().numpy()[:k], r["touched"])
    assert np.array_equal(bits(maps[0].t["mp_pos"].cpu().numpy().reshape(n_mp, 3)), bits(r["points"]))
    status = u["status"].cpu().numpy()[0]
    assert np.array_equal(status[:k], want["status"]) and (status[k:] == -9).all()
    got = planes_of(pts[0], n_mp)
    differ = 0
    for key in PLANES[:3]:
        assert np.array_equal(bits(got[key]), bits(np.asarray(want[key]).reshape(got[key].shape))), key
        differ += int(not np.array_equal(bits(got[key]), bits(np.asarray(stale[key]).reshape(got[key].shape))))
    assert differ > 0                                                                       # the update read the corrected positions
