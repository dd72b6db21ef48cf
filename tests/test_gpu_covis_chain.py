"""Local mapping feeding tracking, resident: slamit_update_connections_batch_dev and then slamit_local_map_batch_dev on one stream,
the second reading the kf_best rows the first has just refreshed (they are the same memory), against the same two steps through the
host forms and against the two restatements, list for list.  The frames are chosen so that the refreshed rows change the answer."""
import numpy as np
import pytest

from tests.covis_fixtures import fixture
from tests.covis_host import uc_expected, uc_tensors
from tests.local_map_host import batch_tensors
from tests.local_map_ref import update_local_map
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

NAMES = ("plain", "first_other")
FRAMES = ((0, 0), (1, 1), (0, 12))          # (map, the keyframe whose points the frame tracks)


def test_the_refreshed_covisibility_feeds_the_local_map_on_one_stream():
    import torch

    fxs = [fixture("uc", n) for n in NAMES]
    frames = []
    for m, kf in FRAMES:
        t = fxs[m]["t"]
        frames.append({"map": m, "frame_mp": t["kf_mp"][t["kf_mp_ptr"][kf]:t["kf_mp_ptr"][kf + 1]].copy(), "frame_seen": np.zeros(0, np.int32),
                       "local_kf": np.zeros(0, np.int32), "ref_kf": -1})
    tables = [fx["t"] for fx in fxs]
    # ---- the host forms, step by step, and the restatements
    want, stale = [], []
    for fr in frames:
        fx, name = fxs[fr["map"]], NAMES[fr["map"]]
        g = api.update_connections(fx["t"], fx["x"], fx["uc"]["k"], first_connection=fx["uc"]["first"])
        assert np.array_equal(g["kf_best"], uc_expected(name)["kf_best"])
        fresh = dict(fx["t"], kf_best=g["kf_best"])
        k = api.local_keyframes(fresh, fr["frame_mp"], kf_cap=96)
        p = api.local_points(fresh, k["frame_mp"], k["local_kf"], q_cap=512)
        r = update_local_map(fresh, fr)
        assert np.array_equal(k["local_kf"], r["local_kf"]) and np.array_equal(p["local_mp"][:p["n_local_mp"]], r["local_mp"]) and k["ref_kf"] == r["ref_kf"]
        want.append((k, p))
        stale.append(update_local_map(fx["t"], fr))
    assert any(not np.array_equal(s["local_kf"], k["local_kf"]) for s, (k, _) in zip(stale, want))      # the refresh matters
    # ---- resident: one stream, no host visit between the calls
    d, maps = batch_tensors({"frames": frames, "maps": tables, "kf_cap": 96, "q_cap": 512})
    covis = [api.CovisIndex(fx["x"], mi) for fx, mi in zip(fxs, maps)]
    u = uc_tensors(fxs)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        api.update_connections_batch_dev(maps, covis, range(len(fxs)), u, stream=st.cuda_stream)
        api.local_map_batch_dev(maps, d, stream=st.cuda_stream)
    st.synchronize()
    assert not u["status"].any()
    for f, (k, p) in enumerate(want):
        n, m = k["n_local_kf"], p["n_local_mp"]
        assert int(d["n_local_kf"][f]) == n and np.array_equal(d["local_kf"][f, :n].cpu().numpy(), k["local_kf"]) and int(d["ref_kf"][f]) == k["ref_kf"]
        assert int(d["n_local_mp"][f]) == m and np.array_equal(d["local_mp"][f, :m].cpu().numpy(), p["local_mp"][:m])
        assert np.array_equal(d["skip"][f, :m].cpu().numpy(), p["skip"][:m]) and np.array_equal(d["votes"][f, :len(k["votes"])].cpu().numpy(), k["votes"])
