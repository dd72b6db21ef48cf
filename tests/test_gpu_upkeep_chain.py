"""Local mapping feeding tracking, resident: some points move, slamit_update_points_batch_dev refreshes their normals and distances,
and slamit_local_map_batch_dev and slamit_frustum_batch_dev follow on the same stream with no host visit.  The gathered planes and the
frustum results must be those of a map whose planes the restatement (tests/upkeep_ref.py) refreshed, and must differ from the stale
ones: the chain reads the memory the update wrote."""
import numpy as np
import pytest

from tests import frustum_ref as fru
from tests.local_map_fixtures import fixture
from tests.local_map_host import batch_tensors, expected
from tests.upkeep_host import PLANES, bits, columns_for, up_expected, up_tensors
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

NAME = "three_frames_two_maps"


def with_geometry(t, g):
    idx = np.arange(t["n_mp"]) % len(g["pos"])
    return dict(t, mp_pos=g["pos"][idx].copy(), mp_normal=g["normal"][idx].copy(), mp_max_dist=g["max_dist"][idx].copy(), mp_min_dist=g["min_dist"][idx].copy())


def test_the_refreshed_planes_feed_the_local_map_and_the_frustum_on_one_stream():
    import torch

    g = fru.fixture(fru.MIXED)
    fx = fixture(NAME)
    rng = np.random.default_rng(31)
    tables, xs, moved, fresh = [], [], [], []
    for m, t in enumerate(fx["maps"]):
        t = with_geometry(t, g)
        which = np.flatnonzero(rng.random(t["n_mp"]) < 0.4).astype(np.int32)                # the points local BA moved
        t["mp_pos"][which] += rng.uniform(-0.3, 0.3, (len(which), 3)).astype(np.float32)
        x = columns_for(t, 40 + m)
        e = up_expected(t, x, which, 3)
        assert not e["status"].any() and len(which) > 10
        tables.append(t); xs.append(x); moved.append(which)
        fresh.append(dict(t, **{k: e[k] for k in PLANES[:3]}))
    # ---- what the chain must give, frame by frame: the restatement's list over the refreshed planes, and over the stale ones
    want, stale = [], []
    for f, fr in enumerate(fx["frames"]):
        ids, skip = expected(NAME, f)["lists"]["local_mp"], expected(NAME, f)["lists"]["skip"]
        for src, dst in ((fresh, want), (tables, stale)):
            t = src[fr["map"]]
            pr = dict(g, n=len(ids), pos=t["mp_pos"][ids], normal=t["mp_normal"][ids], max_dist=t["mp_max_dist"][ids], min_dist=t["mp_min_dist"][ids], skip=skip)
            dst.append((ids, pr, api.frustum(pr)))
    # ---- resident: the maps are uploaded with the moved positions and the STALE planes
    d, maps = batch_tensors(dict(fx, maps=tables), tables=tables)
    pts = [api.PointIndex(x, mi) for x, mi in zip(xs, maps)]
    u = up_tensors([(m, which, 3) for m, which in enumerate(moved)])
    B, q_cap = len(fx["frames"]), fx["q_cap"]
    frames = np.zeros(B, api.FRUSTUM_FRAME_DTYPE)
    frames[:] = api.frustum_frame_record(g)[0]
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    fr_t = dict(frames=torch.from_numpy(frames.view(np.float32).reshape(B, -1)).cuda(), m=d["m"], pos=d["pos"], normal=d["normal"], max_dist=d["max_dist"],
                min_dist=d["min_dist"], skip=d["skip"], uvr=torch.full((B, q_cap, 3), -7.0, device="cuda"), level_min=i32(B, q_cap), level_max=i32(B, q_cap),
                valid=torch.full((B, q_cap), 7, dtype=torch.uint8, device="cuda"), status=torch.full((B, q_cap), 99, dtype=torch.uint8, device="cuda"))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        api.update_points_batch_dev(maps, pts, u, stream=st.cuda_stream)
        api.local_map_batch_dev(maps, d, stream=st.cuda_stream)
        api.frustum_batch_dev(fr_t, stream=st.cuda_stream)
    st.synchronize()
    for m, which in enumerate(moved):
        assert not u["status"][m, :len(which)].any()
    planes_differ = results_differ = 0
    for f, ((ids, pr, out), (_, spr, sout)) in enumerate(zip(want, stale)):
        n = len(ids)
        assert int(d["m"][f]) == n and np.array_equal(d["local_mp"][f, :n].cpu().numpy(), ids)
        for key, a in (("pos", pr["pos"].T), ("normal", pr["normal"].T)):
            assert np.array_equal(bits(d[key][f, :, :n].cpu().numpy()), bits(a)), (f, key)
        for key in ("max_dist", "min_dist"):
            assert np.array_equal(bits(d[key][f, :n].cpu().numpy()), bits(pr[key])), (f, key)
        status, valid = fr_t["status"][f, :n].cpu().numpy(), fr_t["valid"][f, :n].cpu().numpy()
        assert np.array_equal(status, out["status"]) and np.array_equal(valid, out["valid"])
        assert np.array_equal(bits(fr_t["uvr"][f, :n].cpu().numpy()), bits(out["uvr"]))
        assert np.array_equal(fr_t["level_min"][f, :n].cpu().numpy(), out["level_min"]) and np.array_equal(fr_t["level_max"][f, :n].cpu().numpy(), out["level_max"])
        planes_differ += int(not np.array_equal(bits(d["normal"][f, :, :n].cpu().numpy()), bits(spr["normal"].T)))
        results_differ += int((status != sout["status"]).sum())
    assert planes_differ > 0 and results_differ > 0                                         # the chain read the refreshed memory
