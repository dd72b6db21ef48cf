"""slamit_local_keyframes, slamit_local_points and slamit_local_map_batch_dev on the device against the restatement
(tests/local_map_ref.py) on every fixture.

Everything is integer work or a copy of a stored float: the results are equal EXACTLY, the gathered planes as raw bits, and
entries past a count are still what the caller put there."""
import numpy as np
import pytest

from tests.local_map_fixtures import NAMES, fixture
from tests.local_map_host import MP_FILL, OUTPUTS, PLANE_FILL, SKIP_FILL, assert_same, batch_tensors, expected, frame_result, prefilled
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

FRAMES = [(name, i) for name in NAMES for i in range(len(fixture(name)["frames"]))]


@pytest.mark.parametrize("name,i", FRAMES)
def test_host_forms_equal_the_restatement(name, i):
    fx = fixture(name)
    fr = fx["frames"][i]
    t, e = fx["maps"][fr["map"]], expected(name, i)
    k = api.local_keyframes(t, fr["frame_mp"], local_kf=fr["local_kf"], ref_kf=fr["ref_kf"], kf_cap=fx["kf_cap"])
    nk = min(e["n_local_kf"], fx["kf_cap"])
    assert_same(k, dict(e, local_kf=e["local_kf"][:nk], status=e["status"] & 2), ("votes", "frame_mp", "local_kf", "n_local_kf", "ref_kf", "status"), name)
    p = api.local_points(t, k["frame_mp"], k["local_kf"], frame_seen=fr["frame_seen"], q_cap=fx["q_cap"], fill=MP_FILL)
    assert_same(p, dict(e, status=e["status"] & 4), ("local_mp", "skip", "n_local_mp", "status"), name)
    assert np.all(p["local_mp"][e["m"]:] == MP_FILL) and np.all(p["skip"][e["m"]:] == SKIP_FILL)


@pytest.mark.parametrize("name", NAMES)
def test_device_form_equals_the_restatement(name):
    import torch

    fx = fixture(name)
    d, maps = batch_tensors(fx)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.local_map_batch_dev(maps, d, stream=s.cuda_stream)
    s.synchronize()
    for f, fr in enumerate(fx["frames"]):
        e = expected(name, f)
        out = frame_result(d, f, len(fr["frame_mp"]), fx["maps"][fr["map"]]["n_kf"])
        assert_same(out, e, OUTPUTS + ("m",), "%s[%d]" % (name, f))
        # past the count: the caller's sentinels, in every plane
        m = e["m"]
        assert np.all(out["local_mp"][m:] == MP_FILL) and np.all(out["skip"][m:] == SKIP_FILL)
        for key in ("pos", "normal", "max_dist", "min_dist"):
            assert np.all(out[key].view(np.uint32)[..., m:] == PLANE_FILL), key


def test_a_second_call_on_the_same_workspace_is_the_same():
    """No state: the workspace is cleared by the call, so the arrays of one call are the next call's inputs and nothing else is."""
    import torch

    fx = fixture("three_frames_two_maps")
    d, maps = batch_tensors(fx)
    api.local_map_batch_dev(maps, d)
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in d.items() if hasattr(v, "clone") and k != "workspace"}
    api.local_map_batch_dev(maps, d)                                   # frame_mp is already clean, the lists are already these
    torch.cuda.synchronize()
    raw = lambda a: a.view(torch.int32) if a.dtype == torch.float32 else a   # the planes' sentinel is a NaN pattern: compare bits
    for k, v in first.items():
        assert torch.equal(raw(v), raw(d[k])), k


def test_slots_outside_their_tables_are_skipped_and_reported():
    """The device cannot be shown its tables first.  A slot outside its table -- in the frame, in frame_seen, in an observer list, a
    neighbour list, a keyframe's points -- is skipped and sets the status bit; a frame naming a map the batch does not have is left
    alone.  Everything else is what the restatement gives with those entries absent."""
    import torch

    from tests.local_map_ref import update_local_map

    fx = fixture("plain")
    t, fr = fx["maps"][0], fx["frames"][0]
    n_kf, n_mp = t["n_kf"], t["n_mp"]
    live = np.flatnonzero(fr["frame_mp"] >= 0)
    bad_mp, bad_seen = fr["frame_mp"].copy(), fr["frame_seen"].copy()
    bad_mp[live[0]], bad_mp[live[1]] = n_mp, -5
    bad_seen[0] = 2 ** 30
    voted = int(expected("plain")["lists"]["local_kf"][0])
    bad_t = dict(t, obs_kf=t["obs_kf"].copy(), kf_best=t["kf_best"].copy(), kf_mp=t["kf_mp"].copy(), kf_child=t["kf_child"].copy())
    bad_t["obs_kf"][[0, 7]] = n_kf, -1
    bad_t["kf_best"][voted, 0] = n_kf + 7
    bad_t["kf_mp"][t["kf_mp_ptr"][voted] + np.flatnonzero(t["kf_mp"][t["kf_mp_ptr"][voted]:t["kf_mp_ptr"][voted + 1]] >= 0)[0]] = n_mp + 5
    # the same with those entries absent: what the restatement can be asked
    clean_mp, clean_seen = np.where((bad_mp < 0) | (bad_mp >= n_mp), -1, bad_mp), np.where(bad_seen >= n_mp, -1, bad_seen)
    obs = [[k for k in bad_t["obs_kf"][t["obs_ptr"][p]:t["obs_ptr"][p + 1]] if 0 <= k < n_kf] for p in range(n_mp)]
    clean_t = dict(bad_t, obs_ptr=np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32), obs_kf=np.array([k for o in obs for k in o], np.int32),
                   kf_best=np.where(bad_t["kf_best"] >= n_kf, -1, bad_t["kf_best"]), kf_mp=np.where(bad_t["kf_mp"] >= n_mp, -1, bad_t["kf_mp"]))
    want = update_local_map(clean_t, dict(fr, frame_mp=clean_mp, frame_seen=clean_seen))
    frames = [dict(fr, frame_mp=bad_mp, frame_seen=bad_seen), dict(fr)]
    d, maps = batch_tensors(fx, frames=frames, tables=[bad_t], frame_map=[0, 5])
    api.local_map_batch_dev(maps, d)
    torch.cuda.synchronize()
    out = frame_result(d, 0, len(bad_mp), n_kf)
    assert out["status"] == api.LOCAL_MAP_STATUS["BAD_SLOT"]
    kept = np.where(want["frame_mp"] != clean_mp, -1, bad_mp)          # a bad point becomes -1; a slot outside the table stays as it came
    assert np.array_equal(out["frame_mp"], kept) and np.array_equal(out["votes"], want["votes"])
    assert out["n_local_kf"] == want["n_local_kf"] and np.array_equal(out["local_kf"][:want["n_local_kf"]], want["local_kf"]) and out["ref_kf"] == want["ref_kf"]
    assert out["n_local_mp"] == want["n_local_mp"] == out["m"] and np.array_equal(out["local_mp"][:out["m"]], want["local_mp"])
    assert np.array_equal(out["skip"][:out["m"]], want["skip"])
    assert np.array_equal(out["pos"].view(np.uint32)[:, :out["m"]], t["mp_pos"][want["local_mp"]].T.view(np.uint32))
    # the frame of the unknown map: its lists as they were, no points, the bit
    pre = prefilled(dict(fx, frames=frames), 1)
    other = frame_result(d, 1, len(fr["frame_mp"]), 0)
    assert other["status"] == api.LOCAL_MAP_STATUS["BAD_SLOT"] and other["n_local_mp"] == 0 and other["m"] == 0
    assert np.array_equal(other["frame_mp"], fr["frame_mp"]) and np.array_equal(other["local_kf"], pre["local_kf"])
    assert (other["n_local_kf"], other["ref_kf"]) == (pre["n_local_kf"], pre["ref_kf"]) and np.all(other["local_mp"] == MP_FILL)
