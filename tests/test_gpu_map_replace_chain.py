"""A fuse pass between resident steps, on one stream with no host visit: slamit_map_replace_batch_dev applies a list of Replace and
AddObservation ops, EditIndex.swap() exchanges the buffer sets (the ReplaceIndex follows), slamit_update_points_batch_dev runs on
`touched`, slamit_update_connections_batch_dev, slamit_check_replaced_batch_dev on a frame's list and slamit_local_map_batch_dev read
the new map.  Everything must equal the same calls over tables that the restatement (tests/map_replace_ref.py) rebuilt on the host and
that were uploaded afresh."""
import numpy as np
import pytest

from tests.map_replace_host import records
from tests.map_replace_ref import ADD_OBS, REPLACE, apply
from tests.test_gpu_map_edit_chain import N_KF, N_OLD, covis_of, covis_tensors, local_map_tensors, points_tensors, read, same, the_map

pytestmark = pytest.mark.gpu


def the_list(t, x):
    rng = np.random.default_rng(2701)
    pts = rng.permutation(N_OLD)[:40].tolist()
    ops = [(REPLACE, pts[2 * i], pts[2 * i + 1], 0, 0, 0) for i in range(14)]
    ops += [(REPLACE, pts[1], pts[3], 0, 0, 0), (REPLACE, pts[3], pts[5], 0, 0, 0), (REPLACE, pts[0], pts[30], 0, 0, 0)]   # a chain over two targets; a replaced source again
    for p in pts[28:40]:                                                    # keypoint 0 of every keyframe is free
        row = t["obs_kf"][t["obs_ptr"][p]:t["obs_ptr"][p + 1]].tolist()
        k = next(k for k in range(N_KF) if k not in row)
        ops.append((ADD_OBS, p, k, 0, int(x["kf_octave"][t["kf_mp_ptr"][k]]), 1))
    order = rng.permutation(len(ops))
    return [ops[i] for i in order]


def test_a_fuse_pass_between_resident_steps_on_one_stream():
    import torch
    from weiner_slamit_v2_amd import api

    t, x, _, _, frame_mp = the_map()
    n_mp, n_kfmp = t["n_mp"], len(t["kf_mp"])
    x = dict(x, mp_replaced=np.full(n_mp, -1, np.int32))
    ops = the_list(t, x)
    cap, obs_cap = len(ops) + 3, len(t["obs_kf"]) + len(ops)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    i32 = lambda *s, v=-9: torch.full(s, v, dtype=torch.int32, device="cuda")
    # ---- resident: uploaded once
    mi = api.MapIndex(t)
    pi = api.PointIndex(x, mi)
    ci = api.CovisIndex(covis_of(t, x), mi)
    ei = api.EditIndex(x, mi, obs_cap, covis=ci, points=pi)
    ri = api.ReplaceIndex(ei, x)
    assert ri.rec.mp_found == pi.rec.mp_found and ri.rec.mp_nobs == ci.rec.mp_nobs and ri.rec.kf_mp == mi.rec.kf_mp      # the very memory the other records name
    h_ops = np.zeros((1, cap, 20), np.uint8)
    h_ops[0, :len(ops)] = records(ops).view(np.uint8).reshape(-1, 20)
    r = {"ops": cu(h_ops), "n": cu(np.array([len(ops)], np.int32)), "moved": i32(1, cap), "erased": i32(1, cap), "touched": i32(1, n_mp, v=-3), "n_touched": i32(1),
         "n_obs_out": i32(1), "status": i32(1), "kfmp_cap": n_kfmp,
         "workspace": torch.full((api.map_replace_workspace(1, cap, n_mp, n_kfmp),), 0x5a, dtype=torch.uint8, device="cuda")}
    d, u, c = local_map_tensors(frame_mp, n_mp), points_tensors(n_mp, r["touched"], r["n_touched"]), covis_tensors(0)
    chk = {"frame_mp": d["frame_mp"], "frame_map": d["frame_map"], "n": d["n"], "status": i32(1)}
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        api.map_replace_batch_dev([mi], [ri], r, stream=s)
        before = ri.rec.obs_idx
        ei.swap()
        assert ri.rec.obs_idx != before and ri.rec.obs_idx == ei.rec.obs_idx and mi.rec.obs_kf == ei.sets[0]["obs_kf"].data_ptr()   # one swap repoints every record
        api.update_points_batch_dev([mi], [pi], u, stream=s)
        api.update_connections_batch_dev([mi], [ci], [0], c, stream=s)
        api.check_replaced_batch_dev([ri.t["mp_replaced"]], chk, n_mp=[n_mp], stream=s)
        api.local_map_batch_dev([mi], d, stream=s)
    st.synchronize()
    got = read(d, u, c, ci, mi, pi)
    assert int(r["status"][0]) == 0 and int(chk["status"][0]) == 0
    # ---- the same with the tables rebuilt on the host by the restatement and uploaded afresh
    a = apply(t, x, ops, obs_cap)
    assert a["status"] == 0 and a["n_touched"] > 10 and a["erased"].sum() > 0 and a["moved"].sum() > 20 and "replace_of_replaced" in a["events"]
    tables = dict(t, obs_ptr=a["obs_ptr"], obs_kf=a["obs_kf"], mp_bad=a["mp_bad"], kf_mp=a["kf_mp"])
    cols = dict(x, **{k: a[k] for k in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_found", "mp_visible", "mp_replaced")})
    m2 = api.MapIndex(tables)
    p2 = api.PointIndex(cols, m2)
    q2 = api.CovisIndex(covis_of(tables, cols), m2)
    h_t = np.full((1, n_mp), -3, np.int32)
    h_t[0, :a["n_touched"]] = a["touched"]
    u2 = points_tensors(n_mp, cu(h_t), cu(np.array([a["n_touched"]], np.int32)))
    d2, c2 = local_map_tensors(frame_mp, n_mp), covis_tensors(0)
    chk2 = {"frame_mp": d2["frame_mp"], "frame_map": d2["frame_map"], "n": d2["n"], "status": i32(1)}
    api.update_points_batch_dev([m2], [p2], u2)
    api.update_connections_batch_dev([m2], [q2], [0], c2)
    api.check_replaced_batch_dev([cu(a["mp_replaced"])], chk2)
    api.local_map_batch_dev([m2], d2)
    torch.cuda.synchronize()
    same(got, read(d2, u2, c2, q2, m2, p2), "the fuse pass")
    # the pass did something that the readers saw: the frame held replaced points, which gave way to their replacements
    replaced = set(np.flatnonzero(a["mp_replaced"] >= 0).tolist())
    assert replaced & set(frame_mp.tolist()) and not replaced & set(got["local_mp"].tolist())
    hop = np.where(a["mp_replaced"][frame_mp] >= 0, a["mp_replaced"][frame_mp], frame_mp)
    assert np.array_equal(np.where(got["frame_mp"] >= 0, got["frame_mp"], hop), hop) and np.any(hop != frame_mp)
    # and the tables every reader now takes are the restatement's
    n_obs = int(tables["obs_ptr"][-1])
    assert np.array_equal(mi.t["obs_ptr"].cpu().numpy()[:n_mp + 1], tables["obs_ptr"]) and np.array_equal(mi.t["obs_kf"].cpu().numpy()[:n_obs], tables["obs_kf"])
    assert np.array_equal(mi.t["kf_mp"].cpu().numpy()[:n_kfmp], tables["kf_mp"]) and np.array_equal(ci.t["mp_nobs"].cpu().numpy()[:n_mp], cols["mp_nobs"])
    for key in ("mp_found", "mp_visible", "mp_replaced"):
        assert np.array_equal(ri.t[key].cpu().numpy()[:n_mp], cols[key]), key
    assert np.array_equal(pi.t["mp_found"].cpu().numpy()[:n_mp], cols["mp_found"]) and np.array_equal(r["moved"][0, :len(ops)].cpu().numpy(), a["moved"])
