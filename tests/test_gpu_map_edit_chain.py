"""Two resident steps with the map changed in between, on one stream with no host visit: slamit_map_point_culling_batch_dev gives
verdicts, a few torch ops turn verdicts 2 and 3 into SET_BAD edits, slamit_map_edit_batch_dev applies them, EditIndex.swap() exchanges
the buffer sets, slamit_update_points_batch_dev runs on `touched` and slamit_local_map_batch_dev reads the new map.  A second round adds
observations into pre-allotted empty point slots (what CreateNewMapPoints produces) and slamit_update_connections_batch_dev follows.
Everything must equal the same calls over tables that the restatement (tests/map_edit_ref.py) rebuilt on the host and that were uploaded
afresh."""
import numpy as np
import pytest

from tests.map_edit_host import records
from tests.map_edit_ref import ADD_OBS, MATCH, SET_BAD, apply
from tests.upkeep_fixtures import build_map
from tests.upkeep_host import bits

pytestmark = pytest.mark.gpu
N_KF, N_OLD, N_NEW, CUR_ID, ROW_CAP, KF_CAP, Q_CAP = 12, 120, 6, 10, 16, 96, 256
PLANES = ("mp_normal", "mp_max_dist", "mp_min_dist")


def the_map():
    rng = np.random.default_rng(2601)
    points = []
    for p in range(N_OLD):
        obs = rng.permutation(N_KF)[:2 if p % 7 == 0 else int(rng.integers(3, 7))].tolist()
        points.append(dict(obs=obs, ref=obs[0]))
    points += [dict(obs=[], ref=2 * i) for i in range(N_NEW)]               # allotted, unused: an empty row, the reference keyframe already named
    t, x = build_map(N_KF, points, rng)
    x["obs_weight"] = np.ones(len(t["obs_kf"]), np.uint8)
    p = np.arange(N_OLD + N_NEW)
    x["mp_found"], x["mp_visible"] = np.where(p % 5 == 0, 1, 8).astype(np.int32), np.full(len(p), 9, np.int32)   # 1 / 9 < 0.25: verdict 2
    x["mp_first_kf"] = np.where(p % 7 == 0, CUR_ID - 2, CUR_ID).astype(np.int32)                                  # age 2 with two observers: verdict 3
    recent = rng.permutation(N_OLD).astype(np.int32)
    new = []
    for i in range(N_NEW):                                                  # keypoint 0 of every keyframe is free
        for k in (2 * i, 2 * i + 1):
            new.append((ADD_OBS, MATCH, N_OLD + i, k, 0, int(x["kf_octave"][t["kf_mp_ptr"][k]]), 1))
    frame_mp = rng.permutation(N_OLD + N_NEW)[:60].astype(np.int32)
    return t, x, recent, new, frame_mp


def covis_of(t, x):
    z = lambda *s: np.zeros(s, np.int32)
    return {"row_cap": ROW_CAP, "origin_kf": 11, "obs_octave": x["obs_octave"], "obs_weight": x["obs_weight"], "mp_nobs": x["mp_nobs"], "kf_octave": x["kf_octave"],
            "kf_depth": None, "kf_th_depth": None, "kf_not_erase": np.zeros(N_KF, np.uint8), "cw_kf": z(N_KF, ROW_CAP), "cw_w": z(N_KF, ROW_CAP), "cw_n": z(N_KF),
            "ord_kf": z(N_KF, ROW_CAP), "ord_w": z(N_KF, ROW_CAP), "ord_n": z(N_KF)}


def local_map_tensors(frame_mp, n_mp):
    import torch
    from weiner_slamit_v2_amd import api

    i32 = lambda *s, v=-9: torch.full(s, v, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    d = {"frame_map": i32(1, v=0), "n": i32(1, v=len(frame_mp)), "frame_mp": torch.from_numpy(frame_mp.reshape(1, -1).copy()).cuda(), "votes": i32(1, N_KF + 5),
         "local_kf": i32(1, KF_CAP, v=0), "n_local_kf": i32(1, v=0), "ref_kf": i32(1, v=0), "local_mp": i32(1, Q_CAP, v=0), "n_local_mp": i32(1), "pos": f32(1, 3, Q_CAP),
         "normal": f32(1, 3, Q_CAP), "max_dist": f32(1, Q_CAP), "min_dist": f32(1, Q_CAP), "skip": torch.zeros((1, Q_CAP), dtype=torch.uint8, device="cuda"),
         "m": i32(1), "status": i32(1), "mp_cap": n_mp + 3}
    d["workspace"] = torch.full((api.local_map_workspace(1, n_mp + 3, KF_CAP),), 0x5a, dtype=torch.uint8, device="cuda")
    return d


def points_tensors(mp_cap, touched=None, n=None):
    import torch

    i32 = lambda *s, v=-9: torch.full(s, v, dtype=torch.int32, device="cuda")
    u = {"item_map": i32(1, v=0), "what": i32(1, v=3), "status": i32(1, mp_cap), "points": i32(1, mp_cap, v=-3) if touched is None else touched, "n": n}
    return u


def covis_tensors(k):
    import torch

    i32 = lambda *s, v=-9: torch.full(s, v, dtype=torch.int32, device="cuda")
    return {"kf": i32(1, v=k), "first": i32(1, v=1), "counts": i32(1, N_KF + 2), "n_counted": i32(1), "n_listed": i32(1), "parent": i32(1, v=-1), "status": i32(1)}


def verdicts_to_edits(verdict, recent, n, cap):
    """Verdicts 2 and 3 of the first n entries as SET_BAD edits in list order, on the device: (1, cap, 24) bytes and their number."""
    import torch

    j = torch.arange(cap, device="cuda")
    mask = ((verdict == 2) | (verdict == 3)) & (j < n)
    at = torch.where(mask, torch.cumsum(mask, 0) - 1, torch.full_like(j, cap))   # what is not an edit lands in a row past the list
    rows = torch.zeros((cap, 6), dtype=torch.int32, device="cuda")
    rows[:, 0] = SET_BAD
    rows[:, 2] = recent
    edits = torch.zeros((cap + 1, 6), dtype=torch.int32, device="cuda")
    edits.index_copy_(0, at, rows)
    return edits[:cap].view(torch.uint8).reshape(1, cap, 24), mask.sum().to(torch.int32).reshape(1)


def edit_tensors(cap, mp_cap, kfmp_cap):
    import torch
    from weiner_slamit_v2_amd import api

    i32 = lambda *s, v=-9: torch.full(s, v, dtype=torch.int32, device="cuda")
    return {"status_mp": i32(1, mp_cap), "touched": i32(1, mp_cap, v=-3), "n_touched": i32(1), "n_obs_out": i32(1), "status": i32(1), "kfmp_cap": kfmp_cap,
            "workspace": torch.full((api.map_edit_workspace(1, cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}


def read(d, u, c=None, ci=None, mi=None, pi=None):
    g = lambda a: a.cpu().numpy().copy()
    m = int(d["m"][0])
    out = {"votes": g(d["votes"][0, :N_KF]), "n_local_kf": int(d["n_local_kf"][0]), "ref_kf": int(d["ref_kf"][0]), "m": m, "lm_status": int(d["status"][0]),
           "local_kf": g(d["local_kf"][0, :int(d["n_local_kf"][0])]), "local_mp": g(d["local_mp"][0, :m]), "skip": g(d["skip"][0, :m]), "frame_mp": g(d["frame_mp"][0])}
    for key in ("pos", "normal"):
        out["lm_" + key] = bits(g(d[key][0, :, :m]))
    for key in ("max_dist", "min_dist"):
        out["lm_" + key] = bits(g(d[key][0, :m]))
    nt = int(u["n"][0])
    out.update(n_touched=nt, touched=g(u["points"][0, :nt]), up_status=g(u["status"][0, :nt]))
    for key in PLANES + ("mp_desc",):
        out[key] = bits(g(pi.t[key]))
    if c is not None:
        out.update({"uc_" + k: g(c[k]) for k in ("counts", "n_counted", "n_listed", "parent", "status")})
        out.update({k: g(ci.t[k]) for k in ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best")})
    return out


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def test_two_rounds_of_edits_between_resident_steps_on_one_stream():
    import torch
    from weiner_slamit_v2_amd import api

    t, x, recent, new, frame_mp = the_map()
    n_mp, n_kfmp, cap = t["n_mp"], len(t["kf_mp"]), len(recent) + 4
    obs_cap = len(t["obs_kf"]) + len(new) + 8
    # ---- resident: uploaded once
    mi = api.MapIndex(t)
    pi = api.PointIndex(x, mi)
    ci = api.CovisIndex(covis_of(t, x), mi)
    ei = api.EditIndex(x, mi, obs_cap, covis=ci, points=pi)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    h_recent = np.full((1, cap), -3, np.int32)
    h_recent[0, :len(recent)] = recent
    cull = {"list_map": cu(np.zeros(1, np.int32)), "cur_id": cu(np.array([CUR_ID], np.int32)), "monocular": cu(np.ones(1, np.int32)), "n": cu(np.array([len(recent)], np.int32)),
            "recent": cu(h_recent), "verdict": torch.full((1, cap), 0xee, dtype=torch.uint8, device="cuda"), "kept": torch.full((1, cap), -77, dtype=torch.int32, device="cuda"),
            "n_kept": cu(np.full(1, -9, np.int32)), "status": cu(np.full(1, -9, np.int32))}
    e1, e2 = edit_tensors(cap, n_mp, n_kfmp), edit_tensors(len(new), n_mp, n_kfmp)
    e2["edits"], e2["n"] = cu(records(new).view(np.uint8).reshape(1, len(new), 24)), cu(np.array([len(new)], np.int32))
    d1, d2 = local_map_tensors(frame_mp, n_mp), local_map_tensors(frame_mp, n_mp)
    u1, u2 = points_tensors(n_mp, e1["touched"], e1["n_touched"]), points_tensors(n_mp, e2["touched"], e2["n_touched"])
    c2 = covis_tensors(0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        api.map_point_culling_batch_dev([mi], [pi], cull, stream=s)
        e1["edits"], e1["n"] = verdicts_to_edits(cull["verdict"][0], cull["recent"][0], cull["n"], cap)
        api.map_edit_batch_dev([mi], [ei], e1, stream=s)
        ei.swap()
        api.update_points_batch_dev([mi], [pi], u1, stream=s)
        api.local_map_batch_dev([mi], d1, stream=s)
        api.map_edit_batch_dev([mi], [ei], e2, stream=s)
        ei.swap()
        api.update_points_batch_dev([mi], [pi], u2, stream=s)
        api.update_connections_batch_dev([mi], [ci], [0], c2, stream=s)
        api.local_map_batch_dev([mi], d2, stream=s)
    st.synchronize()
    got2 = read(d2, u2, c2, ci, mi, pi)
    got1 = read(d1, u1, pi=pi)
    for key in PLANES + ("mp_desc",):
        del got1[key]                                                       # read after round two: compared there
    assert int(e1["status"][0]) == 0 == int(e2["status"][0]) and not e1["status_mp"].any() and not e2["status_mp"].any()
    # ---- the same with the tables rebuilt on the host by the restatement and uploaded afresh, round by round
    verdict = api.map_point_culling(t, x, CUR_ID, True, recent)["verdict"]
    kill = [(SET_BAD, 0, int(p), 0, 0, 0, 0) for p, v in zip(recent, verdict) if v in (2, 3)]
    assert len(kill) > 20 and {int(v) for v in verdict} >= {0, 2, 3}
    assert np.array_equal(e1["edits"][0, :len(kill)].cpu().numpy().reshape(-1), records(kill).view(np.uint8)) and int(e1["n"][0]) == len(kill)
    tables, cols, want = t, x, []
    for r, edits in enumerate((kill, new)):
        a = apply(tables, cols, edits)
        tables = dict(tables, obs_ptr=a["obs_ptr"], obs_kf=a["obs_kf"], mp_bad=a["mp_bad"], kf_mp=a["kf_mp"])
        cols = dict(cols, obs_idx=a["obs_idx"], obs_octave=a["obs_octave"], obs_weight=a["obs_weight"], mp_nobs=a["mp_nobs"], mp_ref_kf=a["mp_ref_kf"])
        m2 = api.MapIndex(tables)
        p2 = api.PointIndex(cols, m2)
        q2 = api.CovisIndex(covis_of(tables, cols), m2)
        h_t = np.full((1, n_mp), -3, np.int32)
        h_t[0, :a["n_touched"]] = a["touched"]
        u = points_tensors(n_mp, cu(h_t), cu(np.array([a["n_touched"]], np.int32)))
        d, c = local_map_tensors(frame_mp, n_mp), covis_tensors(0) if r == 1 else None
        api.update_points_batch_dev([m2], [p2], u)
        if c is not None:
            api.update_connections_batch_dev([m2], [q2], [0], c)
        api.local_map_batch_dev([m2], d)
        torch.cuda.synchronize()
        want.append(read(d, u, c, q2, m2, p2))
        tables = dict(tables, **{k: p2.t[k].cpu().numpy().reshape(np.shape(tables[k])) for k in PLANES})
        cols = dict(cols, **{k: tables[k] for k in PLANES}, mp_desc=p2.t["mp_desc"].cpu().numpy().reshape(n_mp, 32))
    for key in PLANES + ("mp_desc",):
        del want[0][key]
    same(got1, want[0], "round one")
    same(got2, want[1], "round two")
    # the rounds did something: points went, points came, the new ones got a normal and a descriptor, keyframe 0 got neighbours
    assert want[0]["n_touched"] == len(kill) and want[1]["n_touched"] == N_NEW and not want[1]["up_status"].any()
    assert not np.array_equal(want[1]["mp_normal"].reshape(n_mp, 3)[N_OLD:], bits(t["mp_normal"][N_OLD:])) and int(want[1]["uc_n_counted"][0]) > 0
    assert set(want[1]["local_mp"].tolist()) & set(range(N_OLD, n_mp)) and not set(want[0]["local_mp"].tolist()) & {k[2] for k in kill}
    # and the tables every reader now takes are the restatement's
    n_obs = int(tables["obs_ptr"][-1])
    assert np.array_equal(mi.t["obs_ptr"].cpu().numpy()[:n_mp + 1], tables["obs_ptr"]) and np.array_equal(mi.t["obs_kf"].cpu().numpy()[:n_obs], tables["obs_kf"])
    assert np.array_equal(mi.t["kf_mp"].cpu().numpy()[:n_kfmp], tables["kf_mp"]) and np.array_equal(ci.t["mp_nobs"].cpu().numpy()[:n_mp], cols["mp_nobs"])
