"""SearchInNeighbors' fuse on one stream with no host visit, over two maps in one call of each batched link:
slamit_project_batch_dev (FUSE form) projects the query points into three target keyframes, slamit_guided_search_batch_dev searches them,
slamit_fuse_list_batch_dev turns the matches it left in HBM into FUSE ops (two targets back to back in map 0's list, one in map 1's),
slamit_map_fuse_batch_dev applies both lists, EditIndex.swap() exchanges the buffer sets, and per map slamit_update_points_batch_dev runs
on `touched`, slamit_update_connections_batch_dev, slamit_check_replaced_batch_dev on a frame's list and slamit_local_map_batch_dev read
the new map.  The matches are downloaded only after the final synchronisation; everything must equal the same readers over tables that
the reference walk (tests/map_fuse_ref.py) rebuilt on the host from those matches and that were uploaded afresh.

The queries' geometry, the targets' keypoints and the search rule are the FUSE chain's of tests/test_gpu_project.py (a target with 300
queries, one with none, one with 65); the maps are tests/upkeep_fixtures.py's tables with the target keyframes' rows as wide as the
targets have keypoints, the first keypoints of each occupied by points of the map -- some of them bad -- so that a match replaces one
way, the other way, adds, or is skipped."""
import numpy as np
import pytest

from tests import project_ref as ref
from tests.map_fuse_ref import ADDED, FUSE, OCCUPANT_BAD, P_REPLACED, Q_REPLACED, SKIP_BAD, apply
from tests.test_gpu_map_edit_chain import N_KF, covis_of, covis_tensors, local_map_tensors, points_tensors, read, same
from tests.test_gpu_project import KP_CAP, Q_CAP, RULES, _chain_tensors
from tests.upkeep_fixtures import build_map

pytestmark = pytest.mark.gpu
FRAME_MAP, FRAME_KF, BASE = (0, 0, 1), (2, 5, 1), (0, Q_CAP, 0)            # target f: its map, its keyframe slot, where its slice begins
QUERIES, OCCUPANTS = (300, 65), (200, 60)                                # per map: the points projected, the points standing in the target


def the_targets():
    """The three targets of tests/test_gpu_project.py's FUSE chain: problems, the header's projections, the search's side."""
    full = ref.head(ref.fixture(ref.first_fixture(ref.FUSE)), 300)
    probs = [full, ref.head(full, 0), ref.head(full, 65)]
    hosts = [ref.host_points(pr) for pr in probs]
    sides = [ref.search_side(pr, h, 40 + 10 * ref.FUSE + f, 0.0) for f, (pr, h) in enumerate(zip(probs, hosts))]
    return probs, hosts, sides


def widen(t, x, k, width, rng):
    """Keyframe k's row of kf_mp gets free keypoints at its end until it holds `width`."""
    extra = width - int(t["kf_mp_ptr"][k + 1] - t["kf_mp_ptr"][k])
    if extra <= 0:
        return
    at = int(t["kf_mp_ptr"][k + 1])
    t["kf_mp"] = np.insert(t["kf_mp"], at, np.full(extra, -1, np.int32))
    x["kf_octave"] = np.insert(x["kf_octave"], at, rng.integers(0, 8, extra).astype(np.uint8))
    x["kf_desc"] = np.insert(x["kf_desc"], at, rng.integers(0, 256, (extra, 32)).astype(np.uint8), axis=0)
    t["kf_mp_ptr"] = t["kf_mp_ptr"].copy()
    t["kf_mp_ptr"][k + 1:] += extra


def the_map(m, sides):
    """Map m: QUERIES[m] points outside the target keyframe (slots 0..), OCCUPANTS[m] points in it (they take its first keypoints)."""
    rng = np.random.default_rng(3300 + m)
    mine = [f for f in range(3) if FRAME_MAP[f] == m]
    k0 = FRAME_KF[mine[0]]
    others = [k for k in range(N_KF) if k != k0]
    points = []
    for p in range(QUERIES[m]):
        obs = rng.permutation(others)[:int(rng.integers(2, 6))].tolist()
        points.append(dict(obs=obs, ref=obs[0], bad=int(p % 11 == 7)))
    for p in range(OCCUPANTS[m]):
        obs = rng.permutation([k0] + rng.permutation(others)[:int(rng.integers(1, 5))].tolist()).tolist()
        points.append(dict(obs=obs, ref=obs[0], bad=int(p % 5 == 3)))
    t, x = build_map(N_KF, points, rng)
    for f in mine:
        frame, k = sides[f][0], FRAME_KF[f]
        widen(t, x, k, len(frame["kp_xy"]), rng)
        x["kf_octave"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k] + len(frame["kp_xy"])] = frame["kp_octave"]   # the keyframe IS the target the search sees
    x["obs_octave"] = x["kf_octave"][t["kf_mp_ptr"][t["obs_kf"]] + x["obs_idx"]]
    x["obs_weight"] = np.ones(len(t["obs_kf"]), np.uint8)
    x["mp_found"], x["mp_visible"] = rng.integers(0, 50, t["n_mp"]).astype(np.int32), rng.integers(50, 100, t["n_mp"]).astype(np.int32)
    x["mp_replaced"] = np.full(t["n_mp"], -1, np.int32)
    return t, x, rng.permutation(t["n_mp"])[:60].astype(np.int32)


def the_ops(m, match, n_queries, sides):
    """Map m's list as the builder must write it, from the downloaded matches: three lines of numpy per target."""
    ops = []
    for f in sorted((f for f in range(3) if FRAME_MAP[f] == m), key=lambda f: BASE[f]):
        q = np.arange(Q_CAP) < n_queries[f]
        idx = np.where(q, match[f], -1)
        octave = np.where(idx >= 0, sides[f][0]["kp_octave"][np.maximum(idx, 0)], 0)             # every target has keypoints: clutter at the least
        ops += [(FUSE, int(a), FRAME_KF[f], int(i), int(o), 1) for a, i, o in zip(np.where(q, np.arange(Q_CAP), -1), idx, octave)]
    return ops


def test_search_in_neighbors_on_one_stream_over_two_maps():
    import torch
    from weiner_slamit_v2_amd import api

    probs, hosts, sides = the_targets()
    assert [int(p["n"]) for p in probs] == [300, 0, 65] and max(len(s[0]["kp_xy"]) for s in sides) <= KP_CAP
    maps = [the_map(m, sides) for m in range(2)]
    for f in range(3):                                                   # the builder's kp_cap against the row: every keypoint the search can name is in it
        t = maps[FRAME_MAP[f]][0]
        assert len(sides[f][0]["kp_xy"]) <= t["kf_mp_ptr"][FRAME_KF[f] + 1] - t["kf_mp_ptr"][FRAME_KF[f]] <= KP_CAP
    d, _ = _chain_tensors(probs, hosts, sides)
    bounds = tuple(sides[0][0][key] for key in ("min_x", "min_y", "inv_w", "inv_h"))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    i32 = lambda *sh, v=-9: torch.full(sh, v, dtype=torch.int32, device="cuda")
    n_list = [2 * Q_CAP, Q_CAP]
    cap, mp_cap, kfmp_cap = 2 * Q_CAP + 3, max(t["n_mp"] for t, _, _ in maps) + 2, max(len(t["kf_mp"]) for t, _, _ in maps)
    obs_caps = [len(t["obs_kf"]) + n for (t, _, _), n in zip(maps, n_list)]
    # ---- resident: uploaded once
    mis = [api.MapIndex(t) for t, _, _ in maps]
    pis = [api.PointIndex(x, mi) for (_, x, _), mi in zip(maps, mis)]
    cis = [api.CovisIndex(covis_of(t, x), mi) for (t, x, _), mi in zip(maps, mis)]
    eis = [api.EditIndex(x, mi, oc, covis=ci, points=pi) for (_, x, _), mi, oc, ci, pi in zip(maps, mis, obs_caps, cis, pis)]
    ris = [api.ReplaceIndex(ei, x) for (_, x, _), ei in zip(maps, eis)]
    point = np.full((3, Q_CAP), -7, np.int32)
    for f in range(3):
        point[f, :int(probs[f]["n"])] = np.arange(int(probs[f]["n"]))   # query q of target f is point q of its map
    se = dict(d, match_kp=i32(3, Q_CAP, v=-7), nmatches=i32(3, v=-7), uvr=torch.full((3, Q_CAP, 3), -7.0, device="cuda"), level_min=i32(3, Q_CAP, v=-7),
              level_max=i32(3, Q_CAP, v=-7), valid=torch.full((3, Q_CAP), 7, dtype=torch.uint8, device="cuda"))
    r = {"ops": torch.full((2, cap, 20), 0x77, dtype=torch.uint8, device="cuda"), "n": i32(2), "outcome": i32(2, cap), "moved": i32(2, cap), "erased": i32(2, cap),
         "touched": i32(2, mp_cap, v=-3), "n_touched": i32(2), "n_fused": i32(2), "n_obs_out": i32(2), "status": i32(2), "kfmp_cap": kfmp_cap,
         "workspace": torch.full((api.map_fuse_workspace(2, cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda"),
         # the builder reads what the search wrote, where the search wrote it
         "m": se["m"], "match_kp": se["match_kp"], "kps_un": se["kps_un"], "kp_ur": None, "query_point": cu(point),
         "frame_map": cu(np.array(FRAME_MAP, np.int32)), "frame_kf": cu(np.array(FRAME_KF, np.int32)), "base": cu(np.array(BASE, np.int32)), "list_status": i32(3)}
    ds = [local_map_tensors(fm, t["n_mp"]) for t, _, fm in maps]
    us = [points_tensors(mp_cap, r["touched"][m:m + 1], r["n_touched"][m:m + 1]) for m in range(2)]
    cs = [covis_tensors(0) for _ in range(2)]
    chks = [{"frame_mp": dm["frame_mp"], "frame_map": dm["frame_map"], "n": dm["n"], "status": i32(1)} for dm in ds]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        h = st.cuda_stream
        api.project_batch_dev(se, stream=h)
        api.ORBmatcher.guided_search_batch_dev(se, bounds, stream=h, **RULES[ref.FUSE])
        api.fuse_list_batch_dev(r, 2, stream=h)
        api.map_fuse_batch_dev(mis, ris, r, stream=h)
        for m in range(2):
            eis[m].swap()
            api.update_points_batch_dev([mis[m]], [pis[m]], us[m], stream=h)
            api.update_connections_batch_dev([mis[m]], [cis[m]], [0], cs[m], stream=h)
            api.check_replaced_batch_dev([ris[m].t["mp_replaced"]], chks[m], n_mp=[maps[m][0]["n_mp"]], stream=h)
            api.local_map_batch_dev([mis[m]], ds[m], stream=h)
    st.synchronize()
    # ---- only now the matches come down, to feed the reference walk
    match, nm = se["match_kp"].cpu().numpy(), se["nmatches"].cpu().numpy()
    n_queries = [int(p["n"]) for p in probs]
    assert nm[0] > 30 and nm[1] == 0 and nm[2] > 5 and np.all(match[1] == -7) and np.all(match[0, 300:] == -7)
    assert r["n"].cpu().tolist() == n_list and not r["list_status"].any() and r["status"].cpu().tolist() == [0, 0]
    seen = set()
    for m, (t, x, frame_mp) in enumerate(maps):
        n_mp, n_kfmp, n_ops = t["n_mp"], len(t["kf_mp"]), n_list[m]
        got = read(ds[m], us[m], cs[m], cis[m], mis[m], pis[m])
        assert int(chks[m]["status"][0]) == 0
        ops = the_ops(m, match, n_queries, sides)
        assert np.array_equal(r["ops"][m, :n_ops].cpu().numpy().reshape(-1).view(api.REPLACE_DTYPE), api.replace_records(ops))   # the builder read the search's layout
        a = apply(t, x, ops, obs_caps[m])
        oc = a["outcome"]
        seen.update(oc.tolist())
        assert a["status"] == 0 and a["n_fused"] >= (30 if m == 0 else 3) and int(np.sum(oc >= ADDED)) == a["n_fused"]
        assert np.array_equal(r["outcome"][m, :n_ops].cpu().numpy(), oc) and int(r["n_fused"][m]) == a["n_fused"]
        assert np.array_equal(r["moved"][m, :n_ops].cpu().numpy(), a["moved"]) and np.array_equal(r["erased"][m, :n_ops].cpu().numpy(), a["erased"])
        # the same readers over the walk's tables, uploaded afresh
        tables = dict(t, obs_ptr=a["obs_ptr"], obs_kf=a["obs_kf"], mp_bad=a["mp_bad"], kf_mp=a["kf_mp"])
        cols = dict(x, **{k: a[k] for k in ("obs_idx", "obs_octave", "obs_weight", "mp_nobs", "mp_found", "mp_visible", "mp_replaced")})
        m2 = api.MapIndex(tables)
        p2 = api.PointIndex(cols, m2)
        q2 = api.CovisIndex(covis_of(tables, cols), m2)
        h_t = np.full((1, mp_cap), -3, np.int32)
        h_t[0, :a["n_touched"]] = a["touched"]
        u2 = points_tensors(mp_cap, cu(h_t), cu(np.array([a["n_touched"]], np.int32)))
        d2, c2 = local_map_tensors(frame_mp, n_mp), covis_tensors(0)
        chk2 = {"frame_mp": d2["frame_mp"], "frame_map": d2["frame_map"], "n": d2["n"], "status": i32(1)}
        api.update_points_batch_dev([m2], [p2], u2)
        api.update_connections_batch_dev([m2], [q2], [0], c2)
        api.check_replaced_batch_dev([cu(a["mp_replaced"])], chk2)
        api.local_map_batch_dev([m2], d2)
        torch.cuda.synchronize()
        same(got, read(d2, u2, c2, q2, m2, p2), "map %d" % m)
        # and the tables every reader now takes are the walk's
        n_obs = int(tables["obs_ptr"][-1])
        assert np.array_equal(mis[m].t["obs_ptr"].cpu().numpy()[:n_mp + 1], tables["obs_ptr"]) and np.array_equal(mis[m].t["obs_kf"].cpu().numpy()[:n_obs], tables["obs_kf"])
        assert np.array_equal(mis[m].t["kf_mp"].cpu().numpy()[:n_kfmp], tables["kf_mp"]) and np.array_equal(cis[m].t["mp_nobs"].cpu().numpy()[:n_mp], cols["mp_nobs"])
        for key in ("mp_found", "mp_visible", "mp_replaced"):
            assert np.array_equal(ris[m].t[key].cpu().numpy()[:n_mp], cols[key]), key
    assert {ADDED, P_REPLACED, Q_REPLACED, SKIP_BAD, OCCUPANT_BAD} <= seen, seen   # the search's matches took every branch of the tail
