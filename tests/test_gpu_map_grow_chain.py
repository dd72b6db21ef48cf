"""The grow call and its readers through the index classes, on one stream with no host visit between them: api.GrowIndex re-houses a map's
MapIndex / CovisIndex / PointIndex / EditIndex / ReplaceIndex / TreeIndex in buffers with room; then
  1 slamit_map_grow_batch_dev,  2 slamit_map_edit_batch_dev on the emitted list (its count read on the device),  3 GrowIndex.grown() with
  what the host listed and EditIndex.swap(),  4 slamit_update_points_batch_dev on map_edit's `touched` (it reads the rows, centres and
  descriptors the grow call appended),  5 slamit_update_connections_batch_dev for the new keyframe (over the empty graph row, kf_best row and
  counts NEW_KF appended),  6 SET_PARENT built on the device from its answer through slamit_kf_erase_batch_dev and TreeIndex.swap(),
  7 slamit_map_point_culling_batch_dev on the recent list,  8 slamit_local_map_batch_dev for a frame that sees the new points.
Every tensor of every index and every output must equal, byte for byte, the same calls run on index objects built from tables rebuilt on
the host out of the restatement's end state (tests/map_grow_ref.py); and the readers must have met nothing out of place: the new keyframe
gets a parent, stands in its children row and comes back as a local keyframe."""
import numpy as np
import pytest

from tests import map_grow_ref as ref
from tests.map_grow_fixtures import by_name
from tests.map_grow_host import EDIT_DTYPE, OP_DTYPE, default_caps, inputs, laid_out, records

pytestmark = pytest.mark.gpu
ROW_CAP, KP_CAP, LM_KF_CAP, Q_CAP = 16, 12, 83, 256
NAMES = ("wave_edges", "associate_after_stereo_points", "two_new_kfs", "associate_existing_observer", "pairs_mixed_status")


def dicts_of(fx, e, n_kf, n_mp):
    """The dicts the index classes take, from flat arrays at their capacities (tests.map_grow_host.inputs / laid_out) cut to n_kf / n_mp."""
    t0 = fx["t"]
    n_kfmp = int(e["kf_mp_ptr"][n_kf])
    zeros = lambda: np.zeros((n_kf, ROW_CAP), np.int32)
    t = {"n_kf": n_kf, "n_mp": n_mp, "obs_ptr": e["obs_ptr"][:n_mp + 1], "obs_kf": t0["obs_kf"], "mp_bad": e["mp_bad"][:n_mp], "kf_bad": e["kf_bad"][:n_kf],
         "kf_mp_ptr": e["kf_mp_ptr"][:n_kf + 1], "kf_mp": e["kf_mp"][:n_kfmp], "kf_best": e["kf_best"][:10 * n_kf], "kf_child_ptr": e["kf_child_ptr"][:n_kf + 1],
         "kf_child": t0["kf_child"], "kf_parent": e["kf_parent"][:n_kf], "mp_pos": e["mp_pos"][:3 * n_mp], "mp_normal": e["mp_normal"][:3 * n_mp],
         "mp_max_dist": e["mp_max_dist"][:n_mp], "mp_min_dist": e["mp_min_dist"][:n_mp]}
    covis = {"row_cap": ROW_CAP, "origin_kf": 0, "obs_octave": t0["obs_octave"], "obs_weight": t0["obs_weight"], "mp_nobs": e["mp_nobs"][:n_mp], "kf_octave": e["kf_octave"][:n_kfmp],
             "kf_depth": None if e["kf_depth"] is None else e["kf_depth"][:n_kfmp], "kf_th_depth": None if e["kf_th_depth"] is None else e["kf_th_depth"][:n_kf],
             "kf_not_erase": e["kf_not_erase"][:n_kf], "cw_kf": zeros(), "cw_w": zeros(), "cw_n": e["cw_n"][:n_kf], "ord_kf": zeros(), "ord_w": zeros(), "ord_n": e["ord_n"][:n_kf]}
    x = {"n_levels": 8, "scale_factors": [1.2 ** i for i in range(8)], "obs_idx": t0["obs_idx"], "obs_octave": t0["obs_octave"], "obs_weight": t0["obs_weight"],
         "kf_octave": e["kf_octave"][:n_kfmp], "kf_center": e["kf_center"][:3 * n_kf], "kf_desc": e["kf_desc"][:32 * n_kfmp], "mp_ref_kf": e["mp_ref_kf"][:n_mp],
         "mp_nobs": e["mp_nobs"][:n_mp], "mp_found": e["mp_found"][:n_mp], "mp_visible": e["mp_visible"][:n_mp], "mp_first_kf": e["mp_first_kf"][:n_mp], "mp_desc": e["mp_desc"][:32 * n_mp]}
    return t, covis, x, {"kf_to_be_erased": e["kf_to_be_erased"][:n_kf]}, {"mp_replaced": e["mp_replaced"][:n_mp]}


def run(fxs, caps, grow_on_device):
    import torch
    from weiner_slamit_v2_amd import api

    B = len(fxs)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    some = lambda a: a if len(a) else np.zeros(16, a.dtype)
    st = torch.cuda.current_stream().cuda_stream
    cap, cand_cap, edit_cap, recent_cap = (caps[0][k] for k in ("cap", "cand_cap", "edit_cap", "recent_cap"))
    mp_cap, kfmp_cap, kf_cap = (max(c[k] for c in caps) for k in ("mp_cap", "kfmp_cap", "kf_cap"))
    laid = [laid_out(fx, c)[0] for fx, c in zip(fxs, caps)]
    start = [inputs(fx, c) if grow_on_device else e for fx, c, e in zip(fxs, caps, laid)]
    listed = [(sum(1 for e in fx["ops"] if e["kind"] == ref.NEW_KF), sum(1 for e in fx["ops"] if e["kind"] == ref.NEW_POINT)) for fx in fxs]
    mis, cis, pis, eis, ris, tis, gis, frame_recs, keep = [], [], [], [], [], [], [], [], []
    h_ops = np.zeros((B, cap, OP_DTYPE.itemsize), np.uint8)
    for m, (fx, c, a, (nk, P)) in enumerate(zip(fxs, caps, start, listed)):
        n_kf, n_mp = fx["t"]["n_kf"] + (0 if grow_on_device else nk), fx["t"]["n_mp"] + (0 if grow_on_device else P)
        t, covis, x, tree, cols = dicts_of(fx, a, n_kf, n_mp)
        mi = api.MapIndex(t)
        ci = api.CovisIndex(covis, mi)
        pi = api.PointIndex(x, mi)
        ei = api.EditIndex(x, mi, len(fx["t"]["obs_kf"]) + edit_cap + 1, covis=ci, points=pi)
        ri = api.ReplaceIndex(ei, cols)
        ti = api.TreeIndex(tree, mi, ci, len(fx["t"]["kf_child"]) + 2)
        gis.append(api.GrowIndex(mi, covis=ci, points=pi, edit=ei, replace=ri, tree=ti, kf_cap=c["kf_cap"], mp_cap=c["mp_cap"], kfmp_cap=c["kfmp_cap"]))
        for lst, v in ((mis, mi), (cis, ci), (pis, pi), (eis, ei), (ris, ri), (tis, ti)):
            lst.append(v)
        base = len(frame_recs)
        for f in fx["frames"]:
            fd = {k: cu(some(v)) for k, v in f.items() if k != "th_depth" and v is not None}
            keep.append(fd)
            frame_recs.append(api.grow_frame_rec(dict(fd, th_depth=f["th_depth"])))
        ops = records(fx["ops"])
        ops["src"] += np.where((ops["kind"] == ref.NEW_KF) | (ops["kind"] == ref.ASSOCIATE), base, 0).astype(np.int32)
        h_ops[m, :len(ops)] = ops.view(np.uint8).reshape(-1, OP_DTYPE.itemsize)
    stack = lambda key, src: cu(np.stack([s[key] for s in src]))
    i32 = lambda v, *s: cu(np.full(s or (B,), v, np.int32))
    g = {"ops": cu(h_ops), "n": cu(np.array([len(fx["ops"]) for fx in fxs], np.int32)), "cand_status": stack("cand_status", start), "cand_x3d": stack("cand_x3d", start),
         "op_status": stack("op_status", start), "edits": stack("edits", start).reshape(B, edit_cap, EDIT_DTYPE.itemsize), "recent": stack("recent", start),
         "n_edits_out": cu(np.array([-11 if grow_on_device else e["n_edits_out"] for e in start], np.int32)),
         "n_recent": cu(np.array([len(fx["recent"]) if grow_on_device else e["n_recent"] for fx, e in zip(fxs, start)], np.int32)),
         "n_new": i32(-11), "need": i32(-1, B, api.GROW_NEEDS), "status": i32(-11), "mp_cap": mp_cap,
         "workspace": torch.full((api.map_grow_workspace(B, mp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}
    if grow_on_device:
        api.map_grow_batch_dev(mis, gis, frame_recs, g, stream=st)                                          # 1
        for gi, (nk, P) in zip(gis, listed):
            gi.grown(nk, P)                                                                                 # 3a: what the host listed, no host visit
    me = {"edits": g["edits"], "n": g["n_edits_out"], "status_mp": i32(-5, B, mp_cap), "touched": i32(-6, B, mp_cap), "n_touched": i32(-1), "n_obs_out": i32(-1),
          "status": i32(-1), "kfmp_cap": kfmp_cap, "workspace": torch.full((api.map_edit_workspace(B, edit_cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}
    api.map_edit_batch_dev(mis, eis, me, stream=st)                                                         # 2
    for ei in eis:
        ei.swap()                                                                                           # 3b
    up = {"item_map": cu(np.arange(B, dtype=np.int32)), "n": me["n_touched"], "what": i32(3), "points": me["touched"], "status": i32(-4, B, mp_cap)}
    api.update_points_batch_dev(mis, pis, up, stream=st)                                                    # 4
    K = [fx["t"]["n_kf"] + nk - 1 if nk else 1 for fx, (nk, _) in zip(fxs, listed)]                         # a map without a new keyframe: keyframe 1
    uc = {"kf": cu(np.array(K, np.int32)), "first": i32(1), "counts": i32(-2, B, kf_cap), "n_counted": i32(-1), "n_listed": i32(-1), "parent": i32(-1), "status": i32(-1)}
    api.update_connections_batch_dev(mis, cis, list(range(B)), uc, stream=st)                               # 5
    ops = torch.zeros((B, 1, 4), dtype=torch.int32, device="cuda")
    ops[:, 0, 0], ops[:, 0, 1], ops[:, 0, 2] = 1, uc["kf"], uc["parent"]
    child_max = max(ti.child_cap for ti in tis)
    ke = {"ops": ops, "n": (uc["parent"] >= 0).to(torch.int32), "op_status": i32(-9, B, 1), "edits": cu(np.full((B, 4, 24), 0xee, np.uint8)), "n_edits_out": i32(-1),
          "n_child_out": i32(-1), "status": i32(-1), "kf_cap": kf_cap, "row_cap": ROW_CAP, "child_cap": child_max,
          "workspace": torch.full((api.kf_erase_workspace(B, 1, kf_cap, ROW_CAP, child_max),), 0x5a, dtype=torch.uint8, device="cuda")}
    api.kf_erase_batch_dev(mis, tis, ke, stream=st)                                                         # 6
    for ti in tis:
        ti.swap()
    mc = {"list_map": cu(np.arange(B, dtype=np.int32)), "cur_id": i32(23), "monocular": i32(0), "n": g["n_recent"], "recent": g["recent"],
          "verdict": cu(np.full((B, recent_cap), 0x77, np.uint8)), "kept": i32(-3, B, recent_cap), "n_kept": i32(-1), "status": i32(-1)}
    api.map_point_culling_batch_dev(mis, pis, mc, stream=st)                                                # 7
    h_fm = np.full((B, KP_CAP), -1, np.int32)
    for m, (fx, (_, P)) in enumerate(zip(fxs, listed)):
        n_mp = fx["t"]["n_mp"]
        seen = list(range(n_mp, n_mp + min(P, 6))) + list(range(min(n_mp, 3)))       # the first new slots, accepted and inert, and three old points
        h_fm[m, :len(seen)] = seen
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")
    lm = {"frame_map": cu(np.arange(B, dtype=np.int32)), "n": i32(KP_CAP), "frame_mp": cu(h_fm), "votes": i32(-2, B, kf_cap), "local_kf": i32(0, B, LM_KF_CAP),
          "n_local_kf": i32(0), "ref_kf": i32(0), "local_mp": i32(0, B, Q_CAP), "n_local_mp": i32(-1), "pos": z(torch.float32, B, 3, Q_CAP), "normal": z(torch.float32, B, 3, Q_CAP),
          "max_dist": z(torch.float32, B, Q_CAP), "min_dist": z(torch.float32, B, Q_CAP), "skip": z(torch.uint8, B, Q_CAP), "m": i32(-1), "status": i32(-1), "mp_cap": mp_cap,
          "workspace": torch.full((api.local_map_workspace(B, mp_cap, LM_KF_CAP),), 0x5a, dtype=torch.uint8, device="cuda")}
    api.local_map_batch_dev(mis, lm, stream=st)                                                             # 8
    torch.cuda.synchronize()
    out = []
    for m in range(B):
        o = {"K": np.array(K[m]), "n_kf": np.array(mis[m].rec.n_kf), "n_mp": np.array(mis[m].rec.n_mp)}
        for name, d in (("map", mis[m].t), ("covis", cis[m].t), ("points", pis[m].t), ("edit", eis[m].t), ("edit0", eis[m].sets[0]), ("edit1", eis[m].sets[1]),
                        ("replace", ris[m].t), ("tree", tis[m].t), ("tree0", tis[m].sets[0]), ("tree1", tis[m].sets[1])):
            for k, v in d.items():
                o[name + "." + k] = v.cpu().numpy()
        for name, t in (("me", me), ("up", up), ("conn", uc), ("ke", ke), ("cull", mc), ("lm", lm), ("grow", g)):
            for k, v in t.items():
                if hasattr(v, "cpu") and k != "workspace" and (name != "grow" or k in ("edits", "recent", "n_recent", "n_edits_out")):
                    o[name + "." + k] = v[m].cpu().numpy()
        out.append(o)
    return out


def test_the_chain_equals_the_same_calls_on_tables_rebuilt_on_the_host():
    fxs = [by_name(n) for n in NAMES]
    caps = [default_caps(fx) for fx in fxs]
    for key in ("cap", "cand_cap", "edit_cap", "recent_cap"):
        for c in caps:
            c[key] = max(q[key] for q in caps)
    for fx in fxs:
        if fx["t"]["kf_depth"] is None:                                    # a monocular map: the stereo columns are absent from every record
            assert fx["name"] == "two_new_kfs"
        fx["t"]["cw_n"][:] = 0                                             # the covisibility graph starts empty
        fx["t"]["ord_n"][:] = 0
    got, want = run(fxs, caps, True), run(fxs, caps, False)
    for fx, a, b in zip(fxs, got, want):
        assert set(a) == set(b)
        for k in sorted(a):
            assert a[k].shape == b[k].shape, (fx["name"], k, a[k].shape, b[k].shape)
            x, y = np.ascontiguousarray(a[k]).reshape(-1).view(np.uint8), np.ascontiguousarray(b[k]).reshape(-1).view(np.uint8)
            assert np.array_equal(x, y), (fx["name"], k, np.flatnonzero(x != y)[:8])
        assert int(a["me.status"]) == 0 and int(a["me.n_touched"]) > 0 and int(a["cull.n_kept"]) >= 0
        w = ref.apply(fx)
        assert int(a["n_kf"]) == len(w["kfs"]) and int(a["n_mp"]) == fx["t"]["n_mp"] + w["P"]     # grown() with what the host listed
        # the readers of what NEW_KF appended met nothing out of place: the new keyframe got a parent, entered its children row, and is a local keyframe
        K, par = int(a["K"]), int(a["conn.parent"])
        assert int(a["conn.status"]) == 0 and int(a["ke.status"]) == 0 and int(a["lm.status"]) == 0 and int(a["ke.op_status"][0]) == 0, fx["name"]
        assert par >= 0 and par != K and int(a["map.kf_parent"][K]) == par and int(a["covis.cw_n"][K]) == int(a["conn.n_counted"]) > 0
        row = a["map.kf_child"][a["map.kf_child_ptr"][par]:a["map.kf_child_ptr"][par + 1]].tolist()
        assert K in row and row == sorted(row)
        assert int(a["lm.m"]) > 0 and int(a["lm.n_local_kf"]) > 0
        if any(e["kind"] == ref.NEW_KF for e in fx["ops"]):               # the frame sees points the new keyframe observes
            assert K in a["lm.local_kf"][:int(a["lm.n_local_kf"])].tolist(), fx["name"]
    # the chain did something: new points were observed, described and judged
    w = got[0]
    n_mp = fxs[0]["t"]["n_mp"]
    assert w["points.mp_nobs"][n_mp] > 0 and w["points.mp_desc"][32 * n_mp:32 * n_mp + 32].any() and w["map.mp_max_dist"][n_mp] > 0 and int(w["cull.n_kept"]) > 0
