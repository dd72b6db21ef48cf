"""slamit_map_fuse_apply and slamit_map_fuse_batch_dev on the GPU against the literal sequential restatement (tests/map_fuse_ref.py) on
every fixture: the new table and its three columns, mp_bad, mp_nobs, mp_found, mp_visible, mp_replaced, kf_mp, outcome, moved and erased
op by op, touched and the counts, all exact; the all-or-nothing gate of each overflow; the bytes past the counts; the same bytes from
the same input twice; slots outside their tables; two lists at the ceiling; slamit_fuse_list_batch_dev against three lines of numpy; and
the lists of the map-replace fixtures, which hold no FUSE op, through both modules: the in-order walk against the rounds over one world."""
import functools

import numpy as np
import pytest

from tests import map_replace_fixtures, map_replace_host
from tests.map_fuse_fixtures import F, all_fixtures, by_name, expected
from tests.map_fuse_host import FILL, INPLACE, assert_same, default_cap, fills, laid_out, of_api, records
from tests.map_fuse_ref import ADD_OBS, BAD_SLOT, FUSE, OBS_OVERFLOW, REPLACE, TABLE_OVERFLOW, apply

pytestmark = pytest.mark.gpu
NAMES = [fx["name"] for fx in all_fixtures()]


def want_of(fx, cap):
    full = expected(fx["name"])
    return full if "n_obs_out" not in full else expected(fx["name"], cap - full["n_obs_out"])


@pytest.mark.parametrize("name", NAMES)
def test_the_host_form_equals_the_restatement(name):
    from weiner_slamit_v2_amd import api

    fx, cap = by_name(name), default_cap(by_name(name)) + 3
    out = api.map_fuse(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=fills(fx, cap))
    want = expected(name)
    assert_same(of_api(out), laid_out(fx, want, cap), name)
    if not want["status"] & api.FUSE_REFUSED:                          # what api.map_fuse hands back is a map: the readers' tables
        assert np.array_equal(out["obs_ptr"], want["obs_ptr"]) and np.array_equal(out["obs_kf"], want["obs_kf"]) and np.array_equal(out["touched"], want["touched"])
        assert np.array_equal(out["outcome"], want["outcome"]) and out["n_fused"] == want["n_fused"]
        rec, keep = api._map_index_host(dict(fx["t"], **{k: out[k] for k in ("obs_ptr", "obs_kf", "mp_bad", "kf_mp")}))
        assert rec.n_mp == fx["t"]["n_mp"] and len(keep["obs_kf"]) == want["n_obs_out"]


PLAIN_NAMES = [fx["name"] for fx in map_replace_fixtures.all_fixtures()]


@functools.lru_cache(maxsize=None)
def plain_want(name):
    fx = map_replace_fixtures.by_name(name)
    return apply(fx["t"], fx["x"], fx["ops"], map_replace_host.default_cap(fx) + 3)


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_a_plain_list_equals_the_restatement_and_map_replace(name):
    """(a) A list of REPLACE and ADD_OBS ops through api.map_fuse equals the restatement, every outcome PLAIN and nothing fused; (b) unless
    map_replace meets its per-point ceiling of ops, which map_fuse does not have (one fixture of the 19, fan65), every byte both entry points
    write is the same: the two schedulers run one world (map_rows_dev.h)."""
    from weiner_slamit_v2_amd import api

    fx, cap = map_replace_fixtures.by_name(name), map_replace_host.default_cap(map_replace_fixtures.by_name(name)) + 3
    out = api.map_fuse(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=fills(fx, cap))
    want = plain_want(name)
    assert_same(of_api(out), laid_out(fx, want, cap), name)
    if not want["status"] & api.FUSE_REFUSED:
        assert np.all(want["outcome"] == api.FUSE_OUT["PLAIN"]) and want["n_fused"] == 0
        assert np.all(out["outcome"] == api.FUSE_OUT["PLAIN"]) and out["n_fused"] == 0 and len(out["outcome"]) == len(fx["ops"])
    over = [n for n in PLAIN_NAMES if map_replace_fixtures.expected(n)["status"] & api.REPLACE_STATUS["OP_OVERFLOW"]]
    assert len(PLAIN_NAMES) - len(over) >= 18                           # what the condition below leaves out
    if name in over:
        return
    rep = api.map_replace(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=map_replace_host.fills(fx, cap))
    map_replace_host.assert_same(of_api(out), map_replace_host.of_api(rep), name)   # the table, the columns, kf_mp, moved, erased, touched, the counts, status


def resident_run(fxs, caps, pad=5):
    """One call over the maps of fxs, every map with its own list length.  -> per map the arrays of OUT_KEYS in full (the output
    columns: the whole other buffer set), and the index objects."""
    import torch
    from weiner_slamit_v2_amd import api

    B = len(fxs)
    maps = [api.MapIndex(fx["t"]) for fx in fxs]
    eds = [api.EditIndex(fx["x"], mi, cap) for fx, mi, cap in zip(fxs, maps, caps)]
    reps = [api.ReplaceIndex(ei, fx["x"]) for fx, ei in zip(fxs, eds)]
    for ei in eds:
        for key, name in (("obs_ptr", "obs_ptr_out"), ("obs_kf", "obs_kf_out"), ("obs_idx", "obs_idx_out"), ("obs_octave", "obs_octave_out"), ("obs_weight", "obs_weight_out")):
            ei.sets[1][key].fill_(FILL[name])
    cap = max(len(fx["ops"]) for fx in fxs) + pad
    mp_cap = max(fx["t"]["n_mp"] for fx in fxs) + 2
    kfmp_cap = max(len(fx["t"]["kf_mp"]) for fx in fxs)
    h_ops = np.full((B, cap, 20), 0xff, np.uint8)
    for m, fx in enumerate(fxs):
        h_ops[m, :len(fx["ops"])] = records(fx["ops"]).view(np.uint8).reshape(-1, 20)
    cu = lambda a: torch.from_numpy(a).cuda()
    per_op = lambda key: cu(np.full((B, cap), FILL[key], np.int32))
    t = {"ops": cu(h_ops), "n": cu(np.array([len(fx["ops"]) for fx in fxs], np.int32)), "outcome": per_op("outcome"), "moved": per_op("moved"), "erased": per_op("erased"),
         "touched": cu(np.full((B, mp_cap), FILL["touched"], np.int32)), "n_touched": cu(np.full(B, FILL["n_touched"], np.int32)),
         "n_fused": cu(np.full(B, FILL["n_fused"], np.int32)), "n_obs_out": cu(np.full(B, FILL["n_obs_out"], np.int32)), "status": cu(np.full(B, -1, np.int32)),
         "kfmp_cap": kfmp_cap,
         "workspace": torch.full((api.map_fuse_workspace(B, cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}   # dirty: the call clears what it needs
    api.map_fuse_batch_dev(maps, reps, t, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outs = []
    for m, (fx, ei, ri) in enumerate(zip(fxs, eds, reps)):
        n_mp, n_kfmp, n = fx["t"]["n_mp"], len(fx["t"]["kf_mp"]), len(fx["ops"])
        nxt = ei.sets[1]
        got = {"obs_ptr_out": nxt["obs_ptr"].cpu().numpy()[:n_mp + 1], "mp_bad": ei.t["mp_bad"].cpu().numpy()[:n_mp], "mp_nobs": ei.t["mp_nobs"].cpu().numpy()[:n_mp],
               "kf_mp": ei.t["kf_mp"].cpu().numpy()[:n_kfmp]}
        for key in ("mp_found", "mp_visible", "mp_replaced"):
            got[key] = ri.t[key].cpu().numpy()[:n_mp]
        for key in ("obs_kf", "obs_idx", "obs_octave", "obs_weight"):
            got[key + "_out"] = nxt[key].cpu().numpy()[:ei.obs_cap]
        row = lambda key: t[key][m].cpu().numpy()
        assert np.all(row("touched")[n_mp:] == FILL["touched"]) and all(np.all(row(k)[n:] == FILL[k]) for k in ("outcome", "moved", "erased"))   # past the map's own
        got.update(outcome=row("outcome")[:n], moved=row("moved")[:n], erased=row("erased")[:n], touched=row("touched")[:n_mp], n_touched=int(row("n_touched")),
                   n_fused=int(row("n_fused")), n_obs_out=int(row("n_obs_out")), status=int(row("status")))
        outs.append(got)
    return outs, eds, reps


@pytest.mark.parametrize("part", (0, 1, 2))
def test_the_resident_form_equals_the_restatement(part):
    """One call over several maps with lists of different lengths (among them none); every fixture is in one of the three calls."""
    every = all_fixtures()
    fxs = list(every[:8] if part == 0 else every[8:16] if part == 1 else every[16:] + every[:2])
    assert len(every) <= 24 and len({len(fx["ops"]) for fx in fxs}) > 1
    caps = [default_cap(fx) + 3 for fx in fxs]
    outs, _, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_each_overflow_refuses_its_map_alone():
    """The map that meets a ceiling keeps every byte; its neighbours in the same call are written.  The capacity at the need and one below."""
    from weiner_slamit_v2_amd import api

    for name in ("mixed", "ops65"):
        fx, need = by_name(name), expected(name)["n_obs_out"]
        for cap in (need - 1, need):
            want = expected(name, cap - need)
            assert bool(want["status"] & TABLE_OVERFLOW) == (cap < need)
            out = api.map_fuse(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=fills(fx, cap))
            assert_same(of_api(out), laid_out(fx, want, cap), "%s cap %d" % (name, cap))
    fxs = [by_name(n) for n in ("outcomes", "row513_add", "mixed", "row513_rep", "ops1025", "row513_in", "neighbours", "row513_in_occupant")]
    caps = [default_cap(fx) for fx in fxs]
    caps[4] = expected("ops1025")["n_obs_out"] - 1
    caps[6] = expected("neighbours")["n_obs_out"]
    outs, _, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, want_of(fx, cap), cap), fx["name"])
    assert [o["status"] for o in outs] == [0, OBS_OVERFLOW, 0, OBS_OVERFLOW, TABLE_OVERFLOW, OBS_OVERFLOW, 0, OBS_OVERFLOW] and outs[4]["n_obs_out"] == caps[4] + 1
    for i in (1, 3, 4, 5, 7):
        for key in INPLACE:
            src = fxs[i]["t"] if key in ("mp_bad", "kf_mp") else fxs[i]["x"]
            assert np.array_equal(outs[i][key], np.asarray(src[key]).reshape(-1)), (fxs[i]["name"], key)


def test_lists_at_the_ceiling_of_ops():
    """SLAMIT_FUSE_MAX_OPS ops per list, AT the ceiling, two maps in one call: 16,384 ops that never meet (the most involved points a list
    can name) and a single chain 16,384 deep."""
    from tests.map_fuse_fixtures import ceiling_fixtures
    from weiner_slamit_v2_amd import api

    fxs = list(ceiling_fixtures())
    assert all(len(fx["ops"]) == api.FUSE_MAX_OPS for fx in fxs)
    caps = [default_cap(fx) for fx in fxs]
    outs, _, _ = resident_run(fxs, caps, pad=0)
    for fx, cap, got in zip(fxs, caps, outs):
        want = apply(fx["t"], fx["x"], fx["ops"])
        assert want["status"] == 0 and want["n_fused"] > 10000
        assert_same(got, laid_out(fx, want, cap), fx["name"])


def test_the_same_call_twice_gives_the_same_bytes():
    fxs = [by_name(n) for n in ("ops1025", "chain", "outcomes", "neighbours", "shared")]
    caps = [default_cap(fx) for fx in fxs]
    a, _, _ = resident_run(fxs, caps)
    b, _, _ = resident_run(fxs, caps)
    for fx, cap, x, y in zip(fxs, caps, a, b):
        assert_same(x, y, fx["name"])
        assert_same(x, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_a_slot_outside_its_table_is_skipped():
    """The device cannot be shown its list or its tables first: such an op does nothing but set the bit, and so does a FUSE op that meets
    an occupant that is no slot of the table; an observation outside kf_mp is carried along without its write."""
    fx = by_name("mixed")
    t, n_kf, n_mp = fx["t"], fx["t"]["n_kf"], fx["t"]["n_mp"]
    row = int(t["kf_mp_ptr"][2] - t["kf_mp_ptr"][1])
    bad = [F(n_mp, 0, 0), F(-1, 0, 0), F(1, n_kf, 0), F(1, -1, 0), F(2, 1, row), F(3, 2, 0, 0, 3), F(3, 2, 0, 0, 0), (REPLACE, n_mp, 0, 0, 0, 0), (ADD_OBS, 1, n_kf, 0, 0, 1),
           (0, 0, 1, 0, 0, 0), (4, 0, 1, 0, 0, 0)]
    ops = list(fx["ops"])
    for i, e in enumerate(bad):
        ops.insert(min(2 * i + 1, len(ops)), e)
    ops += [F(n_mp + 5, -7, -1, 9, 9)]                                  # without a match nothing else is read: no bad slot
    mixed = dict(fx, ops=ops)
    want = apply(fx["t"], fx["x"], ops)
    clean = apply(fx["t"], fx["x"], fx["ops"])
    assert want["status"] == BAD_SLOT and all(np.array_equal(want[k], clean[k]) for k in ("obs_kf", "kf_mp", "mp_replaced", "mp_found", "touched"))
    assert want["outcome"][-1] == 1 and want["n_fused"] == clean["n_fused"]
    cap = default_cap(mixed)
    outs, _, _ = resident_run([mixed], [cap])
    assert_same(outs[0], laid_out(mixed, want, cap), "bad ops")
    # an occupant that is no slot of the table: the op that meets it is skipped, the others go on
    i = fx["ops"][1][3]
    for v in (n_mp, -2):
        odd_t = dict(t, kf_mp=t["kf_mp"].copy())
        odd_t["kf_mp"][t["kf_mp_ptr"][2] + i] = v
        odd = dict(fx, t=odd_t)
        want = apply(odd_t, fx["x"], fx["ops"])
        assert want["status"] == BAD_SLOT and want["outcome"][1] == 0 and want["n_fused"] > 0
        cap = default_cap(odd)
        outs, _, _ = resident_run([odd], [cap])
        assert_same(outs[0], laid_out(odd, want, cap), "bad occupant")
    # an observation whose keypoint index lies outside its keyframe's row: it moves with its row, kf_mp is not written for it
    x = dict(fx["x"], obs_idx=fx["x"]["obs_idx"].copy())
    x["obs_idx"][t["obs_ptr"][1] + 1] = 10 ** 6                        # point 1's entry of keyframe 3, moved to point 0 by 1 -> 0
    odd = dict(fx, x=x)
    want = apply(t, x, fx["ops"])
    assert want["status"] == BAD_SLOT and 10 ** 6 in want["obs_idx"]
    cap = default_cap(odd)
    outs, _, _ = resident_run([odd], [cap])
    assert_same(outs[0], laid_out(odd, want, cap), "bad observations")


def test_the_list_builder_is_three_lines_of_numpy():
    """Targets back to back in two maps' lists: a target without queries, one without a match, stereo keypoints, a slice that does not fit."""
    import torch
    from weiner_slamit_v2_amd import api

    rng = np.random.default_rng(71)
    nf, q_cap, kp_cap, cap, n_maps = 6, 70, 300, 4 * 70 + 3, 2
    m = np.array([70, 0, 33, 64, 1, 5], np.int32)
    match = np.where(rng.random((nf, q_cap)) < 0.4, -1, rng.integers(0, kp_cap, (nf, q_cap))).astype(np.int32)
    match[0, 0], match[2] = 5, -1                                                        # a target whose search found nothing
    point = rng.integers(0, 5000, (nf, q_cap)).astype(np.int32)
    kps = np.zeros((nf, kp_cap), np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")]))
    kps["octave"] = rng.integers(0, 8, (nf, kp_cap))
    ur = np.where(rng.random((nf, kp_cap)) < 0.5, -1.0, rng.uniform(0, 600, (nf, kp_cap))).astype(np.float32)
    ur[0, match[0, 0]] = 0.0                                             # >= 0 is stereo
    fmap, fkf = np.array([0, 0, 0, 1, 1, 1], np.int32), np.array([7, 8, 9, 3, 4, 5], np.int32)
    base = np.array([0, 70, 140, 70, 0, cap - q_cap + 1], np.int32)      # map 1 out of order; the last slice does not fit
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for stereo in (True, False):
        t = {"m": cu(m), "match_kp": cu(match), "query_point": cu(point), "kps_un": cu(kps.view(np.uint8).reshape(nf, kp_cap, 28)), "kp_ur": cu(ur) if stereo else None,
             "frame_map": cu(fmap), "frame_kf": cu(fkf), "base": cu(base), "ops": cu(np.full((n_maps, cap, 20), 0x77, np.uint8)), "n": cu(np.full(n_maps, -5, np.int32)),
             "list_status": cu(np.full(nf, -1, np.int32))}
        api.fuse_list_batch_dev(t, n_maps, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = t["ops"].cpu().numpy().reshape(n_maps, cap * 20).view(api.REPLACE_DTYPE).reshape(n_maps, cap)
        want = np.full((n_maps, cap, 20), 0x77, np.uint8).reshape(n_maps, cap * 20).view(api.REPLACE_DTYPE).reshape(n_maps, cap).copy()
        for f in range(nf - 1):
            sl = want[fmap[f], base[f]:base[f] + q_cap]
            sl[:] = np.zeros(1, api.REPLACE_DTYPE)
            q = np.arange(q_cap) < m[f]
            idx = np.where(q, match[f], -1)
            sl["kind"], sl["a"], sl["b"], sl["idx"] = FUSE, np.where(q, point[f], -1), fkf[f], idx
            sl["octave"] = np.where(idx >= 0, kps["octave"][f][idx], 0)
            sl["weight"] = np.where((idx >= 0) & stereo & (ur[f][idx] >= 0), 2, 1)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert t["n"].cpu().numpy().tolist() == [210, 140] and t["list_status"].cpu().numpy().tolist() == [0, 0, 0, 0, 0, BAD_SLOT]
        assert (got[0, 0]["weight"] == 2) == stereo and np.all(got[0, 140:210]["idx"] == -1) and np.all(got[0, 70:140]["idx"] == -1)
