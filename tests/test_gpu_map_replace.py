"""slamit_map_replace_apply and slamit_map_replace_batch_dev on the GPU against the literal sequential restatement
(tests/map_replace_ref.py) on every fixture: the new table and its three columns, mp_bad, mp_nobs, mp_found, mp_visible, mp_replaced,
kf_mp, moved and erased op by op, touched and the counts, all exact; the all-or-nothing gate of each overflow; the bytes past the
counts; the same bytes from the same input twice; slots outside their tables; slamit_check_replaced in both forms."""
import numpy as np
import pytest

from tests.map_replace_fixtures import all_fixtures, by_name, expected
from tests.map_replace_host import FILL, INPLACE, assert_same, default_cap, fills, laid_out, of_api, records
from tests.map_replace_ref import ADD_OBS, BAD_SLOT, OBS_OVERFLOW, OP_OVERFLOW, REPLACE, TABLE_OVERFLOW, apply, check_replaced

pytestmark = pytest.mark.gpu
NAMES = [fx["name"] for fx in all_fixtures()]


def want_of(fx, cap):
    full = expected(fx["name"])
    return full if "n_obs_out" not in full else expected(fx["name"], cap - full["n_obs_out"])


@pytest.mark.parametrize("name", NAMES)
def test_the_host_form_equals_the_restatement(name):
    from weiner_slamit_v2_amd import api

    fx, cap = by_name(name), default_cap(by_name(name)) + 3
    out = api.map_replace(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=fills(fx, cap))
    want = expected(name)
    assert_same(of_api(out), laid_out(fx, want, cap), name)
    if not want["status"] & api.REPLACE_REFUSED:                       # what api.map_replace hands back is a map: the readers' tables
        assert np.array_equal(out["obs_ptr"], want["obs_ptr"]) and np.array_equal(out["obs_kf"], want["obs_kf"]) and np.array_equal(out["touched"], want["touched"])
        rec, keep = api._map_index_host(dict(fx["t"], **{k: out[k] for k in ("obs_ptr", "obs_kf", "mp_bad", "kf_mp")}))
        assert rec.n_mp == fx["t"]["n_mp"] and len(keep["obs_kf"]) == want["n_obs_out"]


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
    t = {"ops": cu(h_ops), "n": cu(np.array([len(fx["ops"]) for fx in fxs], np.int32)), "moved": cu(np.full((B, cap), FILL["moved"], np.int32)),
         "erased": cu(np.full((B, cap), FILL["erased"], np.int32)), "touched": cu(np.full((B, mp_cap), FILL["touched"], np.int32)),
         "n_touched": cu(np.full(B, FILL["n_touched"], np.int32)), "n_obs_out": cu(np.full(B, FILL["n_obs_out"], np.int32)), "status": cu(np.full(B, -1, np.int32)),
         "kfmp_cap": kfmp_cap,
         "workspace": torch.full((api.map_replace_workspace(B, cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}   # dirty: the call clears what it needs
    api.map_replace_batch_dev(maps, reps, t, stream=torch.cuda.current_stream().cuda_stream)
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
        assert np.all(row("touched")[n_mp:] == FILL["touched"]) and np.all(row("moved")[n:] == FILL["moved"]) and np.all(row("erased")[n:] == FILL["erased"])   # past the map's own
        got.update(moved=row("moved")[:n], erased=row("erased")[:n], touched=row("touched")[:n_mp], n_touched=int(row("n_touched")), n_obs_out=int(row("n_obs_out")),
                   status=int(row("status")))
        outs.append(got)
    return outs, eds, reps


@pytest.mark.parametrize("part", (0, 1, 2))
def test_the_resident_form_equals_the_restatement(part):
    """One call over several maps with lists of different lengths (among them none); every fixture is in one of the three calls."""
    every = all_fixtures()
    fxs = list(every[:8] if part == 0 else every[8:16] if part == 1 else every[16:] + every[:3])
    assert len(every) <= 24 and len({len(fx["ops"]) for fx in fxs}) > 1
    caps = [default_cap(fx) + 3 for fx in fxs]
    outs, _, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_each_overflow_refuses_its_map_alone():
    """The map that meets a ceiling keeps every byte; its neighbours in the same call are written."""
    from weiner_slamit_v2_amd import api

    for name in ("single", "indep"):
        fx, need = by_name(name), expected(name)["n_obs_out"]
        for cap in (need - 1, need):
            want = expected(name, cap - need)
            assert bool(want["status"] & TABLE_OVERFLOW) == (cap < need)
            out = api.map_replace(fx["t"], fx["x"], records(fx["ops"]), obs_cap_out=cap, fill=fills(fx, cap))
            assert_same(of_api(out), laid_out(fx, want, cap), "%s cap %d" % (name, cap))
    fxs = [by_name(n) for n in ("single", "fan65", "chains", "row513", "indep", "row513_in", "add_order", "row512_add")]
    caps = [default_cap(fx) for fx in fxs]
    caps[4] = expected("indep")["n_obs_out"] - 1
    caps[6] = expected("add_order")["n_obs_out"]
    outs, _, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, want_of(fx, cap), cap), fx["name"])
    assert [o["status"] for o in outs] == [0, OP_OVERFLOW, 0, OBS_OVERFLOW, TABLE_OVERFLOW, OBS_OVERFLOW, 0, OBS_OVERFLOW] and outs[4]["n_obs_out"] == caps[4] + 1
    for i in (1, 3, 4, 5, 7):
        for key in INPLACE:
            src = fxs[i]["t"] if key in ("mp_bad", "kf_mp") else fxs[i]["x"]
            assert np.array_equal(outs[i][key], np.asarray(src[key]).reshape(-1)), (fxs[i]["name"], key)


def test_lists_at_the_ceiling_of_ops():
    """SLAMIT_REPLACE_MAX_OPS ops per list, AT the ceiling, two maps in one call: 16,384 independent ops in one round (no point named twice),
    and a chain 16,384 deep in as many rounds, the slowest list there is (the whole test, fixtures and restatement included, took 1.0 s on
    one MI355X)."""
    from tests.map_replace_fixtures import ceiling_fixtures
    from weiner_slamit_v2_amd import api

    fxs = list(ceiling_fixtures())
    assert all(len(fx["ops"]) == api.REPLACE_MAX_OPS for fx in fxs)
    caps = [default_cap(fx) for fx in fxs]
    outs, _, _ = resident_run(fxs, caps, pad=0)
    for fx, cap, got in zip(fxs, caps, outs):
        want = apply(fx["t"], fx["x"], fx["ops"])
        assert want["status"] == 0 and want["moved"].sum() > 10000
        assert_same(got, laid_out(fx, want, cap), fx["name"])


def test_the_same_call_twice_gives_the_same_bytes():
    """The buckets' order, the kf_mp words and which wavefront takes which op differ from run to run: none of it may show."""
    fxs = [by_name(n) for n in ("ops1025", "deep", "single", "indep", "fan64")]
    caps = [default_cap(fx) for fx in fxs]
    a, _, _ = resident_run(fxs, caps)
    b, _, _ = resident_run(fxs, caps)
    for fx, cap, x, y in zip(fxs, caps, a, b):
        assert_same(x, y, fx["name"])
        assert_same(x, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_a_slot_outside_its_table_is_skipped():
    """The device cannot be shown its list or its tables first: such an op does nothing but set the bit; an observation outside kf_mp
    is carried along without its write."""
    fx = by_name("single")
    t, n_kf, n_mp = fx["t"], fx["t"]["n_kf"], fx["t"]["n_mp"]
    row = int(t["kf_mp_ptr"][2] - t["kf_mp_ptr"][1])
    bad = [(REPLACE, n_mp, 0, 0, 0, 0), (REPLACE, 0, -1, 0, 0, 0), (REPLACE, -1, -1, 0, 0, 0), (ADD_OBS, n_mp, 0, 0, 0, 1), (ADD_OBS, 1, n_kf, 0, 0, 1),
           (ADD_OBS, 1, -1, 0, 0, 1), (ADD_OBS, 2, 1, row, 0, 1), (ADD_OBS, 2, 1, -1, 0, 1), (ADD_OBS, 13, 6, 0, 0, 3), (ADD_OBS, 13, 6, 0, 0, 0), (0, 0, 1, 0, 0, 0),
           (3, 0, 1, 0, 0, 0)]
    ops = list(fx["ops"])
    for i, e in enumerate(bad):
        ops.insert(min(2 * i + 1, len(ops)), e)
    mixed = dict(fx, ops=ops)
    want = apply(fx["t"], fx["x"], ops)
    clean = apply(fx["t"], fx["x"], fx["ops"])
    assert want["status"] == BAD_SLOT and all(np.array_equal(want[k], clean[k]) for k in ("obs_kf", "kf_mp", "mp_replaced", "mp_found", "touched"))
    cap = default_cap(mixed)
    outs, _, _ = resident_run([mixed], [cap])
    assert_same(outs[0], laid_out(mixed, want, cap), "bad ops")
    # an observation whose keypoint index lies outside its keyframe's row: it moves with its row, kf_mp is not written for it
    x = dict(fx["x"], obs_idx=fx["x"]["obs_idx"].copy())
    x["obs_idx"][t["obs_ptr"][0] + 1] = 10 ** 6                        # point 0's entry of keyframe 1, moved to point 1 by 0 -> 1
    x["obs_idx"][t["obs_ptr"][16]] = -3                                # point 16's entry of keyframe 0, which dies
    odd = dict(fx, x=x)
    want = apply(t, x, fx["ops"])
    assert want["status"] == BAD_SLOT and 10 ** 6 in want["obs_idx"] and np.array_equal(want["moved"], clean["moved"])
    outs, _, _ = resident_run([odd], [cap])
    assert_same(outs[0], laid_out(odd, want, cap), "bad observations")


def test_moved_and_erased_follow_the_walk_op_by_op():
    """Every prefix of a list: the state after k ops is the sequential walk's, and moved / erased of op k are what it did there."""
    from weiner_slamit_v2_amd import api

    for name in ("chains", "add_order", "shared"):
        fx = by_name(name)
        for k in range(len(fx["ops"]) + 1):
            pre = dict(fx, ops=fx["ops"][:k])
            cap = default_cap(pre)
            want = apply(fx["t"], fx["x"], pre["ops"])
            out = api.map_replace(fx["t"], fx["x"], records(pre["ops"]), obs_cap_out=cap, fill=fills(pre, cap))
            assert_same(of_api(out), laid_out(pre, want, cap), "%s[:%d]" % (name, k))
            if k:
                full = expected(name)
                assert out["moved"][k - 1] == full["moved"][k - 1] and out["erased"][k - 1] == full["erased"][k - 1]


def test_check_replaced_in_both_forms():
    import torch
    from weiner_slamit_v2_amd import api

    rng = np.random.default_rng(32)
    n_mps = (300, 70000)
    reps = []
    for n_mp in n_mps:
        rep = np.where(rng.random(n_mp) < 0.3, rng.integers(0, n_mp, n_mp), -1).astype(np.int32)
        rep[7], rep[9], rep[11] = 9, 11, -1                            # a chain of two: ONE hop is followed
        reps.append(rep)
    cap = 1000
    frames = [np.where(rng.random(n) < 0.2, -1, rng.integers(0, n_mps[m], n)).astype(np.int32) for m, n in ((0, 1000), (1, 257), (0, 0), (1, 64))]
    frames[0][:3] = [7, 9, -1]
    fmap = [0, 1, 0, 1]
    for f, m in zip(frames, fmap):
        got, st = api.check_replaced(reps[m], f)
        assert st == 0 and np.array_equal(got, check_replaced(reps[m], f))
    assert api.check_replaced(reps[0], frames[0])[0][:3].tolist() == [9, 11, -1]
    outside = frames[1].copy()
    outside[[5, 6]] = [n_mps[1], -2]
    h = np.full((5, cap), -77, np.int32)
    for i, f in enumerate(frames + [outside]):
        h[i, :len(f)] = f
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {"frame_mp": cu(h), "frame_map": cu(np.array(fmap + [1], np.int32)), "n": cu(np.array([len(f) for f in frames] + [len(outside)], np.int32)),
         "status": cu(np.full(5, -1, np.int32))}
    api.check_replaced_batch_dev([cu(r) for r in reps], t, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, st = t["frame_mp"].cpu().numpy(), t["status"].cpu().numpy()
    for i, (f, m) in enumerate(zip(frames, fmap)):
        assert np.array_equal(got[i, :len(f)], check_replaced(reps[m], f)) and np.all(got[i, len(f):] == -77) and st[i] == 0
    want = check_replaced(reps[1], np.where((outside < -1) | (outside >= n_mps[1]), -1, outside))
    want[[5, 6]] = [n_mps[1], -2]
    assert np.array_equal(got[4, :len(outside)], want) and st[4] == BAD_SLOT
