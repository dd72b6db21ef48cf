"""slamit_map_edit_apply and slamit_map_edit_batch_dev on the GPU against the literal sequential restatement (tests/map_edit_ref.py) on
every fixture: the new table and its three columns, mp_bad, mp_nobs, mp_ref_kf, kf_mp, the per-point status, touched and the counts,
all exact; the capacity gate; the bytes past the counts; the same bytes from the same input twice."""
import numpy as np
import pytest

from tests.map_edit_fixtures import all_fixtures, by_name, expected
from tests.map_edit_host import FILL, OUT_TYPES, assert_same, default_cap, fills, laid_out, of_api, records
from tests.map_edit_ref import ADD_OBS, BAD_SLOT, ERASE_OBS, MATCH, TABLE_OVERFLOW, apply

pytestmark = pytest.mark.gpu
NAMES = [fx["name"] for fx in all_fixtures()]


@pytest.mark.parametrize("name", NAMES)
def test_the_host_form_equals_the_restatement(name):
    from weiner_slamit_v2_amd import api

    fx, cap = by_name(name), default_cap(by_name(name)) + 3
    out = api.map_edit(fx["t"], fx["x"], records(fx["edits"]), obs_cap_out=cap, fill=fills(fx, cap))
    want = expected(name)
    assert_same(of_api(out), laid_out(fx, want, cap), name)
    # what api.map_edit hands back is a map: the readers' tables
    assert np.array_equal(out["obs_ptr"], want["obs_ptr"]) and np.array_equal(out["obs_kf"], want["obs_kf"]) and np.array_equal(out["touched"], want["touched"])
    rec, keep = api._map_index_host(dict(fx["t"], **{k: out[k] for k in ("obs_ptr", "obs_kf", "mp_bad", "kf_mp")}))
    assert rec.n_mp == fx["t"]["n_mp"] and len(keep["obs_kf"]) == want["n_obs_out"]


def resident_run(fxs, caps, pad=5):
    """One call over the maps of fxs, list m cut to nothing it is not: every map with its own length.  -> per map the arrays of
    OUT_KEYS in full (the output columns: the whole other buffer set), and the EditIndex objects."""
    import torch
    from weiner_slamit_v2_amd import api

    B = len(fxs)
    maps = [api.MapIndex(fx["t"]) for fx in fxs]
    eds = [api.EditIndex(fx["x"], mi, cap) for fx, mi, cap in zip(fxs, maps, caps)]
    for ei in eds:
        for key, name in (("obs_ptr", "obs_ptr_out"), ("obs_kf", "obs_kf_out"), ("obs_idx", "obs_idx_out"), ("obs_octave", "obs_octave_out"), ("obs_weight", "obs_weight_out")):
            ei.sets[1][key].fill_(FILL[name])
    cap = max(len(fx["edits"]) for fx in fxs) + pad
    mp_cap = max(fx["t"]["n_mp"] for fx in fxs) + 2
    kfmp_cap = max(len(fx["t"]["kf_mp"]) for fx in fxs)
    h_edits = np.full((B, cap, 24), 0xff, np.uint8)
    for m, fx in enumerate(fxs):
        h_edits[m, :len(fx["edits"])] = records(fx["edits"]).view(np.uint8).reshape(-1, 24)
    cu = lambda a: torch.from_numpy(a).cuda()
    t = {"edits": cu(h_edits), "n": cu(np.array([len(fx["edits"]) for fx in fxs], np.int32)), "status_mp": cu(np.full((B, mp_cap), FILL["status_mp"], np.int32)),
         "touched": cu(np.full((B, mp_cap), FILL["touched"], np.int32)), "n_touched": cu(np.full(B, FILL["n_touched"], np.int32)),
         "n_obs_out": cu(np.full(B, -1, np.int32)), "status": cu(np.full(B, -1, np.int32)), "kfmp_cap": kfmp_cap,
         "workspace": torch.full((api.map_edit_workspace(B, cap, mp_cap, kfmp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}   # dirty: the call clears what it needs
    api.map_edit_batch_dev(maps, eds, t, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outs = []
    for m, (fx, ei) in enumerate(zip(fxs, eds)):
        n_mp, n_kfmp = fx["t"]["n_mp"], len(fx["t"]["kf_mp"])
        nxt = ei.sets[1]
        got = {"obs_ptr_out": nxt["obs_ptr"].cpu().numpy()[:n_mp + 1], "mp_bad": ei.t["mp_bad"].cpu().numpy()[:n_mp], "mp_nobs": ei.t["mp_nobs"].cpu().numpy()[:n_mp],
               "mp_ref_kf": ei.t["mp_ref_kf"].cpu().numpy()[:n_mp], "kf_mp": ei.t["kf_mp"].cpu().numpy()[:n_kfmp]}
        for key in ("obs_kf", "obs_idx", "obs_octave", "obs_weight"):
            got[key + "_out"] = nxt[key].cpu().numpy()[:ei.obs_cap]
        row = lambda key: t[key][m].cpu().numpy()
        assert np.all(row("status_mp")[n_mp:] == FILL["status_mp"]) and np.all(row("touched")[n_mp:] == FILL["touched"])   # past the map's points
        got.update(status_mp=row("status_mp")[:n_mp], touched=row("touched")[:n_mp], n_touched=int(row("n_touched")), n_obs_out=int(row("n_obs_out")), status=int(row("status")))
        outs.append(got)
    return outs, eds


@pytest.mark.parametrize("part", (0, 1))
def test_the_resident_form_equals_the_restatement(part):
    """One call over several maps with lists of different lengths (among them none); every fixture is in one of the two calls."""
    fxs = list(all_fixtures()[:8] if part == 0 else all_fixtures()[8:] + all_fixtures()[:2])
    assert len(all_fixtures()) <= 16 and len({len(fx["edits"]) for fx in fxs}) > 1
    caps = [default_cap(fx) + 3 for fx in fxs]
    outs, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        assert_same(got, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_one_below_the_need_nothing_is_written():
    from weiner_slamit_v2_amd import api

    for name in ("single", "shuffled"):
        fx, need = by_name(name), expected(name)["n_obs_out"]
        for cap in (need - 1, need):
            want = expected(name, cap - need)
            assert bool(want["status"] & TABLE_OVERFLOW) == (cap < need)
            out = api.map_edit(fx["t"], fx["x"], records(fx["edits"]), obs_cap_out=cap, fill=fills(fx, cap))
            assert_same(of_api(out), laid_out(fx, want, cap), "%s cap %d" % (name, cap))
    # resident: the map whose table does not fit keeps every byte, its neighbours in the same call are written
    fxs = [by_name("single"), by_name("shuffled"), by_name("limits")]
    caps = [default_cap(fxs[0]), expected("shuffled")["n_obs_out"] - 1, expected("limits")["n_obs_out"]]
    outs, _ = resident_run(fxs, caps)
    for fx, cap, got in zip(fxs, caps, outs):
        want = expected(fx["name"], cap - expected(fx["name"])["n_obs_out"])
        assert_same(got, laid_out(fx, want, cap), fx["name"])
    assert outs[1]["status"] == TABLE_OVERFLOW and outs[1]["n_obs_out"] == caps[1] + 1 and outs[0]["status"] == 0 == outs[2]["status"]


def test_the_same_call_twice_gives_the_same_bytes():
    """The bucket's order and the kf_mp words come from atomics whose order differs from run to run: none of it may show."""
    fxs = [by_name("shuffled"), by_name("limits"), by_name("single")]
    caps = [default_cap(fx) for fx in fxs]
    a, _ = resident_run(fxs, caps)
    b, _ = resident_run(fxs, caps)
    for fx, cap, x, y in zip(fxs, caps, a, b):
        assert_same(x, y, fx["name"])
        assert_same(x, laid_out(fx, expected(fx["name"]), cap), fx["name"])


def test_a_slot_outside_its_table_is_skipped():
    """The device cannot be shown its list first: such an edit does nothing but set the bit."""
    fx = by_name("single")
    t, n_kf, n_mp = fx["t"], fx["t"]["n_kf"], fx["t"]["n_mp"]
    row = int(t["kf_mp_ptr"][2] - t["kf_mp_ptr"][1])
    bad = [(ADD_OBS, MATCH, n_mp, 0, 0, 0, 1), (ERASE_OBS, MATCH, -1, 0, 0, 0, 0), (ADD_OBS, MATCH, 1, n_kf, 0, 0, 1), (ERASE_OBS, 0, 1, -1, 0, 0, 0),
           (ADD_OBS, MATCH, 2, 1, row, 0, 1), (ADD_OBS, MATCH, 2, 1, -1, 0, 1), (ADD_OBS, MATCH, 14, 6, 0, 0, 3), (9, 0, 0, 0, 0, 0, 1)]
    edits = list(fx["edits"])
    for i, e in enumerate(bad):
        edits.insert(2 * i + 1, e)
    mixed = dict(fx, edits=edits)
    want = dict(apply(fx["t"], fx["x"], fx["edits"]))
    want["status_mp"] = want["status_mp"].copy()
    want["status_mp"][[1, 2, 14, 0]] |= BAD_SLOT
    want["status"] = BAD_SLOT
    cap = default_cap(mixed)
    outs, _ = resident_run([mixed], [cap])
    assert_same(outs[0], laid_out(mixed, want, cap), "bad slots")
