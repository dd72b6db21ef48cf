"""slamit_frustum on the device against the g++-built csrc/frustum.h and tests/frustum_ref.py.

Every operation of the header is an IEEE +, -, *, /, sqrt or its own log built from them, compiled without contraction on both
sides: the device's statuses, levels and floats equal the host build's BIT FOR BIT, and no tolerance appears below."""
import ctypes as C

import numpy as np
import pytest

from tests import frustum_ref as ref
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

OUT_FLOATS = ("proj", "view_cos", "uvr")
OUT_INTS = ("status", "level", "level_min", "level_max", "valid")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_as_header(out, h, n):
    """Device result `out` against the header's `h` on the first n points, bit for bit."""
    assert out["status"].shape == (n,) and out["proj"].shape == (n, 3) and out["uvr"].shape == (n, 3)
    assert np.array_equal(out["status"], h["status"][:n]), np.flatnonzero(out["status"] != h["status"][:n])
    assert np.array_equal(out["level"], h["level"][:n])
    assert np.array_equal(bits(out["proj"]), bits(h["proj"][:n])) and np.array_equal(bits(out["view_cos"]), bits(h["viewCos"][:n]))
    assert np.array_equal(bits(out["uvr"]), bits(h["uvr"][:n])) and np.array_equal(bits(out["uvr"][:, 2]), bits(h["r"][:n]))
    assert np.array_equal(out["level_min"], h["level_min"][:n]) and np.array_equal(out["level_max"], h["level_max"][:n])
    assert np.array_equal(out["valid"], h["valid"][:n])
    assert out["n_in_view"] == int((out["status"] == 0).sum())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 300])
def test_wavefront_and_workgroup_edges(n):
    out = api.frustum(ref.head(ref.fixture(ref.MIXED), n))
    same_as_header(out, ref.host_fixture(ref.MIXED), n)
    if n >= 65:
        assert set(int(s) for s in out["status"]) == set(range(8))


def test_a_ragged_batch_equals_its_problems_run_singly():
    full = ref.fixture(ref.MIXED)
    probs = [full, ref.head(full, 0), ref.fixture(ref.SMALL)]
    assert [int(p["n"]) for p in probs] == [300, 0, 65]
    batch = api.frustum_batch(probs)
    for pr, b in zip(probs, batch):
        one = api.frustum(pr)
        for k in OUT_INTS:
            assert np.array_equal(one[k], b[k]), k
        for k in OUT_FLOATS:
            assert np.array_equal(bits(one[k]), bits(b[k])), k
        assert one["n_in_view"] == b["n_in_view"]
    assert batch[0]["n_in_view"] > 50 and batch[1]["n_in_view"] == 0 and batch[2]["n_in_view"] > 10
    assert api.frustum_batch([]) == []
    assert api.lib().slamit_frustum_batch(0, 0, None, None) == 0


def test_every_fixture_in_one_batch():
    ks = range(len(ref.FIXTURES))
    outs = api.frustum_batch([ref.fixture(k) for k in ks])
    seen = set()
    for k, out in zip(ks, outs):
        a, n = ref.admissibility(k), ref.FIXTURES[k][1]
        r32, d = a["r32"], a["decided"]
        print("fixture %d: device differs from ref32 on %d statuses and %d levels of %d" %
              (k, int((out["status"] != r32["status"]).sum()), int((out["level"] != r32["level"]).sum()), n))
        assert np.array_equal(out["status"][d], r32["status"][d]) and np.array_equal(out["level"][d], r32["level"][d])
        for f, dev in (("u", out["proj"][:, 0]), ("v", out["proj"][:, 1]), ("uR", out["proj"][:, 2]), ("viewCos", out["view_cos"]), ("r", out["uvr"][:, 2])):
            assert np.array_equal(bits(dev)[d], bits(r32[f])[d]), (k, f)
        # the query arrays are what ORBmatcher::SearchByProjection builds from the stored members
        uvr, l0, l1, valid = ref.queries_of(out)
        assert np.array_equal(bits(out["uvr"]), bits(uvr)) and np.array_equal(out["level_min"], l0) and np.array_equal(out["level_max"], l1)
        assert np.array_equal(out["valid"], valid)
        same_as_header(out, ref.host_fixture(k), n)
        seen |= set(int(s) for s in out["status"])
    assert seen == set(range(8))


def test_argument_errors_launch_nothing():
    pr = ref.head(ref.fixture(ref.MIXED), 8)
    big = api.FRUSTUM_MAX_N + 1
    with pytest.raises(api.SlamitError, match="SLAMIT_FRUSTUM_MAX_N") as e:
        api.frustum(dict(pr, n=big, pos=np.ones((big, 3), np.float32), normal=np.ones((big, 3), np.float32), max_dist=np.ones(big, np.float32),
                         min_dist=np.ones(big, np.float32), skip=np.zeros(big, np.uint8)))
    assert "(-1)" in str(e.value)                                    # SLAMIT_ERR_ARG
    for nl in (0, 17):
        with pytest.raises(api.SlamitError, match="n_levels"):
            api.frustum(dict(pr, n_levels=nl, scale_factors=np.ones(nl, np.float32)))
    with pytest.raises(api.SlamitError, match="same length"):
        api.frustum(dict(pr, skip=pr["skip"][:5]))
    # negative n and a null array, straight through the C-ABI: SLAMIT_ERR_ARG, a message, and the outputs untouched
    P, R = api.FrustumProblem(), api.FrustumResult()
    C.memmove(C.byref(P.frame), api.frustum_frame_record(pr).ctypes.data, C.sizeof(api.FrustumFrame))
    keep = {k: np.ascontiguousarray(pr[k]) for k in ("pos", "normal", "max_dist", "min_dist", "skip")}
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    outs = {"status": np.full(8, 99, np.uint8), "proj": np.full((8, 3), 7.0, np.float32), "view_cos": np.full(8, 7.0, np.float32),
            "level": np.full(8, 99, np.int32), "uvr": np.full((8, 3), 7.0, np.float32), "level_min": np.full(8, 99, np.int32),
            "level_max": np.full(8, 99, np.int32), "valid": np.full(8, 99, np.uint8)}
    for k, a in outs.items():
        setattr(R, k, a.ctypes.data)
    R.n_in_view = -5

    def untouched():
        return all(np.all(a == (7.0 if a.dtype == np.float32 else 99)) for a in outs.values()) and R.n_in_view == -5

    P.n = -1
    assert api.lib().slamit_frustum(0, C.byref(P), C.byref(R)) == -1 and b"negative count" in api.lib().slamit_last_error() and untouched()
    P.n = 8
    for field in ("normal", "skip"):
        setattr(P, field, None)
        assert api.lib().slamit_frustum(0, C.byref(P), C.byref(R)) == -1 and b"null array" in api.lib().slamit_last_error() and untouched()
        setattr(P, field, keep[field].ctypes.data)
    R.uvr = None
    assert api.lib().slamit_frustum(0, C.byref(P), C.byref(R)) == -1 and b"null array" in api.lib().slamit_last_error() and untouched()
    R.uvr = outs["uvr"].ctypes.data
    assert api.lib().slamit_frustum(0, C.byref(P), C.byref(R)) == 0            # the same record, whole again
    assert np.all(outs["status"] <= 7) and R.n_in_view == int((outs["status"] == 0).sum())
    assert api.lib().slamit_frustum_batch_dev(0, None, None) == -1


def _chain_tensors(probs, hosts, sides, q_cap, kp_cap):
    import torch

    B = len(probs)
    t = dict(frames=np.zeros(B, api.FRUSTUM_FRAME_DTYPE), m=np.zeros(B, np.int32), pos=np.zeros((B, 3, q_cap), np.float32), normal=np.zeros((B, 3, q_cap), np.float32),
             max_dist=np.zeros((B, q_cap), np.float32), min_dist=np.zeros((B, q_cap), np.float32), skip=np.zeros((B, q_cap), np.uint8),
             n=np.zeros(B, np.int32), desc=np.zeros((B, kp_cap, 32), np.uint8), kp_taken=np.zeros((B, kp_cap), np.uint8),
             qdesc=np.zeros((B, q_cap, 32), np.uint8), takes=np.ones((B, q_cap), np.uint8))
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    # the host-built route's query arrays: the g++-built header's
    hq = dict(uvr=np.zeros((B, q_cap, 3), np.float32), level_min=np.zeros((B, q_cap), np.int32), level_max=np.zeros((B, q_cap), np.int32),
              valid=np.zeros((B, q_cap), np.uint8))
    for f, (pr, h, (frame, qdesc, takes)) in enumerate(zip(probs, hosts, sides)):
        m, n = int(pr["n"]), len(frame["kp_xy"])
        t["frames"][f] = api.frustum_frame_record(pr)[0]
        t["m"][f], t["n"][f] = m, n
        t["pos"][f, :, :m], t["normal"][f, :, :m] = pr["pos"].T, pr["normal"].T
        t["max_dist"][f, :m], t["min_dist"][f, :m], t["skip"][f, :m] = pr["max_dist"], pr["min_dist"], pr["skip"]
        kps["x"][f, :n], kps["y"][f, :n], kps["octave"][f, :n] = frame["kp_xy"][:, 0], frame["kp_xy"][:, 1], frame["kp_octave"]
        t["desc"][f, :n], t["kp_taken"][f, :n] = frame["desc"], frame["kp_taken"]
        t["qdesc"][f, :m], t["takes"][f, :m] = qdesc, takes
        for k in hq:
            hq[k][f, :m] = h[k]
    d = {k: torch.from_numpy(v.view(np.float32).reshape(B, -1) if k == "frames" else v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, q_cap), dtype=torch.uint8, device="cuda")
    return d, {k: torch.from_numpy(v).cuda() for k, v in hq.items()}


def test_the_device_chain_equals_the_host_built_route():
    """frustum_batch_dev -> guided_search_batch_dev with nothing but device pointers in between, against the same search fed with
    query arrays built on the host, and against per-frame guided_search calls on COMPACTED queries: a query with valid = 0 at its own
    index changes nothing, so leaving the queries where the points are keeps the reference's order."""
    import torch

    full = ref.fixture(ref.MIXED)
    probs = [full, ref.head(full, 0), ref.fixture(ref.SMALL)]
    hosts = [ref.host_fixture(ref.MIXED), ref.host_points(probs[1]), ref.host_fixture(ref.SMALL)]
    sides = [ref.search_side(pr, h, 30 + f) for f, (pr, h) in enumerate(zip(probs, hosts))]
    q_cap, kp_cap, B = 320, 512, 3
    assert [int(p["n"]) for p in probs] == [300, 0, 65] and max(len(s[0]["kp_xy"]) for s in sides) <= kp_cap
    d, hq = _chain_tensors(probs, hosts, sides, q_cap, kp_cap)
    bounds = tuple(sides[0][0][k] for k in ("min_x", "min_y", "inv_w", "inv_h"))
    results = []
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for route in ("device", "host"):
        t = dict(d, match_kp=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), nmatches=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        if route == "device":
            t.update(uvr=torch.full((B, q_cap, 3), -7.0, device="cuda"), level_min=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"),
                     level_max=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), valid=torch.full((B, q_cap), 7, dtype=torch.uint8, device="cuda"),
                     status=torch.full((B, q_cap), 99, dtype=torch.uint8, device="cuda"), n_in_view=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
            api.frustum_batch_dev(t, stream=s.cuda_stream)
        else:
            t.update(hq)
        api.ORBmatcher.guided_search_batch_dev(t, bounds, 100, True, 0.8, stream=s.cuda_stream)
        s.synchronize()
        results.append((t["match_kp"].cpu().numpy(), t["nmatches"].cpu().numpy()))
        if route == "device":
            for f, (pr, h) in enumerate(zip(probs, hosts)):
                m = int(pr["n"])
                assert np.array_equal(t["status"][f, :m].cpu().numpy(), h["status"]) and np.all(t["status"][f, m:].cpu().numpy() == 99)
                assert np.array_equal(bits(t["uvr"][f, :m].cpu().numpy()), bits(h["uvr"])) and np.all(t["valid"][f, m:].cpu().numpy() == 7)
                assert np.array_equal(t["valid"][f, :m].cpu().numpy(), h["valid"])
                assert int(t["n_in_view"][f]) == int((h["status"] == 0).sum())
    (dev_match, dev_nm), (host_match, host_nm) = results
    assert np.array_equal(dev_nm, host_nm)
    for f, (pr, h, (frame, qdesc, takes)) in enumerate(zip(probs, hosts, sides)):
        m = int(pr["n"])
        assert np.array_equal(dev_match[f, :m], host_match[f, :m])
        keep = np.flatnonzero(h["valid"])
        q = dict(uvr=h["uvr"][keep], level_min=h["level_min"][keep], level_max=h["level_max"][keep], desc=qdesc[keep], takes=takes[keep])
        gm, gn, _ = api.ORBmatcher.guided_search(frame, q, 100, True, 0.8) if len(keep) and len(frame["kp_xy"]) else (np.zeros(0, np.int32), 0, None)
        want = np.full(m, -1, np.int32)
        want[keep] = gm
        assert np.array_equal(dev_match[f, :m], want) and dev_nm[f] == gn
    assert dev_nm[0] > 30 and dev_nm[1] == 0 and dev_nm[2] > 5
