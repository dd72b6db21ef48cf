"""slamit_project* and slamit_rotation_check_batch_dev on the device against the g++-built csrc/project.h, tests/project_ref.py and
tests/rotation_ref.py.

Every operation of the header is an IEEE +, -, *, /, sqrt or frustum.h's own log built from them, compiled without contraction on
both sides: the device's statuses, levels and floats equal the host build's BIT FOR BIT, and no tolerance appears below."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import project_ref as ref
from tests import rotation_ref as rot
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

OUT_FLOATS = ("proj", "uvr")
OUT_INTS = ("status", "level", "level_min", "level_max", "valid")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_as_header(out, h, n):
    """Device result `out` against the header's `h` on the first n points, bit for bit."""
    assert out["status"].shape == (n,) and out["proj"].shape == (n, 2) and out["uvr"].shape == (n, 3)
    assert np.array_equal(out["status"], h["status"][:n]), np.flatnonzero(out["status"] != h["status"][:n])
    assert np.array_equal(out["level"], h["level"][:n])
    assert np.array_equal(bits(out["proj"]), bits(h["proj"][:n]))
    assert np.array_equal(bits(out["uvr"]), bits(h["uvr"][:n])) and np.array_equal(bits(out["uvr"][:, 2]), bits(h["r"][:n]))
    assert np.array_equal(out["level_min"], h["level_min"][:n]) and np.array_equal(out["level_max"], h["level_max"][:n])
    assert np.array_equal(out["valid"], h["valid"][:n])
    if "n_valid" in out:
        assert out["n_valid"] == int((out["status"] == 0).sum())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("form", range(6))
def test_wavefront_and_workgroup_edges(form, n):
    k = ref.first_fixture(form)
    out = api.project(ref.head(ref.fixture(k), n))
    same_as_header(out, ref.host_fixture(k), n)
    if n >= 65:
        assert set(int(s) for s in out["status"]) == ref.POSSIBLE[form]


def test_every_fixture_and_the_boundary_points_in_one_batch():
    probs = [ref.fixture(k) for k in range(len(ref.FIXTURES))] + [ref.boundary_fixture(form)[0] for form in range(6)]
    hosts = [ref.host_fixture(k) for k in range(len(ref.FIXTURES))] + [ref.host_points(pr) for pr in probs[len(ref.FIXTURES):]]
    outs = api.project_batch(probs)
    for pr, out, h in zip(probs, outs, hosts):
        same_as_header(out, h, int(pr["n"]))
    for form in range(6):
        assert outs[len(ref.FIXTURES) + form]["status"].tolist() == ref.boundary_fixture(form)[1]
    for k in range(len(ref.FIXTURES)):                              # and the restatement itself, which every point of a fixture is decided by
        r32 = ref.admissibility(k)["r32"]
        assert np.array_equal(outs[k]["status"], r32["status"]) and np.array_equal(outs[k]["level"], r32["level"])
        assert np.array_equal(bits(outs[k]["proj"][:, 0]), bits(r32["u"])) and np.array_equal(bits(outs[k]["uvr"][:, 2]), bits(r32["r"]))


def test_a_ragged_batch_of_all_six_forms_equals_its_problems_run_singly():
    ns = (300, 0, 1, 65, 257, 64)
    probs = [ref.head(ref.fixture(ref.first_fixture(form)), n) for form, n in enumerate(ns)]
    assert [int(p["form"]) for p in probs] == list(range(6)) and [int(p["n"]) for p in probs] == list(ns)
    batch = api.project_batch(probs)
    for form, (pr, b) in enumerate(zip(probs, batch)):
        one = api.project(pr)
        for k in OUT_INTS:
            assert np.array_equal(one[k], b[k]), k
        for k in OUT_FLOATS:
            assert np.array_equal(bits(one[k]), bits(b[k])), k
        assert one["n_valid"] == b["n_valid"]
        same_as_header(b, ref.host_fixture(ref.first_fixture(form)), ns[form])
    assert batch[0]["n_valid"] > 50 and batch[1]["n_valid"] == 0 and batch[4]["n_valid"] > 30
    assert api.project_batch([]) == []
    assert api.lib().slamit_project_batch(0, 0, None, None) == 0


def test_argument_errors_launch_nothing():
    pr = ref.head(ref.fixture(ref.first_fixture(ref.FUSE)), 8)
    big = api.PROJECT_MAX_N + 1
    with pytest.raises(api.SlamitError, match="SLAMIT_PROJECT_MAX_N") as e:
        api.project(dict(pr, n=big, pos=np.ones((big, 3), np.float32), normal=np.ones((big, 3), np.float32), max_dist=np.ones(big, np.float32),
                         min_dist=np.ones(big, np.float32), skip=np.zeros(big, np.uint8)))
    assert "(-1)" in str(e.value)                                    # SLAMIT_ERR_ARG
    for nl in (0, 17):
        with pytest.raises(api.SlamitError, match="n_levels"):
            api.project(dict(pr, n_levels=nl, scale_factors=np.ones(nl, np.float32)))
    for form in (-1, 6):
        with pytest.raises(api.SlamitError, match="unknown form"):
            api.project(dict(pr, form=form))
    for direction in (-1, 3):
        with pytest.raises(api.SlamitError, match="unknown direction"):
            api.project(dict(pr, direction=direction))
    with pytest.raises(api.SlamitError, match="same length"):
        api.project(dict(pr, skip=pr["skip"][:5]))
    with pytest.raises(api.SlamitError, match="null array"):          # FUSE reads the normals
        api.project(dict(pr, normal=None))
    with pytest.raises(api.SlamitError, match="null array"):          # LAST_FRAME reads the octaves
        api.project(dict(pr, form=ref.LAST_FRAME))
    same_as_header(api.project(dict(pr, form=ref.RELOC, normal=None)), ref.host_points(dict(pr, form=ref.RELOC)), 8)   # RELOC does not
    # negative n and a null array, straight through the C-ABI: SLAMIT_ERR_ARG, a message, and the outputs untouched
    P, R = api.ProjectProblem(), api.ProjectResult()
    C.memmove(C.byref(P.camera), api.project_camera_record(pr).ctypes.data, C.sizeof(api.ProjectCamera))
    keep = {k: np.ascontiguousarray(pr[k]) for k in ("pos", "normal", "max_dist", "min_dist", "skip")}
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    outs = {"status": np.full(8, 99, np.uint8), "proj": np.full((8, 2), 7.0, np.float32), "level": np.full(8, 99, np.int32), "uvr": np.full((8, 3), 7.0, np.float32),
            "level_min": np.full(8, 99, np.int32), "level_max": np.full(8, 99, np.int32), "valid": np.full(8, 99, np.uint8)}
    for k, a in outs.items():
        setattr(R, k, a.ctypes.data)
    R.n_valid = -5

    def untouched():
        return all(np.all(a == (7.0 if a.dtype == np.float32 else 99)) for a in outs.values()) and R.n_valid == -5

    P.n = -1
    assert api.lib().slamit_project(0, C.byref(P), C.byref(R)) == -1 and b"negative count" in api.lib().slamit_last_error() and untouched()
    P.n = 8
    for field in ("pos", "normal", "min_dist", "skip"):
        setattr(P, field, None)
        assert api.lib().slamit_project(0, C.byref(P), C.byref(R)) == -1 and b"null array" in api.lib().slamit_last_error() and untouched()
        setattr(P, field, keep[field].ctypes.data)
    R.uvr = None
    assert api.lib().slamit_project(0, C.byref(P), C.byref(R)) == -1 and b"null array" in api.lib().slamit_last_error() and untouched()
    R.uvr = outs["uvr"].ctypes.data
    P.camera.form = 9
    assert api.lib().slamit_project(0, C.byref(P), C.byref(R)) == -1 and b"unknown form" in api.lib().slamit_last_error() and untouched()
    P.camera.form = ref.FUSE
    assert api.lib().slamit_project(0, C.byref(P), C.byref(R)) == 0            # the same record, whole again
    assert np.all(outs["status"] <= 7) and R.n_valid == int((outs["status"] == 0).sum())
    assert api.lib().slamit_project_batch_dev(0, None, None) == -1
    assert api.lib().slamit_rotation_check_batch_dev(0, None, None) == -1
    rec = api.ProjectBatchRec(1, api.PROJECT_MAX_N + 1)
    assert api.lib().slamit_project_batch_dev(0, C.byref(rec), None) == -1 and b"SLAMIT_PROJECT_MAX_N" in api.lib().slamit_last_error()
    rec = api.ProjectBatchRec(1, 8)
    assert api.lib().slamit_project_batch_dev(0, C.byref(rec), None) == -1 and b"null array" in api.lib().slamit_last_error()


# ---- the resident chain ------------------------------------------------------------------------------------------------------------

Q_CAP, KP_CAP = 320, 512
INV_LEVEL_SIGMA2 = [float(np.float32(1) / (np.float32(1.2) ** np.float32(l)) ** 2) for l in range(8)]
RULES = {ref.LAST_FRAME: dict(th_dist=100, use_ratio=False, nnratio=0.9), ref.FUSE: dict(th_dist=50, use_ratio=False, nnratio=0.6, chi2_gate=5.99,
                                                                                        inv_level_sigma2=INV_LEVEL_SIGMA2)}


def _chain_tensors(probs, hosts, sides):
    import torch

    B = len(probs)
    t = dict(cameras=np.zeros(B, api.PROJECT_CAMERA_DTYPE), m=np.zeros(B, np.int32), pos=np.zeros((B, 3, Q_CAP), np.float32), normal=np.zeros((B, 3, Q_CAP), np.float32),
             max_dist=np.zeros((B, Q_CAP), np.float32), min_dist=np.zeros((B, Q_CAP), np.float32), octave=np.zeros((B, Q_CAP), np.int32),
             skip=np.zeros((B, Q_CAP), np.uint8), n=np.zeros(B, np.int32), desc=np.zeros((B, KP_CAP, 32), np.uint8), kp_taken=np.zeros((B, KP_CAP), np.uint8),
             qdesc=np.zeros((B, Q_CAP, 32), np.uint8), takes=np.ones((B, Q_CAP), np.uint8), qangle=np.zeros((B, Q_CAP), np.float32))
    kps = np.zeros((B, KP_CAP), api.KP_DTYPE)
    hq = dict(uvr=np.zeros((B, Q_CAP, 3), np.float32), level_min=np.zeros((B, Q_CAP), np.int32), level_max=np.zeros((B, Q_CAP), np.int32),
              valid=np.zeros((B, Q_CAP), np.uint8))                      # the host-built route's query arrays: the g++-built header's
    for f, (pr, h, (frame, qdesc, takes, qangle)) in enumerate(zip(probs, hosts, sides)):
        m, n = int(pr["n"]), len(frame["kp_xy"])
        t["cameras"][f] = api.project_camera_record(pr)[0]
        t["m"][f], t["n"][f] = m, n
        t["pos"][f, :, :m], t["skip"][f, :m] = pr["pos"].T, pr["skip"]
        for key in ("max_dist", "min_dist", "octave"):
            if pr[key] is not None:
                t[key][f, :m] = pr[key]
        if pr["normal"] is not None:
            t["normal"][f, :, :m] = pr["normal"].T
        kps["x"][f, :n], kps["y"][f, :n], kps["octave"][f, :n], kps["angle"][f, :n] = frame["kp_xy"][:, 0], frame["kp_xy"][:, 1], frame["kp_octave"], frame["kp_angle"]
        t["desc"][f, :n], t["kp_taken"][f, :n] = frame["desc"], frame["kp_taken"]
        t["qdesc"][f, :m], t["takes"][f, :m], t["qangle"][f, :m] = qdesc, takes, qangle
        for k in hq:
            hq[k][f, :m] = h[k]
    d = {k: torch.from_numpy(v.view(np.float32).reshape(B, -1) if k == "cameras" else v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, KP_CAP, 7)).cuda()
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, Q_CAP), dtype=torch.uint8, device="cuda")
    return d, {k: torch.from_numpy(v).cuda() for k, v in hq.items()}


@functools.lru_cache(maxsize=None)
def chain(form):
    """project_batch_dev -> guided_search_batch_dev (-> rotation_check_batch_dev for LAST_FRAME) with nothing but device pointers in
    between, and the same search fed with query arrays built on the host; run once per form and shared by the tests below."""
    import torch

    k = ref.first_fixture(form)
    full = ref.head(ref.fixture(k), 300)                                 # a copy: the twins below are written into it
    acc = np.flatnonzero(ref.host_fixture(k)["status"] == 0)[:24]
    first, twin = acc[0::2], acc[1::2]
    if form == ref.LAST_FRAME:                                           # twelve points seen twice (same position and octave), further down the walk
        full["pos"][twin], full["octave"][twin] = full["pos"][first], full["octave"][first]
    probs = [full, ref.head(full, 0), ref.head(full, 65)]
    hosts = [ref.host_points(pr) for pr in probs]
    takes_frac = 0.6 if form == ref.LAST_FRAME else 0.0                  # SearchByProjection: Observations() > 0 or not; Fuse takes no keypoint
    sides = [ref.search_side(pr, h, 40 + 10 * form + f, takes_frac) for f, (pr, h) in enumerate(zip(probs, hosts))]
    if form == ref.LAST_FRAME:
        # ... with the same descriptor, the first of each pair leaving its keypoint free (takes = 0): the twin takes the same keypoint,
        # and comes from a keypoint turned by 100 degrees more, so the two entries fall into different bins of the rotation histogram
        _, qdesc, takes, qangle = sides[0]
        qdesc[twin], takes[first], qangle[twin] = qdesc[first], 0, np.mod(qangle[first] + np.float32(100.0), np.float32(360.0))
    B = 3
    assert [int(p["n"]) for p in probs] == [300, 0, 65] and max(len(s[0]["kp_xy"]) for s in sides) <= KP_CAP
    d, hq = _chain_tensors(probs, hosts, sides)
    bounds = tuple(sides[0][0][key] for key in ("min_x", "min_y", "inv_w", "inv_h"))
    rule = RULES[form]
    results = {}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for route in ("device", "host"):
        t = dict(d, match_kp=torch.full((B, Q_CAP), -7, dtype=torch.int32, device="cuda"), nmatches=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        if route == "device":
            t.update(uvr=torch.full((B, Q_CAP, 3), -7.0, device="cuda"), level_min=torch.full((B, Q_CAP), -7, dtype=torch.int32, device="cuda"),
                     level_max=torch.full((B, Q_CAP), -7, dtype=torch.int32, device="cuda"), valid=torch.full((B, Q_CAP), 7, dtype=torch.uint8, device="cuda"),
                     status=torch.full((B, Q_CAP), 99, dtype=torch.uint8, device="cuda"), proj=torch.full((B, Q_CAP, 2), -7.0, device="cuda"),
                     level=torch.full((B, Q_CAP), -7, dtype=torch.int32, device="cuda"), n_valid=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
            api.project_batch_dev(t, stream=s.cuda_stream)
        else:
            t.update(hq)
        api.ORBmatcher.guided_search_batch_dev(t, bounds, stream=s.cuda_stream, **rule)
        s.synchronize()
        results[route] = {key: t[key].cpu().numpy() for key in ("match_kp", "nmatches")}
        if route == "device":
            results["queries"] = {key: t[key].cpu().numpy() for key in ("uvr", "level_min", "level_max", "valid", "status", "proj", "level", "n_valid")}
            if form == ref.LAST_FRAME:
                t.update(kp_query=torch.full((B, KP_CAP), -7, dtype=torch.int32, device="cuda"), bins=torch.full((B, 3), -7, dtype=torch.int32, device="cuda"))
                api.ORBmatcher.rotation_check_batch_dev(t, stream=s.cuda_stream)
                s.synchronize()
                results["rotation"] = {key: t[key].cpu().numpy() for key in ("kp_query", "nmatches", "bins")}
    return probs, hosts, sides, results


@pytest.mark.parametrize("form", [ref.LAST_FRAME, ref.FUSE])
def test_the_device_chain_equals_the_host_built_route(form):
    """The chain against the same search fed with host-built query arrays, and against per-frame guided_search calls on COMPACTED
    queries: a query with valid = 0 at its own index changes nothing, so leaving the queries where the points are keeps the driver's
    order.  LAST_FRAME: takes mixed 0 / 1; FUSE: the chi2 gate."""
    probs, hosts, sides, res = chain(form)
    q = res["queries"]
    for f, (pr, h) in enumerate(zip(probs, hosts)):
        m = int(pr["n"])
        assert np.array_equal(q["status"][f, :m], h["status"]) and np.all(q["status"][f, m:] == 99)       # sentinels past d_m[f] survive
        assert np.array_equal(bits(q["uvr"][f, :m]), bits(h["uvr"])) and np.all(q["uvr"][f, m:] == -7.0)
        assert np.array_equal(q["valid"][f, :m], h["valid"]) and np.all(q["valid"][f, m:] == 7)
        assert np.array_equal(q["level_min"][f, :m], h["level_min"]) and np.array_equal(q["level_max"][f, :m], h["level_max"])
        assert np.all(q["level_min"][f, m:] == -7) and np.all(q["level_max"][f, m:] == -7) and np.all(q["level"][f, m:] == -7) and np.all(q["proj"][f, m:] == -7.0)
        assert np.array_equal(bits(q["proj"][f, :m]), bits(h["proj"])) and np.array_equal(q["level"][f, :m], h["level"])
        assert int(q["n_valid"][f]) == int((h["status"] == 0).sum())
    dev, host = res["device"], res["host"]
    assert np.array_equal(dev["nmatches"], host["nmatches"])
    rule = dict(RULES[form])
    for f, (pr, h, (frame, qdesc, takes, _)) in enumerate(zip(probs, hosts, sides)):
        m = int(pr["n"])
        assert np.array_equal(dev["match_kp"][f, :m], host["match_kp"][f, :m]) and np.all(dev["match_kp"][f, m:] == -7)
        keep = np.flatnonzero(h["valid"])
        qq = dict(uvr=h["uvr"][keep], level_min=h["level_min"][keep], level_max=h["level_max"][keep], desc=qdesc[keep], takes=takes[keep])
        gm, gn, _ = api.ORBmatcher.guided_search(frame, qq, **rule) if len(keep) and len(frame["kp_xy"]) else (np.zeros(0, np.int32), 0, None)
        want = np.full(m, -1, np.int32)
        want[keep] = gm
        assert np.array_equal(dev["match_kp"][f, :m], want) and dev["nmatches"][f] == gn
    assert dev["nmatches"][0] > 30 and dev["nmatches"][1] == 0 and dev["nmatches"][2] > 5
    if form == ref.LAST_FRAME:
        assert 0 < sides[0][2].sum() < 300                               # takes is mixed


def test_the_rotation_check_on_the_last_frame_chain_equals_the_restatement():
    probs, hosts, sides, res = chain(ref.LAST_FRAME)
    dev, r = res["device"], res["rotation"]
    dropped = shared = 0
    for f, (pr, (frame, _, _, qangle)) in enumerate(zip(probs, sides)):
        m, n = int(pr["n"]), len(frame["kp_xy"])
        owner, nm, ind = rot.rotation_check(dev["match_kp"][f, :m], qangle, frame["kp_angle"], int(dev["nmatches"][f]))
        assert np.array_equal(r["kp_query"][f, :n], owner) and np.all(r["kp_query"][f, n:] == -1)
        assert int(r["nmatches"][f]) == nm and tuple(int(b) for b in r["bins"][f]) == ind
        dropped += int(dev["nmatches"][f]) - nm
        mk = dev["match_kp"][f, :m]
        shared += len(mk[mk >= 0]) - len(np.unique(mk[mk >= 0]))
    print("rotation check on the chain: %d entries dropped, %d keypoints taken twice" % (dropped, shared))
    assert dropped > 3 and shared > 0                                    # the check had matches to drop, and a keypoint two queries took
    assert tuple(r["bins"][1]) == (-1, -1, -1) and r["nmatches"][1] == 0


def test_the_rotation_check_on_the_hand_cases():
    import torch

    cases = rot.hand_cases()
    names = sorted(cases)
    B, kp_cap, q_cap = len(names), 48, 32
    t = dict(n=np.zeros(B, np.int32), m=np.zeros(B, np.int32), match_kp=np.full((B, q_cap), 5, np.int32), qangle=np.zeros((B, q_cap), np.float32),
             nmatches=np.zeros(B, np.int32))
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    for f, name in enumerate(names):
        c = cases[name][0]
        m, n = len(c["match_kp"]), len(c["kp_angle"])
        assert m <= q_cap and n <= kp_cap
        t["n"][f], t["m"][f], t["nmatches"][f] = n, m, c["nmatches"]
        t["match_kp"][f, :m], t["qangle"][f, :m] = c["match_kp"], c["qangle"]   # entries past m point at keypoint 5: they must not be read
        kps["angle"][f, :n] = c["kp_angle"]
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d.update(kp_query=torch.full((B, kp_cap), -7, dtype=torch.int32, device="cuda"), bins=torch.full((B, 3), -7, dtype=torch.int32, device="cuda"))
    api.ORBmatcher.rotation_check_batch_dev(d)
    torch.cuda.synchronize()
    kp_query, nmatches, bins = d["kp_query"].cpu().numpy(), d["nmatches"].cpu().numpy(), d["bins"].cpu().numpy()
    for f, name in enumerate(names):
        c, owners, nm, ind = cases[name]
        owner, nm_ref, ind_ref = rot.rotation_check(**c)
        n = len(c["kp_angle"])
        assert np.array_equal(kp_query[f, :n], owner) and np.all(kp_query[f, n:] == -1), name
        assert int(nmatches[f]) == nm == nm_ref and tuple(int(b) for b in bins[f]) == ind == ind_ref, name
        for k, q in owners.items():
            assert kp_query[f, k] == q, (name, k)
