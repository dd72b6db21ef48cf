"""The right-image gate of the guided search on the device (slamit_guided_search_stereo, _stereo_batch_dev) against
the numpy restatement tests/search_stereo_ref.py, on the fixtures tests/test_search_stereo_ref.py qualifies on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import frustum_ref
from tests import search_stereo_fixtures as fx
from tests import search_stereo_ref as ref
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

_model = {}


def model(key):
    """the restatement's answer on a fixture, computed once"""
    if key not in _model:
        f, q, st = fx.fixture(*key)
        _model[key] = ref.guided_search(f, q, **fx.rule(key[0], st), **fx.model_kw(st))
    return _model[key]


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert np.array_equal(got[2], want[2])


@pytest.mark.parametrize("n", fx.SIZES)
@pytest.mark.parametrize("er_mode", (fx.RADIUS, fx.CHI2))
def test_device_equals_model(er_mode, n):
    key = (er_mode, n, False)
    f, q, st = fx.fixture(*key)
    got = api.ORBmatcher.guided_search(f, q, stereo=fx.api_stereo(st), **fx.rule(er_mode, st))
    _same(got, model(key))
    if n >= 63:   # and the gate did something: the monocular call answers differently
        mono = api.ORBmatcher.guided_search(f, q, **fx.rule(er_mode, st))
        assert (mono[0] != got[0]).sum() >= 20


HAND = fx.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_cases(case):
    _, frame, queries, rule, st, expect = case
    match, nm, _ = api.ORBmatcher.guided_search(frame, queries, stereo=fx.api_stereo(st), **rule)
    assert match[0] == expect and nm == (expect >= 0)


def _batch(problems, kp_cap, q_cap):
    """(frame, queries, stereo) triples as guided_search_batch_dev's tensors, plus kp_ur (B, kp_cap) and q_ur (B, q_cap); the entries
    past a frame's counts hold values that would change the answer if they were read"""
    import torch

    B = len(problems)
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    t = dict(n=np.zeros(B, np.int32), desc=np.zeros((B, kp_cap, 32), np.uint8), kp_taken=np.zeros((B, kp_cap), np.uint8),
             m=np.zeros(B, np.int32), uvr=np.zeros((B, q_cap, 3), np.float32), level_min=np.zeros((B, q_cap), np.int32),
             level_max=np.zeros((B, q_cap), np.int32), qdesc=np.zeros((B, q_cap, 32), np.uint8), valid=np.ones((B, q_cap), np.uint8),
             takes=np.ones((B, q_cap), np.uint8), kp_ur=np.full((B, kp_cap), 1e6, np.float32), q_ur=np.full((B, q_cap), -1e6, np.float32))
    for i, (f, q, st) in enumerate(problems):
        n, m = len(f["kp_xy"]), len(q["uvr"])
        t["n"][i], t["m"][i] = n, m
        kps["x"][i, :n], kps["y"][i, :n], kps["octave"][i, :n] = f["kp_xy"][:, 0], f["kp_xy"][:, 1], f["kp_octave"]
        t["desc"][i, :n], t["kp_taken"][i, :n] = f["desc"], f["kp_taken"]
        t["uvr"][i, :m], t["level_min"][i, :m], t["level_max"][i, :m] = q["uvr"], q["level_min"], q["level_max"]
        t["qdesc"][i, :m], t["valid"][i, :m], t["takes"][i, :m] = q["desc"], q["valid"], q["takes"]
        t["kp_ur"][i, :n], t["q_ur"][i, :m] = st["kp_ur"], st["q_ur"][:m]
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, q_cap), dtype=torch.uint8, device="cuda")
    return d


def _fresh_outputs(d):
    import torch

    B, q_cap = d["uvr"].shape[0], d["uvr"].shape[1]
    return dict(d, match_kp=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), nmatches=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
                out4=torch.full((B, q_cap, 4), -7, dtype=torch.int32, device="cuda"))


def _bounds(f):
    return tuple(f[k] for k in ("min_x", "min_y", "inv_w", "inv_h"))


def _frame_result(t, i, m):
    return t["match_kp"][i, :m].cpu().numpy(), int(t["nmatches"][i]), t["out4"][i, :m].cpu().numpy()


def test_crowd_windows_go_through_the_rewalk():
    """300 keypoints in 60 x 60 px through the batch form, whose stored list is SLAMIT_SEARCH_BATCH_CAND = 128: 26 windows hold more
    gated candidates than that and 4 of them lose their tentative pair to an earlier query (tests/test_search_stereo_ref.py), so the
    frame's keypoints are walked again with the gate."""
    import torch

    key = (fx.RADIUS, 300, True)
    f, q, st = fx.fixture(*key)
    t = _fresh_outputs(_batch([(f, q, st)], 300, fx.M))
    api.ORBmatcher.guided_search_batch_dev(t, _bounds(f), stereo=dict(er_mode=fx.RADIUS, kp_ur=t["kp_ur"], q_ur=t["q_ur"]), **fx.rule(fx.RADIUS, st))
    torch.cuda.synchronize()
    _same(_frame_result(t, 0, fx.M), model(key))
    # the host form stores up to 1024 candidates: the same answer without the re-walk
    _same(api.ORBmatcher.guided_search(f, q, stereo=fx.api_stereo(st), **fx.rule(fx.RADIUS, st)), model(key))


def _head(q, st, m):
    return {k: v[:m] for k, v in q.items()}, dict(st, q_ur=st["q_ur"][:m])


@pytest.mark.parametrize("er_mode", (fx.RADIUS, fx.CHI2))
def test_ragged_batch_equals_the_host_form(er_mode):
    import torch

    f0, q0, s0 = fx.fixture(er_mode, 300)
    f1, q1, s1 = fx.fixture(er_mode, 0)
    q1, s1 = _head(q1, s1, 0)                       # the empty frame: no keypoints, no queries
    f2, q2, s2 = fx.fixture(er_mode, 65)
    q2, s2 = _head(q2, s2, 130)
    problems = [(f0, q0, s0), (f1, q1, s1), (f2, q2, s2)]
    t = _fresh_outputs(_batch(problems, 320, 256))
    rule = fx.rule(er_mode, s0)
    api.ORBmatcher.guided_search_batch_dev(t, _bounds(f0), stereo=dict(er_mode=er_mode, kp_ur=t["kp_ur"], q_ur=t["q_ur"], chi2_gate_stereo=7.8), **rule)
    torch.cuda.synchronize()
    for i, (f, q, st) in enumerate(problems):
        m = len(q["uvr"])
        host = api.ORBmatcher.guided_search(f, q, stereo=fx.api_stereo(st), **rule)
        _same(_frame_result(t, i, m), host)
        assert np.all(t["match_kp"][i, m:].cpu().numpy() == -7)   # nothing is written past a frame's queries
    _same(_frame_result(t, 0, fx.M), model((er_mode, 300, False)))
    assert int(t["nmatches"][0]) > 20 and int(t["nmatches"][1]) == 0 and int(t["nmatches"][2]) > 5


def _raw_host(symbol, f, q, rule_kw, st=None):
    """a call of the C symbol itself, as api.ORBmatcher.guided_search makes it"""
    fr = dict(kp_xy=np.ascontiguousarray(f["kp_xy"], np.float32), kp_octave=np.ascontiguousarray(f["kp_octave"], np.int32),
              desc=np.ascontiguousarray(f["desc"], np.uint8), kp_taken=np.ascontiguousarray(f["kp_taken"], np.uint8))
    qq = {k: np.ascontiguousarray(q[k], dt) for k, dt in (("uvr", np.float32), ("level_min", np.int32), ("level_max", np.int32), ("desc", np.uint8),
                                                         ("valid", np.uint8), ("takes", np.uint8))}
    n, m = len(fr["kp_xy"]), len(qq["uvr"])
    p = api._np_ptr
    fv = api.FrameView(n, p(fr["kp_xy"]), p(fr["kp_octave"]), p(fr["desc"]), p(fr["kp_taken"]), f["min_x"], f["min_y"], f["inv_w"], f["inv_h"])
    sq = api.SearchQueries(m, p(qq["uvr"]), p(qq["level_min"]), p(qq["level_max"]), p(qq["desc"]), p(qq["valid"]), p(qq["takes"]))
    rule = api._search_rule(**rule_kw)
    match, out4, nm = np.full(m, -7, np.int32), np.full((4, m), -7, np.int32), C.c_int32(-7)
    outs = (p(match), C.byref(nm), p(out4[0]), p(out4[1]), p(out4[2]), p(out4[3]))
    L = api.lib()
    if symbol == "slamit_guided_search":
        rc = L.slamit_guided_search(0, C.byref(fv), C.byref(sq), C.byref(rule), *outs)
    else:
        rc = L.slamit_guided_search_stereo(0, C.byref(fv), C.byref(sq), C.byref(rule), C.byref(st) if st is not None else None, *outs)
    return rc, (match, nm.value, out4.T.copy())


def test_null_record_and_mode_0_are_the_old_entry_point():
    import torch

    f, q, st = fx.fixture(fx.RADIUS, 300)
    for rule in (fx.rule(fx.RADIUS, st), dict(th_dist=50, use_ratio=False, nnratio=0.6, chi2_gate=5.99, inv_level_sigma2=np.ones(8, np.float32))):
        rc, old = _raw_host("slamit_guided_search", f, q, rule)
        assert rc == 0 and old[1] > 0
        rc, null = _raw_host("slamit_guided_search_stereo", f, q, rule, None)
        assert rc == 0
        _same(null, old)
        rc, none = _raw_host("slamit_guided_search_stereo", f, q, rule, api.SearchStereo(0, 7.8, None, None, 0))   # mode 0 reads nothing of the record
        assert rc == 0
        _same(none, old)
    # the batch form
    d = _batch([(f, q, st)], 300, fx.M)
    results = []
    for stereo in ("old", None, dict(er_mode=0, kp_ur=None, q_ur=None, q_ur_stride=0)):
        t = _fresh_outputs(d)
        if stereo == "old":
            api.ORBmatcher.guided_search_batch_dev(t, _bounds(f), **fx.rule(fx.RADIUS, st))
        else:
            sb_stereo = stereo
            if stereo is None:   # a NULL record through the new symbol
                b, kp_cap, q_cap = 1, 300, fx.M
                sb = api.SearchBatch(b, kp_cap, q_cap, t["n"].data_ptr(), t["kps_un"].data_ptr(), t["desc"].data_ptr(), t["kp_taken"].data_ptr(),
                                     *[float(v) for v in _bounds(f)], t["m"].data_ptr(), t["uvr"].data_ptr(), t["level_min"].data_ptr(),
                                     t["level_max"].data_ptr(), t["qdesc"].data_ptr(), t["valid"].data_ptr(), t["takes"].data_ptr())
                rule = api._search_rule(**fx.rule(fx.RADIUS, st))
                assert api.lib().slamit_guided_search_stereo_batch_dev(0, C.byref(sb), C.byref(rule), None, t["match_kp"].data_ptr(), t["nmatches"].data_ptr(),
                                                                       t["out4"].data_ptr(), t["workspace"].data_ptr(), t["workspace"].numel(), None) == 0
            else:
                api.ORBmatcher.guided_search_batch_dev(t, _bounds(f), stereo=sb_stereo, **fx.rule(fx.RADIUS, st))
        torch.cuda.synchronize()
        results.append(_frame_result(t, 0, fx.M))
    _same(results[1], results[0])
    _same(results[2], results[0])
    _same(results[0], api.ORBmatcher.guided_search(f, q, **fx.rule(fx.RADIUS, st)))


def test_stride_3_reads_a_proj_array_in_place():
    """q_ur = proj + 2 with stride 3, the layout of slamit_frustum_result.proj, against the packed copy"""
    import torch

    key = (fx.RADIUS, 300, False)
    f, q, st = fx.fixture(*key)
    proj = np.full((fx.M, 3), 12345.0, np.float32)
    proj[:, 2] = st["q_ur"]
    got = api.ORBmatcher.guided_search(f, q, stereo=dict(fx.api_stereo(st), q_ur=proj.reshape(-1)[2:], q_ur_stride=3), **fx.rule(fx.RADIUS, st))
    _same(got, model(key))
    t = _fresh_outputs(_batch([(f, q, st)], 300, fx.M))
    d_proj = torch.from_numpy(proj).cuda().reshape(-1)
    api.ORBmatcher.guided_search_batch_dev(t, _bounds(f), stereo=dict(er_mode=fx.RADIUS, kp_ur=t["kp_ur"], q_ur=d_proj[2:], q_ur_stride=3),
                                           **fx.rule(fx.RADIUS, st))
    torch.cuda.synchronize()
    _same(_frame_result(t, 0, fx.M), model(key))


def test_argument_errors():
    """every refusal returns -1 with its message before anything is launched, and leaves the outputs as they were"""
    import torch

    f, q, st = fx.fixture(fx.RADIUS, 65)
    kur, qur = np.ascontiguousarray(st["kp_ur"]), np.ascontiguousarray(st["q_ur"])
    rule = fx.rule(fx.RADIUS, st)
    L = api.lib()

    def refused(record, message, rule_kw=rule):
        rc, out = _raw_host("slamit_guided_search_stereo", f, q, rule_kw, record)
        assert rc == -1 and message in L.slamit_last_error(), L.slamit_last_error()
        assert np.all(out[0] == -7) and out[1] == -7 and np.all(out[2] == -7)

    p = api._np_ptr
    refused(api.SearchStereo(3, 7.8, p(kur), p(qur), 1), b"er_mode outside 0..2")
    refused(api.SearchStereo(-1, 7.8, p(kur), p(qur), 1), b"er_mode outside 0..2")
    refused(api.SearchStereo(1, 7.8, None, p(qur), 1), b"null kp_ur or q_ur")
    refused(api.SearchStereo(2, 7.8, p(kur), None, 1), b"null kp_ur or q_ur")
    refused(api.SearchStereo(1, 7.8, p(kur), p(qur), 0), b"q_ur_stride < 1")
    refused(api.SearchStereo(1, 7.8, p(kur), p(qur), 1), b"rule mode 1", dict(rule, mode=1))
    rc, out = _raw_host("slamit_guided_search_stereo", f, q, rule, api.SearchStereo(1, 7.8, p(kur), p(qur), 1))   # the same record, whole
    assert rc == 0
    _same(out, model((fx.RADIUS, 65, False)))
    with pytest.raises(api.SlamitError, match="er_mode outside"):
        api.ORBmatcher.guided_search(f, q, stereo=dict(fx.api_stereo(st), er_mode=7), **rule)

    # the batch form
    t = _fresh_outputs(_batch([(f, q, st)], 65, fx.M))

    def refused_dev(stereo, message, **kw):
        with pytest.raises(api.SlamitError, match=message):
            api.ORBmatcher.guided_search_batch_dev(t, _bounds(f), stereo=stereo, **dict(rule, **kw))
        torch.cuda.synchronize()
        assert bool((t["match_kp"] == -7).all()) and bool((t["nmatches"] == -7).all()) and bool((t["out4"] == -7).all())

    refused_dev(dict(er_mode=3, kp_ur=t["kp_ur"], q_ur=t["q_ur"]), "er_mode outside")
    refused_dev(dict(er_mode=1, kp_ur=None, q_ur=t["q_ur"]), "null d_kp_ur or d_q_ur")
    refused_dev(dict(er_mode=2, kp_ur=t["kp_ur"], q_ur=None), "null d_kp_ur or d_q_ur")
    refused_dev(dict(er_mode=1, kp_ur=t["kp_ur"], q_ur=t["q_ur"], q_ur_stride=-3), "q_ur_stride < 1")
    sb = api.SearchBatch(1, 65, fx.M, t["n"].data_ptr(), t["kps_un"].data_ptr(), t["desc"].data_ptr(), t["kp_taken"].data_ptr(), *[float(v) for v in _bounds(f)],
                         t["m"].data_ptr(), t["uvr"].data_ptr(), t["level_min"].data_ptr(), t["level_max"].data_ptr(), t["qdesc"].data_ptr(),
                         t["valid"].data_ptr(), t["takes"].data_ptr())
    r1 = api._search_rule(**dict(rule, mode=1))
    rec = api.SearchStereoDev(1, 7.8, t["kp_ur"].data_ptr(), t["q_ur"].data_ptr(), 1)
    assert L.slamit_guided_search_stereo_batch_dev(0, C.byref(sb), C.byref(r1), C.byref(rec), t["match_kp"].data_ptr(), t["nmatches"].data_ptr(),
                                                   t["out4"].data_ptr(), t["workspace"].data_ptr(), t["workspace"].numel(), None) == -1
    assert b"rule mode 1" in L.slamit_last_error()
    torch.cuda.synchronize()
    assert bool((t["match_kp"] == -7).all())


def _frustum_problem(k, n):
    pr = frustum_ref.head(frustum_ref.fixture(k), n)
    assert float(pr["bf"]) != 0.0
    return pr


def test_resident_chain_frustum_to_stereo_search():
    """slamit_frustum_batch_dev -> slamit_guided_search_stereo_batch_dev reading d_proj + 2 with stride 3 (mTrackProjXR where
    isInFrustum left it), 2 frames x 300 points, nothing but device pointers in between; against api.frustum followed by the host
    search on the same data, and against the restatement."""
    import torch

    from tests.test_gpu_frustum import _chain_tensors

    probs = [_frustum_problem(0, 300), _frustum_problem(1, 300)]
    hosts, sides, kurs = [], [], []
    for i, pr in enumerate(probs):
        o = api.frustum(pr)
        h = dict(o, u=o["proj"][:, 0], v=o["proj"][:, 1], uR=o["proj"][:, 2], r=o["uvr"][:, 2])
        frame, qdesc, takes = frustum_ref.search_side(pr, h, 70 + i)
        # mvuRight of the frame: a keypoint derived from a point carries that point's uR, moved within a quarter of its window or, for
        # four in ten, 150 px away; half the keypoints are monocular
        rs = np.random.RandomState(90 + i)
        bits, qbits = np.unpackbits(frame["desc"], axis=1).astype(np.int16), np.unpackbits(qdesc, axis=1).astype(np.int16)
        owner = np.argmin(bits @ (1 - qbits).T + (1 - bits) @ qbits.T, axis=1)
        n = len(owner)
        kur = (h["uR"][owner] + rs.uniform(-0.25, 0.25, n) * h["r"][owner] + np.where(rs.rand(n) < 0.4, 150.0, 0.0)).astype(np.float32)
        kur[(rs.rand(n) < 0.5) | (kur <= 0)] = -1.0
        hosts.append(h), sides.append((frame, qdesc, takes)), kurs.append(kur)
    q_cap, kp_cap, B = 320, 640, 2
    assert max(len(k) for k in kurs) <= kp_cap
    d, _ = _chain_tensors(probs, hosts, sides, q_cap, kp_cap)
    kp_ur = np.full((B, kp_cap), 1e6, np.float32)
    for i, k in enumerate(kurs):
        kp_ur[i, :len(k)] = k
    t = dict(d, match_kp=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), nmatches=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             out4=torch.full((B, q_cap, 4), -7, dtype=torch.int32, device="cuda"),
             uvr=torch.full((B, q_cap, 3), -7.0, device="cuda"), level_min=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"),
             level_max=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), valid=torch.full((B, q_cap), 7, dtype=torch.uint8, device="cuda"),
             proj=torch.full((B, q_cap, 3), -7.0, device="cuda"))
    d_kp_ur = torch.from_numpy(kp_ur).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.frustum_batch_dev(t, stream=s.cuda_stream)
    bounds = _bounds(sides[0][0])
    api.ORBmatcher.guided_search_batch_dev(t, bounds, 100, True, 0.8, stream=s.cuda_stream,
                                           stereo=dict(er_mode=fx.RADIUS, kp_ur=d_kp_ur, q_ur=t["proj"].reshape(-1)[2:], q_ur_stride=3))
    s.synchronize()
    gated = 0
    for i, (pr, h, (frame, qdesc, takes)) in enumerate(zip(probs, hosts, sides)):
        m = int(pr["n"])
        q = dict(uvr=h["uvr"], level_min=h["level_min"], level_max=h["level_max"], desc=qdesc, valid=h["valid"], takes=takes)
        st = dict(er_mode=fx.RADIUS, kp_ur=kurs[i], q_ur=np.ascontiguousarray(h["proj"]).reshape(-1)[2:], q_ur_stride=3)
        host = api.ORBmatcher.guided_search(frame, q, 100, True, 0.8, stereo=st)
        _same(_frame_result(t, i, m), host)
        _same(host, ref.guided_search(frame, q, 100, True, 0.8, **st))
        mono = api.ORBmatcher.guided_search(frame, q, 100, True, 0.8)
        gated += int((mono[0] != host[0]).sum())
        assert host[1] > 20
    assert gated >= 20
