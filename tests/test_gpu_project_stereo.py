"""slamit_project_batch_stereo / slamit_project_batch_dev_stereo on the device: the right-image column ur bit-equal to the g++ build
of csrc/project.h and to the numpy restatement (tests/project_stereo_ref.py), every other output bit-equal to the plain call."""
import ctypes as C

import numpy as np
import pytest

from tests import project_ref as ref
from tests import project_stereo_ref as sref
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
PLAIN = ("status", "proj", "level", "uvr", "level_min", "level_max", "valid")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _mixed_batch():
    """forms 0 and 2 in turn, at every size"""
    probs, bfs = [], []
    for n in SIZES:
        for form in (ref.LAST_FRAME, ref.FUSE):
            probs.append(ref.head(ref.fixture(ref.first_fixture(form)), n))
            bfs.append(sref.BF[form])
    return probs, bfs


def test_host_form_mixed_batch():
    probs, bfs = _mixed_batch()
    outs = api.project_batch(probs, bf=bfs)
    plain = api.project_batch(probs)
    accepted = 0
    for pr, bf, o, p in zip(probs, bfs, outs, plain):
        h = sref.host_points_stereo(pr, bf)
        assert np.array_equal(bits(o["ur"]), bits(h["ur"]))
        assert np.array_equal(bits(o["ur"]), bits(sref.ur_numpy(pr, bf, o["status"])[0]))
        assert np.all(bits(o["ur"][o["status"] != 0]) == 0)
        for key in PLAIN:
            assert np.array_equal(bits(o[key]), bits(p[key])), key
        assert o["n_valid"] == p["n_valid"]
        accepted += int((o["status"] == 0).sum())
    assert accepted > 100
    one = api.project(probs[-1], bf=bfs[-1])
    assert np.array_equal(bits(one["ur"]), bits(outs[-1]["ur"]))


def test_device_form_mixed_batch():
    import torch

    probs, bfs = _mixed_batch()
    B, q_cap = len(probs), 288
    t = dict(cameras=np.zeros(B, api.PROJECT_CAMERA_DTYPE), m=np.zeros(B, np.int32), pos=np.zeros((B, 3, q_cap), np.float32), normal=np.zeros((B, 3, q_cap), np.float32),
             max_dist=np.zeros((B, q_cap), np.float32), min_dist=np.zeros((B, q_cap), np.float32), octave=np.zeros((B, q_cap), np.int32),
             skip=np.zeros((B, q_cap), np.uint8), bf=np.asarray(bfs, np.float32))
    for f, pr in enumerate(probs):
        m = int(pr["n"])
        t["cameras"][f] = api.project_camera_record(pr)[0]
        t["m"][f] = m
        t["pos"][f, :, :m], t["skip"][f, :m] = pr["pos"].T, pr["skip"]
        for key in ("max_dist", "min_dist", "octave"):
            if pr[key] is not None:
                t[key][f, :m] = pr[key]
        if pr["normal"] is not None:
            t["normal"][f, :, :m] = pr["normal"].T
    d = {k: torch.from_numpy(v.view(np.float32).reshape(B, -1) if k == "cameras" else v).cuda() for k, v in t.items()}

    def outputs():
        return dict(uvr=torch.full((B, q_cap, 3), -7.0, device="cuda"), level_min=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"),
                    level_max=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), valid=torch.full((B, q_cap), 7, dtype=torch.uint8, device="cuda"),
                    status=torch.full((B, q_cap), 99, dtype=torch.uint8, device="cuda"), proj=torch.full((B, q_cap, 2), -7.0, device="cuda"),
                    level=torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda"), n_valid=torch.full((B,), -7, dtype=torch.int32, device="cuda"))

    plain = dict({k: v for k, v in d.items() if k != "bf"}, **outputs())
    api.project_batch_dev(plain)
    st = dict(d, ur=torch.full((B, q_cap), -7.0, device="cuda"), **outputs())
    api.project_batch_dev(st)
    torch.cuda.synchronize()
    for key in PLAIN + ("n_valid",):
        assert torch.equal(st[key].view(torch.int32) if st[key].dtype == torch.float32 else st[key],
                           plain[key].view(torch.int32) if plain[key].dtype == torch.float32 else plain[key]), key
    ur = st["ur"].cpu().numpy()
    for f, (pr, bf) in enumerate(zip(probs, bfs)):
        m = int(pr["n"])
        h = sref.host_points_stereo(pr, bf)
        assert np.array_equal(bits(ur[f, :m]), bits(h["ur"]))
        assert np.all(ur[f, m:] == -7.0)              # nothing is written past a frame's points
    # exactly one of bf / ur: refused before the launch, outputs untouched
    for missing in ("bf", "ur"):
        bad = dict(st, **outputs())
        bad["ur"] = torch.full((B, q_cap), -7.0, device="cuda")
        bad[missing] = None
        with pytest.raises(api.SlamitError, match="exactly one of"):
            api.project_batch_dev(bad)
        torch.cuda.synchronize()
        assert bool((bad["status"] == 99).all()) and bool((bad["valid"] == 7).all())


def test_host_form_argument_errors():
    pr = ref.head(ref.fixture(ref.first_fixture(ref.FUSE)), 8)
    P, R = api.ProjectProblem(), api.ProjectResult()
    C.memmove(C.byref(P.camera), api.project_camera_record(pr).ctypes.data, C.sizeof(api.ProjectCamera))
    keep = {k: np.ascontiguousarray(pr[k]) for k in ("pos", "normal", "max_dist", "min_dist", "skip")}
    P.n = 8
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    outs = {"status": np.full(8, 99, np.uint8), "proj": np.full((8, 2), 7.0, np.float32), "level": np.full(8, 99, np.int32), "uvr": np.full((8, 3), 7.0, np.float32),
            "level_min": np.full(8, 99, np.int32), "level_max": np.full(8, 99, np.int32), "valid": np.full(8, 99, np.uint8)}
    for k, a in outs.items():
        setattr(R, k, a.ctypes.data)
    R.n_valid = -5
    ur = np.full(8, 7.0, np.float32)
    urp = (C.c_void_p * 1)(ur.ctypes.data)
    bf = np.array([40.0], np.float32)
    L = api.lib()

    def untouched():
        return all(np.all(a == (7.0 if a.dtype == np.float32 else 99)) for a in outs.values()) and R.n_valid == -5 and np.all(ur == 7.0)

    assert L.slamit_project_batch_stereo(0, 1, C.byref(P), C.byref(R), bf.ctypes.data, None) == -1 and b"exactly one of" in L.slamit_last_error() and untouched()
    assert L.slamit_project_batch_stereo(0, 1, C.byref(P), C.byref(R), None, C.cast(urp, C.c_void_p)) == -1 and b"exactly one of" in L.slamit_last_error() and untouched()
    nullp = (C.c_void_p * 1)(None)
    assert L.slamit_project_batch_stereo(0, 1, C.byref(P), C.byref(R), bf.ctypes.data, C.cast(nullp, C.c_void_p)) == -1 and b"null ur" in L.slamit_last_error() and untouched()
    assert L.slamit_project_batch_stereo(0, 1, C.byref(P), C.byref(R), bf.ctypes.data, C.cast(urp, C.c_void_p)) == 0   # whole again
    assert R.n_valid == int((outs["status"] == 0).sum()) and np.all(ur[outs["status"] != 0] == 0)
    assert L.slamit_project_batch_stereo(0, 1, C.byref(P), C.byref(R), None, None) == 0                                # both null: the plain call
