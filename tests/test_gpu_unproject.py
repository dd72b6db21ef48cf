"""slamit_unproject_closest* and slamit_rgbd_depth* on the device against the numpy restatement of the reference's loops
(tests/unproject_ref.py).

Every operation of csrc/unproject.h is an IEEE +, -, *, / or sqrt compiled without contraction on both sides, and the walk is an
exact order on unique integer keys: statuses, order, counters and every float equal the restatement's BIT FOR BIT (two NaNs equal),
and no tolerance appears below."""
import ctypes as C

import numpy as np
import pytest

from tests import unproject_ref as ur
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


def test_every_fixture_in_one_batch():
    names = sorted(ur.FIXTURES)
    outs = api.unproject_closest_batch([ur.fixture(k) for k in names])
    seen = set()
    for name, out in zip(names, outs):
        ur.assert_same(out, ur.ref_fixture(name), name)
        seen |= set(out["status"].tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_shapes_in_a_ragged_batch_and_singly():
    """n in {0, 1, 63, 64, 65, 1023, 1024, 1025}, M in {0, 1, 99, 100, 101, 102}, c below, at and above min_points and c == M"""
    ks = range(len(ur.SHAPES))
    assert {s[0] for s in ur.SHAPES} >= {0, 1, 63, 64, 65, 1023, 1024, 1025} and {s[1] for s in ur.SHAPES} >= {0, 1, 99, 100, 101, 102}
    assert {np.sign(s[2] - 100) for s in ur.SHAPES if s[1]} == {-1, 0, 1} and any(s[1] == s[2] and s[1] > 100 for s in ur.SHAPES)
    batch = api.unproject_closest_batch([ur.shape_fixture(k) for k in ks])
    for k, b in zip(ks, batch):
        ur.assert_same(b, ur.ref_shape(k), "shape %d %r" % (k, ur.SHAPES[k]))
        assert (b["n_candidates"], b["n_close"]) == ur.SHAPES[k][1:]
    for k in (1, 4, 7, 9):
        ur.assert_same(api.unproject_closest(ur.shape_fixture(k)), batch[k], "single %d" % k)
    assert api.unproject_closest_batch([]) == []


def test_a_workgroup_of_1024_and_one_of_256_give_the_same_walk():
    """A batch is launched at the size of its largest problem: the 300-keypoint fixture beside the 2048-keypoint one runs in the
    1,024-thread workgroup, alone in the 256-thread one."""
    small, large = ur.fixture("mixed"), ur.fixture("levels16")
    both = api.unproject_closest_batch([small, large])
    ur.assert_same(both[0], ur.ref_fixture("mixed"), "beside 2048")
    ur.assert_same(api.unproject_closest(small), ur.ref_fixture("mixed"), "alone")
    ur.assert_same(both[1], ur.ref_fixture("levels16"), "2048")


def test_argument_errors_launch_nothing():
    pr = ur.fixture("min0")
    n = int(pr["n"])
    for bad, word in ((dict(pr, n_levels=0), "n_levels"), (dict(pr, n_levels=17), "n_levels"), (dict(pr, mode=2), "mode"), (dict(pr, min_points=-1), "min_points")):
        with pytest.raises(api.SlamitError, match=word) as e:
            api.unproject_closest(bad)
        assert "(-1)" in str(e.value)
    P, R = api.UnprojectProblem(), api.UnprojectResult()
    C.memmove(C.byref(P.frame), api.unproject_frame_record(pr).ctypes.data, C.sizeof(api.UnprojectFrame))
    keep = {"kps_un": np.ascontiguousarray(pr["kps_un"]), "depth": np.ascontiguousarray(pr["depth"]), "tracked": np.ascontiguousarray(pr["tracked"])}
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data)
    outs = {"status": np.full(n, 99, np.uint8), "order": np.full(n, 99, np.int32), "pos": np.full((n, 3), 7.0, np.float32), "normal": np.full((n, 3), 7.0, np.float32),
            "max_dist": np.full(n, 7.0, np.float32), "min_dist": np.full(n, 7.0, np.float32)}
    for k, a in outs.items():
        setattr(R, k, a.ctypes.data)
    R.counts.n_visited = -5
    L = api.lib()

    def untouched():
        return all(np.all(a == (7.0 if a.dtype == np.float32 else 99)) for a in outs.values()) and R.counts.n_visited == -5

    P.n = -1
    assert L.slamit_unproject_closest(0, C.byref(P), C.byref(R)) == -1 and b"negative count" in L.slamit_last_error() and untouched()
    P.n = 8192
    assert L.slamit_unproject_closest(0, C.byref(P), C.byref(R)) == -3 and b"SLAMIT_STEREO_MAX_KP" in L.slamit_last_error() and untouched()
    P.n = n
    for field in ("depth", "tracked", "kps_un"):
        setattr(P, field, None)
        assert L.slamit_unproject_closest(0, C.byref(P), C.byref(R)) == -1 and b"null array" in L.slamit_last_error() and untouched()
        setattr(P, field, keep[field].ctypes.data)
    R.order = None
    assert L.slamit_unproject_closest(0, C.byref(P), C.byref(R)) == -1 and b"null array" in L.slamit_last_error() and untouched()
    R.order = outs["order"].ctypes.data
    assert L.slamit_unproject_closest(0, C.byref(P), C.byref(R)) == 0            # the same record, whole again
    ref = ur.ref_fixture("min0")
    assert np.array_equal(outs["status"], ref["status"]) and R.counts.n_visited == ref["n_visited"]
    assert L.slamit_unproject_closest_batch_dev(0, None, None) == -1 and L.slamit_rgbd_depth_batch_dev(0, None, None) == -1
    big = api.UnprojectBatchRec(1, 8192)
    assert L.slamit_unproject_closest_batch_dev(0, C.byref(big), None) == -3


def test_rgbd_host_form():
    names = sorted(ur.RGBD_CASES)
    assert {ur.RGBD_CASES[k]["kind"] for k in names} == {"u16", "f32"} and {ur.RGBD_CASES[k]["factor"] for k in names} == {1.0, 1.0 / 5000.0}
    assert any(ur.RGBD_CASES[k]["pad"] > 0 for k in names)
    outs = api.rgbd_depth_batch([ur.rgbd_fixture(k) for k in names])
    for name, out in zip(names, outs):
        ur.assert_same_rgbd(out, ur.ref_rgbd(name), name)
        assert set(out["status"].tolist()) == {0, 1, 2}
    one = api.rgbd_depth(ur.rgbd_fixture(names[1]))
    ur.assert_same_rgbd(one, outs[1], "single")
    assert api.rgbd_depth_batch([]) == []
    empty = api.rgbd_depth(dict(ur.rgbd_fixture(names[0]), kps=np.zeros(0, api.KP_DTYPE), kps_un=np.zeros(0, api.KP_DTYPE)))
    assert len(empty["depth"]) == 0


def test_rgbd_resident_form_on_strided_planes():
    """u16 and f32 planes with a pitch larger than the width, resident; a frame's count below cap leaves the rest untouched"""
    import torch

    names = ("u16_pitch", "f32_one")
    probs = [ur.rgbd_fixture(k) for k in names]
    B, cap = len(probs), 320
    kps, kun = np.zeros((B, cap), api.KP_DTYPE), np.zeros((B, cap), api.KP_DTYPE)
    planes = np.zeros(B, api.DEPTH_PLANE_DTYPE)
    stores = [torch.from_numpy(p["storage"].view(np.int16) if p["kind"] == "u16" else p["storage"]).cuda() for p in probs]
    for f, (p, s) in enumerate(zip(probs, stores)):
        n = int(p["n"])
        kps[f, :n], kun[f, :n] = p["kps"], p["kps_un"]
        kps["x"][f, n:] = np.nan                       # would be status 2 if it were read
        planes[f] = (s.data_ptr(), p["storage"].strides[0], p["width"], p["height"], api.DEPTH_TYPES.index(p["kind"]), p["factor"])
    t = dict(planes=torch.from_numpy(planes.view(np.int32).reshape(B, -1)).cuda(), mbf=torch.tensor([float(p["mbf"]) for p in probs], dtype=torch.float32, device="cuda"),
             kps=torch.from_numpy(kps.view(np.float32).reshape(B, cap, 7)).cuda(), kps_un=torch.from_numpy(kun.view(np.float32).reshape(B, cap, 7)).cuda(),
             n=torch.tensor([int(p["n"]) for p in probs], dtype=torch.int32, device="cuda"), u_right=torch.full((B, cap), -7.0, device="cuda"),
             depth=torch.full((B, cap), -7.0, device="cuda"), status=torch.full((B, cap), 99, dtype=torch.uint8, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.rgbd_depth_batch_dev(t, stream=s.cuda_stream)
    s.synchronize()
    for f, name in enumerate(names):
        n = int(probs[f]["n"])
        got = dict(u_right=t["u_right"][f, :n].cpu().numpy(), depth=t["depth"][f, :n].cpu().numpy(), status=t["status"][f, :n].cpu().numpy())
        ur.assert_same_rgbd(got, ur.ref_rgbd(name), name)
        assert bool((t["status"][f, n:] == 99).all()) and bool((t["depth"][f, n:] == -7.0).all())
    del stores

