"""shim/Tracking.h's UpdateLastFrame / CreateNewKeyFramePoints / StereoInitializationPoints / CloseRatio and shim/FrameOps.h's
ComputeStereoFromRGBD over mock Frame / KeyFrame / MapPoint / Map types (shim_test unproject) against the numpy restatement of the
reference's loops (tests/unproject_ref.py): the same points, created in the same order, with the same positions, and the
reference's bookkeeping around them."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import unproject_ref as ur
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_headers_list_what_they_need():
    _build()
    hdr = open(os.path.join(SHIM, "Tracking.h")).read()
    for want in ("static int UpdateLastFrame(FrameT& F, float thDepth, TemporalT& temporal, MakeFn&& make", "static int CreateNewKeyFramePoints(",
                 "static int StereoInitializationPoints(", "static bool CloseRatio(", "slamit_unproject_closest(device, &P, &R)", "mlpTemporalPoints",
                 "ComputeDistinctiveDescriptors", "static slamit_unproject_counts LastCounts()"):
        assert want in hdr, want
    fo = open(os.path.join(SHIM, "FrameOps.h")).read()
    assert "void ComputeStereoFromRGBD(FrameT& F, const cv::Mat& imDepth" in fo and "slamit_rgbd_depth(0, &P, &R)" in fo
    assert 'mode == "unproject"' in open(os.path.join(SHIM, "shim_main.cc")).read()


def _state(pr, seed):
    """0 no point, 1 a point with observations, 2 a point WITHOUT observations (a third of the untracked keypoints): the walk treats
    2 as 0, and CreateNewKeyFrame also takes it out of the frame (Tracking.cc:1370)"""
    rs = np.random.RandomState(seed)
    st = np.asarray(pr["tracked"], np.uint8).copy()
    st[(st == 0) & (rs.rand(len(st)) < 0.33)] = 2
    return st


def _run(tmp_path, variant, pr, state):
    from weiner_slamit_v2_amd import api

    n = int(pr["n"])
    blob = struct.pack("<ii", variant, n) + api.unproject_frame_record(pr).tobytes() + np.ascontiguousarray(pr["kps_un"], api.KP_DTYPE).tobytes()
    blob += np.ascontiguousarray(pr["depth"], np.float32).tobytes() + state.tobytes()
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(pin, "wb").write(blob)
    subprocess.check_call([EXE, "unproject", pin, pout])
    raw = open(pout, "rb").read()
    head = np.frombuffer(raw, np.int32, 12, 0)
    out = dict(status=int(head[0]), made=int(head[1]), close_ok=int(head[2]), n_map=int(head[3]), n_total=int(head[4]),
               counts=dict(zip(ur.COUNTS, (int(v) for v in head[5:11]))))
    nc, o = int(head[11]), 48
    rec = np.dtype([("id", "<i4"), ("kp", "<i4"), ("seq", "<i4", 5), ("pos", "<f4", 3), ("normal", "<f4", 3), ("maxd", "<f4"), ("mind", "<f4")])
    out["created"] = np.frombuffer(raw, rec, nc, o).copy(); o += nc * rec.itemsize
    out["owner"] = np.frombuffer(raw, np.int32, n, o).copy(); o += 4 * n
    out["temporal"], out["kf_points"], out["map_points"] = (int(v) for v in np.frombuffer(raw, np.int32, 3, o)); o += 12
    assert o == len(raw)
    return out


CASES = [(0, "mixed", 0), (0, "few_close", 0), (1, "keyframe", 1), (1, "many_close", 1), (2, "all", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,name,ctor", CASES)
def test_the_same_points_in_the_same_order(tmp_path, variant, name, ctor):
    _build()
    pr = dict(ur.fixture(name), ctor=ctor, mode=1 if variant == 2 else 0)
    state = _state(pr, 5 + variant)
    tracked = (state == 1).astype(np.uint8)
    close = ur.walk(dict(pr, tracked=tracked, mode=0))     # NeedNewKeyFrame's counts are taken with mThDepth whatever the walk was
    # StereoInitialization has no threshold: the shim passes 0, and the walk's own counters are those of th_depth = 0
    ref = ur.walk(dict(pr, tracked=tracked, th_depth=np.float32(0.0))) if variant == 2 else close
    out = _run(tmp_path, variant, pr, state)
    assert out["status"] == 0 and out["counts"] == {k: ref[k] for k in ur.COUNTS}
    want = [i for i in ref["order"][:ref["n_visited"]] if ref["status"][i] == 3]       # the reference's order of creation
    c = out["created"]
    assert out["made"] == len(want) == len(c) > 20
    assert c["kp"].tolist() == want and c["id"].tolist() == list(range(1000, 1000 + len(want)))    # mnId rises along the walk
    assert ur.same_bits(c["pos"], ref["pos"][want]) and ur.same_bits(c["normal"], ref["normal"][want])
    assert ur.same_bits(c["maxd"], ref["max_dist"][want]) and ur.same_bits(c["mind"], ref["min_dist"][want])
    # the frame's mvpMapPoints afterwards
    owner = np.where(state == 1, -2, np.where(state == 2, -3, -1))
    owner[want] = c["id"]
    if variant == 1:                                       # :1370: a visited point without observations leaves the frame even where nothing is made
        visited = ref["order"][:ref["n_visited"]]
        dropped = [i for i in visited if state[i] == 2 and ref["status"][i] == 4]
        owner[dropped] = -1
    assert np.array_equal(out["owner"], owner)
    if variant == 0:
        assert (out["temporal"], out["kf_points"], out["map_points"]) == (len(want), 0, 0) and np.all(c["seq"] == -1)
    else:                                                  # AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Map::AddMapPoint
        assert (out["temporal"], out["kf_points"], out["map_points"]) == (0, len(want), len(want))
        assert np.array_equal(c["seq"].reshape(-1), np.arange(5 * len(want)))
    # NeedNewKeyFrame's two counts, by the literal loop
    assert out["close_ok"] == 1 and (out["n_map"], out["n_total"]) == (close["n_map"], close["n_total"])
    assert 0 < close["n_map"] < close["n_total"]


@pytest.mark.gpu
def test_compute_stereo_from_rgbd_through_frameops(tmp_path):
    from weiner_slamit_v2_amd import api

    _build()
    pr = ur.rgbd_fixture("f32_5000")
    ref = ur.ref_rgbd("f32_5000")
    n, plane = int(pr["n"]), np.ascontiguousarray(pr["plane"])
    blob = struct.pack("<iiiiiff", 3, n, plane.shape[1], plane.shape[0], 0, float(pr["factor"]), float(pr["mbf"]))
    blob += np.ascontiguousarray(pr["kps"], api.KP_DTYPE).tobytes() + np.ascontiguousarray(pr["kps_un"], api.KP_DTYPE).tobytes() + plane.tobytes()
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(pin, "wb").write(blob)
    res = subprocess.run([EXE, "unproject", pin, pout], stderr=subprocess.PIPE, check=True)
    raw = open(pout, "rb").read()
    status, refused = np.frombuffer(raw, np.int32, 2, 0)
    assert status == 0 and refused == -1 and b"has no mbf" in res.stderr          # a Frame type without the stereo members is refused aloud
    got = dict(u_right=np.frombuffer(raw, np.float32, n, 8), depth=np.frombuffer(raw, np.float32, n, 8 + 4 * n), status=np.frombuffer(raw, np.uint8, n, 8 + 8 * n))
    ur.assert_same_rgbd(got, ref, "FrameOps")
