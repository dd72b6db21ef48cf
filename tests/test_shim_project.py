"""shim/ORBmatcher.h with deviceProjection: each of the six drivers that project map points themselves, on mock types (shim_test), run
once with its host loop and once with ONE slamit_project call in its place.  The mocks' PredictScale is the real formula over
csrc/frustum.h's log, so the two runs must give the same bytes: matches, replace lists, observation calls and LastStatus.  And the
multi-target Fuse against the per-target calls, with one target's Replace turning a point bad for the next and another changing a
survivor's descriptor.

The host loops index mvScaleFactors with the predicted level unchecked, which the device path refuses (status 7):
the scenarios mark such points bad, so that the comparison is between two defined computations."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import project_ref as ref
from tests.helpers import ROOT
from weiner_slamit_v2_amd import synth

pytestmark = pytest.mark.gpu

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")
LSF = np.float32(0.18232)                                               # the mocks' mfLogScaleFactor
f32, i32 = np.float32, np.int32


def _build():
    from weiner_slamit_v2_amd import build

    build.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def _run(tmp_path, command, blob, *modes):
    """shim_test <command> in out <modes...> -> the output's bytes; nothing on stderr."""
    _build()
    pin, pout = tmp_path / "in.bin", tmp_path / ("out_%s.bin" % "_".join(modes))
    pin.write_bytes(blob)
    p = subprocess.run([EXE, command, str(pin), str(pout)] + list(modes), stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode()
    return pout.read_bytes()


def _scene(form, seed, n=300, th=3.0, direction=0, **kw):
    """synth_project with the mocks' log scale factor, the header's verdict on it, and the searched frame's keypoints."""
    pr = synth.synth_project(seed, n, form, th, direction, octave_frac=0.0, **kw)
    pr["log_scale_factor"] = LSF
    h = ref.host_points(pr)
    frame, qdesc, takes, qangle = ref.search_side(pr, h, 60 + seed, 0.7)
    return pr, h, frame, qdesc, takes, qangle


def _b(*parts):
    return b"".join(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else p for p in parts)


def _bounds(pr, frame):
    return np.array([pr["min_x"], pr["max_x"], pr["min_y"], pr["max_y"], frame["inv_w"], frame["inv_h"]], f32)


def _pose12(R, t):
    return np.concatenate([np.asarray(R, f32).reshape(9), np.asarray(t, f32).reshape(3)])


def _both(tmp_path, command, blob, extra=()):
    host, dev = _run(tmp_path, command, blob, "host", *extra), _run(tmp_path, command, blob, "device", *extra)
    status, count = struct.unpack_from("<ii", dev)
    print("%s: status %d, count %d, %d bytes" % (command, status, count, len(dev)))
    assert status == 0 and struct.unpack_from("<ii", host) == (0, count)
    assert host == dev
    return count, dev


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_search_by_projection_last_frame(tmp_path, direction):
    pr, h, frame, qdesc, takes, qangle = _scene(ref.LAST_FRAME, 3, th=7.0, direction=direction)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    R, t = np.asarray(pr["R"], f32).reshape(3, 3), np.asarray(pr["t"], f32)
    # the last frame's camera half a unit behind (forward), ahead (backward) of the current one along its axis; mono otherwise
    tlw = t + f32([0, 0, 0.5]) * f32({0: 0, 1: 1, 2: -1}[direction])
    state = np.where(frame["kp_taken"] != 0, 1, 0).astype(i32)
    blob = _b(struct.pack("<iiiff", 1, n, m, 7.0, 0.9), _bounds(pr, frame), pr["scale_factors"], frame["kp_xy"], frame["kp_octave"], frame["kp_angle"], state,
              frame["desc"], _pose12(R, t), _pose12(R, tlw), np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"], 0.1], f32),
              struct.pack("<i", 1 if direction == 0 else 0), pr["pos"], qangle, (1 - pr["skip"]).astype(i32), np.zeros(m, i32), pr["octave"],
              takes.astype(i32), qdesc)
    count, _ = _both(tmp_path, "search", blob)
    assert count > 20


def test_search_by_projection_relocalization(tmp_path):
    pr, h, frame, qdesc, takes, qangle = _scene(ref.RELOC, 4, th=10.0)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    bad = (h["status"] == 7).astype(i32)                                  # the host loop would index mvScaleFactors out of bounds
    assert bad.sum() >= 3 and (h["status"] == 5).sum() >= 3
    state = np.where(frame["kp_taken"] != 0, 1, 0).astype(i32)
    blob = _b(struct.pack("<iiiff", 2, n, m, 10.0, 0.9), _bounds(pr, frame), pr["scale_factors"], frame["kp_xy"], frame["kp_octave"], frame["kp_angle"], state,
              frame["desc"], _pose12(pr["R"], pr["t"]), np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), struct.pack("<i", 100), pr["pos"], qangle,
              pr["max_dist"], pr["min_dist"], (1 - pr["skip"]).astype(i32), bad, np.zeros(m, i32), np.zeros(m, i32), qdesc)
    count, _ = _both(tmp_path, "search", blob)
    assert count > 20


def _fuse_kf_state(seed, n):
    """keypoints of the keyframe: 30 % free, 40 % hold a point of its own with 5 observations (the map point is replaced by it), 30 % one
    with none (it is replaced by the map point)"""
    r = np.random.RandomState(900 + seed).rand(n)
    return np.where(r < 0.3, 0, np.where(r < 0.7, 6, 1)).astype(i32)


INVSIG = (f32(1) / ((f32(1.2) ** np.arange(8, dtype=f32)) ** 2)).astype(f32)


def test_fuse(tmp_path):
    pr, h, frame, qdesc, takes, qangle = _scene(ref.FUSE, 5)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    bad = (h["status"] == 7).astype(i32)
    assert bad.sum() >= 3
    blob = _b(struct.pack("<iif", n, m, 3.0), pr["R"], pr["t"], pr["O"], np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), _bounds(pr, frame), pr["scale_factors"],
              INVSIG, frame["kp_xy"], frame["kp_octave"], _fuse_kf_state(5, n), frame["desc"], pr["pos"], pr["normal"], pr["max_dist"], pr["min_dist"],
              np.zeros(m, i32), np.full(m, 2, i32), bad, np.zeros(m, i32), pr["skip"].astype(i32), qdesc)
    count, out = _both(tmp_path, "fuse", blob)
    per_point = np.frombuffer(out, i32, 3 * m, 8).reshape(m, 3)
    assert count > 20 and (per_point[:, 0] >= 0).sum() > 3 and (per_point[:, 1] == -2).sum() > 3   # observations added, points replaced


def _sim3_points(pr, bad, qdesc):
    m = int(pr["n"])
    normal = pr["normal"] if pr["normal"] is not None else np.zeros((m, 3), f32)
    return _b(struct.pack("<i", m), pr["pos"], normal, pr["max_dist"], pr["min_dist"], np.zeros(m, i32), bad.astype(i32), np.full(m, -1, i32), qdesc)


def _sim3_kf(pr, frame, R, t, mp):
    n = len(frame["kp_xy"])
    return _b(np.asarray(R, f32).reshape(9), np.asarray(t, f32).reshape(3), np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), _bounds(pr, frame),
              pr["scale_factors"], struct.pack("<i", n), frame["kp_xy"], frame["kp_octave"], mp.astype(i32), frame["desc"])


@pytest.mark.parametrize("variant", [0, 1])
def test_sim3_projection_and_fuse(tmp_path, variant):
    form, th = (ref.SIM3_PROJ, 10.0) if variant == 0 else (ref.SIM3_FUSE, 4.0)
    pr, h, frame, qdesc, takes, qangle = _scene(form, 6 + variant, th=th)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    bad = (h["status"] == 7) | (pr["skip"] != 0)
    rs = np.random.RandomState(77 + variant)
    mp = np.where(rs.rand(n) < 0.3, rs.randint(0, m, n), -1)              # keypoints that hold a map point already
    Scw = pr["true"]["Scw"]
    blob = _b(struct.pack("<iif", variant, 1, th), _sim3_points(pr, bad, qdesc), _sim3_kf(pr, frame, np.eye(3), np.zeros(3), mp), Scw.astype(f32).reshape(12))
    if variant == 0:
        blob += np.where(rs.rand(n) < 0.1, rs.randint(0, m, n), -1).astype(i32).tobytes()   # vpMatched on entry
    count, _ = _both(tmp_path, "sim3", blob)
    assert count > 20


def _owners(frame, qdesc, limit=70):
    """the map point whose descriptor each keypoint was made from (tests.project_ref.search_side), or -1 for clutter"""
    d = np.unpackbits(frame["desc"][:, None, :] ^ qdesc[None, :, :], axis=2).sum(2)
    j = d.argmin(1)
    return np.where(d[np.arange(len(j)), j] <= limit, j, -1)


def test_search_by_sim3(tmp_path):
    """Both directions: keyframe 1's points into keyframe 2 through (sR21, t21) and back.  s12 = 1 here, so that one set of world points
    serves both keyframes; the similarity's scale is in the fixtures of tests/project_ref.py."""
    pr, h, frame2, qdesc, takes, qangle = _scene(ref.SIM3_PAIR, 8, th=7.5, scale=1.0)
    m = int(pr["n"])
    R1w, t1w = np.asarray(pr["R"], f32).reshape(3, 3), np.asarray(pr["t"], f32)
    base = synth.synth_frustum(8, m, 7.5)
    R2w, t2w = base["Rcw"].reshape(3, 3), base["tcw"]
    R12 = (R1w.astype(np.float64) @ R2w.astype(np.float64).T).astype(f32)
    t12 = (t1w.astype(np.float64) - R12.astype(np.float64) @ t2w.astype(np.float64)).astype(f32)
    # the other direction as the driver computes it: keyframe 2's pose, then (s12 R12, t12), searched in keyframe 1
    back = dict(pr, R=R2w.reshape(9), t=t2w, R2=R12.reshape(9), t2=t12)
    hb = ref.host_points(back)
    frame1, q1, _, _ = ref.search_side(back, hb, 60 + 8, 0.7)           # the seed of _scene: the same descriptors, keypoints around keyframe 1's projections
    assert np.array_equal(q1, qdesc)
    own1, own2 = _owners(frame1, qdesc), _owners(frame2, qdesc)
    assert (own1 >= 0).sum() > 50 and (own2 >= 0).sum() > 50
    bad = (h["status"] == 7) | (hb["status"] == 7) | (pr["skip"] != 0)
    blob = _b(struct.pack("<iif", 2, 2, 7.5), _sim3_points(pr, bad, qdesc), _sim3_kf(pr, frame1, R1w, t1w, own1), _sim3_kf(pr, frame2, R2w, t2w, own2),
              struct.pack("<f", 1.0), R12.reshape(9), t12, np.full(len(frame1["kp_xy"]), -1, i32))
    count, _ = _both(tmp_path, "sim3", blob)
    assert count > 5


def test_the_multi_target_fuse_equals_the_per_target_calls(tmp_path):
    """Three targets, the same points.  Target 0's Replace turns points bad that target 1's projection had accepted, and replaces
    points of the target's own by map points whose descriptor changes with it: the batched call must test and read both at each
    target's turn, as the per-target calls do."""
    pr, h0, _, qdesc, _, _ = _scene(ref.FUSE, 9)
    R, t = np.asarray(pr["R"], f32).reshape(3, 3), np.asarray(pr["t"], f32)
    cams, hs = [], []
    for k in range(3):
        tk = (t + f32([0.05, -0.03, 0.02]) * f32(k)).astype(f32)
        Ok = (-(R.astype(np.float64).T @ tk.astype(np.float64))).astype(f32)
        cams.append(dict(pr, t=tk, O=Ok))
        hs.append(ref.host_points(cams[-1]))
    keep = np.flatnonzero(np.all([hk["status"] != 7 for hk in hs], 0) & (pr["skip"] == 0))   # the host loop's undefined case; no null points
    m = len(keep)
    parts = [struct.pack("<iif", 3, m, 3.0), pr["pos"][keep], pr["normal"][keep], pr["max_dist"][keep], pr["min_dist"][keep], np.full(m, 2, i32), qdesc[keep]]
    for k, (cam, hk) in enumerate(zip(cams, hs)):
        frame = ref.search_side(cam, hk, 60 + 9, 0.7)[0]                  # the same seed: the same descriptors, keypoints around this camera's projections
        n = len(frame["kp_xy"])
        parts += [cam["R"], cam["t"], cam["O"], np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), _bounds(pr, frame), pr["scale_factors"], INVSIG,
                  struct.pack("<i", n), frame["kp_xy"], frame["kp_octave"], _fuse_kf_state(20 + k, n), frame["desc"]]
    blob = _b(*parts)
    outs = {mode: _run(tmp_path, "fuse_targets", blob, *mode) for mode in (("device", "batch"), ("device", "single"), ("host", "single"), ("host", "batch"))}
    first = outs[("device", "batch")]
    status, count = struct.unpack_from("<ii", first)
    assert status == 0 and count > 40
    for mode, out in outs.items():
        assert out == first, mode
    rec = np.frombuffer(first, np.dtype([("added", "<i4"), ("replaced", "<i4"), ("bad", "<i4"), ("nobs", "<i4"), ("desc", "u1", 32)]), m, 8)
    ok1 = hs[1]["status"][keep] == 0
    print("multi-target fuse: %d fused, %d points bad, %d of them accepted by target 1's projection, %d survivors with a new descriptor" %
          (count, rec["bad"].sum(), (rec["bad"] != 0)[ok1].sum(), ((rec["desc"] != qdesc[keep]).any(1) & (rec["bad"] == 0)).sum()))
    assert (rec["bad"] != 0)[ok1].sum() >= 3                              # bad after an earlier target, though the batched projection took them
    assert ((rec["desc"] != qdesc[keep]).any(1) & (rec["bad"] == 0)).sum() >= 3   # survivors whose descriptor an earlier target changed
