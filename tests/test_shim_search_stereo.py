"""The shim's three guided-search drivers and Tracking::SearchLocalPoints on frames that carry stereo keypoints (mvuRight set), over
the mock types of shim_test, which have mTrackProjXR and mbf as the reference's own types do: matches and the mvpMapPoints /
Replace / AddObservation bookkeeping against the numpy restatement tests/search_stereo_ref.py, and the host loop of a driver against
its deviceProjection form byte for byte."""
import struct

import numpy as np
import pytest

from tests import frustum_ref
from tests import project_ref as pref
from tests import project_stereo_ref as sref
from tests import search_stereo_fixtures as fx
from tests import search_stereo_ref as model
from tests.test_shim import _apply_in_order, _search_frame_blob, _three_maxima
from tests.test_shim_frustum import blob as frustum_blob
from tests.test_shim_frustum import scenario as frustum_scenario
from tests.test_shim_project import INVSIG, _b, _bounds, _fuse_kf_state, _pose12, _run, _scene

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
SCALE = (f32(1.2) ** np.arange(8, dtype=f32)).astype(f32)


def mvu_right(frame, qdesc, q_ur, q_r, seed, shift, noise=0.25):
    """mvuRight for a frame whose keypoints were derived from points: a keypoint carries its point's right-image column, moved within
    `noise` of that point's window (`noise` px when q_r is None) or, for four in ten, `shift` px away; half the keypoints are
    monocular (-1) and two carry exactly 0."""
    rs = np.random.RandomState(4000 + seed)
    bits, qbits = np.unpackbits(frame["desc"], axis=1).astype(np.int16), np.unpackbits(qdesc, axis=1).astype(np.int16)
    owner = np.argmin(bits @ (1 - qbits).T + (1 - bits) @ qbits.T, axis=1)
    n = len(owner)
    width = q_r[owner] if q_r is not None else np.ones(n, f32)
    kur = (q_ur[owner] + rs.uniform(-noise, noise, n) * width + np.where(rs.rand(n) < 0.4, shift, 0.0)).astype(f32)
    kur[(rs.rand(n) < 0.5) | ~(kur > 0)] = -1.0
    kur[rs.permutation(n)[:2]] = 0.0
    return kur


# ---- SearchByProjection(F, vpMapPoints, th) ---------------------------------------------------------------------------------------

def local_map_case():
    frame, qs, st = fx.fixture(fx.RADIUS, 300)
    n, m, th, nnratio = 300, fx.M, 3.0, 0.8
    rs = np.random.RandomState(6)
    state = np.where(frame["kp_taken"] > 0, 1, rs.randint(0, 2, n) * 2).astype(i32)
    viewcos = rs.choice(np.array([0.9995, 0.95], f32), m)
    level = np.clip(np.where(qs["level_max"] >= 0, qs["level_max"], qs["level_min"]), 0, 7).astype(i32)
    inview = (rs.rand(m) < 0.9).astype(i32)
    bad = (rs.rand(m) < 0.05).astype(i32)
    nobs = (rs.rand(m) < 0.95).astype(i32) * 3
    proj = qs["uvr"][:, :2].astype(f32)
    blob = _search_frame_blob(0, frame, n, m, th, nnratio, SCALE, np.zeros(n, f32), state, 645.1, 483.9)
    blob += proj.tobytes() + viewcos.tobytes() + level.tobytes() + inview.tobytes() + bad.tobytes() + nobs.tobytes() + qs["desc"].tobytes()
    tail = st["kp_ur"].astype(f32).tobytes() + st["q_ur"].astype(f32).tobytes()          # mvuRight[n], mTrackProjXR[m]
    keep = np.nonzero((inview != 0) & (bad == 0))[0]
    rad = (np.where(viewcos > f32(0.998), f32(2.5), f32(4.0)).astype(f32) * f32(th)) * SCALE[level]
    q = dict(uvr=np.concatenate([proj, rad[:, None]], 1)[keep], level_min=level[keep] - 1, level_max=level[keep], desc=qs["desc"][keep],
             takes=(nobs[keep] > 0).astype(np.uint8))
    f = dict(frame, kp_taken=(state == 1).astype(np.uint8))
    want = model.guided_search(f, q, 100, True, nnratio, er_mode=fx.RADIUS, kp_ur=st["kp_ur"], q_ur=st["q_ur"][keep])
    mono = model.guided_search(f, q, 100, True, nnratio)
    full = np.full(m, -1, i32)
    full[keep] = want[0]
    return blob, tail, want[1], _apply_in_order(n, state, full), int((mono[0] != want[0]).sum())


def test_search_by_projection_local_map(tmp_path):
    blob, tail, nm, owner, differ = local_map_case()
    assert nm > 20 and differ >= 10
    r = np.frombuffer(_run(tmp_path, "search", blob + tail), i32)
    assert r[0] == 0 and r[1] == nm
    assert np.array_equal(r[2:], owner)
    mono = np.frombuffer(_run(tmp_path, "search", blob), i32)                            # the same blob without its tail: a monocular frame
    assert mono[0] == 0 and not np.array_equal(mono[2:], owner)


# ---- SearchByProjection(CurrentFrame, LastFrame, th, bMono) -----------------------------------------------------------------------

MBF = 40.0


def last_frame_case():
    pr, _, frame, qdesc, takes, qangle = _scene(pref.LAST_FRAME, 3, th=7.0, direction=0)
    h = sref.host_points_stereo(pr, MBF)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    kur = mvu_right(frame, qdesc, h["ur"], h["r"], 1, 120.0)
    state = np.where(frame["kp_taken"] != 0, 1, 0).astype(i32)
    blob = _b(struct.pack("<iiiff", 1, n, m, 7.0, 0.9), _bounds(pr, frame), pr["scale_factors"], frame["kp_xy"], frame["kp_octave"], frame["kp_angle"], state,
              frame["desc"], _pose12(pr["R"], pr["t"]), _pose12(pr["R"], pr["t"]), np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"], 0.1], f32),
              struct.pack("<i", 0), pr["pos"], qangle, (1 - pr["skip"]).astype(i32), np.zeros(m, i32), pr["octave"], takes.astype(i32), qdesc)
    tail = struct.pack("<f", MBF) + kur.tobytes()
    keep = np.flatnonzero(h["valid"])
    q = dict(uvr=h["uvr"][keep], level_min=h["level_min"][keep], level_max=h["level_max"][keep], desc=qdesc[keep], takes=takes[keep])
    f = dict(frame, kp_taken=(state == 1).astype(np.uint8))
    want = model.guided_search(f, q, 100, False, 0.9, er_mode=fx.RADIUS, kp_ur=kur, q_ur=h["ur"][keep])
    mono = model.guided_search(f, q, 100, False, 0.9)
    full = np.full(m, -1, i32)
    full[keep] = want[0]
    owner = _apply_in_order(n, state, full)
    nm = want[1]
    # the rotation histogram (ORBmatcher.cc:1436-1469): bins of bestIdx2 in visiting order, float32
    hist = [[] for _ in range(30)]
    for qi in keep:
        k = full[qi]
        if k < 0:
            continue
        rot = f32(qangle[qi] - frame["kp_angle"][k])
        if rot < 0:
            rot = f32(rot + f32(360))
        b = int(np.floor(f32(rot * (f32(1.0) / f32(30))) + f32(0.5)))
        hist[0 if b == 30 else b].append(k)
    kept = _three_maxima([len(x) for x in hist])
    for i in range(30):
        if i not in kept:
            for k in hist[i]:
                owner[k] = -1
                nm -= 1
    return blob, tail, nm, owner, int((mono[0] != want[0]).sum())


def test_search_by_projection_last_frame(tmp_path):
    blob, tail, nm, owner, differ = last_frame_case()
    assert nm > 20 and differ >= 10
    host, dev = _run(tmp_path, "search", blob + tail, "host"), _run(tmp_path, "search", blob + tail, "device")
    assert host == dev
    r = np.frombuffer(dev, i32)
    assert r[0] == 0 and r[1] == nm
    assert np.array_equal(r[2:], owner)


# ---- Fuse(pKF, vpMapPoints, th) ---------------------------------------------------------------------------------------------------

def fuse_case():
    pr, _, frame, qdesc, _, _ = _scene(pref.FUSE, 5)
    h = sref.host_points_stereo(pr, MBF)
    n, m = len(frame["kp_xy"]), int(pr["n"])
    kur = mvu_right(frame, qdesc, h["ur"], None, 2, 4.0, noise=0.5)     # half a pixel keeps the third term small; 4 px fails 7.8
    bad = (h["status"] == 7).astype(i32)
    kf_state = _fuse_kf_state(5, n)
    blob = _b(struct.pack("<iif", n, m, 3.0), pr["R"], pr["t"], pr["O"], np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), _bounds(pr, frame), pr["scale_factors"],
              INVSIG, frame["kp_xy"], frame["kp_octave"], kf_state, frame["desc"], pr["pos"], pr["normal"], pr["max_dist"], pr["min_dist"],
              np.zeros(m, i32), np.full(m, 2, i32), bad, np.zeros(m, i32), pr["skip"].astype(i32), qdesc)
    tail = struct.pack("<f", MBF) + kur.tobytes()
    keep = np.flatnonzero(h["valid"])
    q = dict(uvr=h["uvr"][keep], level_min=h["level_min"][keep], level_max=h["level_max"][keep], desc=qdesc[keep], takes=np.zeros(len(keep), np.uint8))
    f = dict(frame, kp_taken=np.zeros(n, np.uint8))
    rule = dict(th_dist=50, use_ratio=False, nnratio=0.6, chi2_gate=5.99, inv_level_sigma2=INVSIG)
    want = model.guided_search(f, q, er_mode=fx.CHI2, kp_ur=kur, q_ur=h["ur"][keep], **rule)
    mono = model.guided_search(f, q, **rule)
    # the bookkeeping of ORBmatcher.cc:955-976, in order (tests/test_shim.py::test_shim_fuse)
    owner = np.where(kf_state > 0, -2, -1).astype(np.int64)
    own_obs, own_bad = kf_state - 1, np.zeros(n, bool)
    p_bad, p_inkf, p_nobs = np.zeros(m, bool), np.zeros(m, bool), np.full(m, 2)
    p_bad[bad != 0] = True
    added, replaced, own_replaced = np.full(m, -1), np.full(m, -1), np.full(n, -1)
    nfused = 0
    for k, j in enumerate(keep):
        bi = want[0][k]
        if bi < 0 or p_bad[j] or p_inkf[j]:
            continue
        if owner[bi] == -2:
            if not own_bad[bi]:
                if own_obs[bi] > p_nobs[j]:
                    replaced[j], p_bad[j] = -2, True
                else:
                    own_replaced[bi], own_bad[bi] = j, True
        elif owner[bi] >= 0:
            o = owner[bi]
            if not p_bad[o]:
                if p_nobs[o] > p_nobs[j]:
                    replaced[j], p_bad[j] = o, True
                else:
                    replaced[o], p_bad[o] = j, True
        else:
            added[j], p_inkf[j], owner[bi] = bi, True, j
            p_nobs[j] += 1
        nfused += 1
    expect = np.concatenate([[0, nfused], np.stack([added, replaced, p_bad.astype(np.int64)], 1).reshape(-1), owner, own_replaced]).astype(i32)
    return blob, tail, expect, nfused, int((mono[0] != want[0]).sum())


def test_fuse(tmp_path):
    blob, tail, expect, nfused, differ = fuse_case()
    assert nfused > 20 and differ >= 10
    host, dev = _run(tmp_path, "fuse", blob + tail, "host"), _run(tmp_path, "fuse", blob + tail, "device")
    assert host == dev
    assert np.array_equal(np.frombuffer(dev, i32), expect)


def test_fuse_over_several_targets(tmp_path):
    """Fuse(vector<KeyFrame*>, points, th) on three stereo keyframes: the batched device projection, the per-target device calls and
    the host loops leave the same bytes, and not the bytes of the same keyframes without their mvuRight."""
    pr, _, _, qdesc, _, _ = _scene(pref.FUSE, 9)
    R, t = np.asarray(pr["R"], f32).reshape(3, 3), np.asarray(pr["t"], f32)
    cams, hs = [], []
    for k in range(3):
        tk = (t + f32([0.05, -0.03, 0.02]) * f32(k)).astype(f32)
        Ok = (-(R.astype(np.float64).T @ tk.astype(np.float64))).astype(f32)
        cams.append(dict(pr, t=tk, O=Ok))
        hs.append(sref.host_points_stereo(cams[-1], MBF + k))
    keep = np.flatnonzero(np.all([hk["status"] != 7 for hk in hs], 0) & (pr["skip"] == 0))
    m = len(keep)
    parts = [struct.pack("<iif", 3, m, 3.0), pr["pos"][keep], pr["normal"][keep], pr["max_dist"][keep], pr["min_dist"][keep], np.full(m, 2, i32), qdesc[keep]]
    tail = []
    for k, (cam, hk) in enumerate(zip(cams, hs)):
        frame = pref.search_side(cam, hk, 60 + 9, 0.7)[0]
        n = len(frame["kp_xy"])
        parts += [cam["R"], cam["t"], cam["O"], np.array([pr["fx"], pr["fy"], pr["cx"], pr["cy"]], f32), _bounds(pr, frame), pr["scale_factors"], INVSIG,
                  struct.pack("<i", n), frame["kp_xy"], frame["kp_octave"], _fuse_kf_state(20 + k, n), frame["desc"]]
        kur = mvu_right(frame, qdesc, hk["ur"], None, 10 + k, 4.0, noise=0.5)
        if k == 1:
            kur[:] = -1.0                                                   # a monocular keyframe among stereo ones
        tail += [struct.pack("<f", MBF + k), kur]
    blob, tail = _b(*parts), _b(*tail)
    outs = {mode: _run(tmp_path, "fuse_targets", blob + tail, *mode) for mode in (("device", "batch"), ("device", "single"), ("host", "single"), ("host", "batch"))}
    first = outs[("device", "batch")]
    status, count = struct.unpack_from("<ii", first)
    assert status == 0 and count > 20
    for mode, out in outs.items():
        assert out == first, mode
    mono = _run(tmp_path, "fuse_targets", blob, "device", "batch")
    assert struct.unpack_from("<i", mono)[0] == 0 and mono != first


# ---- Tracking::SearchLocalPoints --------------------------------------------------------------------------------------------------

def local_points_case():
    pr, frame, qdesc, nobs, state = frustum_scenario()
    h = frustum_ref.host_points(pr)
    nkp = len(frame["kp_xy"])
    kur = mvu_right(frame, qdesc, h["uR"], h["r"], 3, 150.0)
    keep = np.flatnonzero(h["valid"])
    q = dict(uvr=h["uvr"][keep], level_min=h["level_min"][keep], level_max=h["level_max"][keep], desc=qdesc[keep], takes=(nobs[keep] > 0).astype(np.uint8))
    want = model.guided_search(frame, q, 100, True, 0.8, er_mode=fx.RADIUS, kp_ur=kur, q_ur=h["uR"][keep])
    mono = model.guided_search(frame, q, 100, True, 0.8)
    owner = np.where(state == 1, -2, np.where(state == 2, -3, -1)).astype(i32)          # the frame's own bad point (3) is cleared first
    for k, j in zip(want[0], keep):
        if k >= 0:
            owner[k] = j
    return frustum_blob(pr, frame, qdesc, nobs, state, 0.8), kur.tobytes(), want[1], owner, int((mono[0] != want[0]).sum()), int(pr["n"]), nkp


def test_search_local_points_on_a_stereo_frame(tmp_path):
    blob, tail, nm, owner, differ, n, nkp = local_points_case()
    assert nm > 20 and differ >= 10
    out = _run(tmp_path, "frustum", blob + tail)
    status, got_nm, _ = struct.unpack_from("<iii", out)
    assert status == 0 and got_nm == nm
    assert np.array_equal(np.frombuffer(out, i32, nkp, 12 + 28 * n), owner)
