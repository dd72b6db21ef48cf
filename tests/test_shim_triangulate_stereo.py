"""shim/LocalMapping.h on stereo keyframes: CreateNewMapPoints(..., monocular = false, ...) over mock keyframes that have mb, mbf,
mvDepth and mvKeys (shim_test triangulate_stereo) against a Python model of the reference's loop -- the baseline gate against mb,
SearchForTriangulation as tests/bow_stereo_ref.py restates it, and the per-pair body by the same device entry point.  The mock's
mvKeys differ from its mvKeysUn, so a read of the wrong one shows in the unprojected points.  A keyframe type without the four
members still compiles and refuses (compile only)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bow_stereo_ref
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")
F32 = np.float32
SCALE = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
INTR = np.array([517.3, 516.5, 318.6, 255.3], F32)
MEDIAN_DEPTH = 4.0
MB = F32(0.12)
MBF = F32(MB * INTR[0])


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_header_lists_what_it_needs():
    hdr = open(os.path.join(SHIM, "LocalMapping.h")).read()
    for want in ("mb, mbf, mvDepth, mvKeys", "slamit_triangulate(device, &P, &R)", "slamit_triangulate_stereo(device, &P, &T, &R, NULL)",
                 "baseline < pKF2->mb", "T.bf = cur->mbf", "cur->mvKeys[i1].pt.x"):
        assert want in hdr, want
    main = open(os.path.join(SHIM, "shim_main.cc")).read()
    assert 'mode == "triangulate_stereo"' in main
    m = open(os.path.join(SHIM, "ORBmatcher.h")).read()
    assert "gate.onlyStereo = bOnlyStereo" in m and "monocular path only (the reference application is MONOCULAR)" not in m


def scenario(seed=0, m=140):
    """The current keyframe at the origin and three neighbours without rotation: 0.3 FORWARD (the rays of the points near the image
    centre are nearly parallel: UnprojectStereo; its epipole lies inside the image), 0.4 to the right, and 0.1 to the right -- under
    the rig's baseline of 0.12, over a hundredth of the median depth 4: only the stereo gate skips it.  m points seen by all four,
    one keypoint each, in a different order in every keyframe; the first 20 keypoints of the current keyframe already hold a map
    point.  60 % of the keypoints of every keyframe are stereo; mvKeys is mvKeysUn moved radially by up to about a pixel."""
    rs = np.random.RandomState(7900 + seed)
    X = np.stack([rs.uniform(-1.2, 1.2, m), rs.uniform(-0.9, 0.9, m), rs.uniform(2.5, 6.0, m)], 1)
    X[20:60, :2] *= 0.08                                                # a cluster near the optical axis: little parallax under forward motion
    centres = [np.zeros(3), np.array([0.0, 0.0, 0.3]), np.array([0.4, 0.0, 0.0]), np.array([0.1, 0.0, 0.0])]
    desc = rs.randint(0, 256, (m, 32)).astype(np.uint8)
    octave = rs.randint(0, 8, m).astype(np.int32)
    node = (np.arange(m) % 20).astype(np.int32)
    kfs = []
    for k, c in enumerate(centres):
        Xc = X - c
        xy = np.stack([INTR[0] * Xc[:, 0] / Xc[:, 2] + INTR[2], INTR[1] * Xc[:, 1] / Xc[:, 2] + INTR[3]], 1) + rs.normal(0, 0.25, (m, 2)) * SCALE[octave][:, None]
        xy = xy.astype(F32)
        ur = (xy[:, 0] - float(MBF) / Xc[:, 2] + rs.normal(0, 0.25, m) * SCALE[octave]).astype(F32)
        stereo = (rs.rand(m) < 0.6) & (ur >= 0)
        ur = np.where(stereo, ur, F32(-1)).astype(F32)
        with np.errstate(all="ignore"):
            depth = np.where(stereo, MBF / (xy[:, 0] - ur), F32(-1)).astype(F32)
        dxy = xy.astype(np.float64) - INTR[2:4]
        raw = (xy + 4e-8 * (dxy ** 2).sum(1)[:, None] * dxy + np.array([0.3, -0.2])).astype(F32)
        d = desc.copy()
        for i in range(m):
            for b in rs.randint(0, 256, rs.randint(0, 8)):
                d[i, b >> 3] ^= np.uint8(1 << (b & 7))
        order = np.arange(m) if k == 0 else rs.permutation(m)          # order[j] = the point at keypoint j
        mp = np.zeros(m, np.int32)
        if k == 0:
            mp[:20] = 1
        kfs.append(dict(t=(-c).astype(F32), order=order, xy=xy[order], desc=d[order], octave=octave[order], node=node[order], mp=mp,
                        ur=ur[order], depth=depth[order], raw=raw[order]))
    return kfs


def blob(kfs, monocular=0):
    out = [struct.pack("<ii", len(kfs), monocular), SCALE.tobytes(), (SCALE * SCALE).astype(F32).tobytes()]
    for kf in kfs:
        n = len(kf["order"])
        out += [struct.pack("<i", n), np.eye(3, dtype=F32).tobytes(), kf["t"].tobytes(), INTR.tobytes(), struct.pack("<fff", MEDIAN_DEPTH, float(MB), float(MBF))]
        out += [kf["desc"].tobytes(), np.zeros(n, F32).tobytes(), kf["node"].tobytes(), kf["mp"].tobytes(), kf["xy"].tobytes(), kf["octave"].tobytes()]
        out += [kf["ur"].tobytes(), kf["depth"].tobytes(), kf["raw"].tobytes()]
    return b"".join(out)


def run(tmp_path, data):
    pin, pout = tmp_path / "tri.bin", tmp_path / "tri.out"
    pin.write_bytes(data)
    p = subprocess.run([EXE, "triangulate_stereo", str(pin), str(pout)], stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    raw = pout.read_bytes()
    status, nnew = struct.unpack("<ii", raw[:8])
    rec = np.frombuffer(raw[8:], np.uint8).reshape(nnew, 24)
    return status, rec[:, :12].copy().view(np.int32), rec[:, 12:].copy().view(np.float32), p.stderr.decode()


def compute_f12(t1, t2):
    """LocalMapping.h's ComputeF12 for two keyframes without rotation, float operation by float operation."""
    z, o = F32(0), F32(1)
    R12 = np.eye(3, dtype=F32)
    t12 = [-(R12[r, 0] * t2[0] + R12[r, 1] * t2[1] + R12[r, 2] * t2[2]) + t1[r] for r in range(3)]
    tx = [[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]]
    fx, fy, cx, cy = INTR
    Ki = [[o / fx, z, -cx / fx], [z, o / fy, -cy / fy], [z, z, o]]
    a = [[Ki[0][r] * tx[0][c] + Ki[1][r] * tx[1][c] + Ki[2][r] * tx[2][c] for c in range(3)] for r in range(3)]
    b = [[a[r][0] * R12[0, c] + a[r][1] * R12[1, c] + a[r][2] * R12[2, c] for c in range(3)] for r in range(3)]
    return np.array([[b[r][0] * Ki[0][c] + b[r][1] * Ki[1][c] + b[r][2] * Ki[2][c] for c in range(3)] for r in range(3)], F32)


def groups_of(cur, nb):
    """ORBmatcher::CommonNodes: the nodes present on both sides in ascending order, their features in index order."""
    qp, qi, cp, ci = [0], [], [0], []
    for node in sorted(set(cur["node"].tolist()) & set(nb["node"].tolist())):
        qi += np.flatnonzero(cur["node"] == node).tolist(); ci += np.flatnonzero(nb["node"] == node).tolist()
        qp.append(len(qi)); cp.append(len(ci))
    return dict(q_ptr=np.array(qp, np.int32), q_idx=np.array(qi, np.int32), c_ptr=np.array(cp, np.int32), c_idx=np.array(ci, np.int32))


def model(kfs, raw_key="raw"):
    """The reference's loop on stereo keyframes: the gate against mb, the restated matcher, the device's per-pair body."""
    from weiner_slamit_v2_amd import api

    cur = kfs[0]
    has1 = cur["mp"].astype(bool).copy()
    calls, points, sources, skipped = [], [], [], []
    K = np.concatenate([INTR, F32(1) / INTR[:2]]).astype(F32)
    for k, nb in enumerate(kfs[1:]):
        Ow1, Ow2 = -cur["t"], -nb["t"]
        d = (Ow2 - Ow1).astype(np.float64)
        baseline = F32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if baseline < MB:                                               # :278-283, not monocular
            skipped.append(k)
            continue
        with np.errstate(all="ignore"):
            I = np.eye(3, dtype=F32)                                     # ORBmatcher.h's epipole: R2w Cw + t2w, float operation by float operation
            C2 = [I[r, 0] * Ow1[0] + I[r, 1] * Ow1[1] + I[r, 2] * Ow1[2] + nb["t"][r] for r in range(3)]
            invz = F32(1) / C2[2]
            epi = dict(F12=compute_f12(cur["t"], nb["t"]).reshape(9), ex=INTR[0] * C2[0] * invz + INTR[2], ey=INTR[1] * C2[1] * invz + INTR[3],
                       scale_factor=SCALE.tolist(), level_sigma2=(SCALE * SCALE).tolist())
            s1 = dict(desc=cur["desc"], valid=(~has1).astype(np.uint8), kp_xy=cur["xy"])
            s2 = dict(desc=nb["desc"], valid=np.ones(len(nb["order"]), np.uint8), kp_xy=nb["xy"], kp_octave=nb["octave"])
            m12, _, _ = bow_stereo_ref.search_for_triangulation(s1, s2, groups_of(cur, nb), epi, th=50, stereo=dict(ur1=cur["ur"], ur2=nb["ur"], only_stereo=False))
        idx1 = np.flatnonzero(m12 >= 0)
        idx2 = m12[idx1]
        T = [np.concatenate([np.eye(3, dtype=F32), kf["t"][:, None]], 1).reshape(12) for kf in (cur, nb)]
        out = api.triangulate(dict(n=len(idx1), Tcw1=T[0], Tcw2=T[1], intr1=K, intr2=K, kp1_xy=cur["xy"][idx1], kp2_xy=nb["xy"][idx2],
                                   octave1=cur["octave"][idx1], octave2=nb["octave"][idx2], n_levels=8, scale_factors1=SCALE, level_sigma2_1=SCALE * SCALE,
                                   scale_factors2=SCALE, level_sigma2_2=SCALE * SCALE, ratio_factor=F32(1.5) * SCALE[1],
                                   ur1=cur["ur"][idx1], ur2=nb["ur"][idx2], depth1=cur["depth"][idx1], depth2=nb["depth"][idx2],
                                   raw1_xy=cur[raw_key][idx1], raw2_xy=nb[raw_key][idx2], mb1=MB, mb2=MB, bf=MBF))
        for j in np.flatnonzero(out["status"] == 0):
            calls.append((k, int(idx1[j]), int(idx2[j])))
            points.append(out["x3d"][j])
            sources.append(int(out["source"][j]))
            has1[idx1[j]] = True
    return np.array(calls, np.int32).reshape(-1, 3), np.array(points, np.float32).reshape(-1, 3), np.array(sources), skipped


@pytest.mark.gpu
def test_create_new_map_points_on_stereo_keyframes(tmp_path):
    _build()
    kfs = scenario()
    status, calls, points, err = run(tmp_path, blob(kfs))
    assert status == 0, err
    want_calls, want_points, sources, skipped = model(kfs)
    assert np.array_equal(calls, want_calls)
    assert np.array_equal(points.view(np.uint32), want_points.view(np.uint32))           # the device's points, untouched
    nb = calls[:, 0]
    assert skipped == [2] and set(nb.tolist()) == {0, 1}                                  # 0.1 < mb: the near neighbour is skipped ...
    assert 0.1 / MEDIAN_DEPTH >= 0.01                                                     # ... by the stereo gate, not by the monocular one
    assert np.all(np.diff(nb) >= 0)
    first, second = set(calls[nb == 0, 1].tolist()), set(calls[nb == 1, 1].tolist())
    assert len(first) > 40 and len(second) > 10 and not (first & second)                  # a point made for neighbour 0 is gone for neighbour 1
    assert not (first | second) & set(range(20))
    # all three sources, and the unprojected points come from mvKeys: the model fed with mvKeysUn instead makes other points
    assert (sources == 1).sum() > 20 and (sources == 2).sum() > 5 and (sources == 3).sum() >= 1, np.bincount(sources)
    _, wrong_points, wrong_sources, _ = model(kfs, raw_key="xy")
    un = np.flatnonzero(sources >= 2)
    assert len(wrong_points) != len(points) or not np.array_equal(wrong_points[un].view(np.uint32), points[un].view(np.uint32))
    j = un[0]                                                                             # one of them by hand: KeyFrame::UnprojectStereo on mvKeys
    kf = kfs[0] if sources[j] == 2 else kfs[1 + calls[j, 0]]
    i = calls[j, 1] if sources[j] == 2 else calls[j, 2]
    z = kf["depth"][i]
    x, y = (kf["raw"][i, 0] - INTR[2]) * z * (F32(1) / INTR[0]), (kf["raw"][i, 1] - INTR[3]) * z * (F32(1) / INTR[1])
    Ow = -kf["t"]
    assert np.allclose(points[j], np.array([x, y, z]) + Ow, atol=1e-5)


@pytest.mark.gpu
def test_monocular_flag_on_a_stereo_type_takes_the_median_depth_gate(tmp_path):
    """monocular = true with the same keyframes: the gate is baseline / median depth again, so the near neighbour is searched."""
    _build()
    kfs = scenario()
    status, calls, _, err = run(tmp_path, blob(kfs, monocular=1))
    assert status == 0, err
    status0, calls0, _, err0 = run(tmp_path, blob(kfs, monocular=0))
    assert status0 == 0, err0
    assert np.array_equal(calls[calls[:, 0] < 2], calls0) and len(calls0) > 50         # the first two neighbours pass either gate


TU = r'''
#include <map>
#include "LocalMapping.h"
using namespace ORB_SLAM2;
struct Point { bool isBad() { return false; } };
struct KF {
    int N;
    std::map<unsigned, std::vector<unsigned> > mFeatVec;
    cv::Mat mDescriptors;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvScaleFactors, mvLevelSigma2;
    float fx, fy, cx, cy, invfx, invfy, mfScaleFactor;
#if STEREO_MEMBERS
    float mb, mbf;
    std::vector<float> mvDepth;
    std::vector<cv::KeyPoint> mvKeys;
#endif
    Point* GetMapPoint(size_t) { return 0; }
    cv::Mat GetCameraCenter() { return cv::Mat(3, 1, CV_32F); }
    cv::Mat GetRotation() { return cv::Mat(3, 3, CV_32F); }
    cv::Mat GetTranslation() { return cv::Mat(3, 1, CV_32F); }
    float ComputeSceneMedianDepth(int) { return 1.f; }
};
int drive(KF* cur, std::vector<KF*>& neigh) {
    return LocalMapping::CreateNewMapPoints(cur, neigh, false, [](const cv::Mat&, int, int, KF*) {});
}
'''


@pytest.mark.parametrize("stereo_members", (1, 0))
def test_the_stereo_path_is_chosen_at_compile_time(tmp_path, stereo_members):
    """A keyframe type with mb, mbf, mvDepth and mvKeys instantiates the stereo call; one without them still compiles, never names
    them, and keeps the monocular call and its three refusals."""
    src = tmp_path / "tu.cc"
    src.write_text(TU)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-DSTEREO_MEMBERS=%d" % stereo_members,
                           "-I", SHIM, "-c", str(src), "-o", str(tmp_path / "tu.o")])
    names = subprocess.check_output(["nm", "-C", str(tmp_path / "tu.o")]).decode()
    strings = subprocess.check_output(["strings", str(tmp_path / "tu.o")]).decode()
    assert "CreateNewMapPoints" in names
    if stereo_members:
        assert "slamit_triangulate_stereo" in names and "only the monocular path" not in strings
    else:
        assert "slamit_triangulate_stereo" not in names and "slamit_triangulate" in names
        for word in ("only the monocular path is on the device", "the current keyframe carries stereo", "a neighbour keyframe carries stereo"):
            assert word in strings, word
