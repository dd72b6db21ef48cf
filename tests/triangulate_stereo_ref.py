"""The checker of the stereo triangulation: LocalMapping::CreateNewMapPoints' per-pair body with stereo keypoints
(ORB_SLAM2/src/LocalMapping.cc:335-483, KeyFrame::UnprojectStereo KeyFrame.cc:623-639) restated in numpy from the reference's text,
over all pairs of a problem dict (synth.synth_triangulation_stereo) at once.  A problem without the stereo keys is all-monocular.

The three variants are those of tests/triangulate_ref.py: "32" (float / double as the reference, LAPACK SVD), "32j"
(the same with cv::SVD's one-sided Jacobi) and "64" (everything in double).  The stereo cosine is the reference's chain
cos(2 * atan2(mb / 2, depth)): in float32 through numpy's float32 arctan2 / cos in "32" / "32j", in double in "64" -- never the
double-angle identity of csrc/triangulate.h, which is what is under test.

Every gate is a list of comparisons (a, b).  A comparison is DECIDED when |a32 - b32| > 4 max over "32", "32j" of
(|a - a64| + |b - b64|); against a threshold (b the same in all variants) this is §14's rule, and it extends it to the two comparisons
between computed values, cosParallaxRays < cosParallaxStereo and cosParallaxStereo1 < cosParallaxStereo2.  A pair is decided when
the three variants agree on status and source and every comparison of every gate it reaches is decided.  Gate 1 is the choice of
:369-399 (codes 1 and 9 end there), gate 2 (w == 0) is reached by triangulated pairs only.
"""
import functools

import numpy as np

from tests import triangulate_ref as TR

CODES = dict(TR.CODES)
CODES[9] = "UnprojectStereo of depth <= 0"
STEREO_KEYS = ("ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy")

# (n, seed, baseline, outlier_frac, noise_px, options of synth.synth_triangulation_stereo)
FIXTURES = [
    (300, 0, 0.30, 0.15, 0.7, {"depth": (1.5, 45.0)}),                                          # far points: stereo pairs triangulated at cos >= 0.9998
    (300, 1, 0.05, 0.10, 0.7, {"depth": (1.5, 20.0)}),                                          # keyframes closer than the rig's baseline: UnprojectStereo
    (300, 2, 0.60, 0.15, 1.0, {"depth": (1.5, 30.0), "mb": 0.25}),
    (300, 3, 0.12, 0.10, 0.9, {"depth": (2.0, 40.0), "ur_outlier_frac": 0.15}),
    (300, 4, 0.40, 0.10, 0.5, {"behind_frac": 0.2, "octave_jump_frac": 0.25, "depth": (1.5, 25.0)}),          # codes 3 and 8
    (300, 5, 2.50, 0.10, 0.5, {"direction": (0.05, 0.02, 1.0), "depth": (1.2, 9.0)}),            # forward motion: code 4
    (257, 6, 0.004, 0.0, 0.3, {"stereo_frac": (0.15, 0.15, 0.15)}),                               # a tiny baseline: code 1 or UnprojectStereo
    (65, 7, 0.20, 0.3, 1.0, {"octave_jump_frac": 0.1, "depth": (1.5, 40.0)}),
]
MIXED = 3   # the fixture the size cuts are taken from: every wavefront holds all four kinds of pair and all three sources


@functools.lru_cache(maxsize=None)
def fixture(k):
    from weiner_slamit_v2_amd import synth

    n, seed, baseline, outl, noise, opts = FIXTURES[k]
    return synth.synth_triangulation_stereo(n, seed, baseline, outl, noise, **opts)


def with_mono_stereo(pr):
    """pr (monocular) with a stereo side in which nothing is stereo."""
    n = int(pr["n"])
    m1 = np.full(n, -1, np.float32)
    return dict(pr, ur1=m1, ur2=m1.copy(), depth1=m1.copy(), depth2=m1.copy(), raw1_xy=np.asarray(pr["kp1_xy"], np.float32).copy(),
                raw2_xy=np.asarray(pr["kp2_xy"], np.float32).copy(), mb1=np.float32(0.12), mb2=np.float32(0.12), bf=np.float32(60.0))


def head(pr, n):
    out = TR.head(pr, n)
    for key in STEREO_KEYS:
        if key in pr:
            out[key] = pr[key][:n].copy()
    return out


def evaluate(pr, mode):
    """-> dict(status (n) uint8, source (n) uint8, x3d (n, 3), comps {gate: [(a, b, applies), ...]}, A (n, 4, 4), cosp, cs1, cs2,
    err2_1, err2_2 (the two-term errors), err3_1, err3_2 (the three-term ones; NaN where the keypoint is not stereo))."""
    if "ur1" not in pr:
        pr = with_mono_stereo(pr)
    hi = mode == "64"
    lo = np.float64 if hi else np.float32
    f64 = np.float64
    n = int(pr["n"])
    T1, T2 = np.asarray(pr["Tcw1"], lo).reshape(3, 4), np.asarray(pr["Tcw2"], lo).reshape(3, 4)
    fx1, fy1, cx1, cy1, ifx1, ify1 = [lo(v) for v in pr["intr1"]]
    fx2, fy2, cx2, cy2, ifx2, ify2 = [lo(v) for v in pr["intr2"]]
    if hi:
        ifx1, ify1, ifx2, ify2 = 1.0 / fx1, 1.0 / fy1, 1.0 / fx2, 1.0 / fy2
    kp1, kp2 = np.asarray(pr["kp1_xy"], lo).reshape(n, 2), np.asarray(pr["kp2_xy"], lo).reshape(n, 2)
    raw1, raw2 = np.asarray(pr["raw1_xy"], lo).reshape(n, 2), np.asarray(pr["raw2_xy"], lo).reshape(n, 2)
    ur1, ur2 = np.asarray(pr["ur1"], lo).reshape(n), np.asarray(pr["ur2"], lo).reshape(n)
    dp1, dp2 = np.asarray(pr["depth1"], lo).reshape(n), np.asarray(pr["depth2"], lo).reshape(n)
    mb1, mb2, bf = lo(pr["mb1"]), lo(pr["mb2"]), lo(pr["bf"])
    o1, o2 = np.asarray(pr["octave1"]), np.asarray(pr["octave2"])
    sig1, sig2 = np.asarray(pr["level_sigma2_1"], lo)[o1], np.asarray(pr["level_sigma2_2"], lo)[o2]
    sf1, sf2 = np.asarray(pr["scale_factors1"], lo)[o1], np.asarray(pr["scale_factors2"], lo)[o2]
    rf = lo(pr["ratio_factor"])
    one, two = lo(1), lo(2)
    bS1, bS2 = ur1 >= 0, ur2 >= 0                                                                 # :337, :345

    def dot_d(a, b):
        a, b = a.astype(f64), b.astype(f64)
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    with np.errstate(all="ignore"):
        xn1 = np.stack([(kp1[:, 0] - cx1) * ifx1, (kp1[:, 1] - cy1) * ify1, np.full(n, one)], 1)
        xn2 = np.stack([(kp2[:, 0] - cx2) * ifx2, (kp2[:, 1] - cy2) * ify2, np.full(n, one)], 1)
        R1, R2 = T1[:, :3], T2[:, :3]
        ray1 = np.stack([(R1[0, i] * xn1[:, 0] + R1[1, i] * xn1[:, 1]) + R1[2, i] * xn1[:, 2] for i in range(3)], 1)
        ray2 = np.stack([(R2[0, i] * xn2[:, 0] + R2[1, i] * xn2[:, 1]) + R2[2, i] * xn2[:, 2] for i in range(3)], 1)
        cosp = (dot_d(ray1, ray2) / (np.sqrt(dot_d(ray1, ray1)) * np.sqrt(dot_d(ray2, ray2)))).astype(lo)
        # :355-364
        cs1, cs2 = cosp + one, cosp + one
        c1v = np.cos(two * np.arctan2(np.full(n, mb1 / two, lo), dp1)).astype(lo)
        c2v = np.cos(two * np.arctan2(np.full(n, mb2 / two, lo), dp2)).astype(lo)
        cs1 = np.where(bS1, c1v, cs1).astype(lo)
        cs2 = np.where(~bS1 & bS2, c2v, cs2).astype(lo)
        cs = np.where(cs2 < cs1, cs2, cs1)
        tri = (cosp < cs) & (cosp > 0) & (bS1 | bS2 | (cosp.astype(f64) < 0.9998))                # :369
        un1 = ~tri & bS1 & (cs1 < cs2)                                                            # :389
        un2 = ~tri & ~un1 & bS2 & (cs2 < cs1)                                                     # :393
        # :372-387
        A = np.stack([xn1[:, 0:1] * T1[2] - T1[0], xn1[:, 1:2] * T1[2] - T1[1], xn2[:, 0:1] * T2[2] - T2[0], xn2[:, 1:2] * T2[2] - T2[1]], 1)
        A = A.astype(lo)
        safe = np.where(np.isfinite(A).all((1, 2))[:, None, None], A, np.eye(4, dtype=lo))
        if mode == "32j":
            v = TR._jacobi_vt_last(safe)
        else:
            v = np.linalg.svd(safe)[2][:, 3, :].astype(lo)
        w = v[:, 3]
        inv = (1.0 / w.astype(f64)).astype(lo)
        Xt = v[:, :3] * inv[:, None]
        O1 = -np.array([(R1[0, i] * T1[0, 3] + R1[1, i] * T1[1, 3]) + R1[2, i] * T1[2, 3] for i in range(3)], lo)
        O2 = -np.array([(R2[0, i] * T2[0, 3] + R2[1, i] * T2[1, 3]) + R2[2, i] * T2[2, 3] for i in range(3)], lo)

        def unproject(raw, z, cx, cy, ifx, ify, R, O):                                            # KeyFrame.cc:623-639
            x, y = (raw[:, 0] - cx) * z * ifx, (raw[:, 1] - cy) * z * ify
            return np.stack([((R[0, i] * x + R[1, i] * y) + R[2, i] * z) + O[i] for i in range(3)], 1).astype(lo)

        Xu1, Xu2 = unproject(raw1, dp1, cx1, cy1, ifx1, ify1, R1, O1), unproject(raw2, dp2, cx2, cy2, ifx2, ify2, R2, O2)
        X = np.where(tri[:, None], Xt, np.where(un1[:, None], Xu1, Xu2)).astype(lo)

        def cam(T, X):
            return [(dot_d(T[r, :3][None, :], X) + f64(T[r, 3])).astype(lo) for r in range(3)]

        x1, y1, z1 = cam(T1, X)
        x2, y2, z2 = cam(T2, X)
        invz1, invz2 = (1.0 / z1.astype(f64)).astype(lo), (1.0 / z2.astype(f64)).astype(lo)
        u1, v1 = fx1 * x1 * invz1 + cx1, fy1 * y1 * invz1 + cy1
        u2, v2 = fx2 * x2 * invz2 + cx2, fy2 * y2 * invz2 + cy2
        ex1, ey1, er1 = u1 - kp1[:, 0], v1 - kp1[:, 1], (u1 - bf * invz1) - ur1                   # :430: the current keyframe's mbf
        ex2, ey2, er2 = u2 - kp2[:, 0], v2 - kp2[:, 1], (u2 - bf * invz2) - ur2                   # :458: the current keyframe's mbf again
        e2_1, e2_2 = (ex1 * ex1 + ey1 * ey1).astype(lo), (ex2 * ex2 + ey2 * ey2).astype(lo)
        e3_1, e3_2 = (ex1 * ex1 + ey1 * ey1 + er1 * er1).astype(lo), (ex2 * ex2 + ey2 * ey2 + er2 * er2).astype(lo)
        err1, err2 = np.where(bS1, e3_1, e2_1).astype(f64), np.where(bS2, e3_2, e2_2).astype(f64)
        thr1 = np.where(bS1, 7.8, 5.991) * sig1.astype(f64)
        thr2 = np.where(bS2, 7.8, 5.991) * sig2.astype(f64)
        d1v, d2v = X - O1, X - O2
        dist1, dist2 = np.sqrt(dot_d(d1v, d1v)).astype(lo), np.sqrt(dot_d(d2v, d2v)).astype(lo)
        ratioDist, ratioOctave = dist2 / dist1, sf1 / sf2
        zero, yes = np.zeros(n), np.ones(n, bool)
        comps = {
            1: [(cosp, cs, yes), (cosp, zero, yes), (cosp, np.full(n, 0.9998), ~(bS1 | bS2)), (cs1, cs2, ~tri & (bS1 | bS2))],
            2: [(np.abs(w), zero, tri)],
            3: [(z1, zero, yes)], 4: [(z2, zero, yes)],
            5: [(err1, thr1, yes)], 6: [(err2, thr2, yes)],
            7: [(dist1, zero, yes), (dist2, zero, yes)],
            8: [(ratioDist * rf, ratioOctave, yes), (ratioDist, ratioOctave * rf, yes)],
        }
        fails = {
            2: tri & (w == 0), 3: z1 <= 0, 4: z2 <= 0, 5: err1 > thr1, 6: err2 > thr2,
            7: (dist1 == 0) | (dist2 == 0),
            8: (ratioDist * rf < ratioOctave) | (ratioDist > ratioOctave * rf),
        }
    status = np.zeros(n, np.uint8)
    for code in range(8, 1, -1):
        status[fails[code]] = code
    status[~tri & ~un1 & ~un2] = 1
    status[(un1 & (dp1 <= 0)) | (un2 & (dp2 <= 0))] = 9
    source = np.where(tri, 1, np.where(un1, 2, np.where(un2, 3, 0))).astype(np.uint8)
    nopoint = (status == 1) | (status == 2) | (status == 9)
    source[nopoint] = 0
    X = np.where(nopoint[:, None], 0, X)
    comps = {k: [(np.asarray(a, f64), np.asarray(b, f64), np.asarray(m, bool)) for a, b, m in g] for k, g in comps.items()}
    nan = np.full(n, np.nan)
    return dict(status=status, source=source, x3d=X.astype(lo), comps=comps, A=A, cosp=cosp.astype(f64), cs1=cs1.astype(f64), cs2=cs2.astype(f64),
                err2_1=e2_1.astype(f64), err2_2=e2_2.astype(f64), err3_1=np.where(bS1, e3_1.astype(f64), nan), err3_2=np.where(bS2, e3_2.astype(f64), nan),
                sigma2_1=sig1.astype(f64), sigma2_2=sig2.astype(f64), stereo1=bS1, stereo2=bS2)


def reached(status):
    """(n, 9) bool: column g is set when a pair with this status got as far as gate g (code 9 ends at gate 1)."""
    last = np.where(status == 0, 8, np.where(status == 9, 1, status)).astype(int)
    return np.arange(9)[None, :] <= last[:, None]


def analyse(pr):
    """The three variants on a problem -> dict(r32, r32j, r64, decided (n) bool, undecided_frac, all_accept (n) bool: accepted and
    triangulated in every variant, e32, e32j (n))."""
    r32, r32j, r64 = evaluate(pr, "32"), evaluate(pr, "32j"), evaluate(pr, "64")
    n = int(pr["n"])
    reach = reached(r32["status"])
    decided = (r32["status"] == r32j["status"]) & (r32["status"] == r64["status"]) & (r32["source"] == r32j["source"]) & (r32["source"] == r64["source"])
    with np.errstate(all="ignore"):
        for g in range(1, 9):
            for (a32, b32, m), (a32j, b32j, _), (a64, b64, _) in zip(r32["comps"][g], r32j["comps"][g], r64["comps"][g]):
                spread = np.maximum(np.abs(a32 - a64) + np.abs(b32 - b64), np.abs(a32j - a64) + np.abs(b32j - b64))
                ok = np.abs(a32 - b32) > 4 * spread
                decided &= ok | ~reach[:, g] | ~m
    acc = np.ones(n, bool)
    for r in (r32, r32j, r64):
        acc &= (r["status"] == 0) & (r["source"] == 1)
    return dict(r32=r32, r32j=r32j, r64=r64, decided=decided, undecided_frac=float((~decided).sum()) / max(n, 1), all_accept=acc,
                e32=TR.point_error(r64, r32["x3d"]), e32j=TR.point_error(r64, r32j["x3d"]))


@functools.lru_cache(maxsize=None)
def admissibility(k):
    return analyse(fixture(k))


@functools.lru_cache(maxsize=None)
def yardstick():
    """Y by §14's definition over these fixtures: the largest e(x32) / e(x32j) over the triangulated pairs every variant accepts."""
    y = 0.0
    for k in range(len(FIXTURES)):
        a = admissibility(k)
        if a["all_accept"].any():
            y = max(y, float(a["e32"][a["all_accept"]].max()), float(a["e32j"][a["all_accept"]].max()))
    return y


def hand_made(X, t2=(-0.5, 0.0, 0.0), rot2_deg=0.0, kp2=None, o1=0, o2=0, **stereo):
    """One pair: keyframe 1 at the origin, keyframe 2 turned by rot2_deg about y and translated by t2, the exact projections of X
    (keypoint 2 at kp2 if given), and the stereo side from **stereo over the defaults "nothing is stereo, mb 0.12, bf 60"."""
    f32 = np.float32
    K = np.array([500.0, 500.0, 320.0, 240.0, 1 / 500.0, 1 / 500.0], f32)
    a = np.deg2rad(rot2_deg)
    R2 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T1 = np.eye(4)[:3].astype(f32)
    T2 = np.concatenate([R2, np.asarray(t2, np.float64)[:, None]], 1).astype(f32)
    X = np.asarray(X, np.float64)
    X2 = R2 @ X + np.asarray(t2, np.float64)
    sf = f32(1.2) ** np.arange(8, dtype=f32)
    kp1 = np.array([[500 * X[0] / X[2] + 320, 500 * X[1] / X[2] + 240]], f32)
    kp2 = np.array([[500 * X2[0] / X2[2] + 320, 500 * X2[1] / X2[2] + 240]] if kp2 is None else [kp2], f32)
    pr = dict(n=1, Tcw1=T1.reshape(12), Tcw2=T2.reshape(12), intr1=K, intr2=K, kp1_xy=kp1, kp2_xy=kp2, octave1=np.array([o1], np.int32),
              octave2=np.array([o2], np.int32), n_levels=8, scale_factors1=sf, level_sigma2_1=sf * sf, scale_factors2=sf, level_sigma2_2=sf * sf,
              ratio_factor=f32(1.5) * f32(1.2), ur1=[-1.0], ur2=[-1.0], depth1=[-1.0], depth2=[-1.0], raw1_xy=kp1.copy(), raw2_xy=kp2.copy(),
              mb1=f32(0.12), mb2=f32(0.12), bf=f32(60.0), z2=float(X2[2]))
    for key, v in stereo.items():
        assert key in pr
        pr[key] = v
    for key in STEREO_KEYS:
        pr[key] = np.asarray(pr[key], f32).reshape((1, 2) if key[:3] == "raw" else (1,))
    return pr


def hand_cases():
    """name -> (problem, expected status or None, expected source): the single pairs of the stereo branches, one branch each."""
    near = (-0.001, 0.0, 0.0)                                   # keyframes a millimetre apart: the rays are parallel to float precision
    P = (-2.44, 0.1, 4.0)                                       # projects to u = 15 in keyframe 1: with bf 60 and depth 4 its ur is exactly 0
    Q = (0.2, 0.1, 4.0)
    u2 = 500 * (0.2 - 0.5) / 4.0 + 320                          # keypoint 2 of Q under the default t2
    c = {}
    c["ur 0.0f is stereo: UnprojectStereo(1)"] = (hand_made(P, near, ur1=[0.0], depth1=[4.0]), 0, 2)
    c["the same pair with ur -1: no stereo and very low parallax"] = (hand_made(P, near), 1, 0)
    c["NaN ur is monocular"] = (hand_made(P, near, ur1=[np.nan], depth1=[4.0]), 1, 0)
    c["depth 0 on the chosen keypoint"] = (hand_made(P, near, ur1=[0.0], depth1=[0.0]), 9, 0)
    c["depth < 0 on the chosen keypoint"] = (hand_made(P, near, ur1=[0.0], depth1=[-1.0]), 9, 0)
    c["depth <= 0 on keypoint 2"] = (hand_made(Q, near, ur2=[5.0], depth2=[0.0]), 9, 0)
    c["UnprojectStereo(2)"] = (hand_made(Q, near, ur2=[500 * (0.2 - 0.001) / 4 + 320 - 15.0], depth2=[4.0]), 0, 3)
    # rays more than 90 degrees apart (cosParallaxRays < 0, so :369 fails): cosParallaxStereo1 < cosParallaxRays + 1 decides
    Z = (0.0, 0.0, 4.0)                                         # on keyframe 1's axis; keypoint 2 at the principal point: cos = cos(rot2)
    c["rays 100 degrees apart, stereo 1: skipped"] = (hand_made(Z, (0.0, 0.0, 0.0), rot2_deg=100.0, kp2=(320.0, 240.0), ur1=[305.0], depth1=[4.0]), 1, 0)
    c["rays 90.01 degrees apart, stereo 1: UnprojectStereo(1)"] = (hand_made(Z, (0.0, 0.0, 0.0), rot2_deg=90.01, kp2=(320.0, 240.0), ur1=[305.0], depth1=[4.0]), None, 2)
    # both stereo: only keyframe 1's cosine is computed (:359-362), so a nearer depth 2 cannot make it UnprojectStereo(2)
    c["both stereo falls to UnprojectStereo(1)"] = (hand_made(Q, near, ur1=[345.0 - 15.0], depth1=[4.0], ur2=[330.0 - 30.0], depth2=[2.0]), None, 2)
    # a stereo pair triangulated above 0.9998: depth 60, baseline 0.5, cos = 0.99997
    far = (1.0, 0.5, 60.0)
    c["stereo triangulates above 0.9998"] = (hand_made(far, ur1=[500 * 1.0 / 60 + 320 - 1.0], depth1=[60.0]), 0, 1)
    c["monocular does not"] = (hand_made(far), 1, 0)
    # the current keyframe's bf on side 2 (:458): mb2 = 0.3 would make 150; ur2 is right for bf = 60
    c["bf of the current keyframe on side 2: accepted"] = (hand_made(Q, ur2=[u2 - 60.0 / 4.0], depth2=[4.0], mb2=np.float32(0.3)), 0, 1)
    c["ur2 right for the neighbour's own bf: rejected"] = (hand_made(Q, ur2=[u2 - 150.0 / 4.0], depth2=[4.0], mb2=np.float32(0.3)), 6, 1)
    # the third term alone (:435): ur1 3 px off at octave 0 is 9 > 7.8, the other two terms are zero
    c["third term alone rejects in keyframe 1"] = (hand_made(Q, ur1=[345.0 - 15.0 + 3.0], depth1=[4.0]), 5, 1)
    c["2.7 px is inside 7.8"] = (hand_made(Q, ur1=[345.0 - 15.0 + 2.7], depth1=[4.0]), 0, 1)
    # 7.8 instead of 5.991 (:435): keypoint 1 moved 5.2 px along v puts about 2.6 px = 6.8 px^2 into each image
    moved = hand_made(Q, ur1=[345.0 - 15.0], depth1=[4.0], ur2=[u2 - 15.0], depth2=[4.0])
    moved["kp1_xy"] = moved["kp1_xy"] + np.array([[0.0, 5.2]], np.float32)
    c["two-term error between 5.991 and 7.8: stereo accepts"] = (moved, 0, 1)
    mono = dict(moved, ur1=np.array([-1.0], np.float32), ur2=np.array([-1.0], np.float32))
    c["the same pair monocular: rejected"] = (mono, 5, 1)
    # the raw keypoint feeds UnprojectStereo: mvKeys (6, 4) px from mvKeysUn moves the point by (0.048, 0.032); octave 7 lets it pass
    c["UnprojectStereo reads mvKeys"] = (hand_made(P, near, ur1=[0.0], depth1=[4.0], raw1_xy=[[21.0, 256.5]], o1=7, o2=7), 0, 2)
    return c
