"""The checker of the stereo SearchForTriangulation: the matching loop of ORBmatcher::SearchForTriangulation
(ORB_SLAM2/src/ORBmatcher.cc:695-793, CheckDistEpipolarLine :135-158) restated in numpy / Python from the reference's text, one
query and one candidate at a time in the reference's order.  Float expressions are float32 operation by operation, as the
reference's floats without contraction; the comparison of :157 is in double.  The rotation-histogram filter that follows is the
shim's and is not part of it.  side1 / side2 / groups / epi are those of synth.synth_bow(mode=1) / synth.synth_bow_stereo;
stereo = dict(ur1, ur2, only_stereo) or None (nothing is stereo)."""
import numpy as np


def descriptor_distance(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def search_for_triangulation(side1, side2, groups, epi, th=50, stereo=None):
    """-> (match12 (n1) int32, dist12 (n1) int32: the best distance the query saw, 256 if none, nmatches)."""
    f32 = np.float32
    d1, d2 = np.asarray(side1["desc"], np.uint8).reshape(-1, 32), np.asarray(side2["desc"], np.uint8).reshape(-1, 32)
    n1, n2 = len(d1), len(d2)
    v1 = np.ones(n1, bool) if side1.get("valid") is None else np.asarray(side1["valid"]) != 0
    v2 = np.ones(n2, bool) if side2.get("valid") is None else np.asarray(side2["valid"]) != 0
    k1, k2 = np.asarray(side1["kp_xy"], f32).reshape(-1, 2), np.asarray(side2["kp_xy"], f32).reshape(-1, 2)
    oct2 = np.asarray(side2["kp_octave"])
    F = np.asarray(epi["F12"], f32).reshape(3, 3)
    ex, ey = f32(epi["ex"]), f32(epi["ey"])
    sf = np.asarray(list(epi["scale_factor"]), f32)
    sg = np.asarray(list(epi["level_sigma2"]), f32)
    if stereo is None:
        s1, s2, only = np.zeros(n1, bool), np.zeros(n2, bool), False
    else:
        with np.errstate(invalid="ignore"):
            s1, s2 = np.asarray(stereo["ur1"], f32) >= 0, np.asarray(stereo["ur2"], f32) >= 0      # :709, :732 (NaN >= 0 is false)
        only = bool(stereo.get("only_stereo", False))
    match12, dist12 = np.full(n1, -1, np.int32), np.full(n1, 256, np.int32)
    nmatches = 0
    qp, qi, cp, ci = (np.asarray(groups[k]) for k in ("q_ptr", "q_idx", "c_ptr", "c_idx"))
    for g in range(len(qp) - 1):
        for idx1 in qi[qp[g]:qp[g + 1]]:
            if not v1[idx1]:                                       # :706 (the caller's mask: the keypoint has a MapPoint)
                continue
            if only and not s1[idx1]:                              # :711-713
                continue
            x1, y1 = k1[idx1]
            a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]              # :144-146
            b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
            c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
            bestDist, bestIdx2 = th, -1
            for idx2 in ci[cp[g]:cp[g + 1]]:
                if not v2[idx2]:                                   # :729
                    continue
                if only and not s2[idx2]:                          # :734-736
                    continue
                dist = descriptor_distance(d1[idx1], d2[idx2])
                if dist > th or dist > bestDist:                   # :742
                    continue
                x2, y2 = k2[idx2]
                if not s1[idx1] and not s2[idx2]:                  # :747-753
                    distex, distey = ex - x2, ey - y2
                    if distex * distex + distey * distey < f32(100) * sf[oct2[idx2] & 15]:
                        continue
                num = a * x2 + b * y2 + c                          # :148-157
                den = a * a + b * b
                if den == 0:
                    continue
                with np.errstate(all="ignore"):
                    dsqr = num * num / den
                if float(dsqr) < 3.84 * float(sg[oct2[idx2] & 15]):
                    bestIdx2, bestDist = int(idx2), dist
            if bestIdx2 >= 0:
                match12[idx1], dist12[idx1] = bestIdx2, bestDist
                nmatches += 1
    return match12, dist12, nmatches
