"""The rotation-consistency check that follows a guided search (ORB_SLAM2/src/ORBmatcher.cc:1430-1471, ComputeThreeMaxima :1605-1646),
restated sequentially in Python from the reference's text: what slamit_rotation_check_batch_dev must give, and hand-made cases."""
import math

import numpy as np

HISTO_LENGTH = 30


def bin_of(angle1, angle2):
    """:1436-1443.  float rot = a1 - a2; if (rot < 0.0) rot += 360.0f; int bin = round(rot * factor) with factor = 1.0f / HISTO_LENGTH;
    if (bin == HISTO_LENGTH) bin = 0.  -> the bin, or None where the reference's assert would stop a debug build."""
    f32 = np.float32
    rot = f32(angle1) - f32(angle2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    x = float(f32(rot * (f32(1.0) / f32(HISTO_LENGTH))))
    if not math.isfinite(x):
        return None
    b = int(math.copysign(math.floor(abs(x) + 0.5), x))                 # roundf: halves away from zero (exact in double)
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else None


def three_maxima(sizes):
    """ComputeThreeMaxima (:1605-1646) over the bins' sizes: strict '>' in ascending bin order, then the 10 % rule in float."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rotation_check(match_kp, qangle, kp_angle, nmatches):
    """One frame.  match_kp (m): the keypoint each query took or -1; qangle (m); kp_angle (n); nmatches: the search's count.
    -> (kp_query (n) int32: the query that owns each keypoint, or -1; nmatches after the check; the three maxima)."""
    n = len(kp_angle)
    owner = np.full(n, -1, np.int32)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    for q, k in enumerate(match_kp):
        k = int(k)
        if k < 0 or k >= n:
            continue
        owner[k] = q                                                    # CurrentFrame.mvpMapPoints[bestIdx2] = pMP
        b = bin_of(qangle[q], kp_angle[k])
        if b is not None:
            rotHist[b].append(k)
    ind = three_maxima([len(h) for h in rotHist])
    for i in range(HISTO_LENGTH):
        if i not in ind:
            for k in rotHist[i]:
                owner[k] = -1                                           # mvpMapPoints[...] = NULL
                nmatches -= 1                                           # once per entry: a keypoint entered twice counts twice
    return owner, int(nmatches), ind


def _case(entries, n_kp, extra_queries=0):
    """entries: (keypoint, bin) per matched query, in query order; unmatched queries are appended."""
    m = len(entries) + extra_queries
    match = np.full(m, -1, np.int32)
    qangle = np.full(m, 11.0, np.float32)
    kp_angle = np.full(n_kp, 3.0, np.float32)
    for q, (k, b) in enumerate(entries):
        match[q] = k
        qangle[q] = np.float32(30.0 * b + 3.0)
    return dict(match_kp=match, qangle=qangle, kp_angle=kp_angle, nmatches=len(entries))


def hand_cases():
    """name -> (case, expected owner of selected keypoints {k: q}, expected nmatches, expected bins)."""
    cases = {}
    # twenty matches in bin 0, keypoint 5 first taken by query 0 in bin 7 (one entry: below 10 % of 20) and again by query 21 in bin 0:
    # the later query owns it, and the rejected bin's entry still clears it
    e = [(5, 7)] + [(10 + i, 0) for i in range(20)] + [(5, 0)]
    cases["shared_keypoint_one_entry_rejected"] = (_case(e, 40, 3), {5: -1, 10: 1, 29: 20}, 22 - 1, (0, -1, -1))
    # both entries of keypoint 5 in rejected bins: it is counted twice
    e = [(5, 7)] + [(10 + i, 0) for i in range(20)] + [(5, 9)]
    cases["shared_keypoint_counted_twice"] = (_case(e, 40), {5: -1, 10: 1}, 22 - 2, (0, -1, -1))
    # four bins of four entries: the first three by index are the maxima, the fourth falls
    e = [(4 * j + i, b) for j, b in enumerate((3, 5, 8, 12)) for i in range(4)]
    cases["first_index_tie"] = (_case(e, 16), {0: 0, 7: 7, 11: 11, 12: -1, 15: -1}, 16 - 4, (3, 5, 8))
    # 0.1f * 10 rounds to 1.0f: a second and third bin of ONE entry are not below it and stay (in double they would fall)
    e = [(i, 0) for i in range(10)] + [(10, 4), (11, 9)]
    cases["ten_percent_at_equality"] = (_case(e, 12), {10: 10, 11: 11}, 12, (0, 4, 9))
    # 0.1f * 20 = 2: one entry is below
    e = [(i, 0) for i in range(20)] + [(20, 4), (21, 9)]
    cases["ten_percent_below"] = (_case(e, 22), {20: -1, 21: -1, 3: 3}, 22 - 2, (0, -1, -1))
    # a negative rotation gains 360 (2 - 358 -> 4: bin 0); 356 degrees is bin 12, the highest a rotation below 360 reaches
    c = _case([(0, 0), (1, 0), (2, 0)], 3)
    c["qangle"][:] = (359.0, 2.0, 14.9)
    c["kp_angle"][:] = (3.0, 358.0, 0.0)
    cases["wrap_around"] = (c, {0: 0, 1: 1, 2: 2}, 3, (0, 12, -1))
    return cases
