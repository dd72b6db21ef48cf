"""A literal restatement of the tail of ORBmatcher::Fuse (ORB_SLAM2/src/ORBmatcher.cc:853, :955-975) walked SEQUENTIALLY over an op list.
Replace and the add pair are imported from tests/map_replace_ref.py / tests/map_edit_ref.py as they stand; what this file adds is the
branch: which of them the op becomes, read from pKF->GetMapPoint(bestIdx) and both points' Observations() at that moment.  Written
apart from csrc/map_fuse.h: observations are a dict per point, mvpMapPoints a list per keyframe, nothing is marked involved before the
walk but for the one thing the C-ABI defines by it (an involved row above the ceiling on input refuses the call).

What the C-ABI adds to the reference is stated in `apply`, as in tests/map_replace_ref.py; `events` names what happened."""
import numpy as np

from tests.map_edit_ref import AddMapPoint, AddObservation
from tests.map_replace_ref import ADD_OBS, BAD_SLOT, MAX_OBS, OBS_OVERFLOW, REPLACE, TABLE_OVERFLOW, ObsOverflow, Replace, objects, one_op, op_ok as plain_ok, room

FUSE = 3
PLAIN, NOMATCH, SKIP_BAD, SKIP_IN_KF, ADDED, OCCUPANT_BAD, P_REPLACED, Q_REPLACED = range(8)
OUT_NAMES = ("plain", "nomatch", "skip_bad", "skip_in_kf", "added", "occupant_bad", "p_replaced", "q_replaced")
MAX_OPS = 16384


class Skipped(Exception):
    """The device form's answer to an occupant that is no slot of the table."""


def Fuse(world, mps, pMP, pKF, bestIdx, octave, weight):
    """One point of the loop of :846-976 whose search has ended with bestIdx (-1: bestDist > TH_LOW).  -> outcome, moved, erased."""
    if bestIdx < 0:
        return NOMATCH, 0, 0
    if pMP.mbBad:                                                       # :853 pMP->isBad()
        return SKIP_BAD, 0, 0
    if pKF in pMP.mObservations:                                        # :853 pMP->IsInKeyFrame(pKF)
        return SKIP_IN_KF, 0, 0
    q = world.mvpMapPoints[pKF][bestIdx]                                # :958 pKF->GetMapPoint(bestIdx)
    if q != -1:                                                         # :959
        if not 0 <= q < len(mps):
            raise Skipped()
        pMPinKF = mps[q]
        if pMPinKF.mbBad:                                               # :961
            return OCCUPANT_BAD, 0, 0
        if pMPinKF.nObs == pMP.nObs:
            world.events.append("fuse_tie")
        if pMPinKF.slot == pMP.slot:
            world.events.append("fuse_same_point")
        if pMPinKF.nObs > pMP.nObs:                                     # :963
            return (P_REPLACED,) + Replace(pMP, pMPinKF, world)         # :964
        return (Q_REPLACED,) + Replace(pMPinKF, pMP, world)             # :966
    room(pMP)
    AddObservation(pMP, pKF, bestIdx, octave, weight, world)            # :971
    AddMapPoint(world, pKF, pMP, bestIdx)                               # :972
    return ADDED, 1, 0


def op_ok(t, op):
    kind, a, b, idx, _, weight = op
    if kind != FUSE:
        return plain_ok(t, op)
    if idx < 0:
        return True
    if not (0 <= a < t["n_mp"] and 0 <= b < t["n_kf"]):
        return False
    return idx < int(t["kf_mp_ptr"][b + 1] - t["kf_mp_ptr"][b]) and weight in (1, 2)


def default_cap(t, ops):
    return int(np.asarray(t["obs_ptr"])[-1]) + sum(1 for op in ops if int(op[0]) in (ADD_OBS, FUSE))


def apply(t, x, ops, obs_cap_out=None):
    """ops: tuples (kind, a, b, idx, octave, weight).  -> what slamit_map_fuse_apply leaves: status, and unless an overflow bit is set
    the new table (obs_ptr, obs_kf, obs_idx, obs_octave, obs_weight), mp_bad, mp_nobs, mp_found, mp_visible, mp_replaced, kf_mp, outcome,
    moved, erased, touched, n_touched, n_fused, n_obs_out; with TABLE_OVERFLOW n_obs_out alone.  Always `events`."""
    ops = [tuple(int(v) for v in op) for op in ops]
    good = [op_ok(t, op) for op in ops]
    op_bad = BAD_SLOT if not all(good) else 0
    kf_ptr, kf_mp = np.asarray(t["kf_mp_ptr"]), np.asarray(t["kf_mp"])
    named = set()                                                       # the rows whose input length the call looks at
    for op, ok in zip(ops, good):
        if not ok or (op[0] == REPLACE and op[1] == op[2]) or (op[0] == FUSE and op[3] < 0):
            continue
        named.add(op[1])
        if op[0] == REPLACE:
            named.add(op[2])
        if op[0] == FUSE:
            q = int(kf_mp[kf_ptr[op[2]] + op[3]])
            if 0 <= q < t["n_mp"]:
                named.add(q)
    rows_in = np.diff(np.asarray(t["obs_ptr"]))
    mps, world = objects(t, x)
    out = {"events": world.events}
    outcome, moved, erased = [PLAIN] * len(ops), [0] * len(ops), [0] * len(ops)
    try:
        if any(rows_in[p] > MAX_OBS for p in named):
            raise ObsOverflow()
        for i, (op, ok) in enumerate(zip(ops, good)):
            if not ok:
                continue
            if op[0] != FUSE:
                moved[i], erased[i] = one_op(world, mps, op)
                continue
            try:
                outcome[i], moved[i], erased[i] = Fuse(world, mps, mps[op[1]] if op[3] >= 0 else None, op[2], op[3], op[4], op[5])
                world.events.append("fuse_" + OUT_NAMES[outcome[i]])
            except Skipped:
                op_bad = BAD_SLOT
    except ObsOverflow:
        out["status"] = OBS_OVERFLOW | op_bad
        return out
    need = sum(len(m.mObservations) for m in mps)
    cap = default_cap(t, ops) if obs_cap_out is None else obs_cap_out
    out["n_obs_out"] = need
    if need > cap:
        out["status"] = TABLE_OVERFLOW | op_bad
        return out
    flat = [(k,) + v for m in mps for k, v in m.mObservations.items()]
    col = lambda i, dt: np.array([f[i] for f in flat], dt).reshape(-1)
    i32 = lambda vals: np.array(list(vals), np.int32).reshape(-1)
    out.update(status=op_bad | (BAD_SLOT if world.obs_bad else 0),
               obs_ptr=np.concatenate([[0], np.cumsum([len(m.mObservations) for m in mps])]).astype(np.int32),
               obs_kf=col(0, np.int32), obs_idx=col(1, np.int32), obs_octave=col(2, np.uint8), obs_weight=col(3, np.uint8),
               mp_bad=np.array([m.mbBad for m in mps], np.uint8).reshape(-1), mp_nobs=i32(m.nObs for m in mps), mp_found=i32(m.mnFound for m in mps),
               mp_visible=i32(m.mnVisible for m in mps), mp_replaced=i32(m.mpReplaced for m in mps),
               kf_mp=i32(v for row in world.mvpMapPoints for v in row), outcome=i32(outcome), moved=i32(moved), erased=i32(erased),
               touched=i32(m.slot for m in mps if m.touched), n_fused=sum(1 for o in outcome if o >= ADDED))
    out["n_touched"] = len(out["touched"])
    return out
