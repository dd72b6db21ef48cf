"""A literal restatement of MapPoint::Replace (ORB_SLAM2/src/MapPoint.cc:183-221) walked SEQUENTIALLY over an op list, with the pair
AddObservation + AddMapPoint that ORBmatcher::Fuse interleaves with it (ORBmatcher.cc:956-973), which is imported from
tests/map_edit_ref.py as it stands.  Observations are a dict per point (insertion-ordered: a row is the old order with moved-out
entries gone and received ones at the end); the loop over a std::map<KeyFrame*, size_t> is `sorted`, the keyframes being numbered by
address.  Written apart from csrc/map_replace.h: no bucket, no round, no list index -- a later write to kf_mp simply overwrites.

What the C-ABI adds to the reference is stated in `apply`: the all-or-nothing ceilings, the table's capacity, touched, moved / erased,
the status bits, the slots outside their tables.  `events` names what happened, for the fixtures' own test."""
import numpy as np

from tests import map_edit_ref
from tests.map_edit_ref import AddMapPoint, AddObservation, World

REPLACE, ADD_OBS = 1, 2
OP_OVERFLOW, OBS_OVERFLOW, TABLE_OVERFLOW, BAD_SLOT = 1, 2, 4, 8
MAX_OPS, MAX_PER_POINT, MAX_OBS = 16384, 64, 512


class ObsOverflow(Exception):
    pass


class MapPoint(map_edit_ref.MapPoint):
    def __init__(self, slot, obs, nobs, bad, found, visible, replaced):
        map_edit_ref.MapPoint.__init__(self, slot, obs, nobs, bad, -1)
        self.mnFound, self.mnVisible, self.mpReplaced = found, visible, replaced


def wrap(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def set_match(world, kf, idx, value):
    """mvpMapPoints[idx] = value of keyframe kf; a pair outside the table (a table held wrongly) is skipped and noted."""
    if 0 <= kf < len(world.mvpMapPoints) and 0 <= idx < len(world.mvpMapPoints[kf]):
        world.mvpMapPoints[kf][idx] = value
    else:
        world.obs_bad = True


def room(mp):
    if len(mp.mObservations) >= MAX_OBS:
        raise ObsOverflow()


def Replace(S, D, world):                                               # MapPoint.cc:183-221
    if D.slot == S.slot:
        world.events.append("replace_self")
        return 0, 0
    if S.mpReplaced >= 0:
        world.events.append("replace_of_replaced")
    if D.mbBad:
        world.events.append("replace_onto_bad")
    if not D.mObservations:
        world.events.append("replace_onto_empty")
    obs = dict(S.mObservations)
    S.mObservations.clear()
    S.mbBad = True
    nvisible, nfound = S.mnVisible, S.mnFound
    S.mpReplaced = D.slot
    moved = erased = 0
    for kf in sorted(obs):                                              # a std::map<KeyFrame*, size_t>
        idx, octave, weight = obs[kf]
        if kf not in D.mObservations:                                   # !pMP->IsInKeyFrame(pKF)
            set_match(world, kf, idx, D.slot)                           # pKF->ReplaceMapPointMatch(idx, pMP)
            room(D)
            AddObservation(D, kf, idx, octave, weight, world)
            moved += 1
        else:
            set_match(world, kf, idx, -1)                               # pKF->EraseMapPointMatch(idx)
            erased += 1
    D.mnFound, D.mnVisible = wrap(D.mnFound + nfound), wrap(D.mnVisible + nvisible)   # IncreaseFound / IncreaseVisible
    world.events.append("replace_%s" % ("nothing" if not obs else "all_move" if not erased else "all_die" if not moved else "some_die"))
    return moved, erased


def one_op(world, mps, op):
    kind, a, b, idx, octave, weight = op
    if kind == REPLACE:
        return Replace(mps[a], mps[b], world)
    mp = mps[a]
    before = len(mp.mObservations)
    if b not in mp.mObservations:
        room(mp)
    AddObservation(mp, b, idx, octave, weight, world)
    AddMapPoint(world, b, mp, idx)
    return len(mp.mObservations) - before, 0


def op_ok(t, op):
    kind, a, b, idx, _, weight = op
    if kind == REPLACE:
        return 0 <= a < t["n_mp"] and 0 <= b < t["n_mp"]
    if kind != ADD_OBS or not (0 <= a < t["n_mp"] and 0 <= b < t["n_kf"]):
        return False
    return 0 <= idx < int(t["kf_mp_ptr"][b + 1] - t["kf_mp_ptr"][b]) and weight in (1, 2)


def objects(t, x):
    ptr, kf_ptr = np.asarray(t["obs_ptr"]), np.asarray(t["kf_mp_ptr"])
    kf, idx, octv, wgt = (np.asarray(a).tolist() for a in (t["obs_kf"], x["obs_idx"], x["obs_octave"], x["obs_weight"]))
    nobs, bad, fnd, vis, rep = (np.asarray(a).tolist() for a in (x["mp_nobs"], t["mp_bad"], x["mp_found"], x["mp_visible"], x["mp_replaced"]))
    mps = [MapPoint(p, {kf[o]: (idx[o], octv[o], wgt[o]) for o in range(ptr[p], ptr[p + 1])}, nobs[p], bool(bad[p]), fnd[p], vis[p], rep[p]) for p in range(t["n_mp"])]
    flat = np.asarray(t["kf_mp"]).tolist()
    world = World([flat[kf_ptr[k]:kf_ptr[k + 1]] for k in range(t["n_kf"])])
    world.obs_bad = False
    return mps, world


def default_cap(t, ops):
    return int(np.asarray(t["obs_ptr"])[-1]) + sum(1 for op in ops if int(op[0]) == ADD_OBS)


def apply(t, x, ops, obs_cap_out=None):
    """ops: tuples (kind, a, b, idx, octave, weight).  -> what slamit_map_replace_apply leaves: status, and unless an overflow bit is
    set the new table (obs_ptr, obs_kf, obs_idx, obs_octave, obs_weight), mp_bad, mp_nobs, mp_found, mp_visible, mp_replaced, kf_mp,
    moved, erased, touched, n_touched, n_obs_out; with TABLE_OVERFLOW n_obs_out alone.  Always `events`."""
    ops = [tuple(int(v) for v in op) for op in ops]
    good = [op_ok(t, op) for op in ops]
    op_bad = BAD_SLOT if not all(good) else 0
    named = {}
    for op, ok in zip(ops, good):
        if ok and not (op[0] == REPLACE and op[1] == op[2]):
            for p in (op[1], op[2]) if op[0] == REPLACE else (op[1],):
                named[p] = named.get(p, 0) + 1
    out = {"events": []}
    if any(v > MAX_PER_POINT for v in named.values()):
        out["status"] = OP_OVERFLOW | op_bad
        return out
    rows_in = np.diff(np.asarray(t["obs_ptr"]))
    mps, world = objects(t, x)
    out["events"] = world.events
    moved, erased = [0] * len(ops), [0] * len(ops)
    try:
        if any(rows_in[p] > MAX_OBS for p in named):
            raise ObsOverflow()
        for i, (op, ok) in enumerate(zip(ops, good)):
            if ok:
                moved[i], erased[i] = one_op(world, mps, op)
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
               kf_mp=i32(v for row in world.mvpMapPoints for v in row), moved=i32(moved), erased=i32(erased), touched=i32(m.slot for m in mps if m.touched))
    out["n_touched"] = len(out["touched"])
    return out


def check_replaced(mp_replaced, frame_mp):
    """Tracking::CheckReplacedInLastFrame (Tracking.cc:959-974): three lines of numpy."""
    lst, rep = np.array(frame_mp, np.int32), np.asarray(mp_replaced, np.int32)
    hit = (lst >= 0) & (rep[np.clip(lst, 0, len(rep) - 1)] >= 0)
    lst[hit] = rep[lst[hit]]
    return lst
