"""A literal restatement of the reference's three point-side mutators and the two keyframe-side ones they are paired with, walked
SEQUENTIALLY over an edit list (ORB_SLAM2/src/MapPoint.cc:104-174, src/KeyFrame.cc:215-243).  Observations are a dict per point
(insertion-ordered, so a row is the old order with erased entries gone and added ones at the end); mObservations.begin() is the
smallest key, the keyframes being numbered by address.  Written apart from csrc/map_edit.h: no bucket, no dead entry, no list index
carried anywhere -- a later write to kf_mp simply overwrites an earlier one.

What the C-ABI adds to the reference is stated in `apply`: the ceilings (a point with too many edits or too long a row takes part in
nothing), the table's capacity, touched, the status bits.  `events` names what happened, for the fixtures' own test."""
import numpy as np

ADD_OBS, ERASE_OBS, SET_BAD, MATCH = 1, 2, 3, 1
REF_END, EDIT_OVERFLOW, OBS_OVERFLOW, BAD_SLOT, TABLE_OVERFLOW = 1, 2, 4, 8, 16
MAX_PER_POINT, MAX_OBS = 64, 512


class MapPoint:
    def __init__(self, slot, obs, nobs, bad, ref):
        self.slot, self.mObservations, self.nObs, self.mbBad, self.mpRefKF = slot, obs, nobs, bad, ref
        self.status, self.touched = 0, False


class World:
    """mvpMapPoints of every keyframe, by slot; the events of the walk."""

    def __init__(self, kf_rows):
        self.mvpMapPoints, self.events = kf_rows, []


def AddObservation(mp, kf, idx, octave, weight, world):                 # MapPoint.cc:104-115
    if kf in mp.mObservations:
        world.events.append("add_present")
        return
    if mp.mbBad:
        world.events.append("add_on_bad")
    mp.mObservations[kf] = (idx, octave, weight)
    mp.nObs += weight
    mp.touched = True


def EraseObservation(mp, kf, world):                                    # MapPoint.cc:117-143
    bBad = False
    if kf in mp.mObservations:
        before = mp.nObs
        mp.nObs -= mp.mObservations[kf][2]
        del mp.mObservations[kf]
        mp.touched = True
        if mp.mpRefKF == kf:
            if mp.mObservations:
                mp.mpRefKF = min(mp.mObservations)                      # begin() of a std::map
                world.events.append("erase_ref_remaining")
            else:
                mp.mpRefKF = -1                                         # the reference reads end(): the stated departure
                mp.status |= REF_END
                world.events.append("erase_ref_end")
        if mp.nObs <= 2:
            bBad = True
            world.events.append("cascade_%d_%d" % (before, mp.nObs))
        else:
            world.events.append("erase_leaves_%d" % mp.nObs)
    else:
        world.events.append("erase_absent")
    if bBad:
        SetBadFlag(mp, world)


def SetBadFlag(mp, world):                                              # MapPoint.cc:157-174
    if mp.mbBad:
        world.events.append("set_bad_on_bad")
    mp.mbBad = True
    obs = dict(mp.mObservations)
    if obs:
        mp.touched = True
    mp.mObservations.clear()
    for kf, (idx, _, _) in obs.items():
        world.mvpMapPoints[kf][idx] = -1                                # KeyFrame::EraseMapPointMatch(const size_t&)


def AddMapPoint(world, kf, mp, idx):                                    # KeyFrame.cc:215-219
    world.mvpMapPoints[kf][idx] = mp.slot


def EraseMapPointMatch(world, kf, mp):                                  # KeyFrame.cc:227-232
    if kf in mp.mObservations:
        world.mvpMapPoints[kf][mp.mObservations[kf][0]] = -1


def one_edit(world, mp, e):
    kind, flags, _, kf, idx, octave, weight = e
    if kind == ADD_OBS:
        AddObservation(mp, kf, idx, octave, weight, world)
        if flags & MATCH:
            AddMapPoint(world, kf, mp, idx)
    elif kind == ERASE_OBS:
        if flags & MATCH:
            EraseMapPointMatch(world, kf, mp)
        EraseObservation(mp, kf, world)
    else:
        SetBadFlag(mp, world)


def objects(t, x):
    ptr, kf_ptr = np.asarray(t["obs_ptr"]), np.asarray(t["kf_mp_ptr"])
    kf, idx, octv, wgt = (np.asarray(a).tolist() for a in (t["obs_kf"], x["obs_idx"], x["obs_octave"], x["obs_weight"]))
    nobs, bad, ref = (np.asarray(a).tolist() for a in (x["mp_nobs"], t["mp_bad"], x["mp_ref_kf"]))
    mps = [MapPoint(p, {kf[o]: (idx[o], octv[o], wgt[o]) for o in range(ptr[p], ptr[p + 1])}, nobs[p], bool(bad[p]), ref[p]) for p in range(t["n_mp"])]
    flat = np.asarray(t["kf_mp"]).tolist()
    return mps, World([flat[kf_ptr[k]:kf_ptr[k + 1]] for k in range(t["n_kf"])])


def apply(t, x, edits, obs_cap_out=None):
    """edits: tuples (kind, flags, mp, kf, idx, octave, weight).  -> what slamit_map_edit_apply leaves: the new table (obs_ptr, obs_kf,
    obs_idx, obs_octave, obs_weight), mp_bad, mp_nobs, mp_ref_kf, kf_mp, status_mp, touched, n_touched, n_obs_out, status, events."""
    edits = [tuple(int(v) for v in e) for e in edits]
    n_mp = t["n_mp"]
    rows_in = np.diff(np.asarray(t["obs_ptr"]))
    # the ceilings: such a point takes part in nothing.  Whether adds push a row past the ceiling is seen on the point alone, which is
    # fact 1 of the design: its row depends on its own edits only.
    own = {}
    for e in edits:
        own.setdefault(e[2], []).append(e)
    refused = {}
    for p, lst in own.items():
        if len(lst) > MAX_PER_POINT:
            refused[p] = EDIT_OVERFLOW
        elif rows_in[p] > MAX_OBS:
            refused[p] = OBS_OVERFLOW
        else:
            mps, world = objects_of_point(t, x, p)
            for e in lst:
                if e[0] == ADD_OBS and e[3] not in mps.mObservations and len(mps.mObservations) >= MAX_OBS:
                    refused[p] = OBS_OVERFLOW
                    break
                one_edit(world, mps, e)
    mps, world = objects(t, x)
    for e in edits:
        if e[2] not in refused:
            one_edit(world, mps[e[2]], e)
    need = sum(len(m.mObservations) for m in mps)
    cap = int(np.asarray(t["obs_ptr"])[-1]) + len(edits) if obs_cap_out is None else obs_cap_out
    out = {"n_obs_out": need, "events": world.events}
    if need > cap:
        out["status"] = TABLE_OVERFLOW
        return out
    flat = [(k,) + v for m in mps for k, v in m.mObservations.items()]
    col = lambda i, dt: np.array([f[i] for f in flat], dt).reshape(-1)
    out.update(status=0, obs_ptr=np.concatenate([[0], np.cumsum([len(m.mObservations) for m in mps])]).astype(np.int32),
               obs_kf=col(0, np.int32), obs_idx=col(1, np.int32), obs_octave=col(2, np.uint8), obs_weight=col(3, np.uint8),
               mp_bad=np.array([m.mbBad for m in mps], np.uint8).reshape(-1), mp_nobs=np.array([m.nObs for m in mps], np.int32).reshape(-1),
               mp_ref_kf=np.array([m.mpRefKF for m in mps], np.int32).reshape(-1),
               kf_mp=np.array([v for row in world.mvpMapPoints for v in row], np.int32).reshape(-1),
               status_mp=np.array([refused.get(m.slot, m.status) for m in mps], np.int32).reshape(-1),
               touched=np.array([m.slot for m in mps if m.touched], np.int32).reshape(-1))
    out["n_touched"] = len(out["touched"])
    assert len(out["obs_ptr"]) == n_mp + 1
    return out


def objects_of_point(t, x, p):
    """Point p alone over a scratch world (its own writes to mvpMapPoints go nowhere that is read)."""
    ptr = np.asarray(t["obs_ptr"])
    sl = slice(int(ptr[p]), int(ptr[p + 1]))
    obs = {int(k): (int(i), int(o), int(w)) for k, i, o, w in zip(np.asarray(t["obs_kf"])[sl], np.asarray(x["obs_idx"])[sl], np.asarray(x["obs_octave"])[sl],
                                                                 np.asarray(x["obs_weight"])[sl])}
    mp = MapPoint(p, obs, int(np.asarray(x["mp_nobs"])[p]), bool(np.asarray(t["mp_bad"])[p]), int(np.asarray(x["mp_ref_kf"])[p]))

    class Sink(dict):
        def __missing__(self, k):
            return Sink()

        def __setitem__(self, k, v):
            pass
    w = World(Sink())
    return mp, w
