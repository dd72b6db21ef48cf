"""A literal restatement of how the reference's map grows, walked SEQUENTIALLY over an op list: KeyFrame::KeyFrame(Frame&, ...) with
Map::AddKeyFrame, the map point constructor with AddObservation / AddMapPoint / Map::AddMapPoint (ORB_SLAM2/src/LocalMapping.cc:486-500,
src/Tracking.cc:1376-1383, :718-723, :875-891) and the loop of LocalMapping::ProcessNewKeyFrame (:156-175).  Keyframes and points are
objects; a point's observations are a dict, IsInKeyFrame is a lookup in it, and AddObservation is really performed op by op.  Written
apart from csrc/map_grow.h: no stamp, no first-occurrence key, no scan.

What the C-ABI adds to the reference is stated in `apply`: the gate and its needs, the slots, the inert tail, the op statuses, the emitted
edit list."""
import numpy as np

NEW_KF, NEW_POINT, ASSOCIATE, RECENT = 1, 2, 3, 1
OP_REJECTED, OP_BAD = -1, -2
KF_OVERFLOW, MP_OVERFLOW, KFMP_OVERFLOW, EDIT_OVERFLOW, RECENT_OVERFLOW, KP_OVERFLOW, OPS_OVERFLOW, BAD_SLOT = 1, 2, 4, 8, 16, 32, 64, 128
MAX_KP = 30000
ADD_OBS = 1


class KeyFrame:
    def __init__(self, slot, mps, octave, desc, depth, th_depth, center, new):
        self.slot, self.mvpMapPoints, self.octave, self.desc, self.depth, self.th_depth, self.center, self.new = slot, mps, octave, desc, depth, th_depth, center, new


class MapPoint:
    def __init__(self, slot, pos, ref, first_kf, obs, bad, new):
        self.slot, self.pos, self.mpRefKF, self.mnFirstKFid, self.mObservations, self.mbBad, self.new = slot, pos, ref, first_kf, obs, bad, new
        self.nObs = 0


def center_of(Tcw):
    """-Rcw^T tcw in float32, each component ((R0j t0 + R1j t1) + R2j t2) negated."""
    T = np.asarray(Tcw, np.float32).reshape(12)
    f = np.float32
    return [-f(f(f(T[j] * T[3]) + f(T[4 + j] * T[7])) + f(T[8 + j] * T[11])) for j in range(3)]


def objects(t):
    ptr, optr = np.asarray(t["kf_mp_ptr"]), np.asarray(t["obs_ptr"])
    kfs = [KeyFrame(k, np.asarray(t["kf_mp"])[ptr[k]:ptr[k + 1]].tolist(), np.asarray(t["kf_octave"])[ptr[k]:ptr[k + 1]].tolist(), None, None, None, None, False)
           for k in range(t["n_kf"])]
    mps = [MapPoint(p, None, int(t["mp_ref_kf"][p]), None, {int(k): int(i) for k, i in zip(np.asarray(t["obs_kf"])[optr[p]:optr[p + 1]], np.asarray(t["obs_idx"])[optr[p]:optr[p + 1]])},
                    bool(t["mp_bad"][p]), False) for p in range(t["n_mp"])]
    for mp in mps:
        mp.nObs = int(t["mp_nobs"][mp.slot])
    return kfs, mps


def needs(fx, caps):
    t, frames, ops = fx["t"], fx["frames"], fx["ops"]
    frame = lambda e: frames[e["src"]] if 0 <= e.get("src", 0) < len(frames) else None
    n_kp = lambda f: len(f["frame_mp"])
    new_kf = [frame(e) for e in ops if e["kind"] == NEW_KF and frame(e) is not None]
    assoc = [frame(e) for e in ops if e["kind"] == ASSOCIATE and frame(e) is not None]
    P = sum(1 for e in ops if e["kind"] == NEW_POINT)
    over = any(n_kp(f) > MAX_KP for f in new_kf + assoc)
    new_kf, assoc = [f for f in new_kf if n_kp(f) <= MAX_KP], [f for f in assoc if n_kp(f) <= MAX_KP]
    sa = sum(n_kp(f) for f in assoc)
    need = [t["n_kf"] + len(new_kf), t["n_mp"] + P, int(t["kf_mp_ptr"][t["n_kf"]]) + sum(n_kp(f) for f in new_kf), 2 * P + sa,
            len(fx.get("recent", [])) + sum(1 for e in ops if e["kind"] == NEW_POINT and e.get("flags", 0) & RECENT) + sa]
    names = ("kf_cap", "mp_cap", "kfmp_cap", "edit_cap", "recent_cap")
    status = sum(bit for bit, n, c in zip((KF_OVERFLOW, MP_OVERFLOW, KFMP_OVERFLOW, EDIT_OVERFLOW, RECENT_OVERFLOW), need, names) if n > caps[c])
    return need, status | (KP_OVERFLOW if over else 0)


def apply(fx, caps=None):
    """fx: a fixture of tests/map_grow_fixtures.py.  -> the gate's need and status; unless refused: op_status, edits (tuples of
    map_edit_ref.apply), recent (the whole list), n_new, P, and the objects kfs / mps of the end state."""
    t, frames, ops = fx["t"], fx["frames"], fx["ops"]
    out = {}
    if caps is not None:
        out["need"], out["status"] = needs(fx, caps)
        if out["status"]:
            return out
    kfs, mps = objects(t)
    edits, recent, op_status, bad_slot = [], list(fx.get("recent", [])), [], False
    cand_status, cand_x3d = list(fx.get("cand_status", [])), fx.get("cand_x3d", [])
    if caps is not None and caps.get("cand_cap", 0) > len(cand_status):  # the batch's capacity: past a map's own candidates lies the caller's fill, never 0
        cand_status += [0xee] * (caps["cand_cap"] - len(cand_status))

    def AddObservation(mp, kf, idx, weight):                            # MapPoint.cc:104-115, as the emitted edit and as the deed
        edits.append((ADD_OBS, 0, mp.slot, kf.slot, idx, kf.octave[idx], weight))
        if kf.slot in mp.mObservations:
            return
        mp.mObservations[kf.slot] = idx
        mp.nObs += weight

    def obs_ok(k, i, w):
        return 0 <= k < len(kfs) and 0 <= i < len(kfs[k].mvpMapPoints) and w in (1, 2)

    for e in ops:
        kind = e["kind"]
        f = frames[e["src"]] if kind in (NEW_KF, ASSOCIATE) and 0 <= e["src"] < len(frames) else None
        if kind == NEW_KF and f is not None and e["kf"] == len(kfs) and len(f["frame_mp"]) <= MAX_KP:
            row = []
            for p in f["frame_mp"]:
                if not -1 <= p < len(mps):
                    bad_slot, p = True, -1
                row.append(int(p))
            kfs.append(KeyFrame(len(kfs), row, [int(o) for o in f["octave"]], np.array(f["desc"], np.uint8).reshape(-1, 32),
                                None if f.get("depth") is None else np.array(f["depth"], np.float32), np.float32(f["th_depth"]), center_of(f["Tcw"]), True))
            op_status.append(len(kfs) - 1)
        elif kind == NEW_POINT and 0 <= e["kf"] < len(kfs) and -1 <= e["cand"] < len(cand_status) and obs_ok(e["kf_a"], e["idx_a"], e["weight_a"]) and \
                (e["kf_b"] == -1 or obs_ok(e["kf_b"], e["idx_b"], e["weight_b"])):
            if e["cand"] >= 0 and cand_status[e["cand"]] != 0:
                op_status.append(OP_REJECTED)
                continue
            pos = cand_x3d[e["cand"]] if e["cand"] >= 0 else e["pos"]
            mp = MapPoint(len(mps), [np.float32(v) for v in pos], e["kf"], e["kf_id"], {}, False, True)
            mps.append(mp)                                              # Map::AddMapPoint
            for k, i, w in ((e["kf_a"], e["idx_a"], e["weight_a"]),) + (((e["kf_b"], e["idx_b"], e["weight_b"]),) if e["kf_b"] != -1 else ()):
                AddObservation(mp, kfs[k], i, w)
                kfs[k].mvpMapPoints[i] = mp.slot                        # KeyFrame::AddMapPoint
            if e["flags"] & RECENT:
                recent.append(mp.slot)
            op_status.append(mp.slot)
        elif kind == ASSOCIATE and f is not None and 0 <= e["kf"] < len(kfs) and len(kfs[e["kf"]].mvpMapPoints) == len(f["frame_mp"]) <= MAX_KP:
            kf = kfs[e["kf"]]
            for i, p in enumerate(list(kf.mvpMapPoints)):               # ProcessNewKeyFrame :156-175
                if p == -1:
                    continue
                if not 0 <= p < len(mps):
                    bad_slot = True
                    continue
                mp = mps[p]
                if mp.mbBad:
                    continue
                if kf.slot not in mp.mObservations:                     # !IsInKeyFrame
                    AddObservation(mp, kf, i, 2 if f.get("uright") is not None and f["uright"][i] >= 0 else 1)
                else:
                    recent.append(p)
            op_status.append(kf.slot)
        else:
            op_status.append(OP_BAD)
            bad_slot = True
    P = sum(1 for e in ops if e["kind"] == NEW_POINT)
    out.update(op_status=op_status, edits=edits, recent=recent, n_new=len(mps) - t["n_mp"], P=P, kfs=kfs, mps=mps)
    out["status"] = BAD_SLOT if bad_slot else 0
    return out
