"""Tracking::UpdateLocalMap restated literally (ORB_SLAM2 src/Tracking.cc:1467-1626) with the first loop of SearchLocalPoints
(:1412-1428) and its skip test (:1436), over mock KeyFrame / MapPoint objects built from slot-numbered tables.

Written from the reference, statement by statement: Python dicts and sets for std::map and std::set, explicit
mnTrackReferenceForFrame / mnLastFrameSeen marks.  std::map<KeyFrame*, int> and std::set<KeyFrame*> iterate in address order; the
mock objects' "address" is their slot, and a keyframe's children are a list already in the order the set would give.  Nothing of
the device's algorithm (keys, atomics, scans) appears here."""
import numpy as np


class MapPoint:
    def __init__(self, slot, bad):
        self.slot, self.bad = slot, bool(bad)
        self.observations = []                 # KeyFrames (GetObservations)
        self.mnTrackReferenceForFrame = -1
        self.mnLastFrameSeen = -1

    def isBad(self):
        return self.bad


class KeyFrame:
    def __init__(self, slot, bad):
        self.slot, self.bad = slot, bool(bad)
        self.map_point_matches = []            # MapPoint or None by keypoint index (GetMapPointMatches)
        self.ordered_connected = []            # mvpOrderedConnectedKeyFrames
        self.childs = []                       # GetChilds(), in set order
        self.parent = None
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.bad

    def GetBestCovisibilityKeyFrames(self, n):
        return self.ordered_connected[:n]


class Frame:
    def __init__(self, mnId, map_points):
        self.mnId = mnId
        self.mvpMapPoints = list(map_points)
        self.N = len(self.mvpMapPoints)
        self.mpReferenceKF = None


class Tracking:
    def __init__(self, frame, local_kfs, ref_kf):
        self.mCurrentFrame = frame
        self.mvpLocalKeyFrames = list(local_kfs)
        self.mpReferenceKF = ref_kf
        self.mvpLocalMapPoints = []
        self.keyframeCounter = {}

    def UpdateLocalKeyFrames(self):                                   # :1512
        F = self.mCurrentFrame
        keyframeCounter = {}
        for i in range(F.N):                                          # :1518
            if F.mvpMapPoints[i] is not None:
                pMP = F.mvpMapPoints[i]
                if not pMP.isBad():
                    for pKF in pMP.observations:
                        keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
                else:
                    F.mvpMapPoints[i] = None                          # :1535
        self.keyframeCounter = keyframeCounter
        if not keyframeCounter:                                       # :1540, before clear()
            return
        max_ = 0
        pKFmax = None
        self.mvpLocalKeyFrames = []                                   # :1546
        for pKF in sorted(keyframeCounter, key=lambda kf: kf.slot):   # the map's order: by address
            if pKF.isBad():
                continue
            if keyframeCounter[pKF] > max_:
                max_ = keyframeCounter[pKF]
                pKFmax = pKF
            self.mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = F.mnId
        it_end = len(self.mvpLocalKeyFrames)                          # :1569, itEndKF is taken before any push
        for it in range(it_end):
            if len(self.mvpLocalKeyFrames) > 80:                      # :1572
                break
            pKF = self.mvpLocalKeyFrames[it]
            for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != F.mnId:
                        self.mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = F.mnId
                        break
            for pChildKF in pKF.childs:
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != F.mnId:
                        self.mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = F.mnId
                        break
            pParent = pKF.parent
            if pParent is not None:
                if pParent.mnTrackReferenceForFrame != F.mnId:        # no isBad() here
                    self.mvpLocalKeyFrames.append(pParent)
                    pParent.mnTrackReferenceForFrame = F.mnId
                    break                                             # :1615: the OUTER for
        if pKFmax is not None:
            self.mpReferenceKF = pKFmax
            F.mpReferenceKF = pKFmax

    def UpdateLocalPoints(self):                                      # :1477
        F = self.mCurrentFrame
        self.mvpLocalMapPoints = []
        for pKF in self.mvpLocalKeyFrames:
            for pMP in pKF.map_point_matches:
                if pMP is None:
                    continue
                if pMP.mnTrackReferenceForFrame == F.mnId:
                    continue
                if not pMP.isBad():
                    self.mvpLocalMapPoints.append(pMP)
                    pMP.mnTrackReferenceForFrame = F.mnId

    def SearchLocalPointsSkips(self):                                 # :1412-1428, then the tests of :1436-1440
        F = self.mCurrentFrame
        for i in range(F.N):
            pMP = F.mvpMapPoints[i]
            if pMP is not None:
                if pMP.isBad():
                    F.mvpMapPoints[i] = None
                else:
                    pMP.mnLastFrameSeen = F.mnId
        return [1 if (pMP.mnLastFrameSeen == F.mnId or pMP.isBad()) else 0 for pMP in self.mvpLocalMapPoints]


def build_objects(tables):
    """Mock objects of a map's tables (the layout of slamit_map_index)."""
    n_kf, n_mp = int(tables["n_kf"]), int(tables["n_mp"])
    mps = [MapPoint(p, tables["mp_bad"][p]) for p in range(n_mp)]
    kfs = [KeyFrame(k, tables["kf_bad"][k]) for k in range(n_kf)]
    for p in range(n_mp):
        mps[p].observations = [kfs[k] for k in tables["obs_kf"][tables["obs_ptr"][p]:tables["obs_ptr"][p + 1]]]
    best = np.asarray(tables["kf_best"]).reshape(n_kf, 10)
    for k in range(n_kf):
        row = tables["kf_mp"][tables["kf_mp_ptr"][k]:tables["kf_mp_ptr"][k + 1]]
        kfs[k].map_point_matches = [mps[p] if p >= 0 else None for p in row]
        kfs[k].ordered_connected = [kfs[b] for b in best[k] if b >= 0]
        kfs[k].childs = [kfs[c] for c in tables["kf_child"][tables["kf_child_ptr"][k]:tables["kf_child_ptr"][k + 1]]]
        kfs[k].parent = kfs[tables["kf_parent"][k]] if tables["kf_parent"][k] >= 0 else None
    return kfs, mps


def update_local_map(tables, frame):
    """One frame (dict: frame_mp, frame_seen, local_kf, ref_kf as they stand) through UpdateLocalKeyFrames, UpdateLocalPoints and the
    skip flags -> dict(votes, frame_mp, local_kf, n_local_kf, ref_kf, local_mp, n_local_mp, skip), lists in full (no capacity)."""
    kfs, mps = build_objects(tables)
    mnId = 7
    F = Frame(mnId, [mps[p] if p >= 0 else None for p in frame["frame_mp"]])
    for p in frame.get("frame_seen", ()):
        if p >= 0:
            mps[p].mnLastFrameSeen = mnId                             # the outliers of :1015 / :1146 carry the frame's id already
    T = Tracking(F, [kfs[k] for k in frame["local_kf"]], kfs[frame["ref_kf"]] if frame["ref_kf"] >= 0 else None)
    T.UpdateLocalKeyFrames()
    T.UpdateLocalPoints()
    skip = T.SearchLocalPointsSkips()
    votes = np.zeros(len(kfs), np.int32)
    for kf, c in T.keyframeCounter.items():
        votes[kf.slot] = c
    return {"votes": votes,
            "frame_mp": np.array([mp.slot if mp is not None else -1 for mp in F.mvpMapPoints], np.int32),
            "local_kf": np.array([kf.slot for kf in T.mvpLocalKeyFrames], np.int32), "n_local_kf": len(T.mvpLocalKeyFrames),
            "ref_kf": T.mpReferenceKF.slot if T.mpReferenceKF is not None else -1,
            "local_mp": np.array([mp.slot for mp in T.mvpLocalMapPoints], np.int32), "n_local_mp": len(T.mvpLocalMapPoints),
            "skip": np.array(skip, np.uint8)}
