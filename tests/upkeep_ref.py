"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (ORB_SLAM2 src/MapPoint.cc:248-313, :336-377), with
GetFoundRatio (:241-246), and LocalMapping::MapPointCulling (src/LocalMapping.cc:184-219), restated line for line over mock objects with
dicts and lists.  No keys, no ranks, no scans: this text is what the device is compared against, bit for bit.

A std::map<KeyFrame*, size_t> iterates in ADDRESS order; a mock keyframe's address is its `addr` (the slot of the tables), so by_addr()
is the reference's iteration.  The float steps are np.float32 / np.float64 scalars in the order csrc/unproject.h states for these lines:
the difference in float, cv::norm as the square root of the double sum of double squares in order, Mat / s as a product with
(float)(1.0 / s), the sum one observer after the other."""
import numpy as np

f32, f64 = np.float32, np.float64
INT_MAX = 2 ** 31 - 1


def by_addr(d):
    return sorted(d.items(), key=lambda kv: kv[0].addr)


def cv_norm(v):                            # cv::norm of a 3 x 1 CV_32F Mat: double
    with np.errstate(all="ignore"):
        return np.sqrt((f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1])) + f64(v[2]) * f64(v[2]))


def mat_div(v, s):                         # Mat / double: convertTo with scale 1. / s
    with np.errstate(all="ignore"):
        inv = f32(f64(1.0) / f64(s))
        return [f32(x * inv) for x in v]


def mat_sub(a, b):
    with np.errstate(all="ignore"):
        return [f32(f32(x) - f32(y)) for x, y in zip(a, b)]


def mat_add(a, b):
    with np.errstate(all="ignore"):
        return [f32(f32(x) + f32(y)) for x, y in zip(a, b)]


def DescriptorDistance(a, b):              # ORBmatcher.cc:1651-1668: the popcount of the xor
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class KeyFrame:
    def __init__(self, addr, bad, center, octaves, descriptors, scale_factors):
        self.addr, self.bad = addr, bool(bad)
        self.center = [f32(c) for c in center]        # GetCameraCenter()
        self.octave = list(octaves)                   # mvKeysUn[i].octave
        self.mDescriptors = descriptors               # (n_keypoints, 32) uint8
        self.mvScaleFactors = [f32(s) for s in scale_factors]
        self.mnScaleLevels = len(self.mvScaleFactors)

    def isBad(self):
        return self.bad

    def GetCameraCenter(self):
        return self.center


class MapPoint:
    def __init__(self, slot, bad, pos, ref, normal, max_dist, min_dist, desc, nobs, found, visible, first_kf):
        self.slot, self.mbBad = slot, bool(bad)
        self.mWorldPos = [f32(x) for x in pos]
        self.mpRefKF = ref
        self.mObservations = {}                       # KeyFrame -> keypoint index
        self.mNormalVector = [f32(x) for x in normal]
        self.mfMaxDistance, self.mfMinDistance = f32(max_dist), f32(min_dist)
        self.mDescriptor = np.array(desc, np.uint8)
        self.nObs, self.mnFound, self.mnVisible, self.mnFirstKFid = int(nobs), int(found), int(visible), int(first_kf)
        self.default_inserted = False                 # observations[pRefKF] made an entry

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def GetFoundRatio(self):                          # :241-246: static_cast<float>(mnFound) / mnVisible
        with np.errstate(all="ignore"):
            return f32(self.mnFound) / f32(self.mnVisible)

    def ComputeDistinctiveDescriptors(self):          # :248-313
        vDescriptors = []
        if self.mbBad:
            return
        observations = dict(self.mObservations)
        if not observations:
            return
        for pKF, idx in by_addr(observations):
            if not pKF.isBad():
                vDescriptors.append(pKF.mDescriptors[idx])
        if not vDescriptors:
            return
        N = len(vDescriptors)
        Distances = [[0] * N for _ in range(N)]
        for i in range(N):
            Distances[i][i] = 0
            for j in range(i + 1, N):
                distij = DescriptorDistance(vDescriptors[i], vDescriptors[j])
                Distances[i][j] = distij
                Distances[j][i] = distij
        BestMedian = INT_MAX
        BestIdx = 0
        for i in range(N):
            vDists = sorted(Distances[i])
            median = vDists[int(0.5 * (N - 1))]
            if median < BestMedian:
                BestMedian = median
                BestIdx = i
        self.mDescriptor = vDescriptors[BestIdx].copy()

    def UpdateNormalAndDepth(self):                   # :336-377
        if self.mbBad:
            return
        observations = dict(self.mObservations)
        pRefKF = self.mpRefKF
        Pos = list(self.mWorldPos)
        if not observations:
            return
        normal = [f32(0), f32(0), f32(0)]
        n = 0
        for pKF, _ in by_addr(observations):
            Owi = pKF.GetCameraCenter()
            normali = mat_sub(self.mWorldPos, Owi)
            normal = mat_add(normal, mat_div(normali, cv_norm(normali)))
            n += 1
        PC = mat_sub(Pos, pRefKF.GetCameraCenter())
        dist = f32(cv_norm(PC))
        if pRefKF not in observations:                # operator[] default-inserts 0 into the local copy
            observations[pRefKF] = 0
            self.default_inserted = True
        level = pRefKF.octave[observations[pRefKF]]
        levelScaleFactor = pRefKF.mvScaleFactors[level]
        nLevels = pRefKF.mnScaleLevels
        with np.errstate(all="ignore"):
            self.mfMaxDistance = f32(dist * levelScaleFactor)
            self.mfMinDistance = f32(self.mfMaxDistance / pRefKF.mvScaleFactors[nLevels - 1])
        self.mNormalVector = mat_div(normal, n)


def MapPointCulling(recent, nCurrentKFid, mbMonocular):   # LocalMapping.cc:184-219 -> (verdict per entry, SetBadFlag calls in order)
    """The list `recent` is edited in place as the reference edits mlpRecentAddedMapPoints."""
    nThObs = 2 if mbMonocular else 3
    cnThObs = nThObs
    verdicts, set_bad = [], []
    i = 0
    while i < len(recent):
        pMP = recent[i]
        age = _int32(_int32(nCurrentKFid) - _int32(pMP.mnFirstKFid))
        if pMP.isBad():
            verdicts.append(1)
            del recent[i]
        elif pMP.GetFoundRatio() < f32(0.25):
            set_bad.append(pMP)
            verdicts.append(2)
            del recent[i]
        elif age >= 2 and pMP.Observations() <= cnThObs:
            set_bad.append(pMP)
            verdicts.append(3)
            del recent[i]
        elif age >= 3:
            verdicts.append(4)
            del recent[i]
        else:
            verdicts.append(0)
            i += 1
    return verdicts, set_bad


def _int32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def objects(t, x):
    """Mock keyframes and points from a map's tables t (slamit_map_index) and point columns x (slamit_point_index)."""
    sf = np.asarray(x["scale_factors"], np.float32)[:x["n_levels"]]
    kfs = []
    for k in range(t["n_kf"]):
        a, b = t["kf_mp_ptr"][k], t["kf_mp_ptr"][k + 1]
        kfs.append(KeyFrame(k, t["kf_bad"][k], x["kf_center"][k], x["kf_octave"][a:b].tolist(), x["kf_desc"][a:b], sf))
    mps = []
    for p in range(t["n_mp"]):
        ref = x["mp_ref_kf"][p]
        mp = MapPoint(p, t["mp_bad"][p], t["mp_pos"][p], kfs[ref] if ref >= 0 else None, x["mp_normal"][p], x["mp_max_dist"][p], x["mp_min_dist"][p],
                      x["mp_desc"][p], x["mp_nobs"][p], x["mp_found"][p], x["mp_visible"][p], x["mp_first_kf"][p])
        for o in range(t["obs_ptr"][p], t["obs_ptr"][p + 1]):
            mp.mObservations[kfs[t["obs_kf"][o]]] = int(x["obs_idx"][o])
        mps.append(mp)
    return kfs, mps
