"""KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles (ORB_SLAM2 src/KeyFrame.cc:127-161, :296-386),
LocalMapping::KeyFrameCulling (src/LocalMapping.cc:686-752), KeyFrame::SetBadFlag (the mnId == 0 and mbNotErase exits and the
EraseObservation loop only) and MapPoint::EraseObservation / SetBadFlag, restated line for line over mock objects with dicts and sets.
No keys, no scans, no bitsets: this text is what the device is compared against, with no tolerance.

A std::map<KeyFrame*, T> iterates in ADDRESS order; a mock keyframe's address is its `addr` (the slot of the tables), so by_addr()
is the reference's iteration and (weight, addr) its sort of pair<int, KeyFrame*>."""


class MapPoint:
    def __init__(self, slot, bad, nobs):
        self.slot, self.bad, self.nobs = slot, bool(bad), int(nobs)
        self.obs = {}                     # mObservations: KeyFrame -> keypoint index
        self.turned_bad = False           # SetBadFlag ran in this call

    def isBad(self):
        return self.bad

    def Observations(self):
        return self.nobs

    def EraseObservation(self, pKF):      # MapPoint.cc:117-143
        bBad = False
        if pKF in self.obs:
            idx = self.obs[pKF]
            if pKF.uright[idx] >= 0:
                self.nobs -= 2
            else:
                self.nobs -= 1
            del self.obs[pKF]
            if self.nobs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):                 # MapPoint.cc:145-163
        if not self.bad:
            self.turned_bad = True
        self.bad = True
        obs = self.obs
        self.obs = {}
        for pKF, idx in by_addr(obs):
            pKF.mp[idx] = None            # EraseMapPointMatch


class KeyFrame:
    def __init__(self, addr, mnId):
        self.addr, self.mnId = addr, mnId
        self.mp, self.octave, self.uright, self.depth = [], [], [], []
        self.th_depth, self.not_erase, self.to_be_erased = 0.0, False, False
        self.cw = {}                      # mConnectedKeyFrameWeights
        self.ord_kf, self.ord_w = [], []  # mvpOrderedConnectedKeyFrames, mvOrderedWeights
        self.first_connection, self.parent, self.children = False, None, set()
        self.resorted = False             # UpdateBestCovisibles or UpdateConnections rewrote the ordered vectors

    def AddConnection(self, pKF, weight):         # :127-139
        if pKF not in self.cw:
            self.cw[pKF] = weight
        elif self.cw[pKF] != weight:
            self.cw[pKF] = weight
        else:
            return
        self.UpdateBestCovisibles()

    def UpdateBestCovisibles(self):               # :141-161
        vPairs = []
        for kf, w in by_addr(self.cw):
            vPairs.append((w, kf))
        vPairs.sort(key=pair_key)
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.ord_kf, self.ord_w = lKFs, lWs
        self.resorted = True

    def UpdateConnections(self):                  # :296-386 -> KFcounter, for the tests
        KFcounter = {}
        vpMP = list(self.mp)
        for pMP in vpMP:
            if not pMP:
                continue
            if pMP.isBad():
                continue
            for kf, _ in by_addr(pMP.obs):
                if kf.mnId == self.mnId:
                    continue
                KFcounter[kf] = KFcounter.get(kf, 0) + 1
        if not KFcounter:
            return KFcounter
        nmax, pKFmax, th = 0, None, 15
        vPairs = []
        for kf, n in by_addr(KFcounter):
            if n > nmax:
                nmax, pKFmax = n, kf
            if n >= th:
                vPairs.append((n, kf))
                kf.AddConnection(self, n)
        if not vPairs:
            vPairs.append((nmax, pKFmax))
            pKFmax.AddConnection(self, nmax)
        vPairs.sort(key=pair_key)
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.cw = dict(KFcounter)
        self.ord_kf, self.ord_w = lKFs, lWs
        self.resorted = True
        if self.first_connection and self.mnId != 0:
            self.parent = self.ord_kf[0]
            self.parent.children.add(self)
            self.first_connection = False
        return KFcounter

    def SetBadFlag(self):                         # :444-..., the two exits and the EraseObservation loop
        if self.mnId == 0:
            return
        elif self.not_erase:
            self.to_be_erased = True
            return
        for i in range(len(self.mp)):
            if self.mp[i]:
                self.mp[i].EraseObservation(self)
        self.culled = True


def by_addr(d):
    return sorted(d.items(), key=lambda item: item[0].addr)


def pair_key(pair):
    return (pair[0], pair[1].addr)


def KeyFrameCulling(cur, bMonocular):             # LocalMapping.cc:686-752 -> [(keyframe, nMPs, nRedundantObservations, culled?)]
    trace = []
    vpLocalKeyFrames = list(cur.ord_kf)
    for pKF in vpLocalKeyFrames:
        if pKF.mnId == 0:
            trace.append((pKF, 0, 0, None))
            continue
        vpMapPoints = list(pKF.mp)
        thObs = 3
        nRedundantObservations = 0
        nMPs = 0
        for i in range(len(vpMapPoints)):
            pMP = vpMapPoints[i]
            if pMP:
                if not pMP.isBad():
                    if not bMonocular:
                        if pKF.depth[i] > pKF.th_depth or pKF.depth[i] < 0:
                            continue
                    nMPs += 1
                    if pMP.Observations() > thObs:
                        scaleLevel = pKF.octave[i]
                        nObs = 0
                        for pKFi, idx in by_addr(pMP.obs):
                            if pKFi is pKF:
                                continue
                            scaleLeveli = pKFi.octave[idx]
                            if scaleLeveli <= scaleLevel + 1:
                                nObs += 1
                                if nObs >= thObs:
                                    break
                        if nObs >= thObs:
                            nRedundantObservations += 1
        culled = nRedundantObservations > 0.9 * nMPs
        if culled:
            pKF.SetBadFlag()
        trace.append((pKF, nMPs, nRedundantObservations, culled))
    return trace


# ---- mock objects from the tables of a fixture, and the results as the arrays the calls write --------------------------------

def objects(t, x):
    """The keyframes and map points of a map (tables t in the layout of slamit_map_index, x in that of slamit_covis_index plus the
    test-only column obs_idx: the keypoint index of an observation)."""
    kfs = [KeyFrame(k, 0 if k == x["origin_kf"] else k + 1) for k in range(t["n_kf"])]
    mps = [MapPoint(p, t["mp_bad"][p], x["mp_nobs"][p]) for p in range(t["n_mp"])]
    row_cap = x["row_cap"]
    for k, kf in enumerate(kfs):
        a, b = t["kf_mp_ptr"][k], t["kf_mp_ptr"][k + 1]
        kf.mp = [mps[p] if p >= 0 else None for p in t["kf_mp"][a:b]]
        kf.octave = [int(o) for o in x["kf_octave"][a:b]]
        kf.depth = [x["kf_depth"][e] for e in range(a, b)] if x.get("kf_depth") is not None else None     # float32, compared as such
        kf.th_depth = x["kf_th_depth"][k] if x.get("kf_th_depth") is not None else None
        kf.uright = [-1.0] * (b - a)
        kf.not_erase = bool(x["kf_not_erase"][k])
        kf.cw = {kfs[j]: int(w) for j, w in zip(x["cw_kf"][k][:x["cw_n"][k]], x["cw_w"][k][:x["cw_n"][k]])}
        kf.ord_kf = [kfs[j] for j in x["ord_kf"][k][:x["ord_n"][k]]]
        kf.ord_w = [int(w) for w in x["ord_w"][k][:x["ord_n"][k]]]
    for p, mp in enumerate(mps):
        for o in range(t["obs_ptr"][p], t["obs_ptr"][p + 1]):
            kf, idx = kfs[t["obs_kf"][o]], int(x["obs_idx"][o])
            mp.obs[kf] = idx
            assert kf.octave[idx] == x["obs_octave"][o] and kf.mp[idx] is mp, "the fixture's observation columns disagree with its rows"
            if x["obs_weight"][o] == 2:
                kf.uright[idx] = 1.0
    assert row_cap >= 1
    return kfs, mps
