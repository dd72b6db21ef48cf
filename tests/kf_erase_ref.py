"""KeyFrame::SetBadFlag (ORB_SLAM2 src/KeyFrame.cc:460-552), EraseConnection / UpdateBestCovisibles (:560-574, :142-161) and ChangeParent /
AddChild / EraseChild (:388-405), restated line for line over mock keyframes with dicts and lists.  No keys, no ranks, no CSR, no
bitsets: this text is what the header and the device are compared against, with no tolerance.

A std::map<KeyFrame*, T> and a std::set<KeyFrame*> iterate in ADDRESS order; a mock keyframe's address is its `addr` (the slot of the
tables), so by_addr() is the reference's iteration, a set is a list kept sorted by addr, and (weight, addr) is the reference's sort
of pair<int, KeyFrame*>.

What is not the reference's: SetBadFlag returns a status word; with mpParent NULL on a keyframe that is not the origin, where the
reference dereferences the null pointer, it returns NO_PARENT having changed nothing (the stated departure); MapPoint::EraseObservation
is not run but LOGGED as (point, keyframe), because the point side is the map-edit call that follows."""

SET_PARENT, SET_BAD = 1, 2
ORIGIN, NOT_ERASE, NO_PARENT, BAD_SLOT, ROW_OVERFLOW, CHILD_OVERFLOW, EDIT_OVERFLOW = 1, 2, 4, 8, 16, 32, 64
BEST = 10


def by_addr(d):
    return sorted(d.items(), key=lambda item: item[0].addr)


class KeyFrame:
    def __init__(self, addr, mnId):
        self.addr, self.mnId = addr, mnId
        self.mp = []                      # mvpMapPoints: a point's slot or None
        self.not_erase, self.to_be_erased, self.bad = False, False, False
        self.cw = {}                      # mConnectedKeyFrameWeights
        self.ord_kf, self.ord_w = [], []  # mvpOrderedConnectedKeyFrames, mvOrderedWeights
        self.parent, self.children = None, []   # mspChildrens: a list kept sorted by addr
        self.rewritten = False            # UpdateBestCovisibles or SetBadFlag's clear() rewrote the graph rows

    def AddChild(self, pKF):                      # :388-392, set::insert
        if pKF in self.children:
            return
        at = 0
        while at < len(self.children) and self.children[at].addr < pKF.addr:
            at += 1
        self.children.insert(at, pKF)

    def EraseChild(self, pKF):                    # :394-398
        if pKF in self.children:
            self.children.remove(pKF)

    def ChangeParent(self, pKF):                  # :400-405
        self.parent = pKF
        pKF.AddChild(self)

    def isBad(self):
        return self.bad

    def GetWeight(self, pKF):                     # :283-290
        if pKF in self.cw:
            return self.cw[pKF]
        return 0

    def UpdateBestCovisibles(self):               # :141-161
        vPairs = []
        for kf, w in by_addr(self.cw):
            vPairs.append((w, kf))
        vPairs.sort(key=lambda pair: (pair[0], pair[1].addr))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.ord_kf, self.ord_w = lKFs, lWs
        self.rewritten = True

    def EraseConnection(self, pKF):               # :560-574
        bUpdate = False
        if pKF in self.cw:
            del self.cw[pKF]
            bUpdate = True
        if bUpdate:
            self.UpdateBestCovisibles()

    def SetBadFlag(self, erased):                 # :460-552 -> status; erased: the log of EraseObservation calls
        if self.mnId == 0:
            return ORIGIN
        elif self.not_erase:
            self.to_be_erased = True
            return NOT_ERASE
        if self.parent is None:                   # the stated departure: :544 would dereference NULL
            return NO_PARENT
        for kf, _ in by_addr(self.cw):
            kf.EraseConnection(self)
        for i in range(len(self.mp)):
            if self.mp[i] is not None:
                erased.append((self.mp[i], self.addr))   # mvpMapPoints[i]->EraseObservation(this)
        self.cw = {}
        self.ord_kf, self.ord_w = [], []          # the tables hold one count for both vectors
        self.rewritten = True
        sParentCandidates = [self.parent]
        while self.children:
            bContinue = False
            max_ = -1
            pC = pP = None
            for pKF in list(self.children):
                if pKF.isBad():
                    continue
                vpConnected = list(pKF.ord_kf)
                for i in range(len(vpConnected)):
                    for spc in sParentCandidates:
                        if vpConnected[i].mnId == spc.mnId:
                            w = pKF.GetWeight(vpConnected[i])
                            if w > max_:
                                pC = pKF
                                pP = vpConnected[i]
                                max_ = w
                                bContinue = True
            if bContinue:
                pC.ChangeParent(pP)
                if pC not in sParentCandidates:
                    sParentCandidates.append(pC)
                self.children.remove(pC)
            else:
                break
        if self.children:
            for pKF in list(self.children):
                pKF.ChangeParent(self.parent)
        self.parent.EraseChild(self)
        self.bad = True
        return 0


def objects(t, x):
    """The keyframes of a map: tables t in the layout of slamit_map_index, x in that of slamit_tree_index."""
    kfs = [KeyFrame(k, 0 if k == x["origin_kf"] else k + 1) for k in range(t["n_kf"])]
    for k, kf in enumerate(kfs):
        a, b = t["kf_mp_ptr"][k], t["kf_mp_ptr"][k + 1]
        kf.mp = [int(p) if p >= 0 else None for p in t["kf_mp"][a:b]]
        kf.not_erase, kf.to_be_erased, kf.bad = bool(x["kf_not_erase"][k]), bool(x["kf_to_be_erased"][k]), bool(t["kf_bad"][k])
        kf.cw = {kfs[j]: int(w) for j, w in zip(x["cw_kf"][k][:x["cw_n"][k]], x["cw_w"][k][:x["cw_n"][k]])}
        kf.ord_kf = [kfs[j] for j in x["ord_kf"][k][:x["ord_n"][k]]]
        kf.ord_w = [int(w) for w in x["ord_w"][k][:x["ord_n"][k]]]
        kf.parent = kfs[t["kf_parent"][k]] if t["kf_parent"][k] >= 0 else None
        kf.children = [kfs[c] for c in t["kf_child"][t["kf_child_ptr"][k]:t["kf_child_ptr"][k + 1]]]
    return kfs


def apply(fx):
    """The list of a fixture, one op after the other -> what the maps holds afterwards, in plain Python values: op_status, edits [(point,
    keyframe)], children (a list of slots per keyframe), kf_bad, kf_parent, kf_to_be_erased, and per keyframe whose graph rows were
    rewritten rows[k] = (cw [(slot, weight)], ord [(slot, weight)])."""
    t, x = fx["t"], fx["x"]
    kfs = objects(t, x)
    op_status, erased = [], []
    for op in fx["ops"]:
        kind, k = op[0], op[1]
        if kind == SET_PARENT:                    # the tail of UpdateConnections, :378-383: mpParent = p; p->AddChild(this)
            kfs[k].parent = kfs[op[2]]
            kfs[op[2]].AddChild(kfs[k])
            op_status.append(0)
        else:
            op_status.append(kfs[k].SetBadFlag(erased))
    return {"op_status": op_status, "edits": erased, "children": [[c.addr for c in kf.children] for kf in kfs],
            "kf_bad": [int(kf.bad) for kf in kfs], "kf_parent": [kf.parent.addr if kf.parent is not None else -1 for kf in kfs],
            "kf_to_be_erased": [int(kf.to_be_erased) for kf in kfs],
            "rows": {kf.addr: ([(j.addr, w) for j, w in by_addr(kf.cw)], [(j.addr, w) for j, w in zip(kf.ord_kf, kf.ord_w)]) for kf in kfs if kf.rewritten}}
