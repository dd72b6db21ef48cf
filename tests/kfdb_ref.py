"""Line-by-line Python restatement of the reference's keyframe database and of DBoW2's L1 score (no GPU, no reference access at run
time).  Paths are relative to oRB_SLAM2_Android/src/main/jni/; K = ORB_SLAM2/src/KeyFrameDatabase.cc,
S = Thirdparty/DBoW2/src/ScoringObject.cpp.

The inverted file is kept as real lists, one per word, so the order in which the walk meets the keyframes is the reference's own and
checks the (first shared word, seq) rule of include/slamit.h independently.  Sums are Python floats (IEEE doubles) added one after the
other; the members the reference declares float are np.float32, and every sum into them is rounded to float after each addition.

A BowVector is a pair (word ids ascending i32, values f64), the layout of api.ORBVocabulary.transform."""
import numpy as np

F32 = np.float32


def score(v1, v2):
    """L1Scoring::score (S:23-68).  The walk with lower_bound visits the shared words in ascending word id."""
    w1, x1 = v1
    w2, x2 = v2
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    s = 0.0                                                  # S:32
    while i < n1 and j < n2:                                 # S:34
        if w1[i] == w2[j]:                                   # S:39
            vi, wi = float(x1[i]), float(x2[j])
            s += abs(vi - wi) - abs(vi) - abs(wi)            # S:41
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i += int(np.searchsorted(w1[i:], w2[j], "left"))   # S:50 lower_bound
        else:
            j += int(np.searchsorted(w2[j:], w1[i], "left"))   # S:56
    return -s / 2.0                                          # S:65


def score_reversed(v1, v2):
    """The same terms added from the largest shared word id down: what a sum in another order gives (fixture admissibility only)."""
    w1, x1 = v1
    w2, x2 = v2
    _, i1, i2 = np.intersect1d(w1, w2, assume_unique=True, return_indices=True)
    s = 0.0
    for a, b in zip(i1[::-1], i2[::-1]):
        vi, wi = float(x1[a]), float(x2[b])
        s += abs(vi - wi) - abs(vi) - abs(wi)
    return -s / 2.0


def min_common_words(max_common):
    """int minCommonWords = maxCommonWords*0.8f (K:129, K:254): int -> float, a float product, truncation."""
    return int(F32(max_common) * F32(0.8))


class KeyFrame:
    """The members of KeyFrame the database touches.  mLoopScore / mRelocScore are uninitialised in the reference
    (ORB_SLAM2/src/KeyFrame.cc, constructor list); here they start at 0.0f, the project's one stated departure."""

    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, F32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)
        self.connected = set()                               # GetConnectedKeyFrames()
        self.best_covisibles = []                            # GetBestCovisibilityKeyFrames(10)


class Frame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}                             # word id -> list of KeyFrame (K:41: a vector of std::list)

    def add(self, pKF):                                      # K:45-54
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile.setdefault(int(w), []).append(pKF)

    def erase(self, pKF):                                    # K:56-75: the first occurrence leaves, the rest keep their order
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile.get(int(w), [])
            for k, other in enumerate(lKFs):
                if other is pKF:
                    del lKFs[k]
                    break

    def clear(self):                                         # K:77-81
        self.mvInvertedFile = {}

    def DetectLoopCandidates(self, pKF, minScore):           # K:84-206
        minScore = F32(minScore)
        spConnectedKeyFrames = pKF.connected                 # K:86
        lKFsSharingWords = []
        for w in pKF.mBowVec[0]:                             # K:94-112
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0                     # K:103
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1                        # K:110
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:                        # K:123-127
            if pKFi.mnLoopWords > maxCommonWords:
                maxCommonWords = pKFi.mnLoopWords
        minCommonWords = min_common_words(maxCommonWords)    # K:129
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:                        # K:134-148
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(score(pKF.mBowVec, pKFi.mBowVec))   # K:142: float si
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        self.last = {"sharing": lKFsSharingWords, "minCommonWords": minCommonWords, "nscores": nscores, "scored": lScoreAndMatch}
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore                              # K:154
        for si, pKFi in lScoreAndMatch:                      # K:157-182
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in pKFi.best_covisibles:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)     # K:185
        self.last["acc"] = lAccScoreAndMatch
        return self._retain(lAccScoreAndMatch, minScoreToRetain)

    def DetectRelocalizationCandidates(self, F):             # K:208-328
        lKFsSharingWords = []
        for w in F.mBowVec[0]:                               # K:219-237
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:                        # K:248-252
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = min_common_words(maxCommonWords)    # K:254
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:                        # K:261-272
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F32(score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        self.last = {"sharing": lKFsSharingWords, "minCommonWords": minCommonWords, "nscores": nscores, "scored": lScoreAndMatch}
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)                                # K:278
        for si, pKFi in lScoreAndMatch:                      # K:281-306
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in pKFi.best_covisibles:
                if pKF2.mnRelocQuery != F.mnId:              # K:292
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)  # K:295: this query's score, or what an earlier query left
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)     # K:309
        self.last["acc"] = lAccScoreAndMatch
        return self._retain(lAccScoreAndMatch, minScoreToRetain)

    def _retain(self, lAccScoreAndMatch, minScoreToRetain):  # K:187-202, K:310-325
        spAlreadyAddedKF, out = set(), []
        self.last["duplicates"] = 0
        for s, pKFi in lAccScoreAndMatch:
            if s > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    out.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
                else:
                    self.last["duplicates"] += 1
        return out


def dense(keyframes, query_bow):
    """What slamit_kfdb_query returns for the keyframes in `keyframes` (slot -> KeyFrame or None), from the definitions alone:
    common, first_word, score per slot."""
    n = len(keyframes)
    common, first, sc = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.float64)
    for s, kf in enumerate(keyframes):
        if kf is None:
            continue
        shared = np.intersect1d(query_bow[0], kf.mBowVec[0], assume_unique=True)
        common[s] = len(shared)
        if len(shared):
            first[s] = shared[0]
            sc[s] = score(query_bow, kf.mBowVec)
    return common, first, sc


# ---- fixture builders -------------------------------------------------------------------------------------------------------------

def bow(pool, n, seed):
    """n distinct word ids from range(pool), ascending; values uniform(0.05, 9) x randint(1, 4) -- a weight times a count, as the
    transform sums them -- divided by their sequential sum (BowVector::normalize)."""
    rs = np.random.RandomState(seed)
    words = np.sort(rs.permutation(pool)[:n]).astype(np.int32)
    values = rs.uniform(0.05, 9.0, n) * rs.randint(1, 4, n)
    norm = 0.0
    for v in values:
        norm += abs(float(v))
    if norm > 0.0:
        values = values / norm
    return words, values.astype(np.float64)


def ring(n, reach=5):
    """A ring covisibility graph: keyframe i's best covisibles are i+1, i-1, i+2, i-2 ... i+reach, i-reach (mod n)."""
    out = []
    for i in range(n):
        nb = []
        for d in range(1, reach + 1):
            for j in ((i + d) % n, (i - d) % n):
                if j != i and j not in nb:
                    nb.append(j)
        out.append(nb)
    return out


def scoring_pairs(pool, count=100, seed=0):
    """count (query, keyframe) pairs of lengths 100-260 over one pool."""
    rs = np.random.RandomState(1000 + seed + pool)
    lim = min(pool, 260)
    lo = min(100, lim)
    return [(bow(pool, int(rs.randint(lo, lim + 1)), 7 * i + pool), bow(pool, int(rs.randint(lo, lim + 1)), 7 * i + 3 + pool)) for i in range(count)]


# name -> dict(pool, lengths of the keyframes' vectors, seed, erase, queries).  A query is ("reloc", frame id, seed, length) or
# ("loop", keyframe id, seed, length, connected ids, minScore); the scenario runs them in order on one database, so the keyframes'
# members carry over from one query to the next.
SCENARIOS = {
    "reloc_stale": dict(pool=400, n_kf=80, lengths=(60, 250), seed=6, erase=(7,),
                        queries=[("reloc", 101, 11, 200), ("reloc", 102, 12, 90)]),
    "loop": dict(pool=400, n_kf=80, lengths=(60, 250), seed=1, erase=(7,),
                 queries=[("loop", 500, 21, 220, (0, 1, 2, 79, 78), 0.3)]),
    "mixed": dict(pool=400, n_kf=120, lengths=(60, 250), seed=7, erase=(7,),
                  queries=[("reloc", 101, 11, 200), ("reloc", 102, 12, 90), ("loop", 500, 21, 220, (0, 1, 2, 119, 118), 0.315)]),
}


def scenario_keyframes(sc):
    """The scenario's keyframes (ids 0 .. n_kf - 1, ring covisibility), none added to a database yet."""
    rs = np.random.RandomState(sc["seed"])
    lo, hi = sc["lengths"]
    kfs = [KeyFrame(i, bow(sc["pool"], int(rs.randint(lo, hi + 1)), 100 * sc["seed"] + i)) for i in range(sc["n_kf"])]
    for i, nb in enumerate(ring(sc["n_kf"])):
        kfs[i].best_covisibles = [kfs[j] for j in nb]
    return kfs


def query_bow(sc, q):
    return bow(sc["pool"], q[3], 5000 + q[2])


def run_scenario(sc, reset_scores=False):
    """Adds every keyframe, erases sc["erase"], runs the queries -> (list of candidate id lists, list of the database's `last`).
    reset_scores zeroes mRelocScore / mLoopScore before every query (what a stateless implementation would compute)."""
    kfs = scenario_keyframes(sc)
    db = KeyFrameDatabase()
    for kf in kfs:
        db.add(kf)
    for i in sc["erase"]:
        db.erase(kfs[i])
    out, notes = [], []
    for q in sc["queries"]:
        if reset_scores:
            for kf in kfs:
                kf.mLoopScore, kf.mRelocScore = F32(0), F32(0)
        if q[0] == "reloc":
            got = db.DetectRelocalizationCandidates(Frame(q[1], query_bow(sc, q)))
        else:
            pKF = KeyFrame(q[1], query_bow(sc, q))
            pKF.connected = set(kfs[i] for i in q[4])
            got = db.DetectLoopCandidates(pKF, q[5])
        out.append([kf.mnId for kf in got])
        notes.append(db.last)
    return out, notes
