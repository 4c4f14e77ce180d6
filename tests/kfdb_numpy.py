"""KeyFrameDatabase restated literally (src/KeyFrameDatabase.cc:39-308,
Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68, src/LoopClosing.cc:119-139).

An inverted file (word -> list of keyframes in add() order), keyframe objects
with the reference's mn*Query / mn*Words / m*Score fields, Python floats for
the FP64 sum and np.float32 for every `float` step.  The structure is the
reference's, statement by statement; it shares no formulation with the device
code (no per-member scan, no sort key)."""
import numpy as np

F32 = np.float32


class KeyFrame:
    def __init__(self, mnId, words, values):
        self.mnId = int(mnId)
        # DBoW2::BowVector is a std::map<WordId, WordValue>: iteration ascends
        self.mBowVec = dict(sorted(zip([int(w) for w in words], [float(v) for v in values])))
        self.mnLoopQuery = -1
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)   # the reference leaves it uninitialised (src/KeyFrame.cc:33)
        self.neighbours = []        # GetBestCovisibilityKeyFrames(10): KeyFrame objects or ids


class Query:
    """The Frame / KeyFrame a query is made for: an id no earlier query had."""

    def __init__(self, mnId, words, values):
        self.mnId = mnId
        self.mBowVec = dict(sorted(zip([int(w) for w in words], [float(v) for v in values])))


def l1_score(v1, v2):
    """L1Scoring::score on two ascending (word, value) maps."""
    a, b = list(v1.items()), list(v2.items())
    i = j = 0
    score = 0.0
    while i < len(a) and j < len(b):
        vi, wi = a[i][1], b[j][1]
        if a[i][0] == b[j][0]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif a[i][0] < b[j][0]:
            while i < len(a) and a[i][0] < b[j][0]:   # v1.lower_bound(v2_it->first)
                i += 1
        else:
            while j < len(b) and b[j][0] < a[i][0]:
                j += 1
    return -score / 2.0


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}   # word -> list of KeyFrame
        self.kfs = {}              # id -> KeyFrame (the map's keyframes that are in the database)
        self._next_query = 1 << 40

    # -- the reference's members ------------------------------------------
    def add(self, pKF):
        assert pKF.mnId not in self.kfs
        self.kfs[pKF.mnId] = pKF
        for w in pKF.mBowVec:
            self.mvInvertedFile.setdefault(w, []).append(pKF)

    def erase(self, pKF):
        for w in pKF.mBowVec:
            lKFs = self.mvInvertedFile[w]
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break
        del self.kfs[pKF.mnId]

    def clear(self):
        self.mvInvertedFile = {}
        self.kfs = {}

    def _neighbours(self, pKFi):
        """vpNeighs as far as the database can see them: an entry that names
        no member is skipped (the device's rule for a stale row)."""
        out = []
        for n in pKFi.neighbours:
            kf = n if isinstance(n, KeyFrame) else self.kfs.get(int(n))
            if kf is not None and self.kfs.get(kf.mnId) is kf:
                out.append(kf)
        return out

    def new_query(self, words, values):
        self._next_query += 1
        return Query(self._next_query, words, values)

    def DetectLoopCandidates(self, pKF, minScore, spConnectedKeyFrames=()):
        minScore = F32(minScore)
        spConnectedKeyFrames = set(id(k) for k in spConnectedKeyFrames)
        lKFsSharingWords = []
        for w in pKF.mBowVec:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if id(pKFi) not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        self.last = dict(sharing=lKFsSharingWords, maxCommonWords=0, minCommonWords=0, nscores=0, acc=[])
        if not lKFsSharingWords:
            return []
        lScoreAndMatch = []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(l1_score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        self.last.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, nscores=nscores)
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            self.last["acc"].append((pKFi, accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpLoopCandidates = []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if id(pKFi) not in spAlreadyAddedKF:
                    vpLoopCandidates.append(pKFi)
                    spAlreadyAddedKF.add(id(pKFi))
        return vpLoopCandidates

    def DetectRelocalisationCandidates(self, F):
        lKFsSharingWords = []
        for w in F.mBowVec:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        self.last = dict(sharing=lKFsSharingWords, maxCommonWords=0, minCommonWords=0, nscores=0, acc=[])
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F32(l1_score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        self.last.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, nscores=nscores)
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            self.last["acc"].append((pKFi, accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if id(pKFi) not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(id(pKFi))
        return vpRelocCandidates

    # -- LoopClosing::DetectLoop's reference score (:122-136) ---------------
    def detect_loop_min_score(self, pKF, vpConnectedKeyFrames, start=1.0):
        minScore = F32(start)
        for k in vpConnectedKeyFrames:
            score = F32(l1_score(pKF.mBowVec, k.mBowVec))
            if score < minScore:
                minScore = score
        return minScore

    # -- what the device's taps report, per member id ----------------------
    def taps(self, capacity, loop, query_id):
        """words / score / acc / best / pos arrays as include/orbx.h defines
        the taps, read from the fields the last query left."""
        t = dict(words=np.zeros(capacity, np.int32), score=np.zeros(capacity, np.float32),
                 acc=np.zeros(capacity, np.float32), best=np.full(capacity, -1, np.int32),
                 pos=np.full(capacity, -1, np.int32))
        for p, kf in enumerate(self.last["sharing"]):
            t["pos"][kf.mnId] = p
            t["words"][kf.mnId] = kf.mnLoopWords if loop else kf.mnRelocWords
            if loop and kf.mnLoopWords > self.last["minCommonWords"]:
                t["score"][kf.mnId] = kf.mLoopScore
        if not loop:
            for kf in self.kfs.values():
                t["score"][kf.mnId] = kf.mRelocScore
        for kf, acc, best in self.last["acc"]:
            t["acc"][kf.mnId] = acc
            t["best"][kf.mnId] = best.mnId
        return t
