"""The reference's covisibility graph, restated literally in Python: the test
reference of orbx_covis_*.

KeyFrame::AddConnection, UpdateBestCovisibles, EraseConnection,
UpdateConnections, the reads and the connection part of SetBadFlag
(src/KeyFrame.cc:126-211, :332-421, :436-449, :510-521), and
Tracking::UpdateReferenceKeyFrames / UpdateReferencePoints
(src/Tracking.cc:764-865).

A KeyFrame* is an object with a 64-bit `key`; every std::map<KeyFrame*, ...>
is a dict that is iterated through ordered(), ascending in the key, and
std::sort of pair<int, KeyFrame*> sorts by (weight, key).  The ordered lists
are stored and rewritten where the reference rewrites them, never derived
from the weights: the library derives them, and the tests compare the two.

MapPoint::EraseObservation turns a point bad when two observations or fewer
remain (src/MapPoint.cc:110-113); that is MapPoint::SetBadFlag, which the
caller mirrors with erase_points, so EraseObservation here only removes.
"""


def ordered(d):
    """A std::map<KeyFrame*, T>'s iteration: ascending pointer value."""
    return sorted(d.items(), key=lambda kv: kv[0].key)


class MapPoint:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mbBad = False
        self.mObservations = {}            # KeyFrame -> index
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad

    def GetObservations(self):
        return dict(self.mObservations)

    def AddObservation(self, pKF, idx):
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx

    def EraseObservation(self, pKF):
        self.mObservations.pop(pKF, None)


class KeyFrame:
    def __init__(self, mnId, key, mps):
        self.mnId = mnId
        self.key = key
        self.mvpMapPoints = list(mps)      # MapPoint or None
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames = []
        self.mvOrderedWeights = []
        self.mbBad = False
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad

    # src/KeyFrame.cc:126-139
    def AddConnection(self, pKF, weight):
        if pKF not in self.mConnectedKeyFrameWeights:
            self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight:
            self.mConnectedKeyFrameWeights[pKF] = weight
        else:
            return
        self.UpdateBestCovisibles()

    # :141-160
    def UpdateBestCovisibles(self):
        vPairs = [(w, kf) for kf, w in ordered(self.mConnectedKeyFrameWeights)]
        vPairs.sort(key=lambda p: (p[0], p[1].key))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)             # push_front
            lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames = lKFs
        self.mvOrderedWeights = lWs

    # :436-449
    def EraseConnection(self, pKF):
        bUpdate = False
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            bUpdate = True
        if bUpdate:
            self.UpdateBestCovisibles()

    # :162-211
    def GetConnectedKeyFrames(self):
        return [kf for kf, _ in ordered(self.mConnectedKeyFrameWeights)]   # a std::set<KeyFrame*>

    def GetVectorCovisibleKeyFrames(self):
        return list(self.mvpOrderedConnectedKeyFrames)

    def GetBestCovisibilityKeyFrames(self, N):
        if len(self.mvpOrderedConnectedKeyFrames) < N:
            return list(self.mvpOrderedConnectedKeyFrames)
        return self.mvpOrderedConnectedKeyFrames[:N]

    def GetCovisiblesByWeight(self, w):
        if not self.mvpOrderedConnectedKeyFrames:
            return []
        # upper_bound(begin, end, w, weightComp), weightComp(a, b) = a > b: the
        # first element e with weightComp(w, e), that is w > e
        it = len(self.mvOrderedWeights)
        for k, e in enumerate(self.mvOrderedWeights):
            if w > e:
                it = k
                break
        if it == len(self.mvOrderedWeights):
            return []
        return self.mvpOrderedConnectedKeyFrames[:it]

    def GetWeight(self, pKF):
        return self.mConnectedKeyFrameWeights.get(pKF, 0)

    # :332-421.  Returns (updated, front): whether the function got past
    # `if(KFcounter.empty()) return;`, and mvpOrderedConnectedKeyFrames.front().
    def UpdateConnections(self, th=15):
        KFcounter = {}
        for pMP in list(self.mvpMapPoints):
            if pMP is None:
                continue
            if pMP.isBad():
                continue
            for kf, _ in ordered(pMP.GetObservations()):
                if kf.mnId == self.mnId:
                    continue
                KFcounter[kf] = KFcounter.get(kf, 0) + 1
        if not KFcounter:
            return 0, None
        nmax, pKFmax = 0, None
        vPairs = []
        for kf, c in ordered(KFcounter):
            if c > nmax:
                nmax, pKFmax = c, kf
            if c >= th:
                vPairs.append((c, kf))
                kf.AddConnection(self, c)
        if not vPairs:
            vPairs.append((nmax, pKFmax))
            pKFmax.AddConnection(self, nmax)
        vPairs.sort(key=lambda p: (p[0], p[1].key))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.mConnectedKeyFrameWeights = KFcounter
        self.mvpOrderedConnectedKeyFrames = lKFs
        self.mvOrderedWeights = lWs
        return 1, lKFs[0]

    # the connection part of SetBadFlag, :510-521
    def SetBadFlag(self):
        for kf, _ in ordered(self.mConnectedKeyFrameWeights):
            kf.EraseConnection(self)
        for pMP in self.mvpMapPoints:
            if pMP is not None:
                pMP.EraseObservation(self)
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames = []
        self.mvOrderedWeights = []
        self.mbBad = True


class Frame:
    def __init__(self, mnId, mps):
        self.mnId = mnId
        self.mvpMapPoints = list(mps)


class Tracking:
    """The two functions of Tracking::UpdateReference."""

    def __init__(self):
        self.mvpLocalKeyFrames = []
        self.mvpLocalMapPoints = []
        self.mpReferenceKF = None
        self.n_voters = 0

    # src/Tracking.cc:790-865
    def UpdateReferenceKeyFrames(self, F):
        keyframeCounter = {}
        for i in range(len(F.mvpMapPoints)):
            if F.mvpMapPoints[i] is not None:
                pMP = F.mvpMapPoints[i]
                if not pMP.isBad():
                    for kf, _ in ordered(pMP.GetObservations()):
                        keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
                else:
                    F.mvpMapPoints[i] = None
        mx, pKFmax = 0, None
        self.mvpLocalKeyFrames = []
        for pKF, c in ordered(keyframeCounter):
            if pKF.isBad():
                continue
            if c > mx:
                mx, pKFmax = c, pKF
            self.mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = F.mnId
        self.n_voters = len(self.mvpLocalKeyFrames)
        # the reference takes end() before the loop (the vector was reserved,
        # so its iterators stay valid): the voters alone are visited
        for k in range(self.n_voters):
            if len(self.mvpLocalKeyFrames) > 80:
                break
            pKF = self.mvpLocalKeyFrames[k]
            for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != F.mnId:
                        self.mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = F.mnId
                        break
        self.mpReferenceKF = pKFmax

    # :764-787
    def UpdateReferencePoints(self, F):
        self.mvpLocalMapPoints = []
        for pKF in self.mvpLocalKeyFrames:
            for pMP in pKF.mvpMapPoints:
                if pMP is None:
                    continue
                if pMP.mnTrackReferenceForFrame == F.mnId:
                    continue
                if not pMP.isBad():
                    self.mvpLocalMapPoints.append(pMP)
                    pMP.mnTrackReferenceForFrame = F.mnId


class World:
    """The map as the edits of orbx_covis_* change it, and the three
    operations on it.  Ids are mnIds; a keyframe is added with its
    observations (LocalMapping::ProcessNewKeyFrame), and AddMapPoint /
    AddObservation and EraseMapPointMatch / EraseObservation go in pairs."""

    def __init__(self):
        self.kfs = {}       # id -> KeyFrame, the erased (bad) ones included
        self.mps = {}       # id -> MapPoint
        self.tracking = Tracking()
        self.next_frame = 0

    def mp(self, p):
        if p < 0:
            return None
        if p not in self.mps:
            self.mps[p] = MapPoint(p)
        return self.mps[p]

    def add_keyframe(self, i, key, row):
        kf = KeyFrame(i, key, [self.mp(int(p)) for p in row])
        self.kfs[i] = kf
        for idx, pMP in enumerate(kf.mvpMapPoints):
            if pMP is not None:
                pMP.AddObservation(kf, idx)

    def set_matches(self, i, idx, mp):
        kf = self.kfs[i]
        for a, p in zip(idx, mp):
            old = kf.mvpMapPoints[a]
            if old is not None:            # EraseMapPointMatch + EraseObservation
                old.EraseObservation(kf)
                kf.mvpMapPoints[a] = None
            if p >= 0:                     # AddMapPoint + AddObservation
                pMP = self.mp(int(p))
                kf.mvpMapPoints[a] = pMP
                pMP.AddObservation(kf, a)

    def erase_points(self, ids):
        """MapPoint::SetBadFlag (src/MapPoint.cc:125-141)."""
        for p in ids:
            pMP = self.mp(int(p))
            pMP.mbBad = True
            obs = pMP.mObservations
            pMP.mObservations = {}
            for kf, idx in ordered(obs):
                kf.mvpMapPoints[idx] = None    # EraseMapPointMatch

    def erase_keyframe(self, i):
        self.kfs[i].SetBadFlag()

    def update_connections(self, ids, th=15):
        updated, front = [], []
        for i in ids:
            u, f = self.kfs[i].UpdateConnections(th)
            updated.append(u)
            front.append(f.mnId if f is not None else -1)
        return updated, front

    def ordered_list(self, i):
        kf = self.kfs[i]
        return [k.mnId for k in kf.mvpOrderedConnectedKeyFrames], list(kf.mvOrderedWeights)

    def all_list(self, i):
        kf = self.kfs[i]
        c = kf.GetConnectedKeyFrames()
        return [k.mnId for k in c], [kf.GetWeight(k) for k in c]

    def update_reference(self, frame_mp):
        F = Frame(self.next_frame, [self.mp(int(p)) for p in frame_mp])
        self.next_frame += 1
        before = list(F.mvpMapPoints)
        t = self.tracking
        t.UpdateReferenceKeyFrames(F)
        t.UpdateReferencePoints(F)
        erased = [1 if (b is not None and a is None) else 0 for b, a in zip(before, F.mvpMapPoints)]
        return dict(frame_erased=erased, local_kf=[k.mnId for k in t.mvpLocalKeyFrames], n_voters=t.n_voters,
                    ref_kf=t.mpReferenceKF.mnId if t.mpReferenceKF is not None else -1,
                    local_mp=[p.mnId for p in t.mvpLocalMapPoints])
