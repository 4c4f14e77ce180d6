"""LocalMapping::KeyFrameCulling and MapPointCulling (src/LocalMapping.cc:
539-593, :190-218), restated literally in Python on top of the covisibility
restatement (tests/covis_numpy.py): the test reference of
orbx_covis_cull_keyframes and orbx_covis_cull_points.

What the two walks read beyond the graph: a keyframe's mvKeysUn octaves and
mbNotErase, a point's mnFound, mnVisible and mnFirstKFid.  What they write:
KeyFrame::SetBadFlag (src/KeyFrame.cc:497-521, its graph part; the spanning
tree is the caller's) and, through it, MapPoint::EraseObservation with its
rule that a point left with two observations or fewer turns bad
(src/MapPoint.cc:93-123), which is MapPoint::SetBadFlag (:125-141).

That rule applies on the culling path only.  The edit erase_keyframe of
covis_numpy.World stays what it was, a SetBadFlag whose EraseObservation only
removes and whose caller mirrors the bad points with erase_points; World.culling
tells the two apart.

A point that is bad already and was put back into a row (set_matches allows
it; the reference never adds a bad MapPoint again) is not turned bad a second
time: its observation is removed and that is all.
"""
import numpy as np

import covis_numpy as cn
from covis_numpy import ordered


class MapPoint(cn.MapPoint):
    def __init__(self, mnId, world):
        super().__init__(mnId)
        self.world = world

    def Observations(self):
        return len(self.mObservations)          # nObs of a monocular map: one per keyframe

    # src/MapPoint.cc:93-123
    def EraseObservation(self, pKF):
        bBad = False
        if pKF in self.mObservations:
            del self.mObservations[pKF]
            if len(self.mObservations) <= 2:
                bBad = True
        if bBad and self.world.culling and not self.mbBad:
            self.SetBadFlag()

    # :125-141
    def SetBadFlag(self):
        self.mbBad = True
        obs = self.mObservations
        self.mObservations = {}
        for pKF, idx in ordered(obs):
            pKF.mvpMapPoints[idx] = None        # EraseMapPointMatch
        self.world.bad_log.append(self.mnId)    # mpMap->EraseMapPoint


class KeyFrame(cn.KeyFrame):
    def __init__(self, mnId, key, mps):
        super().__init__(mnId, key, mps)
        self.octave = None                      # mvKeysUn[i].octave
        self.mbNotErase = False
        self.mbToBeErased = False

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)

    def GetKeyPointUnOctave(self, i):
        return int(self.octave[i])

    # src/KeyFrame.cc:497-521 in front of the graph part
    def SetBadFlagChecked(self):
        if self.mnId == 0:
            return 0
        if self.mbNotErase:
            self.mbToBeErased = True
            return 2
        cn.KeyFrame.SetBadFlag(self)
        return 1


class World(cn.World):
    def __init__(self):
        super().__init__()
        self.culling = False
        self.bad_log = []

    def mp(self, p):
        if p < 0:
            return None
        if p not in self.mps:
            self.mps[p] = MapPoint(p, self)
        return self.mps[p]

    def add_keyframe(self, i, key, row):
        kf = KeyFrame(i, key, [self.mp(int(p)) for p in row])
        self.kfs[i] = kf
        for idx, pMP in enumerate(kf.mvpMapPoints):
            if pMP is not None:
                pMP.AddObservation(kf, idx)

    def set_octaves(self, i, octave):
        kf = self.kfs[i]
        assert len(octave) == len(kf.mvpMapPoints)
        kf.octave = [int(o) for o in octave]

    # src/LocalMapping.cc:539-593.  cand: the caller's list of ids in place of
    # mpCurrentKeyFrame's; max_culls: stop right after that many SetBadFlags.
    def KeyFrameCulling(self, cur, keep=(), max_culls=0, cand=None):
        if cand is None:
            vpLocalKeyFrames = self.kfs[cur].GetVectorCovisibleKeyFrames()
        else:
            vpLocalKeyFrames = [self.kfs.get(int(i), int(i)) for i in cand]    # an id that was never added stays an id
        ids = [k.mnId if isinstance(k, cn.KeyFrame) else k for k in vpLocalKeyFrames]
        for kf in self.kfs.values():
            kf.mbNotErase = kf.mnId in set(int(i) for i in keep)
        n_mps, n_red, decision = [], [], []
        first_bad = len(self.bad_log)
        culls = 0
        self.culling = True
        try:
            for pKF in vpLocalKeyFrames:
                # keyframe 0 is skipped; an entry that names no member (a dangling KeyFrame* of a bad keyframe,
                # or an id outside the map) changes nothing
                if not isinstance(pKF, cn.KeyFrame) or pKF.mnId == 0 or pKF.isBad():
                    n_mps.append(0)
                    n_red.append(0)
                    decision.append(-1)
                    continue
                vpMapPoints = pKF.GetMapPointMatches()
                nRedundantObservations = 0
                nMPs = 0
                for i in range(len(vpMapPoints)):
                    pMP = vpMapPoints[i]
                    if pMP is not None:
                        if not pMP.isBad():
                            nMPs += 1
                            if pMP.Observations() > 3:
                                scaleLevel = pKF.GetKeyPointUnOctave(i)
                                observations = pMP.GetObservations()
                                nObs = 0
                                for pKFi, idx in ordered(observations):
                                    if pKFi is pKF:
                                        continue
                                    scaleLeveli = pKFi.GetKeyPointUnOctave(idx)
                                    if scaleLeveli <= scaleLevel + 1:
                                        nObs += 1
                                        if nObs >= 3:
                                            break
                                if nObs >= 3:
                                    nRedundantObservations += 1
                n_mps.append(nMPs)
                n_red.append(nRedundantObservations)
                if nRedundantObservations > 0.9 * nMPs:        # int > double * int: one FP64 product
                    d = pKF.SetBadFlagChecked()
                    decision.append(d)
                    if d == 1:
                        culls += 1
                        if culls == max_culls:
                            break
                else:
                    decision.append(0)
        finally:
            self.culling = False
        return dict(cand=ids, n_done=len(decision), n_mps=n_mps, n_redundant=n_red, decision=decision,
                    bad_points=self.bad_log[first_bad:])

    # src/LocalMapping.cc:190-218 over mlpRecentAddedMapPoints = ids
    def MapPointCulling(self, cur_kf, ids, found, visible, first_kf):
        action = []
        nCurrentKFid = int(cur_kf)
        for p, mnFound, mnVisible, mnFirstKFid in zip(ids, found, visible, first_kf):
            pMP = self.mp(int(p))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.float32(mnFound) / np.float32(mnVisible)    # static_cast<float>(mnFound)/mnVisible
            if pMP.isBad():
                action.append(1)
            elif ratio < np.float32(0.25):
                self.erase_points([p])
                action.append(2)
            elif nCurrentKFid - int(mnFirstKFid) >= 2 and pMP.Observations() <= 2:
                self.erase_points([p])
                action.append(3)
            elif nCurrentKFid - int(mnFirstKFid) >= 3:
                action.append(4)
            else:
                action.append(0)
        return action


def predicate_counts(w, c):
    """(nMPs, nRedundant) of member c as orbx.h states them: without the
    Observations() > 3 gate and without the break."""
    pKF = w.kfs[c]
    nMPs = nRed = 0
    for idx, pMP in enumerate(pKF.mvpMapPoints):
        if pMP is None or pMP.isBad():
            continue
        nMPs += 1
        o = pKF.GetKeyPointUnOctave(idx)
        n = sum(1 for pKFj, j in pMP.mObservations.items()
                if pKFj is not pKF and not pKFj.isBad() and pKFj.GetKeyPointUnOctave(j) <= o + 1)
        nRed += n >= 3
    return nMPs, nRed
