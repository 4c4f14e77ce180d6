"""The oracle's keyframe projection searches (oracle/ref_proj.cpp) against
the float64 restatement of tests/pose_scenes.py under general poses, and the
scene builder itself (CPU).

Every decided point must agree on winner index, distance and rejection.  The
undecided share is capped at 2 % per scene and at zero within the gate rows
and the size-edge winners; each test prints its share.  Measured on the
first green run: 0 .. 1.15 % over the gate scenes (at most 3 of 262 points;
0 in 98 of the 120 scene x entry runs), 0 for the exact, size and
SearchBySim3 scenes; isInFrustum 0 except 0.38 % (one point) in one scene.
"""
import numpy as np
import pytest

import pose_scenes as ps
import proj_data as pd
from test_proj_oracle import ref_distinctive

CAP = 0.02
# (entry, Scw scale, ORBdist, check_ori)
RUNS = [("fuse0", 1.0, 0, 0), ("fuse1", 0.6, 0, 0), ("fuse1", 1.7, 0, 0), ("kfsim3", 0.6, 0, 0), ("kfsim3", 1.7, 0, 0),
        ("framekf", 1.0, 100, 0), ("framekf", 1.0, 40, 0), ("framekf", 1.0, 100, 1), ("framekf", 1.0, 40, 1)]
RUN_IDS = ["-".join(str(v) for v in r) for r in RUNS]


def compare(s, entry, scale, orb, ori, handle=None, nq=None):
    """Oracle (or device) against the float64 reference on the decided points
    of scene s; returns (reference result, call's outputs, undecided share)."""
    res, out, n = ps.reference(s, entry, scale, orb, ori, nq=nq)
    got = ps.run(s, entry, handle, scale, orb, ori, nq=nq)
    assert got[0] == 0
    if entry in ("fuse0", "fuse1"):
        share = ps.check_decided(s, entry, res, got[1], got[2])
    else:
        share = ps.check_decided(s, entry, res, got[1])
        if share == 0:
            assert got[2] == n and np.array_equal(got[1], out)
    print(f"{s.name} {entry} s={scale} orb={orb} ori={ori}: undecided {share:.4f}")
    return res, got, share


@pytest.mark.parametrize("pose,bounds", ps.GATE_SCENES, ids=[f"{p}-{b}" for p, b in ps.GATE_SCENES])
@pytest.mark.parametrize("entry,scale,orb,ori", RUNS, ids=RUN_IDS)
def test_oracle_agrees_with_float64_reference(pose, bounds, entry, scale, orb, ori):
    s = ps.scene(pose, bounds)
    res, _, share = compare(s, entry, scale, orb, ori)
    assert share <= CAP
    assert res.ori_stable        # else no Frame/KF winner of a check_ori run would have been compared
    rows = [p for pair in s.rows.values() for p in pair] + [p for p, _ in s.thresh.values()]
    rows += list(s.levels) + list(s.pred_edges) + list(s.chain) + list(s.rotation) + [t[1] for t in s.ties]
    assert res.decided[rows].all()


@pytest.mark.parametrize("pose,bounds", ps.GATE_SCENES, ids=[f"{p}-{b}" for p, b in ps.GATE_SCENES])
def test_every_gate_has_a_rejected_and_an_accepted_decided_point(pose, bounds):
    """The builder: each gate row's two points are rejected and passed *by
    that gate* in the float64 reference, for every gate of every entry point."""
    s = ps.scene(pose, bounds)
    for entry in ps.ENTRIES:
        res, _, _ = ps.reference(s, entry, 1.7, 100, 0)
        order = ps.GATES[entry] + ("win",)
        for gate in ps.GATES[entry]:
            rej, acc = s.rows[gate]
            assert res.decided[rej] and res.decided[acc], (entry, gate)
            assert res.gate[rej] == gate, (entry, gate, res.gate[rej])
            assert order.index(res.gate[acc]) > order.index(gate), (entry, gate, res.gate[acc])
        if entry == "framekf":      # no z gate: the point behind the camera is searched at its mirrored projection
            assert res.gate[s.rows["z"][0]] == "win"
        # accept thresholds: TH_LOW for KF/Scw, ORBdist 40 and 100 for Frame/KF; Fuse reports the distance
        for limit, orb in ((ps.TH_LOW, 100),) if entry == "kfsim3" else ((40, 40), (100, 100)) if entry == "framekf" else ():
            r2, _, _ = ps.reference(s, entry, 1.7, orb, 0)
            for d, (p, c) in s.thresh.items():
                assert r2.decided[p] and r2.idx[p] == c and r2.dist[p] == d
                assert r2.gate[p] == ("win" if d <= limit else "thresh"), (entry, d)
        # what follows from the construction: level windows, clamped levels, ties, chains, taken candidates
        want = dict(s.expect["fuse"])
        if entry in ("kfsim3", "framekf"):
            want.update(s.expect["seq"])
        if entry == "framekf":
            want.update(s.expect["framekf"])
        for p, c in want.items():
            assert res.decided[p] and res.idx[p] == c, (entry, p, res.gate[p], int(res.idx[p]), c)
    # predicted level 0 (ratio below 1) only where no min_dist gate stands before it, the clamp everywhere
    p0, p7 = s.pred_edges
    assert ps.reference(s, "fuse0")[0].gate[p0] == "dmin" and ps.reference(s, "framekf")[0].gate[p0] == "win"
    K = s.K
    for kind, p, first, second in s.ties:
        assert K.desc[first].tolist() != K.desc[second].tolist()
        if bounds == "image":
            same = (K.cx[first] == K.cx[second], K.cy[first] == K.cy[second])
            assert same == {"ix": (False, True), "iy": (True, False), "cell": (True, True)}[kind]
            assert (K.cell[first], first) < (K.cell[second], second)
    hi = [first > second for kind, _, first, second in s.ties if kind != "cell"]
    assert any(hi) and not all(hi)       # the earlier cell's candidate has the larger index, and the smaller
    # the rotation filter removes the lone bin-9 match and nothing else of the rotation rows
    res, _, _ = ps.reference(s, "framekf", 1.0, 100, 1)
    assert [bool(res.removed[p]) for p in s.rotation] == [False] * 6 + [True]


@pytest.mark.parametrize("pose,bounds", ps.GATE_SCENES + [("exact", "image"), ("size4096", "image")],
                         ids=[f"{p}-{b}" for p, b in ps.GATE_SCENES] + ["exact", "size4096"])
def test_frustum_oracle_agrees_with_float64_reference(pose, bounds):
    """Frame::isInFrustum (the oracle's, ahead of its local-map search) on the
    same scenes: every gate from both sides, bounds inclusive."""
    s = frustum_scene(pose, bounds)
    res = ps.reference_frustum(s)
    got = ps.run_frustum(s)
    assert got[0] == 0
    share = ps.check_frustum(s, res, got)
    print(f"{s.name} frustum: undecided {share:.4f}")
    assert share <= CAP
    if pose == "exact":
        rows = s.exact_rows
        assert all(res.gate[rows[k]] == "win" for k in ("u==max_x", "v==max_y", "u==min_x", "dist==min_dist",
                                                        "dist==max_dist", "ratio==scale"))
        assert res.pred[rows["ratio==scale"]] == 1 and res.pred[rows["dist==min_dist"]] == 0
    elif pose != "size4096":
        order = ps.GATES["frustum"] + ("win",)
        for gate in ps.GATES["frustum"]:
            rej, acc = s.rows[gate]
            assert res.decided[rej] and res.decided[acc] and res.gate[rej] == gate, (gate, res.gate[rej])
            assert order.index(res.gate[acc]) > order.index(gate), (gate, res.gate[acc])
        assert res.pred[s.pred_edges[1]] == ps.NLEV - 1 and res.gate[s.pred_edges[0]] == "dmin"


def frustum_scene(pose, bounds):
    if pose == "exact":
        return ps.built("exact", ps.exact_scene)
    if pose == "size4096":
        return ps.built("size4096", ps.size_scene)
    return ps.scene(pose, bounds)


def test_poses_are_general():
    """All nine entries of R non-zero, no off-diagonal entry equal to its
    transpose, three unequal non-zero translation components."""
    for name, (R, t) in ps.POSES.items():
        T = ps.pose32(R, t)
        R32 = T[:3, :3]
        assert (np.abs(R32) > 1e-2).all(), name
        assert all(abs(R32[i, j] - R32[j, i]) > 1e-2 for i in range(3) for j in range(i)), name
        assert np.allclose(R32.astype(np.float64) @ R32.T.astype(np.float64), np.eye(3), atol=1e-6)
        assert len(set(np.abs(T[:3, 3]).tolist())) == 3 and (T[:3, 3] != 0).all()
    for R in ps.SIM3_R12.values():
        assert (np.abs(R) > 1e-2).all() and all(abs(R[i, j] - R[j, i]) > 1e-2 for i in range(3) for j in range(i))
    # the look-back pose puts many of the other scenes' map points behind the camera
    back = ps.scene("back2.8", "image")
    other = ps.scene("y0.4", "image").mp["pos"].astype(np.float64)
    z = other @ back.R[2] + back.t[2]
    assert (z < 0).mean() > 0.3


def test_exact_edges():
    """u == max_x, v == max_y, u == min_x, dist3D == min_dist / max_dist,
    ratio == a scale factor, a keypoint on the box edge: the oracle and the
    float64 reference take the reference's side of each comparison."""
    s = ps.built("exact", ps.exact_scene)
    rows = s.exact_rows
    for entry, scale, orb, ori in RUNS:
        res, got, share = compare(s, entry, scale if entry != "fuse1" and entry != "kfsim3" else 2.0, orb, ori)
        assert share == 0
        want = dict(s.expect["fuse"])
        if entry == "framekf":
            want.update(s.expect["framekf"])
        for p, c in want.items():
            assert res.idx[p] == c, (entry, p, res.gate[p])
        strict = entry != "framekf"
        assert res.gate[rows["u==max_x"]] == ("umax" if strict else "win")
        assert res.gate[rows["v==max_y"]] == ("vmax" if strict else "win")
        for name in ("u==min_x", "dist==min_dist", "dist==max_dist", "ratio==scale"):
            assert res.gate[rows[name]] == "win", (entry, name, res.gate[rows[name]])


def test_size_edge_scene():
    """A searched keyframe of kMaxFeatures keypoints: winners at indices 0,
    63, 64, 4032 and 4095, in cell 0 and in the highest-numbered cell."""
    s = ps.built("size4096", ps.size_scene)
    K = s.K
    assert K.n == 4096
    for entry, scale, orb, ori in RUNS:
        res, got, share = compare(s, entry, scale, orb, ori)
        assert share == 0
        assert [int(res.idx[p]) for p in s.winners] == [0, 63, 64, 4032, 4095]
        assert all(res.gate[p] == "win" for p in s.winners)
    assert K.cell[4095] == 0 and K.cell[0] == 64 * 48 - 1 == K.cell.max()


@pytest.mark.parametrize("r12,s12", ps.SIM3_CASES)
@pytest.mark.parametrize("bounds", ["image", "undist"])
def test_sim3_oracle_agrees_with_float64_reference(r12, s12, bounds):
    s = ps.built(("sim3", r12, s12, bounds),
                 lambda: ps.sim3_scene(r12, s12, bounds=ps.BOUNDS_IMAGE if bounds == "image" else ps.BOUNDS_UNDIST))
    new, decided, r1, r2 = ps.reference_sim3(s)
    rc, got, n = ps.run_sim3(s)
    share = 1.0 - float(decided.mean())
    print(f"{s.name}: undecided {share:.4f}, found {n}")
    assert rc == 0 and share <= CAP
    assert np.array_equal(got[decided], new[decided])
    if share == 0:
        assert n == int((new >= 0).sum())
    assert n >= 20
    # gate rows of both directions: rejected by that gate, the neighbour passes it
    order = ps.GATES["sim3"] + ("win",)
    for (gate, d), (rej, acc) in s.rows.items():
        res = r1 if d == 1 else r2
        ir, ia = (rej, acc) if d == 1 else (int(s.perm[rej]), int(s.perm[acc]))
        assert res.decided[ir] and res.decided[ia]
        assert res.gate[ir] == gate, (gate, d, res.gate[ir])
        assert order.index(res.gate[ia]) > order.index(gate), (gate, d, res.gate[ia])
        assert new[rej] == -1 and decided[rej]
        if gate not in ("umin", "umax", "vmin", "vmax"):      # (the bound rows' two keypoints share a pixel)
            assert new[acc] == s.perm[acc]
    pr_none, pr_other, pr_victim = s.priors
    assert r1.gate[pr_none] == r1.gate[pr_other] == "skip" and r2.gate[s.perm[pr_victim]] == "skip"
    assert r1.gate[pr_victim] == "win" and new[pr_victim] == -1
    lone, rival = s.lone
    assert r1.idx[lone] == s.perm[lone] and r2.idx[s.perm[lone]] == rival and new[lone] == -1
    # level windows, the clamp and ties, in both directions: the pair's own keypoint wins and the pair agrees
    def side(d, pair):
        """(result of direction d, the pair's point there, its keypoint in the searched keyframe, that keyframe)."""
        return (r1, pair, int(s.perm[pair]), s.K2) if d == 1 else (r2, int(s.perm[pair]), pair, s.K1)

    for (name, d), (main, extras) in s.levels.items():
        res, pt, own, K = side(d, main)
        assert res.decided[pt] and res.gate[pt] == "win" and res.idx[pt] == own, (name, d, res.gate[pt])
        assert new[main] == s.perm[main] and decided[main]
        pred = ps.NLEV - 1 if name == "clamp" else 3
        octs = sorted(int(K.oct[side(d, e)[2]]) for e in extras)
        assert octs == {"lo": [pred - 2], "hi": [pred + 1, pred + 2], "clamp": [pred - 2]}[name]
        assert int(K.oct[own]) == {"lo": pred - 1, "hi": pred, "clamp": pred}[name]
        for e in extras:       # nearer than the winner, and inside the box: only the level window keeps it out
            k = side(d, e)[2]
            assert ps.POP[K.desc[k]].sum() < res.dist[pt]
            assert abs(K.x[k] - K.x[own]) <= 3 and abs(K.y[k] - K.y[own]) <= 3
    assert sorted(s.levels) == [(n_, d) for n_ in ("clamp", "hi", "lo") for d in (1, 2)]
    seen = set()
    for d, kind, hi_first, main, riv in s.ties:
        res, pt, own, K = side(d, main)
        other = side(d, riv)[2]
        assert res.decided[pt] and res.idx[pt] == own and res.dist[pt] == 5 == ps.POP[K.desc[other]].sum()
        assert K.desc[own].tolist() != K.desc[other].tolist()
        assert new[main] == s.perm[main] and decided[main]
        assert (own > other) == hi_first
        if bounds == "image":
            same = (K.cx[own] == K.cx[other], K.cy[own] == K.cy[other])
            assert same == {"ix": (False, True), "iy": (True, False), "cell": (True, True)}[kind]
            assert (K.cell[own], own) < (K.cell[other], other)
        seen.add((d, kind, hi_first))
    assert seen == {(d, k, h) for d in (1, 2) for k, hs in (("ix", (True, False)), ("iy", (True, False)),
                                                             ("cell", (False,))) for h in hs}
    # KF2's indices are a permutation of KF1's: an exchange of the two roles would show
    assert (s.perm != np.arange(s.n)).mean() > 0.9


def test_distinctive_edge_sets():
    p, d, want, names = pd.distinctive_edge_sets()
    best = ref_distinctive(p, d)
    for m, name in enumerate(names):
        N = p[m + 1] - p[m]
        X = np.unpackbits(d[p[m]:p[m + 1]], axis=1).astype(np.int64)
        D = (X[:, None, :] != X[None, :, :]).sum(2)
        med = np.sort(D, 1)[:, (N - 1) // 2]
        assert int(np.argmin(med)) == want[m] == best[m], name
    assert int(D.max()) <= 256
    m = names.index("complement3")
    X = np.unpackbits(d[p[m]:p[m + 1]], axis=1)
    assert (X[0] != X[1]).sum() == 256
