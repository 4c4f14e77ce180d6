"""The hand-built scenes of tests/area_scenes.py on the CPU: each reaches
the form of k_area_lists / k_area_replay it is named for, and the oracle,
the numpy restatements and the construction agree on its result.

The coverage test is a white-box mirror: area_scenes.lds_plan restates
area_replay_lds and launch_area_search's q_lds / ent_cap computation
(orbx_search.hip), entry_offsets the replay's staging scan, rounds() its
claim rounds over preference lists computed with the numpy Grid.  When those
kernels change their layout or limits the mirror has to follow; the GPU test
(test_area_paths_gpu.py) checks the mirror's round counts against the
device's counters.

The local-map search has no numpy restatement: there the oracle is compared
with the mirror's own greedy loop over the lists and with the construction.
"""
import numpy as np
import pytest

import area_scenes as A
from oracle_lib import load
from test_match_numpy import window_search
from test_proj_numpy import motion_search, pair_search


def oracle_fns():
    import ctypes
    L = load()
    L.orbx_ref_search_local_map.argtypes = [ctypes.c_void_p]
    return {"window": L.orbx_ref_window_search, "pair": L.orbx_ref_search_by_projection_pair,
            "motion": L.orbx_ref_search_by_projection_motion, "local": L.orbx_ref_search_by_projection_local,
            "local_map": L.orbx_ref_search_local_map}


# general poses (pose_scenes.POSES) for the scenes that are run posed: the smallest chain scene, the ties
# and the extras.  The posed local kind is another entry point than the unposed one: isInFrustum and the
# search behind it (orbx_search_local_map), band 0 at predicted level 1; its id says so.
POSED = [(name, kind, pose) for name in ("chain10x3", "ties", "extras") for kind in ("pair", "motion", "local")
         for pose in ("y0.4", "axis0.9")]
POSED_IDS = [f"{name}-{'local_map_via_frustum' if kind == 'local' else kind}-{pose}" for name, kind, pose in POSED]


def posed_scene(name, kind, pose):
    """The scene under a general pose and its own mirror, built once."""
    import pose_scenes as ps
    key = (name, kind, pose)
    if key not in A._built:
        s = A.scene(name, kind)[0].posed(*ps.POSES[pose])
        A._built[key] = (s, A.mirror(s))
    return A._built[key]


def classes(m, ids):
    return sorted({int(m["cnt"][i]) for i in ids})


@pytest.mark.parametrize("kind", A.KINDS)
def test_scenes_reach_the_forms_they_are_named_for(kind):
    sc = {name: A.scene(name, kind) for name, (kinds, _) in A.CATALOGUE.items() if kind in kinds}
    # LDS plan of the sizes the issue names, and the limit between the two
    n = A.lds_limit()
    assert A.lds_plan(n, n) == (1, A.K_REPLAY_ENTRIES) and A.lds_plan(n + 1, n + 1)[0] == 0
    assert A.lds_plan(4096, 1536) == (0, A.K_REPLAY_ENTRIES)
    q_lds, ent_cap = A.lds_plan(A.K_MAX_FEATURES, A.K_MAX_FEATURES)
    assert q_lds == 0 and 64 <= ent_cap < A.K_REPLAY_ENTRIES
    # the fixed part always fits at or below kMaxFeatures: ORBX_ERR_UNSUPPORTED is out of reach
    assert all(A.lds_plan(a, b) is not None for a in (1, A.K_MAX_FEATURES) for b in (1, A.K_MAX_FEATURES))

    # chains: rounds and fallback; list forms of the three-chain jobs
    for name, n_chain in (("chain10x3", 10), ("chain24x3", 24), ("chain40x3", 40)):
        s, m = sc[name]
        assert (m["rounds"], m["fallback"]) == ((n_chain + 1, 0) if n_chain < 24 else (A.K_MAX_ROUNDS, 1)), name
        assert [classes(m, s.tags[f"chain{b}"]) for b in range(3)] == [[50], [100], [150]]
    s, m = sc["chain23"]
    assert (m["rounds"], m["fallback"]) == (24, 0) and classes(m, s.tags["chain"]) == [43]
    s, m = sc["chain24"]
    assert (m["rounds"], m["fallback"]) == (24, 1) and classes(m, s.tags["chain"]) == [44]
    s, m = sc["extras"]
    assert (m["rounds"], m["fallback"]) == (11, 0)
    assert classes(m, s.tags["chain"]) == [-1, 32] and (s.kind == "window" or s.assigned.sum() == 2)
    if kind in A.WM:
        s, m = sc["rotation"]
        assert (m["rounds"], m["fallback"]) == (24, 0) and s.check_ori == 1
    if kind == "pair":
        s, m = sc["ratio"]
        assert (m["rounds"], m["fallback"]) == (len(A.RATIO_DIST) + 1, 0)

    # ties: equal distances at the head of the list (or behind a nearer one), in all list forms
    s, m = sc["ties"]
    for tag, lo, hi in (("tie", 2, 64), ("tie_mid", 65, A.K_AREA_CAP), ("tie_long", A.K_AREA_CAP + 1, 4096)):
        for i in s.tags[tag]:
            idx, dist = m["lists"][i]
            assert lo <= len(idx) <= hi
            k = int(np.argmax(dist == 5))
            a, b = int(idx[k]), int(idx[k + 1])
            assert dist[k + 1] == 5 and dist[k + 2] > A.TH_HIGH
            ca, cb = (int(round(float(s.k2["x"][j]) / 10)) for j in (a, b))
            assert ca < cb, "different cells: cell order decides"
    orders = {(int(m["lists"][i][0][0]) > int(m["lists"][i][0][1])) for i in s.tags["tie"][:4]}
    assert orders == {True, False}, "index order agrees with cell order in one case and not in the other"
    assert m["lists"][s.tags["tie"][4]][1][:3].tolist() == [2, 5, 5]

    # boundaries: exact counts
    s, m = sc["boundaries"]
    assert [int(m["cnt"][s.tags[f"count{c}"][0]]) for c in A.BOUNDARY_COUNTS] == list(A.BOUNDARY_COUNTS)

    # budget: the short lists pass the LDS budget; one chain astride it, one past it
    s, m = sc["budget"]
    assert m["q_lds"] == 1 and m["cnt"][m["short"]].sum() > m["ent_cap"] == A.K_REPLAY_ENTRIES
    assert sorted(set(m["in_lds"][s.tags["chain_a"]].tolist())) == [False, True]
    assert not m["in_lds"][s.tags["chain_b"]].any()
    assert (m["rounds"], m["fallback"]) == (7, 0)

    # the large scenes: q_lds, ent_cap, nq over one block, every list form, global short lists
    for name, plan in (("qglob_full", (0, 8192)), ("qglob_shrunk", (0, ent_cap)), ("lds_max", (1, 8192))):
        s, m = sc[name]
        assert (m["q_lds"], m["ent_cap"]) == plan, name
        assert s.nq > A.K_REPLAY_THREADS
        assert [classes(m, s.tags[f"chain{b}"]) for b in range(3)] == [[32], [100], [150]]
        assert (m["short"] & ~m["in_lds"]).sum() > 1000 and (m["short"] & m["in_lds"]).sum() > 100
        assert (m["rounds"], m["fallback"]) == (13, 0)
        assert all(len(m["lists"][i][0]) > 64 for t in ("tie_mid", "tie_long") for i in s.tags[t])
    assert (sc["lds_max"][0].nq, sc["lds_max"][0].n2) == (n, n)

    # edge sizes
    for nq, n2 in A.EDGES:
        s, m = sc[f"edge{nq}x{n2}"]
        assert (s.nq, s.n2) == (nq, n2) and m["fallback"] == 0
    assert sc["edge0x40"][1]["rounds"] == 1
    assert sc["edge17x40"][0].nq % 16 != 0 and sc["edge1025x300"][0].nq > A.K_REPLAY_THREADS


@pytest.mark.parametrize("name,kind", A.CASES)
def test_references_agree(name, kind):
    s, m = A.scene(name, kind)
    rc, om, on = A.search(s, oracle_fns())
    assert rc == 0
    # by construction, independent of both references
    for q, c in s.expect.items():
        want = np.nonzero(om == q)[0].tolist()
        assert want == ([c] if c >= 0 else []), (q, c, want)
    if "chain" in name:
        assert len(s.expect) >= 10 and sum(c >= 0 for c in s.expect.values()) >= 10
    # the mirror's greedy loop over the lists
    mm, mn = A.expected_matches(s, m["state"])
    assert mn == on and np.array_equal(mm, om)
    # the numpy restatements
    if kind == "window":
        nm, nn = window_search(s.k1, s.d1, s.k2, s.d2, s.valid, A.W, A.H, A.R0, 0, 2147483647, s.nnratio, s.check_ori)
    elif kind == "pair":
        nm, nn = pair_search(s.k1, s.d1, s.k2, s.d2, s.xyz, s.valid, s.assigned, A.T_IDENTITY, A.R0, s.nnratio)
    elif kind == "motion":
        nm, nn = motion_search(s.k2, s.d2, s.k1, s.d1, s.xyz, s.valid, s.assigned, A.T_IDENTITY, s.th_motion,
                               s.check_ori)
    else:
        return
    assert nn == on and np.array_equal(nm, om)


@pytest.mark.parametrize("name,kind,pose", POSED, ids=POSED_IDS)
def test_references_agree_under_a_general_pose(name, kind, pose):
    """The same scenes seen from a rotated and translated camera: every entry
    of Rcw is used, and construction, oracle, mirror and numpy restatement
    still agree."""
    s, m = posed_scene(name, kind, pose)
    base, bm = A.scene(name, kind)
    R = s.T.reshape(3, 4)[:, :3]
    assert (np.abs(R) > 1e-2).all() and all(abs(R[i, j] - R[j, i]) > 1e-2 for i in range(3) for j in range(i))
    # every query still projects to its centre, so the lists are the unposed scene's
    u, v, _ = s.centres()
    if kind != "local":
        assert np.abs(u - base.k1["x"]).max() < 1e-3 and np.abs(v - base.k1["y"]).max() < 1e-3
    for a, b in zip(m["lists"], bm["lists"]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a[0], b[0]))
    assert s.expect == base.expect and (m["rounds"], m["fallback"]) == (bm["rounds"], bm["fallback"])
    rc, om, on = A.search(s, oracle_fns())
    assert rc == 0
    for q, c in s.expect.items():
        want = np.nonzero(om == q)[0].tolist()
        assert want == ([c] if c >= 0 else []), (q, c, want)
    assert sum(c >= 0 for c in s.expect.values()) >= 6
    mm, mn = A.expected_matches(s, m["state"])
    assert mn == on and np.array_equal(mm, om)
    if kind == "pair":
        nm, nn = pair_search(s.k1, s.d1, s.k2, s.d2, s.xyz, s.valid, s.assigned, s.T, A.R0, s.nnratio)
    elif kind == "motion":
        nm, nn = motion_search(s.k2, s.d2, s.k1, s.d1, s.xyz, s.valid, s.assigned, s.T, s.th_motion, s.check_ori)
    else:
        # isInFrustum saw every valid point, at its centre and at the level the scene asks for
        in_view, proj, pred = s.frustum
        assert np.array_equal(in_view != 0, s.valid != 0) and np.array_equal(pred[s.valid != 0], s.pred[s.valid != 0])
        assert np.abs(proj[s.valid != 0] - s.proj[s.valid != 0]).max() < 1e-3
        return
    assert nn == on and np.array_equal(nm, om)


def test_track_chain_passes_the_round_limit():
    """The chain built into a tracked frame's motion search (the GPU test
    runs it through orbx_track_frame): 24 queries among natural keypoints,
    query k taking candidate k, one round too many for the parallel replay;
    the frame without it converges."""
    import ctypes

    import track_data as td
    from oracle_lib import RefExtractor, ptr
    import orb_slam_amd as ox
    seed, shift, err = A.TRACK_CASE
    last, cur = td.images(A.W, A.H, shift, seed)
    ex = RefExtractor(1000)
    (kl, dl), (kc, dc) = ex(last), ex(cur)
    scene = td.make_scene(kl, dl, seed)
    Tpred = td.pose_x((shift + err) * td.DEPTH / float(td.CAM[0]))
    plain = A.mirror(A.TrackMotion(kl, dl, kc, dc, scene, Tpred))
    assert plain["fallback"] == 0 and plain["rounds"] < 12
    kl2, dl2, scene2, path = A.track_chain(kl, dl, kc, dc, scene, Tpred)
    s = A.TrackMotion(kl2, dl2, kc, dc, scene2, Tpred)
    m = A.mirror(s)
    assert m["fallback"] == 1 and len(path) == len(set(path)) == 24
    assert m["state"][:24].tolist() == path and (m["cnt"][:24] <= 64).all()
    # the oracle's motion search, before its rotation filter can only remove
    mr, nr = np.zeros(len(kc), np.int32), ctypes.c_int()
    C, Lv = ox.frame_view(kc, dc, A.W, A.H), ox.frame_view(kl2, dl2, A.W, A.H)
    assert load().orbx_ref_search_by_projection_motion(ctypes.byref(C), ctypes.byref(Lv), ptr(s.X), ptr(s.valid),
                                                       ptr(s.assigned), ptr(np.ascontiguousarray(Tpred)), ptr(A.CAM),
                                                       A.TRACK_TH, 0, ptr(mr), ctypes.byref(nr)) == 0
    assert mr[path].tolist() == list(range(24))
    s.check_ori = 0
    mm, mn = A.expected_matches(s, m["state"])
    assert mn == nr.value and np.array_equal(mm, mr)


def test_ratio_rejects_one_member_and_the_rest_move_up():
    s, m = A.scene("ratio", "pair")
    odd = s.tags["chain_odd"][0]
    members = s.tags["chain"]
    assert members[1] < odd < members[2] and s.expect[odd] == -1
    assert all(s.expect[q] >= 0 for q in members) and s.nnratio == np.float32(0.6)
    # without the ratio the odd query would take a candidate and shift the members behind it
    idx, dist = m["lists"][odd]
    assert dist[2] <= A.TH_HIGH
