"""The hand-built scenes of tests/bow_scenes.py on the CPU: for every scene
and mode the expected vector written in the scene, the numpy restatement
(test_bow_numpy.search_by_bow / search_for_triangulation) and the oracle
(oracle/ref_bow.cpp) must be equal, match vector and count.  This pins the
scenes before the device sees them (test_bow_scenes_gpu.py).

The builder asserts its own conditions while a scene is made: every pair
inside a node at its stated Hamming distance and every other one farther than
100 bits; around each epipolar threshold at least one candidate passing and
one failing; the rotation rows in the bins the scene names.
"""
import numpy as np
import pytest

import bow_scenes as bs
from test_bow_numpy import search_by_bow, search_for_triangulation
from test_bow_oracle import run_ref


def restated(S):
    a1, a2 = S["keep"]
    if S["mode"] == 2:
        return search_for_triangulation(a1, a2, S["F12"], S["sigma2"], S["check_ori"])
    return search_by_bow(a1, a2, S["nnratio"], S["check_ori"], kf_kf=S["mode"] == 1)


def wrong_rows(S, got):
    """Labels of the rows whose KF1 feature got another answer than the scene states."""
    got = np.asarray(got)
    bad = []
    for label, i1, i2 in S["rows"]:
        if S["mode"] == 0:
            ok = (got[i2] == i1) if i2 >= 0 else not np.any(got == i1)
        else:
            ok = got[i1] == i2
        if not ok:
            bad.append(label)
    return bad


@pytest.mark.parametrize("name,mode", bs.CASES, ids=[f"{n}-m{m}" for n, m in bs.CASES])
def test_scene_expected_numpy_oracle_agree(name, mode):
    S = bs.scene(name, mode)
    got, n = restated(S)
    assert not wrong_rows(S, got), ("numpy", wrong_rows(S, got))
    assert np.array_equal(got, S["want"]) and n == S["n_want"]
    ro, rn = run_ref(mode, S, S["nnratio"], S["check_ori"])
    assert not wrong_rows(S, ro), ("oracle", wrong_rows(S, ro))
    assert np.array_equal(ro.astype(np.int64), S["want"]) and rn == S["n_want"]


def test_every_row_is_stated_once():
    """Each KF1 feature of a scene belongs to exactly one row, and each mode
    of each gate has rows on both sides (a match and a refusal)."""
    for name, mode in bs.CASES:
        S = bs.scene(name, mode)
        i1s = [r[1] for r in S["rows"]]
        assert len(set(i1s)) == len(i1s), name
        if not name.startswith("walk"):          # the walk scenes add features of unshared nodes
            assert sorted(i1s) == list(range(S["V1"].n)), name
    for mode in (0, 1, 2):
        both = [bs.scene(n, m) for n, m in bs.CASES if m == mode]
        assert any(r[2] >= 0 for S in both for r in S["rows"]) and any(r[2] < 0 for S in both for r in S["rows"])


def test_node_layouts():
    """The layouts the scenes promise: a descending node, empty nodes on
    either side, shared ids at both ends of both vectors."""
    a2 = bs.scene("tri_order", 2)["keep"][1]
    seg = a2["feat"][a2["ptr"][0]:a2["ptr"][1]]
    assert len(seg) == 3 and np.all(np.diff(seg) < 0)
    for n in (4, 5, 9):
        a1, a2 = bs.scene(f"walk{n}", 1)["keep"]
        common = np.intersect1d(a1["ids"], a2["ids"])
        assert len(common) == n
        assert a1["ids"][0] == a2["ids"][0] == common[0] and a1["ids"][-1] == a2["ids"][-1] == common[-1]
        assert len(a1["ids"]) > n and len(a2["ids"]) > n
    a1, a2 = bs.scene("walk9", 1)["keep"]
    assert np.any(np.diff(a1["ptr"]) == 0) and np.any(np.diff(a2["ptr"]) == 0)
    for n in (0, 1):
        a1, a2 = bs.scene(f"walk{n}", 1)["keep"]
        assert len(np.intersect1d(a1["ids"], a2["ids"])) == n


def test_batch_join_keeps_each_scene():
    """batch_jobs' joined KF1 against one scene's KF2 gives that scene's
    answer at its offset and nothing elsewhere (numpy restatement)."""
    scenes = [bs.scene(n, 2) for n in ("distance", "taken", "rot_mid", "walk5")]
    V1, keep1, jobs = bs.batch_jobs(scenes)
    for S, first in jobs:
        got, n = search_for_triangulation(keep1, S["keep"][1], S["F12"], S["sigma2"], S["check_ori"])
        want = np.full(V1.n, -1, np.int64)
        want[first:first + len(S["want"])] = S["want"]
        assert np.array_equal(got, want) and n == S["n_want"], S["name"]
