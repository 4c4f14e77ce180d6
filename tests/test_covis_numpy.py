"""The covisibility restatement (tests/covis_numpy.py) pinned against answers
worked out by hand from the text of src/KeyFrame.cc:126-211, :332-421,
:510-521 and src/Tracking.cc:764-865, one per rule, against scenes whose
generator shows that they exercise every rule, and against the recorded
sequence of tests/golden/covis_sequence.npz (written by
tools/gen_covis_golden.py from this restatement: a change of its results shows
up here).  The ABI test at the end needs the library, not a GPU."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import covis_cases as cc
import covis_numpy as cn

GOLDEN = Path(__file__).resolve().parent / "golden" / "covis_sequence.npz"


@pytest.mark.parametrize("name", sorted(cc.rule_cases()))
def test_rule_known_answer(name):
    """Rules 1 to 9 of the list: the fallback entry and its tie, the order of
    equal weights, AddConnection with the same and with a new weight, the
    empty counter, a point twice in the frame, the 80 limit at 79 to 82
    voters, stale entries and place 11, first-occurrence order with an erased
    point."""
    ops, want = cc.rule_cases()[name]
    got, _ = cc.run_restatement(ops)
    cc.check_answers(got, want)


@pytest.mark.parametrize("v,n", [(79, 81), (80, 81), (81, 81), (82, 82)])
def test_limit_counts(v, n):
    ops, (nv, lk) = cc.limit_case(v)
    r = cc.run_restatement(ops)[0][-1]
    assert (r["head"][0], len(r["local_kf"])) == (v, n) and r["local_kf"].tolist() == lk


def test_covisibles_by_weight_quirk():
    """src/KeyFrame.cc:194-196: upper_bound with a > b finds the first weight
    below w; when every weight is >= w it returns end() and the function an
    empty vector, although every keyframe qualifies."""
    kf = cn.KeyFrame(0, 1, [])
    a, b, c = (cn.KeyFrame(i, 10 + i, []) for i in (1, 2, 3))
    assert kf.GetCovisiblesByWeight(1) == []            # no connections
    kf.mvpOrderedConnectedKeyFrames, kf.mvOrderedWeights = [a, b, c], [5, 3, 2]
    assert kf.GetCovisiblesByWeight(4) == [a]
    assert kf.GetCovisiblesByWeight(3) == [a, b]        # 3 > 2 first at place 2
    assert kf.GetCovisiblesByWeight(2) == []            # the quirk: all of them are >= 2
    assert kf.GetCovisiblesByWeight(1) == []
    assert kf.GetCovisiblesByWeight(6) == []            # none is: begin(), an empty range
    assert kf.GetCovisiblesByWeight(5) == [a]


@pytest.mark.parametrize("members", [64, 65, 130, 200])
def test_window_scene_shows_every_rule(members):
    """The generator's claim, on the restatement alone: a list with entries
    below the threshold, a fallback list, a weight tie, a neighbour pass that
    appends and a stale entry."""
    p = cc.scene_properties(cc.window_scene(members, members))
    assert all(p.values()), p


def test_stored_lists_equal_derived_lists():
    """The library derives the ordered list from the weights, a flag and a
    threshold; the reference stores it.  The derivation, restated here next to
    the stored form, over every keyframe of a scene after every operation."""
    ops = cc.window_scene(5, 40)
    w = cn.World()
    filt, th_of = {}, {}

    def derived(kf):
        e = [(wt, k) for k, wt in kf.mConnectedKeyFrameWeights.items()]
        if filt.get(kf.mnId):
            keep = [x for x in e if x[0] >= th_of[kf.mnId]]
            if not keep and e:
                top = max(x[0] for x in e)
                keep = [min((x for x in e if x[0] == top), key=lambda x: x[1].key)]
            e = keep
        e.sort(key=lambda x: (x[0], x[1].key), reverse=True)
        return [k.mnId for _, k in e], [wt for wt, _ in e]

    for o in ops:
        if o["op"] == "add":
            w.add_keyframe(o["id"], o["key"], o["row"])
        elif o["op"] == "set":
            w.set_matches(o["id"], o["idx"], o["mp"])
        elif o["op"] == "erase_points":
            w.erase_points(o["ids"])
        elif o["op"] == "erase_kf":
            for k in w.kfs[o["id"]].mConnectedKeyFrameWeights:
                if w.kfs[o["id"]] in k.mConnectedKeyFrameWeights:
                    filt[k.mnId] = 0
            w.erase_keyframe(o["id"])
        elif o["op"] == "update":
            for i in o["ids"]:
                before = {k.mnId: dict(k.mConnectedKeyFrameWeights) for k in w.kfs.values()}
                u, _ = w.kfs[i].UpdateConnections(o["th"])
                if u:
                    filt[i], th_of[i] = 1, o["th"]
                    for k in w.kfs.values():
                        if k.mnId != i and k.mConnectedKeyFrameWeights != before[k.mnId]:
                            filt[k.mnId] = 0
        else:
            continue
        for kf in w.kfs.values():
            if not kf.isBad():
                assert derived(kf) == w.ordered_list(kf.mnId), (o["op"], kf.mnId)


def test_golden_sequence():
    d = np.load(GOLDEN)
    ops, want = cc.decode(d)
    got, _ = cc.run_restatement(ops)
    cc.assert_same(got, want)
    assert all(cc.scene_properties(ops).values())
    ids = {o["id"] for o in ops if o["op"] == "add"}
    assert len(ids) <= 16 and max(len(o["row"]) for o in ops if o["op"] == "add") <= 80
    assert GOLDEN.stat().st_size < 64 * 1024


def test_encode_decode_round_trip():
    ops = cc.random_ops(3, 4, 9)
    res, _ = cc.run_restatement(ops)
    ops2, res2 = cc.decode(cc.encode(ops, res))
    cc.assert_same(res2, res)
    cc.assert_same(cc.run_restatement(ops2)[0], res)


def test_abi_exports_the_covisibility_map():
    """Revision 14 of the ABI: every orbx_covis_* entry point is exported, and
    each refuses a null context or object before touching a device."""
    import orb_slam_amd as ox
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 14
    out = ctypes.c_void_p()
    n = ctypes.c_int()
    assert lib.orbx_covis_create(None, 8, 8, 8, ctypes.byref(out)) == -1
    assert lib.orbx_covis_size(None) == -1
    assert lib.orbx_covis_clear(None, None) == -1
    assert lib.orbx_covis_add_keyframe(None, None, 0, 1, 0, None) == -1
    assert lib.orbx_covis_set_matches(None, None, 0, 0, None, None) == -1
    assert lib.orbx_covis_erase_points(None, None, 0, None) == -1
    assert lib.orbx_covis_erase_keyframe(None, None, 0) == -1
    assert lib.orbx_covis_update_connections(None, None, 0, None, 15, None, None) == -1
    assert lib.orbx_covis_connections(None, None, 0, 0, None, None, 0, ctypes.byref(n)) == -1
    assert lib.orbx_covis_update_reference(None, None, None) == -1
    lib.orbx_covis_destroy(None)   # no-op
    assert ctypes.sizeof(ox.CovisReference) == 64
    assert ox.CovisReference.local_kf.offset == 24 and ox.CovisReference.local_mp.offset == 48
