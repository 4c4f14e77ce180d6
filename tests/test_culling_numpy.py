"""The culling restatement (tests/culling_numpy.py) pinned against answers
worked out by hand from the text of src/LocalMapping.cc:190-218 and :539-593,
src/KeyFrame.cc:497-521 and src/MapPoint.cc:93-141, one per rule; the
simplified predicate of orbx.h against the literal loop; the window scenes'
claim that they exercise every rule; and the recorded sequence of
tests/golden/culling_sequence.npz (written by tools/gen_culling_golden.py from
this restatement).  The ABI test at the end needs the library, not a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import culling_cases as kc
import culling_numpy as cu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "culling_sequence.npz"


@pytest.mark.parametrize("name", sorted(kc.rule_cases()))
def test_rule_known_answer(name):
    """Three other observers in scale and two; an observer at o + 1 and one at
    o + 2; the ratio's edges at 10, 20 and 0 points; the order of two
    candidates whose keys are swapped; a point left with two observers that
    flips the next candidate; the stop after max_culls; keyframe 0, a kept
    keyframe, entries that name no member; an erased point in a row; every
    action of MapPointCulling with the found ratio at 1/4, 1/5, inf and NaN."""
    ops, want = kc.rule_cases()[name]
    got, _ = kc.run_restatement(ops)
    kc.check_answers(got, want)


def canon(ops, without=()):
    return [sorted((k, np.asarray(v).tolist()) for k, v in o.items() if k not in without) for o in ops]


def test_order_cases_differ_only_in_the_keys():
    a, b = kc.rule_cases()["order_a_first"][0][:-1], kc.rule_cases()["order_b_first"][0][:-1]   # without the last read
    assert canon(a, ("key",)) == canon(b, ("key",)) and canon(a) != canon(b)


def test_kept_keyframe_changes_nothing():
    ops, _ = kc.rule_cases()["zero_kept_dangling"]
    cut = next(k for k, o in enumerate(ops) if o["op"] == "cull_kf")
    _, w = kc.run_restatement(ops[:cut] + [kc.cull_kf(cand=[0, 1, 7], keep=[1])])
    assert not any(kf.isBad() for kf in w.kfs.values()) and w.kfs[1].mbToBeErased and not w.bad_log
    assert sorted(k.mnId for k in w.mps[10].mObservations) == [0, 1, 2, 3, 4]


def test_erase_keyframe_keeps_its_meaning():
    """The edit erase_keyframe (orbx_covis_erase_keyframe) turns no point bad:
    the two-observer rule belongs to the culling path."""
    ops = kc._world({1: [10], 2: [10], 3: [10]}) + [kc.erase_kf(1)]
    _, w = kc.run_restatement(ops)
    assert not w.mps[10].isBad() and len(w.mps[10].mObservations) == 2 and not w.bad_log


@pytest.mark.parametrize("seed", range(12))
def test_simplified_predicate_equals_the_literal_loop(seed):
    """nMPs and nRedundant as orbx.h states them (no Observations() > 3 gate,
    no break) against the literal loop, on small random worlds: a few
    keyframes over a few points, so that two, three and four observers are all
    common, with octaves that put o + 1 and o + 2 next to each other."""
    rng = np.random.default_rng(seed)
    members, universe, n = int(rng.integers(2, 8)), int(rng.integers(3, 12)), int(rng.integers(1, 9))
    ops = []
    for i in range(members):
        row = rng.choice(universe, size=min(n, universe), replace=False).astype(np.int32)
        row[rng.random(len(row)) < 0.2] = -1
        ops += [kc.add(i + 1, 50 + int(rng.integers(1000)) * 10 + i, row), kc.octaves(i + 1, rng.integers(0, 4, len(row)))]
    ops.append(kc.erase_points(rng.choice(universe, size=1)))
    _, w = kc.run_restatement(ops)
    for c in range(1, members + 1):
        want = cu.predicate_counts(w, c)
        _, w2 = kc.run_restatement(ops)           # a fresh world: the literal call may cull
        r = w2.KeyFrameCulling(-1, cand=[c], keep=[c])
        assert (r["n_mps"][0], r["n_redundant"][0]) == want, (c, r, want)
        assert r["decision"][0] == (2 if want[1] > 0.9 * want[0] else 0)


@pytest.mark.parametrize("members", [64, 65, 130])
def test_window_scene_shows_every_rule(members):
    """On the restatement alone: a cull, a deferred cull, a candidate that
    stays, a point gone bad through a cull, a candidate whose decision depends
    on an earlier cull, and every action of MapPointCulling: the comparison
    with the device cannot pass vacuously."""
    ops, alive = kc.culling_scene(members, members)
    p = kc.scene_properties(ops)
    assert all(p.values()), p
    assert len({o["id"] for o in ops if o["op"] == "add"}) == members and len(alive) < members


def test_resumed_sequence_equals_one_call():
    """max_culls = 1 and resuming with the rest of the list leaves the
    decisions and the state of one unlimited call."""
    ops, _ = kc.culling_scene(65, 65)        # three culls
    cut = next(k for k, o in enumerate(ops) if o["op"] == "cull_kf")
    whole = ops[cut]
    (one,), w1 = (lambda r: ([x for x in r[0] if x["kind"] == "cull_kf"], r[1]))(kc.run_restatement(ops[:cut + 1]))
    _, w2 = kc.run_restatement(ops[:cut])
    r = w2.KeyFrameCulling(whole["cur"], whole["keep"], 1)
    dec, bad, rounds = list(r["decision"]), list(r["bad_points"]), 1
    while r["n_done"] < len(r["cand"]):
        r = w2.KeyFrameCulling(-1, whole["keep"], 1, r["cand"][r["n_done"]:])
        dec += r["decision"]
        bad += r["bad_points"]
        rounds += 1
    assert dec == one["decision"].tolist() and bad == one["bad_points"].tolist() and rounds >= 3
    assert sorted(i for i, k in w1.kfs.items() if k.isBad()) == sorted(i for i, k in w2.kfs.items() if k.isBad())
    for i in w1.kfs:
        assert w1.ordered_list(i) == w2.ordered_list(i)


def test_golden_sequence():
    ops, want = kc.decode(np.load(GOLDEN))
    got, _ = kc.run_restatement(ops)
    kc.assert_same(got, want)
    kinds = {o["op"] for o in ops}
    assert {"add", "octaves", "update", "cull_kf", "cull_mp", "read", "reference"} <= kinds
    assert ops[-1]["op"] == "reference" and [o["op"] for o in ops].index("cull_mp") < len(ops) - 1
    assert len({o["id"] for o in ops if o["op"] == "add"}) <= 16
    assert max(len(o["row"]) for o in ops if o["op"] == "add") <= 70
    assert all(list(kc.scene_properties(ops).values())) and GOLDEN.stat().st_size < 64 * 1024
    ops2, want2 = kc.decode(kc.encode(*kc.decode(np.load(GOLDEN))))
    assert canon(ops2) == canon(ops)
    kc.assert_same(want2, want)
    fresh = kc.golden_ops()
    assert canon(fresh) == canon(ops)


def test_abi_exports_the_culling_calls():
    """Revision 15 of the ABI: the three entry points are exported, each
    refuses a null context or object before touching a device, and the
    argument struct is laid out as the Python binding mirrors it."""
    import orb_slam_amd as ox
    text = (ROOT / "include" / "orbx.h").read_text()
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 15
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 15
    assert lib.orbx_covis_set_octaves(None, None, 0, 0, None) == -1
    assert lib.orbx_covis_cull_keyframes(None, None, None) == -1
    assert lib.orbx_covis_cull_points(None, None, 0, 0, None, None, None, None, None) == -1
    assert ctypes.sizeof(ox.CovisCull) == 80
    f = ox.CovisCull
    assert (f.cur.offset, f.n_keep.offset, f.keep.offset, f.max_culls.offset, f.cand_cap.offset) == (0, 4, 8, 16, 20)
    assert (f.cand.offset, f.n_cand.offset, f.n_done.offset, f.n_mps.offset, f.n_redundant.offset) == (24, 32, 36, 40, 48)
    assert (f.decision.offset, f.bad_points.offset, f.bad_cap.offset, f.n_bad.offset) == (56, 64, 72, 76)
    for name in ("set_octaves", "cull_keyframes", "cull_points"):
        assert callable(getattr(ox.CovisibilityMap, name))
