"""The KeyFrameDatabase restatement (tests/kfdb_numpy.py) pinned against
properties that do not depend on it, against answers worked out by hand for
every rule of src/KeyFrameDatabase.cc:75-308, and against the recorded query
sequence of tests/golden/kfdb_queries.npz (written by tools/gen_kfdb_golden.py
from this restatement: a change of its results shows up here)."""
from pathlib import Path

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_numpy as kn

GOLDEN = Path(__file__).resolve().parent / "golden" / "kfdb_queries.npz"


def test_score_is_one_minus_half_l1_distance():
    """L1Scoring::score = 1 - 0.5 * ||v - w||_1 for L1-normalised vectors."""
    rng = np.random.default_rng(1)
    for n1, n2 in [(1, 1), (5, 9), (63, 64), (257, 100), (300, 300)]:
        a, b = kc.rand_bow(rng, n1, 400), kc.rand_bow(rng, n2, 400)
        va, vb = np.zeros(400), np.zeros(400)
        va[a[0]], vb[b[0]] = a[1], b[1]
        s = kn.l1_score(dict(zip(a[0].tolist(), a[1])), dict(zip(b[0].tolist(), b[1])))
        assert abs(s - (1 - 0.5 * np.abs(va - vb).sum())) < 1e-12


def test_score_of_dyadic_values_is_the_sum_of_minima():
    rng = np.random.default_rng(2)
    for _ in range(20):
        n = int(rng.integers(1, 40))
        wa = np.sort(rng.choice(60, n, replace=False))
        wb = np.sort(rng.choice(60, n, replace=False))
        a = dict(zip(wa.tolist(), (rng.integers(1, 64, n) / 4096.0).tolist()))
        b = dict(zip(wb.tolist(), (rng.integers(1, 64, n) / 4096.0).tolist()))
        want = sum(min(a[w], b[w]) for w in a if w in b)
        assert kn.l1_score(a, b) == want


def test_score_without_common_words_is_zero():
    assert kn.l1_score({1: 1.0}, {2: 1.0}) == 0.0
    assert kn.l1_score({}, {2: 1.0}) == 0.0


@pytest.mark.parametrize("name", sorted(kc.rule_cases()))
def test_rule_known_answer(name):
    ops, capacity, want = kc.rule_cases()[name]
    got = kc.run_restatement(ops, capacity)
    assert [r["cand"].tolist() for r in got] == want


def test_rule_details():
    """The intermediate values the known answers rest on."""
    c = kc.rule_cases()
    r = kc.run_restatement(*c["threshold_075"][:2])[0]
    assert r["acc"][0] == 1.0 and r["acc"][1] == 0.75 and r["n_scored"] == 2
    r = kc.run_restatement(*c["loop_si_equals_min_score"][:2])[0]
    assert r["best"][1] == 1 and r["acc"][1] == 0.5 and r["min_score_used"] == 0.5   # 1 entered lScoreAndMatch
    r = kc.run_restatement(*c["duplicates_keep_first"][:2])[0]
    assert r["acc"][5] == 3.0 and r["best"][5] == 5 and r["pos"][[5, 2, 7]].tolist() == [0, 1, 2]
    r = kc.run_restatement(*c["same_best_once"][:2])[0]
    assert r["best"][[1, 6, 4]].tolist() == [4, 4, 4] and r["acc"][1] == 1.75
    r1, r2 = kc.run_restatement(*c["reloc_state"][:2])
    assert r1["score"][1] == 0.5 and r2["score"][1] == 0.5 and r2["words"][1] == 1   # kept, not scored again
    assert r2["acc"][0] == 1.0 and r2["best"][0] == 0 and r2["score"][3] == 0.0 and r2["n_scored"] == 1
    r = kc.run_restatement(*c["loop_exclusion"][:2])[0]
    assert r["max_common_words"] == 5 and r["min_score_used"] == 0.5 and r["pos"][0] == -1
    assert r["acc"][2] == 0.625 and r["n_sharing"] == 2
    r = kc.run_restatement(*c["neighbour_rows"][:2])
    assert r[0]["acc"][0] == 1.75 and r[0]["best"][0] == 9 and r[2]["acc"][0] == 0.75


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("M", sorted(kc.GATE_MIN))
def test_word_gate(M, loop):
    """minCommonWords = (int)(M * 0.8f); exactly that many words is rejected, one more is kept."""
    assert int(np.float32(M) * np.float32(0.8)) == kc.GATE_MIN[M]
    ops, capacity, scored = kc.gate_case(M, loop)
    r = kc.run_restatement(ops, capacity)[0]
    mc = kc.GATE_MIN[M]
    assert r["max_common_words"] == M and r["n_scored"] == scored
    if mc >= 1:
        assert r["words"][1] == mc and r["best"][1] == -1 and r["pos"][1] >= 0
    if mc + 1 < M:
        assert r["words"][2] == mc + 1 and r["best"][2] >= 0


def test_golden_sequence():
    ops, want, capacity = kc.decode(np.load(GOLDEN))
    assert sum(o["op"] in ("reloc", "loop") for o in ops) == len(want) >= 6
    assert any(len(r["cand"]) > 1 for r in want)
    kc.assert_same(kc.run_restatement(ops, capacity), want)


def test_encode_round_trip():
    ops, capacity = kc.random_ops(5, 6, [3, 0, 7], 20)
    res = kc.run_restatement(ops, capacity)
    ops2, res2, cap2 = kc.decode(kc.encode(ops, res, capacity))
    assert cap2 == capacity
    kc.assert_same(kc.run_restatement(ops2, cap2), res)
    kc.assert_same(res2, res)
