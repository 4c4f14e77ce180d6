"""Operation sequences for the keyframe database tests: builders, the runner
that plays one on the restatement (tests/kfdb_numpy.py), the runner that plays
it on the device, and the array form the golden file stores.

An operation is a dict: {"op": "add", "id", "words", "values"} | {"op":
"erase", "id"} | {"op": "clear"} | {"op": "neigh", "id", "ids"} | {"op":
"reloc", "words", "values"} | {"op": "loop", "words", "values", "min_score",
"ref", "exclude"}.  Every query yields a result dict: cand, max_common_words,
n_sharing, n_scored, min_score_used and the five taps."""
import numpy as np

import kfdb_numpy as kn

TAPS = ("words", "score", "acc", "best", "pos")
CODES = ("add", "erase", "clear", "neigh", "reloc", "loop")


def rand_bow(rng, n, universe):
    """n distinct words of range(universe), ascending, random L1-normalised values."""
    w = np.sort(rng.choice(universe, size=n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 1e-3
    return w, v / v.sum() if n else v


def add(i, bow):
    return dict(op="add", id=int(i), words=np.asarray(bow[0], np.uint32), values=np.asarray(bow[1], np.float64))


def erase(i):
    return dict(op="erase", id=int(i))


def neigh(i, ids):
    return dict(op="neigh", id=int(i), ids=[int(x) for x in ids])


def reloc(bow):
    return dict(op="reloc", words=np.asarray(bow[0], np.uint32), values=np.asarray(bow[1], np.float64))


def loop(bow, min_score=1.0, ref=(), exclude=()):
    return dict(op="loop", words=np.asarray(bow[0], np.uint32), values=np.asarray(bow[1], np.float64),
                min_score=float(min_score), ref=[int(x) for x in ref], exclude=[int(x) for x in exclude])


def random_ops(seed, members, lengths, universe, n_queries=4, capacity=None):
    """`members` keyframes with BowVector lengths cycled from `lengths`, added
    in a shuffled id order with random neighbour rows, one erased and added
    again, then alternating relocalisation and loop queries."""
    rng = np.random.default_rng(seed)
    capacity = capacity or max(members + 3, 4)
    ids = rng.permutation(capacity)[:members]
    ops = [add(i, rand_bow(rng, min(lengths[k % len(lengths)], universe), universe)) for k, i in enumerate(ids)]
    for i in ids:
        k = int(rng.integers(0, 11))
        ops.append(neigh(i, rng.choice(capacity, size=min(k, capacity), replace=False)))
    qlens = [min(l, universe) for l in lengths]
    for k in range(n_queries):
        bow = rand_bow(rng, qlens[k % len(qlens)], universe)
        if k == 1 and members >= 3:
            ops += [erase(ids[1]), add(ids[1], rand_bow(rng, min(lengths[-1], universe), universe)),
                    neigh(ids[1], [ids[0], ids[2]])]
        if k % 2 == 0:
            ops.append(reloc(bow))
        else:
            ne = int(rng.integers(0, max(members // 3, 1) + 1))
            ops.append(loop(bow, 1.0, ref=rng.choice(capacity, size=min(4, capacity), replace=False),
                            exclude=rng.choice(capacity, size=min(ne, capacity), replace=False)))
    return ops, capacity


def run_restatement(ops, capacity):
    db = kn.KeyFrameDatabase()
    out = []
    for o in ops:
        k = o["op"]
        if k == "add":
            db.add(kn.KeyFrame(o["id"], o["words"], o["values"]))
        elif k == "erase":
            db.erase(db.kfs[o["id"]])
        elif k == "clear":
            db.clear()
        elif k == "neigh":
            db.kfs[o["id"]].neighbours = list(o["ids"])
        else:
            q = db.new_query(o["words"], o["values"])
            is_loop = k == "loop"
            if is_loop:
                ms = db.detect_loop_min_score(q, [db.kfs[i] for i in o["ref"] if i in db.kfs], o["min_score"])
                cand = db.DetectLoopCandidates(q, ms, [db.kfs[i] for i in o["exclude"] if i in db.kfs])
            else:
                ms = np.float32(0)
                cand = db.DetectRelocalisationCandidates(q)
            r = dict(cand=np.array([c.mnId for c in cand], np.int32), max_common_words=db.last["maxCommonWords"],
                     n_sharing=len(db.last["sharing"]), n_scored=db.last["nscores"], min_score_used=np.float32(ms))
            r.update(db.taps(capacity, is_loop, q.mnId))
            out.append(r)
    return out


def run_device(ox, ctx, ops, capacity, max_words, taps=True):
    db = ox.KeyFrameDatabase(ctx, capacity, max_words)
    out = []
    try:
        for o in ops:
            k = o["op"]
            if k == "add":
                db.add(o["id"], o["words"], o["values"])
            elif k == "erase":
                db.erase(o["id"])
            elif k == "clear":
                db.clear()
            elif k == "neigh":
                db.set_neighbours([o["id"]], [o["ids"]])
            else:
                bow = (o["words"], o["values"])
                if k == "loop":
                    c, info = db.detect_loop_candidates(bow, o["min_score"], o["ref"], o["exclude"], taps=taps, info=True)
                else:
                    c, info = db.detect_relocalisation_candidates(bow, taps=taps, info=True)
                r = dict(cand=c, max_common_words=info["max_common_words"], n_sharing=info["n_sharing"],
                         n_scored=info["n_scored"], min_score_used=info["min_score_used"])
                if taps:
                    r.update({t: info[t] for t in TAPS})
                out.append(r)
    finally:
        db.close()
    return out


def assert_same(got, want, taps=True):
    """Exact, field by field."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["cand"], w["cand"]), (k, g["cand"], w["cand"])
        for f in ("max_common_words", "n_sharing", "n_scored"):
            assert int(g[f]) == int(w[f]), (k, f, g[f], w[f])
        assert np.float32(g["min_score_used"]) == np.float32(w["min_score_used"]), (k, g["min_score_used"])
        if taps:
            for t in TAPS:
                assert np.array_equal(g[t], w[t]), (k, t, np.flatnonzero(g[t] != w[t])[:8])


# ---- the array form of (ops, results): what tests/golden/kfdb_queries.npz holds ----
def encode(ops, results, capacity):
    code, ident, ms = [], [], []
    bp, bw, bv = [0], [], []
    lp, lv = [0], []
    for o in ops:
        code.append(CODES.index(o["op"]))
        ident.append(o.get("id", -1))
        ms.append(o.get("min_score", 0.0))
        if "words" in o:
            bw += list(o["words"])
            bv += list(o["values"])
        bp.append(len(bw))
        for key in ("ids", "ref", "exclude"):   # three lists per op
            lv += list(o.get(key, []))
            lp.append(len(lv))
    cp, cv = [0], []
    for r in results:
        cv += list(r["cand"])
        cp.append(len(cv))
    d = dict(capacity=np.int32(capacity), code=np.array(code, np.int32), id=np.array(ident, np.int32),
             min_score=np.array(ms, np.float64), bow_ptr=np.array(bp, np.int64), bow_words=np.array(bw, np.uint32),
             bow_values=np.array(bv, np.float64), list_ptr=np.array(lp, np.int64), lists=np.array(lv, np.int32),
             cand_ptr=np.array(cp, np.int64), cand=np.array(cv, np.int32),
             header=np.array([[r["max_common_words"], r["n_sharing"], r["n_scored"]] for r in results],
                             np.int32).reshape(-1, 3),
             min_score_used=np.array([r["min_score_used"] for r in results], np.float32))
    for t in TAPS:
        d["tap_" + t] = np.stack([r[t] for r in results]) if results else np.zeros((0, capacity))
    return d


def decode(d):
    ops, results = [], []
    for k, c in enumerate(d["code"]):
        o = dict(op=CODES[int(c)])
        b0, b1 = d["bow_ptr"][k], d["bow_ptr"][k + 1]
        l = [d["lists"][d["list_ptr"][3 * k + j]:d["list_ptr"][3 * k + j + 1]].tolist() for j in range(3)]
        if o["op"] in ("add", "erase", "neigh"):
            o["id"] = int(d["id"][k])
        if o["op"] in ("add", "reloc", "loop"):
            o["words"], o["values"] = d["bow_words"][b0:b1].copy(), d["bow_values"][b0:b1].copy()
        if o["op"] == "neigh":
            o["ids"] = l[0]
        if o["op"] == "loop":
            o["min_score"], o["ref"], o["exclude"] = float(d["min_score"][k]), l[1], l[2]
        ops.append(o)
    for k in range(len(d["cand_ptr"]) - 1):
        r = dict(cand=d["cand"][d["cand_ptr"][k]:d["cand_ptr"][k + 1]].astype(np.int32),
                 max_common_words=int(d["header"][k, 0]), n_sharing=int(d["header"][k, 1]),
                 n_scored=int(d["header"][k, 2]), min_score_used=np.float32(d["min_score_used"][k]))
        for t in TAPS:
            r[t] = d["tap_" + t][k]
        results.append(r)
    return ops, results, int(d["capacity"])


# ---- hand-built cases, one per rule, with the answer worked out by hand ----
def bow(d):
    """A BowVector from a {word: value} dict."""
    ks = sorted(d)
    return np.array(ks, np.uint32), np.array([d[k] for k in ks], np.float64)


A, B, C, D, E = 10, 20, 30, 40, 50


def rule_cases():
    """name -> (ops, capacity, the candidates every query must return).
    Values are dyadic, so every score is exact: sum of min(vi, wi)."""
    cases = {}
    q = bow({A: .5, B: .5})
    # acc == 0.75f * best exactly is rejected (strict >)
    cases["threshold_075"] = ([add(0, bow({A: .5, B: .5})), add(1, bow({A: .5, B: .25, C: .25})), reloc(q)], 4, [[0]])
    # loop: si == minScore enters lScoreAndMatch (>=); 1 wins, 0.5 == 0.75 * ... is not the point here
    cases["loop_si_equals_min_score"] = ([add(0, bow({A: .5, B: .5})), add(1, bow({A: .25, B: .25, C: .5})),
                                          neigh(1, []), loop(q, .5)], 4, [[0]])
    # loop: the only member sits exactly at minScore: bestAccScore = minScore = acc, kept; above it nothing
    cases["loop_best_starts_at_min_score"] = ([add(0, bow({A: .25, B: .25, C: .5})), loop(q, .5), loop(q, .75)], 4,
                                              [[0], []])
    # identical members: pBestKF keeps the first on equal scores
    same = bow({A: .5, B: .5})
    cases["duplicates_keep_first"] = ([add(5, same), add(2, same), add(7, same), neigh(5, [2, 7]), neigh(2, [5]),
                                       reloc(q)], 8, [[5]])
    # two listed members with the same best neighbour: once, at the first position
    cases["same_best_once"] = ([add(1, bow({A: .5, B: .25, C: .25})), add(6, bow({A: .25, B: .5, D: .25})),
                                add(4, bow({A: .5, B: .5})), neigh(1, [4]), neigh(6, [4]), reloc(q)], 8, [[4]])
    # order: smallest common word, then add order; never the id.  7 is erased and added again: to the back
    q4 = bow({10: .25, 20: .25, 30: .25, 40: .25})
    cases["order_first_word_then_add"] = ([add(9, bow({30: .5, 40: .5})), add(2, bow({20: .5, 40: .5})),
                                           add(7, bow({10: .5, 40: .5})), add(5, bow({10: .5, 30: .5})), reloc(q4),
                                           erase(7), add(7, bow({10: .5, 20: .5})), reloc(q4),
                                           loop(q4, 0.0)], 12, [[7, 5, 2, 9], [5, 7, 2, 9], [5, 7, 2, 9]])
    # relocalisation state: 1 is scored by the first query, fails the second's word gate and is a neighbour
    # of the scored 0: its 0.5 is accumulated; 3 was never scored: 0.0f
    cases["reloc_state"] = ([add(0, bow({1: .5, 2: .5})), add(1, bow({1: .25, 3: .25, 4: .25, 5: .25})),
                             add(3, bow({6: .5, 8: .5})), neigh(0, [3, 1]), reloc(bow({3: .5, 4: .5})),
                             reloc(bow({1: .25, 2: .25, 6: .25, 7: .25}))], 4, [[1], [0]])
    # loop exclusion: 0 shares all 8 words and is excluded: maxCommonWords is 5, so 2 (5 words) passes and
    # 1 (4 words) does not; 0 as 2's neighbour adds nothing; ref (0, 1) gives minScore 0.5
    q8 = bow({w: .125 for w in range(1, 9)})
    cases["loop_exclusion"] = ([add(0, bow({w: .125 for w in range(1, 9)})), add(1, bow({1: .25, 2: .25, 3: .25, 4: .25})),
                                add(2, bow({1: .125, 2: .125, 3: .125, 4: .125, 5: .5})), neigh(2, [0]),
                                loop(q8, 1.0, ref=[0, 1], exclude=[0])], 4, [[2]])
    # neighbour rows: fillers that share nothing, a non-member (11), the scoring neighbour last; then a row
    # that names an erased id
    fill = [add(i, bow({100 + i: 1.0})) for i in range(1, 9)]
    cases["neighbour_rows"] = ([add(0, bow({A: .5, B: .25, C: .25}))] + fill + [add(9, bow({A: .5, B: .5})),
                               neigh(0, [1, 2, 3, 4, 5, 6, 7, 8, 11, 9]), neigh(9, [0]), reloc(q), erase(3), reloc(q),
                               erase(9), reloc(q)], 16, [[9], [9], [0]])
    return cases


GATE_MIN = {1: 0, 4: 3, 5: 4, 10: 8, 15: 12, 40: 32}   # (int)(maxCommonWords * 0.8f)


def gate_case(M, is_loop):
    """maxCommonWords = M: member 0 shares all M words, 1 exactly minCommonWords (rejected), 2 one more (kept)."""
    words = list(range(100, 100 + M))
    qb = bow({w: 1.0 / M for w in words})
    mc = GATE_MIN[M]
    ops = [add(0, qb)]

    def sharing(k, base):   # k of the query's words and one of its own
        d = {w: 1.0 / (k + 1) for w in words[:k]}
        d[base] = 1.0 / (k + 1)
        return bow(d)
    if mc >= 1:
        ops.append(add(1, sharing(mc, 7)))
    if mc + 1 < M:
        ops.append(add(2, sharing(mc + 1, 8)))
    ops.append(loop(qb, 0.0) if is_loop else reloc(qb))
    scored = 1 + (1 if mc + 1 < M else 0)
    return ops, 4, scored
