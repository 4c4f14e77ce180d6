"""The keyframe database in HBM (orbx_kfdb_*, orb_slam_amd/csrc/orbx_kfdb.hip)
against the literal restatement of src/KeyFrameDatabase.cc (tests/
kfdb_numpy.py): every comparison is exact -- the candidate vector in order,
the header, and each tap field by field."""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import kfdb_cases as kc
from orb_slam_amd import synth
from vocab_data import make_vocab

pytestmark = pytest.mark.gpu

MAX_WORDS = 300
LENGTHS = [0, 1, 63, 64, 65, 257, MAX_WORDS]
UNIVERSE = 600   # small: sharing is dense
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=320, max_h=240, slots=3)
    yield c
    c.close()


def both(ctx, ops, capacity, max_words=MAX_WORDS):
    want = kc.run_restatement(ops, capacity)
    got = kc.run_device(ox, ctx, ops, capacity, max_words)
    kc.assert_same(got, want)
    return got, want


@pytest.mark.parametrize("members", [0, 1, 3, 64, 65, 130])
def test_random_sequences(ctx, members):
    """Members and queries of every length in LENGTHS; ids added in shuffled
    order, random neighbour rows (padding, non-members), an erase and a second
    add, relocalisation and loop queries with ref and exclude lists."""
    ops, capacity = kc.random_ops(100 + members, members, LENGTHS, UNIVERSE, n_queries=2 * len(LENGTHS))
    got, _ = both(ctx, ops, capacity)
    if members >= 64:
        assert any(len(r["cand"]) > 1 for r in got) and max(r["n_scored"] for r in got) > 1


def test_dense_sharing(ctx):
    """A tiny word universe: every member shares many words with every query,
    so the gates, the accumulation and the de-duplication all have work."""
    ops, capacity = kc.random_ops(8, 130, [20, 25, 30, 28, 33], 40, n_queries=8)
    got, _ = both(ctx, ops, capacity, max_words=40)
    assert max(len(r["cand"]) for r in got) >= 3 and max(r["n_sharing"] for r in got) >= 128


@pytest.mark.parametrize("name", sorted(kc.rule_cases()))
def test_rule(ctx, name):
    ops, capacity, answer = kc.rule_cases()[name]
    got, _ = both(ctx, ops, capacity)
    assert [r["cand"].tolist() for r in got] == answer


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("M", sorted(kc.GATE_MIN))
def test_word_gate(ctx, M, loop):
    ops, capacity, scored = kc.gate_case(M, loop)
    got, _ = both(ctx, ops, capacity)
    assert got[0]["max_common_words"] == M and got[0]["n_scored"] == scored


def test_golden_sequence(ctx):
    from test_kfdb_numpy import GOLDEN
    ops, want, capacity = kc.decode(np.load(GOLDEN))
    kc.assert_same(kc.run_device(ox, ctx, ops, capacity, 64), want)


def test_score_alone_equals_the_taps(ctx):
    rng = np.random.default_rng(4)
    bows = [kc.rand_bow(rng, n, 80) for n in (30, 40, 1, 0, 64, 65)]
    q = kc.rand_bow(rng, 50, 80)
    db = ox.KeyFrameDatabase(ctx, 8, 80)
    try:
        for i, b in enumerate(bows):
            db.add(i, *b)
        ids = [5, 0, 3, 2, 1, 4]
        s = db.score(q, ids)
        import kfdb_numpy as kn
        want = [np.float32(kn.l1_score(dict(zip(q[0].tolist(), q[1])), dict(zip(bows[i][0].tolist(), bows[i][1]))))
                for i in ids]
        assert np.array_equal(s, np.array(want, np.float32))
        # relocalisation taps: the scored members' mRelocScore is that score
        _, info = db.detect_relocalisation_candidates(q, taps=True)
        scored = np.flatnonzero(info["best"] >= 0)
        assert len(scored) >= 2
        assert np.array_equal(info["score"][scored], db.score(q, scored))
        assert len(db.score(q, [])) == 0
        with pytest.raises(ox.OrbxError) as e:
            db.score(q, [7])   # not a member
        assert e.value.code == ERR_ARG
    finally:
        db.close()


def test_slot_forms(ctx):
    """The query from a slot equals the query from the slot's read-back
    arrays; add_slot equals add of the same arrays."""
    V = make_vocab(k=4, L=3, seed=3)
    voc = ox.Vocabulary(ctx, V["k"], V["L"], V["parent"], V["is_leaf"], V["desc"], V["weight"])
    frames = synth.sequence(320, 240, 3, seed=17)
    ctx.upload(np.stack(frames), 0)
    ctx.extract(0, 3)
    ctx.compute_bow(voc, 0, 3)
    bows = [ctx.read_bow(s)[0] for s in range(3)]
    assert all(len(b[0]) > 4 for b in bows)
    rng = np.random.default_rng(6)
    extra = [kc.rand_bow(rng, 20, voc.n_words()) for _ in range(4)]
    a = ox.KeyFrameDatabase(ctx, 16, 500)
    b = ox.KeyFrameDatabase(ctx, 16, 500)
    try:
        for s in (1, 2):
            a.add_slot(10 + s, s)
            b.add(10 + s, *bows[s])
        for i, e in enumerate(extra):
            a.add(i, *e)
            b.add(i, *e)
        for db in (a, b):
            db.set_neighbours([11, 12, 0], [[12, 0], [11], [12, 11, 3]])
        assert len(a) == len(b) == 6
        res = []
        for db in (a, b):
            for query in (0, bows[0]):
                c, i = db.detect_relocalisation_candidates(query, taps=True)
                c2, i2 = db.detect_loop_candidates(query, 1.0, ref=[11, 0], exclude=[1], taps=True)
                res.append((c, i, c2, i2, db.score(query, [11, 12, 0])))
        assert len(res[0][0]) >= 1 and res[0][1]["max_common_words"] >= 2
        for r in res[1:]:
            assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[2], res[0][2]) and np.array_equal(r[4], res[0][4])
            for i_got, i_want in ((r[1], res[0][1]), (r[3], res[0][3])):
                for f in ("max_common_words", "n_sharing", "n_scored", "min_score_used") + kc.TAPS:
                    assert np.array_equal(i_got[f], i_want[f]), f
        # and the restatement on the read-back arrays
        ops = [kc.add(11, bows[1]), kc.add(12, bows[2])] + [kc.add(i, e) for i, e in enumerate(extra)]
        ops += [kc.neigh(11, [12, 0]), kc.neigh(12, [11]), kc.neigh(0, [12, 11, 3]), kc.reloc(bows[0])]
        want = kc.run_restatement(ops, 16)[0]
        assert np.array_equal(res[0][0], want["cand"]) and np.array_equal(res[0][1]["acc"], want["acc"])
        # a slot without BoW, a database too narrow for a slot
        ctx.extract(2, 1)   # clears slot 2's BoW
        with pytest.raises(ox.OrbxError) as e:
            a.add_slot(5, 2)
        assert e.value.code == ERR_ARG
        with pytest.raises(ox.OrbxError) as e:
            a.detect_relocalisation_candidates(2)
        assert e.value.code == ERR_ARG
        narrow = ox.KeyFrameDatabase(ctx, 4, 100)
        with pytest.raises(ox.OrbxError) as e:
            narrow.add_slot(0, 1)
        assert e.value.code == ERR_CAPACITY
        narrow.close()
    finally:
        a.close()
        b.close()
        voc.close()


def test_without_taps_and_clear(ctx):
    ops, capacity = kc.random_ops(21, 20, [20, 25, 30], 40, n_queries=4)
    want = kc.run_restatement(ops, capacity)
    got = kc.run_device(ox, ctx, ops, capacity, 40, taps=False)
    kc.assert_same(got, want, taps=False)
    # clear: an empty database answers with nothing, the ids are free, the order starts again
    both(ctx, ops + [dict(op="clear"), kc.reloc(kc.bow({1: 1.0}))] + ops, capacity, 40)


def test_error_codes(ctx):
    lib = ox.lib()
    h = ctypes.c_void_p()
    assert lib.orbx_kfdb_create(ctx.handle, ox.KFDB_MAX_MEMBERS + 1, 8, ctypes.byref(h)) == ERR_UNSUPPORTED
    assert lib.orbx_kfdb_create(ctx.handle, 8, ox.KFDB_MAX_WORDS + 1, ctypes.byref(h)) == ERR_UNSUPPORTED
    assert lib.orbx_kfdb_create(ctx.handle, 0, 8, ctypes.byref(h)) == ERR_ARG
    db = ox.KeyFrameDatabase(ctx, 4, 3)
    try:
        w3, w4 = kc.bow({1: .5, 2: .25, 3: .25}), kc.bow({1: .25, 2: .25, 3: .25, 4: .25})

        def code(fn, *a, **k):
            with pytest.raises(ox.OrbxError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(db.add, 4, *w3) == ERR_ARG and code(db.add, -1, *w3) == ERR_ARG   # id out of range
        db.add(2, *w3)
        assert code(db.add, 2, *w3) == ERR_ARG            # id in use
        assert code(db.add, 1, *w4) == ERR_CAPACITY       # too many words
        assert code(db.add, 1, [3, 1], [.5, .5]) == ERR_ARG   # words not ascending
        assert code(db.erase, 1) == ERR_ARG
        assert code(db.set_neighbours, [1], [[2]]) == ERR_ARG
        assert code(db.detect_relocalisation_candidates, w4) == ERR_CAPACITY
        assert code(db.detect_loop_candidates, w3, 1.0, [4], []) == ERR_ARG
        assert code(db.detect_loop_candidates, w3, 1.0, [], [-1]) == ERR_ARG
        db.add(0, *w3)
        db.add(3, *kc.bow({1: .5, 3: .5}))
        assert len(db) == 3
        assert db.detect_relocalisation_candidates(w3).tolist() == [2, 0]
        assert code(db.detect_relocalisation_candidates, w3, cap=1) == ERR_CAPACITY   # cap too small
        db.erase(2)
        assert len(db) == 2 and db.detect_relocalisation_candidates(w3).tolist() == [0]
        # empty query, nothing shared: ORBX_OK and no candidates
        assert len(db.detect_relocalisation_candidates(([], []))) == 0
        assert len(db.detect_loop_candidates(kc.bow({9: 1.0}), 0.0)) == 0
    finally:
        db.close()


def test_largest_database(ctx):
    """ORBX_KFDB_MAX_MEMBERS members (the select kernel's LDS sort at its
    largest): every member shares the query's one word with the same score,
    so all of them are listed, kept and returned, in add order."""
    C = ox.KFDB_MAX_MEMBERS
    db = ox.KeyFrameDatabase(ctx, C, 2)
    try:
        for i in range(C - 1, -1, -1):
            db.add(i, *kc.bow({5: .5, 30 + i: .5}))
        c, info = db.detect_relocalisation_candidates(kc.bow({5: 1.0}), taps=True)
        assert info["n_sharing"] == info["n_scored"] == C and info["max_common_words"] == 1
        assert np.array_equal(c, np.arange(C - 1, -1, -1))
        assert np.array_equal(info["pos"], np.arange(C - 1, -1, -1)) and np.all(info["score"] == 0.5)
        # one member's own word first: it leads the list only if that word is the smaller one
        c = db.detect_loop_candidates(kc.bow({5: .5, 30 + 77: .5}), 0.0)
        assert c.tolist() == [77]   # 2 common words: minCommonWords 1 rejects the rest
        c = db.detect_loop_candidates(kc.bow({5: .5, 30 + 77: .5}), 0.0, exclude=[77])
        assert np.array_equal(c, np.delete(np.arange(C - 1, -1, -1), C - 1 - 77))
    finally:
        db.close()
