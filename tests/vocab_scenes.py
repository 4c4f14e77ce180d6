"""Vocabularies built around a given descriptor array, and a plain restatement
of DBoW2's transform to hold them to.

`transform` restates TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/
TemplatedVocabulary.h:1127-1259) with BowVector::addWeight / normalize(L1)
(BowVector.cpp) and FeatureVector::addFeature (FeatureVector.cpp) in numpy
and Python only: no call into oracle/ or the library.  `mut` names one edit
of the mutation table (MUTATIONS); the empty set is the restatement.

The device-slot forms only see the descriptors a slot holds, so the
vocabulary is the free input: `scene(name, D)` builds the named vocabulary
around the descriptor array D.  Leaves that are exact copies of chosen rows of
D route those rows with distance 0; every other feature goes to its nearest
leaf, first on ties, which the restatement computes.  Each builder asserts
the property it exists for while the scene is made (for the size-dependent
properties: when D has at least BIG rows), and each scene carries `pin(T)`,
the outcome written down beside its reason, to be asserted on any transform
result T (restatement, oracle, device).
"""
import numpy as np

BIG = 1024          # the size-dependent properties are asserted from this many rows on
NO_NODE = 0xFFFFFFFF

MUTATIONS = ("last_min", "le", "reverse_children", "pairwise", "count_times_w", "norm_feature_order", "w_ge_0",
             "nid_level_plus_1", "nid_level_minus_1", "shallow_nid_0", "fv_word_order")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)


def hamming(fa, fb):
    """Hamming distances between two sets of unpacked descriptors:
    |a| + |b| - 2 a.b, exact in float32 (every term is at most 256)."""
    return (fa.sum(1)[:, None] + fb.sum(1)[None, :] - 2.0 * (fa @ fb.T)).astype(np.int32)


def children(V):
    """Per node the ids of its children in increasing id, as
    loadFromTextFile appends them."""
    out = [[] for _ in V["parent"]]
    for i in range(1, len(V["parent"])):
        out[int(V["parent"][i])].append(i)
    return [np.array(k, np.int64) for k in out]


def word_ids(V):
    """Word ids go to the nodes flagged leaf, in id order; every other node keeps 0."""
    w = np.zeros(len(V["parent"]), np.int64)
    w[1:][V["is_leaf"][1:] != 0] = np.arange(int(np.count_nonzero(V["is_leaf"][1:])))
    return w


def pick(dist, mut):
    """Column of the first strict minimum of each row, scanned left to right."""
    if "last_min" in mut:
        return dist.shape[1] - 1 - np.argmax(dist[:, ::-1] == dist.min(1)[:, None], axis=1)
    by_child = np.ascontiguousarray(dist.T)
    best = np.zeros(len(dist), np.int64)
    bd = by_child[0].copy()
    for c in range(1, len(by_child)):
        better = by_child[c] <= bd if "le" in mut else by_child[c] < bd
        bd = np.where(better, by_child[c], bd)
        best = np.where(better, c, best)
    return best


def pairwise_sum(a):
    return a[0] if len(a) == 1 else pairwise_sum(a[:len(a) // 2]) + pairwise_sum(a[len(a) // 2:])


def transform(V, D, levelsup, mut=frozenset()):
    mut = frozenset(mut)
    D = np.ascontiguousarray(D, np.uint8).reshape(-1, 32)
    n = len(D)
    kids = children(V)
    if "reverse_children" in mut:
        kids = [k[::-1] for k in kids]
    n_kids = np.array([len(k) for k in kids])
    fb, nb = bits(D), bits(V["desc"])
    nid_level = V["L"] - levelsup + ("nid_level_plus_1" in mut) - ("nid_level_minus_1" in mut)
    cur = np.zeros(n, np.int64)
    nid = np.full(n, 0 if nid_level <= 0 or "shallow_nid_0" in mut else -1, np.int64)
    level = 0
    while True:
        act = np.nonzero(n_kids[cur] > 0)[0]
        if not len(act):
            break
        level += 1
        for u in np.unique(cur[act]):
            idx = act[cur[act] == u]
            cur[idx] = kids[u][pick(hamming(fb[idx], nb[kids[u]]), mut)]
        if level == nid_level:
            nid[act] = cur[act]
    word = word_ids(V)[cur]
    weight = np.asarray(V["weight"], np.float64)[cur]
    # BowVector: addWeight in feature order, then normalize(L1) over ascending words
    keep = [i for i in range(n) if (weight[i] >= 0 if "w_ge_0" in mut else weight[i] > 0)]
    per_word = {}
    for i in keep:
        per_word.setdefault(int(word[i]), []).append(i)
    value = {}
    for wd, fs in per_word.items():
        if "pairwise" in mut:
            value[wd] = float(pairwise_sum(weight[fs]))
        elif "count_times_w" in mut:
            value[wd] = float(len(fs) * weight[fs[0]])
        else:
            acc = 0.0
            for i in fs:
                acc += float(weight[i])
            value[wd] = acc
    norm = 0.0
    for wd in (per_word if "norm_feature_order" in mut else sorted(value)):
        norm += abs(value[wd])
    bw = np.array(sorted(value), np.uint32)
    bv = np.array([value[w] / norm if norm > 0.0 else value[w] for w in sorted(value)], np.float64)
    # FeatureVector: nodes ascending (as uint32), features ascending inside a node
    per_node = {}
    for i in keep:
        per_node.setdefault(int(nid[i]) & NO_NODE, []).append(i)
    fn = np.array(sorted(per_node), np.uint32)
    fp, ff = [0], []
    for node in sorted(per_node):
        fs = per_node[node]
        ff += sorted(fs, key=lambda i: (word[i], i)) if "fv_word_order" in mut else fs
        fp.append(len(ff))
    return {"word": word.astype(np.int32), "weight": weight, "nid": nid.astype(np.int32), "bw": bw, "bv": bv,
            "nw": len(bw), "fn": fn, "fp": np.array(fp, np.int32), "ff": np.array(ff, np.int32), "nf": len(fn)}


def trim(T):
    """A result with padded arrays (oracle, device) cut to its counts."""
    nw, nf = int(T["nw"]), int(T["nf"])
    m = int(T["fp"][nf])
    return {"word": T["word"], "weight": T["weight"], "nid": T["nid"], "bw": T["bw"][:nw], "bv": T["bv"][:nw],
            "nw": nw, "fn": T["fn"][:nf], "fp": T["fp"][:nf + 1], "ff": T["ff"][:m], "nf": nf}


def differences(A, B):
    """Names of the outputs in which two results differ (float64 as bit patterns)."""
    A, B = trim(A), trim(B)
    bad = [k for k in ("nw", "nf") if A[k] != B[k]]
    for k in ("word", "nid", "bw", "fn", "fp", "ff"):
        if not np.array_equal(np.asarray(A[k]).astype(np.int64), np.asarray(B[k]).astype(np.int64)):
            bad.append(k)
    for k in ("weight", "bv"):
        a, b = (np.ascontiguousarray(x, np.float64).view(np.uint64) for x in (A[k], B[k]))
        if not np.array_equal(a, b):
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def random_descriptors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


FILL = random_descriptors(16, 4242)


def base(D):
    """The rows a vocabulary is built around: D, padded with fixed rows when D is tiny."""
    D = np.ascontiguousarray(D, np.uint8).reshape(-1, 32)
    return D if len(D) >= 16 else np.concatenate([D, FILL])


def distinct_rows(B):
    """Indices of the first occurrence of every distinct row, in feature order."""
    return np.sort(np.unique(B, axis=0, return_index=True)[1])


def tree(parent, desc, weight, L, is_leaf=None):
    parent = np.asarray(parent, np.int32)
    if is_leaf is None:
        is_leaf = np.ones(len(parent), np.uint8)
        is_leaf[parent[1:]] = 0
        is_leaf[0] = 0
    k = int(np.bincount(parent[1:], minlength=len(parent)).max())
    return {"k": k, "L": L, "parent": parent, "is_leaf": np.asarray(is_leaf, np.uint8),
            "desc": np.ascontiguousarray(desc, np.uint8), "weight": np.asarray(weight, np.float64)}


def flat(leaf_desc, weights):
    """Root plus one level of leaves: leaf j is node j + 1 and word j."""
    k = len(leaf_desc)
    return tree(np.zeros(k + 1, np.int32), np.concatenate([np.zeros((1, 32), np.uint8), leaf_desc]),
                np.concatenate([[0.0], weights]), 1)


def sorted_keys(T):
    """The (word, feature) keys of the features with weight > 0 in sorted
    order: what the device's second sort pass produces."""
    f = np.nonzero(T["weight"] > 0)[0]
    o = np.lexsort((f, T["word"][f]))
    return T["word"][f][o], f[o]


def groups(T):
    """Head position and length of every word's run in the sorted keys."""
    w, _ = sorted_keys(T)
    heads = np.nonzero(np.r_[True, w[1:] != w[:-1]])[0] if len(w) else np.zeros(0, np.int64)
    return heads, np.diff(np.r_[heads, len(w)])


def _scene(name, V, levelsup, D, why, pin, T=None, **extra):
    T = transform(V, D, levelsup) if T is None else T
    pin(T)
    S = {"name": name, "V": V, "levelsup": levelsup, "D": D, "why": why, "pin": pin, "T": T,
         "n_words": int(np.count_nonzero(V["is_leaf"][1:]))}
    S.update(extra)
    return S


def _identity_vocab(D, seed=11):
    B = base(D) if len(D) == 0 else D
    rows = distinct_rows(B)
    rng = np.random.default_rng(seed)
    rows = rows[rng.permutation(len(rows))]
    weights = (1.0 + rng.permutation(len(rows))) / 7.0          # distinct
    return flat(B[rows], weights), rows


def identity(name, D, levelsup=0):
    """One leaf per distinct row under the root, leaves in a seeded
    permutation: word order is a real permutation of feature order."""
    V, rows = _identity_vocab(D)
    n, all_distinct = len(D), len(distinct_rows(D)) == len(D) if len(D) else True
    word_of = np.empty(len(base(D)), np.int64)
    word_of[rows] = np.arange(len(rows))

    def pin(T):
        if not (n and all_distinct):
            return
        m = int(T["fp"][T["nf"]])
        assert T["nw"] == m == n == len(rows)
        assert np.array_equal(T["word"], word_of[:n])
        assert np.array_equal(T["weight"], V["weight"][1:][word_of[:n]])
        if levelsup == 0:       # node = leaf: one FeatureVector node per feature, in word order
            assert T["nf"] == n and np.array_equal(T["ff"], rows)
        else:                   # one node, features ascending although the words are permuted
            assert T["nf"] == 1 and T["fn"][0] == 0 and np.array_equal(T["ff"], np.arange(n))

    S = _scene(name, V, levelsup, D, "words are a permutation of the features; distinct weights", pin)
    if n >= BIG:
        assert all_distinct
        _, f = sorted_keys(S["T"])
        assert np.count_nonzero(f != np.arange(n)) > n // 2
    return S


LEADER_WEIGHTS = np.array([0.1, 1.0 / 3.0, 0.7])


def _three_sums(ws):
    """Sequential sum, count * w and pairwise sum of one word's weights."""
    acc = 0.0
    for w in ws:
        acc += float(w)
    return acc, float(len(ws) * ws[0]), float(pairwise_sum(np.asarray(ws)))


def few_words(name, D, n_leaders):
    """One, two or three leaves: every word holds hundreds of features, so
    the order of the float64 sum shows in the bits."""
    B, n = base(D), len(D)
    big = n >= BIG
    for attempt in range(64):
        rng = np.random.default_rng(100 * n_leaders + attempt)
        lead = [0] if n_leaders == 1 else rng.choice(len(B), n_leaders, replace=False)
        V = flat(B[lead], LEADER_WEIGHTS[:n_leaders])
        T = transform(V, D, 0)
        if not big:
            break
        cnt = np.bincount(T["word"], minlength=n_leaders)
        told_apart = [len(set(_three_sums(T["weight"][T["word"] == w]))) == 3 for w in range(n_leaders)]
        # one word: its value is sum / sum = 1.0 whatever the order, so there the sums need not differ
        if cnt.min() >= 200 and (any(told_apart) or n_leaders == 1):
            break
    else:
        raise AssertionError(f"{name}: no leader set with the property")

    def pin(T):
        if n == 0:
            assert T["nw"] == T["nf"] == 0
            return
        assert T["nf"] == T["nw"] <= n_leaders and np.array_equal(T["fn"], T["bw"] + 1)
        if n_leaders == 1:      # a sum divided by itself
            assert T["nw"] == 1 and T["bv"][0] == 1.0 and np.array_equal(T["ff"], np.arange(n))

    return _scene(name, V, 0, D, "hundreds of features a word: sequential sum != count * w != pairwise", pin, T)


def runs(name, D):
    """Two levels.  The first holds a few rows of D; under most of them one
    leaf collects everything that descends there (a long run of one word),
    under the others every feature that descends there finds a copy of itself
    (a block of singleton words).  The sorted keys then hold runs that start
    inside a thread's chunk and go on through the following chunks, and
    chunks made of group heads only, for 2 and 4 keys a thread."""
    B, n = base(D), len(D)
    big = n >= BIG
    rows = distinct_rows(B)
    K1 = min(12, len(rows))
    found = None
    for attempt in range(256):
        rng = np.random.default_rng(7000 + attempt)
        top = B[rows[rng.choice(len(rows), K1, replace=False)]]
        singles = rng.choice(K1, 2, replace=False)
        to = pick(hamming(bits(D), bits(top)), frozenset()) if n else np.zeros(0, np.int64)
        parent, desc = [0] * (K1 + 1), [np.zeros(32, np.uint8)] + list(top)
        for j in range(K1):
            own = np.nonzero(to == j)[0] if j in singles else []
            for d in (D[rng.permutation(own)] if len(own) else top[j:j + 1]):
                parent.append(j + 1)
                desc.append(d)
        n_leaf = len(parent) - K1 - 1
        V = tree(parent, np.array(desc), np.r_[np.zeros(K1 + 1), 0.1 + np.arange(n_leaf) % 7 / 3.0], 2)
        T = transform(V, D, 1)
        if not big:
            break
        heads, length = groups(T)
        is_head = np.zeros(n + 8, bool)
        is_head[heads] = True
        found = {}
        for per in (2, 4):
            a = [int(h) for h, l in zip(heads, length) if h % per and l >= 2]
            b = [int(h) for h, l in zip(heads, length) if l > 3 * per]
            c = [t * per for t in range(n // per) if is_head[t * per:(t + 1) * per].all()]
            d = [int(h) for h, l in zip(heads, length) if h % per == per - 1 and l >= 2]
            if a and b and c and d:
                found[per] = {"starts_inside_chunk": a[0], "longer_than_3_per": b[0], "chunk_of_heads": c[0],
                              "head_last_of_chunk": d[0]}
        if len(found) == 2:
            break
    else:
        raise AssertionError(f"{name}: no tree with the property")

    def pin(T):
        if n and len(rows) == len(B):
            assert np.array_equal(T["nid"], to + 1) and int(T["fp"][T["nf"]]) == n
            cnt = np.bincount(T["word"])
            for j in singles:       # every feature under a singles node is a word of its own
                assert np.all(cnt[T["word"][to == j]] == 1)

    return _scene(name, V, 1, D, "runs across thread chunks in the sorted keys", pin, T, positions=found)


def stopped(name, D, pattern):
    """Stopped words (weight 0): their features leave both vectors."""
    B, n = base(D), len(D)
    all_distinct = n > 0 and len(distinct_rows(D)) == n
    if pattern == "ends":
        # the stopped leader takes feature 0 and feature n - 1: it lies
        # halfway between the two (every second bit in which they differ
        # flipped), far nearer to both than the other leaders are
        first, last = B[0], B[n - 1 if n else 0]
        differ = np.nonzero(np.unpackbits(first ^ last))[0][::2]
        flip = np.zeros(256, np.uint8)
        flip[differ] = 1
        middle = first ^ np.packbits(flip)
        for attempt in range(64):
            rng = np.random.default_rng(300 + attempt)
            others = rng.choice(np.arange(1, len(B)), 2, replace=False)
            V = flat(np.concatenate([middle[None], B[others]]), np.array([0.0, 1.0 / 3.0, 0.7]))
            T = transform(V, D, 0)
            if n == 0 or (T["word"][0] == 0 and T["word"][n - 1] == 0):
                break
        else:
            raise AssertionError(f"{name}: the stopped leader does not take both ends")

        def pin(T):
            if n:
                assert T["word"][0] == 0 and T["word"][n - 1] == 0
                assert 0 not in T["ff"] and n - 1 not in T["ff"] and 0 not in T["bw"]
                assert int(T["fp"][T["nf"]]) == np.count_nonzero(T["word"] != 0)

        return _scene(name, V, 0, D, "the stopped word holds the first and the last feature", pin, T)
    V, rows = _identity_vocab(D)
    k = len(rows)
    if pattern == "all":
        V["weight"][:] = 0.0
    elif pattern == "but_one":
        keep = V["weight"][1 + k // 2]
        V["weight"][:] = 0.0
        V["weight"][1 + k // 2] = keep
    else:
        V["weight"][1::2] = 0.0         # words 0, 2, 4, ...

    def pin(T):
        m = int(T["fp"][T["nf"]])
        if pattern == "all":            # m = 0: no word, no node, norm 0
            assert T["nw"] == T["nf"] == m == 0 and T["fp"][0] == 0
        elif all_distinct:
            if pattern == "but_one":    # m = 1: one word of one feature, value w / w
                assert T["nw"] == T["nf"] == m == 1 and T["bv"][0] == 1.0 and T["ff"][0] == rows[k // 2]
            else:                       # compaction: about half the features stay
                assert T["nw"] == T["nf"] == m == k // 2 and np.all(T["bw"] % 2 == 1)

    return _scene(name, V, 0, D, f"stopped words, pattern {pattern}", pin)


def tie_dup(name, D, j1, j2, K=130):
    """A wide node with identical leaves at child positions j1 < j2 and
    different weights: the lower id wins."""
    B, n = base(D), len(D)
    rng = np.random.default_rng(1000 + 7 * j1 + j2)
    leaves = random_descriptors(K, 500 + j1 + j2)
    r = n // 2 if n else 0
    for j in range(2, K, 9):                    # some more rows at distance 0
        if (r + 1 + j) % len(B) != r:
            leaves[j] = B[(r + 1 + j) % len(B)]
    leaves[j1] = leaves[j2] = B[r]
    V = flat(leaves, (1.0 + rng.permutation(K)) / 11.0)
    assert V["weight"][1 + j1] != V["weight"][1 + j2]

    def pin(T):
        assert j2 not in T["word"]
        same = np.all(D == B[r], axis=1) if n else np.zeros(0, bool)
        assert np.all(T["word"][same] == j1) and np.all(T["weight"][same] == V["weight"][1 + j1])
        assert n == 0 or same.any()

    return _scene(name, V, 0, D, f"identical siblings at child positions {j1} and {j2}", pin)


def tie_equal(name, D):
    """Two siblings at the same non-zero distance from a feature."""
    B, n = base(D), len(D)
    r = n // 3 if n else 0
    leaves = random_descriptors(8, 77)
    leaves[2] = B[r]
    leaves[2, 0] ^= 1
    leaves[5] = B[r]
    leaves[5, 25] ^= 0x10
    V = flat(leaves, np.array([0.9, 0.8, 0.3, 0.6, 0.5, 0.4, 0.2, 0.1]))
    d = hamming(bits(B[r:r + 1]), bits(leaves))[0]
    assert d[2] == d[5] == 1 and np.all(np.delete(d, [2, 5]) > 1)

    def pin(T):
        same = np.all(D == B[r], axis=1) if n else np.zeros(0, bool)
        assert np.all(T["word"][same] == 2) and 5 not in T["word"][same]
        assert n == 0 or (same.any() and 1 + 2 in T["fn"])

    return _scene(name, V, 0, D, "leaves 2 and 5 both one bit from a feature: 2 wins", pin)


def interleaved(name, D):
    """The children of the root and of node 1 alternate in id; nodes 4 and 8
    (both the root's) are identical."""
    B, n = base(D), len(D)
    parent = np.array([0, 0] + [0, 1] * 6, np.int32)            # even ids: root; odd ids >= 3: node 1
    r0, r1 = (n // 2, n // 5) if n >= 5 else (0, 1)
    desc = random_descriptors(len(parent), 88)
    desc[1] = desc[5] = B[r0]
    desc[4] = desc[8] = B[r1]
    V = tree(parent, desc, np.r_[0.0, 0.0, 0.2 + np.arange(12) / 13.0], 2)
    assert np.array_equal(children(V)[0], [1, 2, 4, 6, 8, 10, 12]) and np.array_equal(children(V)[1], np.arange(3, 14, 2))
    wid = word_ids(V)

    def pin(T):
        if n == 0:
            return
        a, b = np.all(D == B[r1], axis=1), np.all(D == B[r0], axis=1)
        assert np.all(T["word"][a] == wid[4]) and np.all(T["nid"][a] == 4) and wid[8] not in T["word"]
        assert np.all(T["word"][b] == wid[5]) and np.all(T["nid"][b] == 1)

    return _scene(name, V, 1, D, "siblings not contiguous in id; a tie among the root's children", pin)


def levels(name, D, levelsup):
    """One three-level tree (L = 3) with a leaf at depth 1 (node 3, word 0)
    under every placement of the FeatureVector level."""
    B, n = base(D), len(D)
    parent = np.array([0, 0, 0, 0, 1, 1, 2, 2, 4, 4, 5, 5, 6, 6, 7, 7], np.int32)
    r = (np.arange(9) * max(len(B) // 9, 1)) % len(B)            # r[0] = 0: the shallow leaf is feature 0
    desc = np.zeros((16, 32), np.uint8)
    desc[3] = B[r[0]]
    desc[8:16] = B[r[1:9]]
    desc[4], desc[5], desc[6], desc[7] = desc[8], desc[10], desc[12], desc[14]
    desc[1], desc[2] = desc[4], desc[6]
    V = tree(parent, desc, np.r_[0.0, 0.0, 0.0, 0.45, np.zeros(4), 0.3 + np.arange(8) / 9.0], 3)
    node_of_word = np.nonzero(V["is_leaf"])[0]

    def pin(T):
        if n == 0:
            return
        shallow = T["word"] == 0
        assert shallow[0]
        leaf = node_of_word[T["word"]]
        nid_level = 3 - levelsup
        if nid_level <= 0:              # levelsup = L and beyond: node 0 holds every feature
            assert T["nf"] == 1 and T["fn"][0] == 0 and np.array_equal(T["ff"], np.arange(n)) and np.all(T["nid"] == 0)
            return
        if nid_level == 3:
            assert np.array_equal(T["nid"][~shallow], leaf[~shallow])
        elif nid_level == 2:
            assert np.array_equal(T["nid"][~shallow], parent[leaf[~shallow]])
        else:
            assert np.array_equal(T["nid"][~shallow], parent[parent[leaf[~shallow]]]) and np.all(T["nid"][shallow] == 3)
            assert NO_NODE not in T["fn"]
            return
        # the shallow leaf ends the descent above the FeatureVector level:
        # nid stays -1, the last node of the map
        assert np.all(T["nid"][shallow] == -1) and T["fn"][-1] == NO_NODE
        assert np.array_equal(T["ff"][T["fp"][-2]:], np.nonzero(shallow)[0]) and T["fp"][-1] == n

    return _scene(name, V, levelsup, D, f"levelsup {levelsup} on a tree with a depth-1 leaf", pin)


def shape(name, D, which):
    B, n = base(D), len(D)
    if which == "depth1_k1":            # the smallest tree orbx_vocab_create accepts
        V = flat(B[:1], np.array([0.3]))
        levelsup = 0

        def pin(T):
            assert np.all(T["word"] == 0) and np.all(T["nid"] == 1)
            assert n == 0 or (T["nw"] == T["nf"] == 1 and T["bv"][0] == 1.0 and T["fn"][0] == 1)
    elif which == "chain20":            # single children down to one leaf at depth 20
        V = tree(np.r_[0, np.arange(20)].astype(np.int32), random_descriptors(21, 5), np.r_[np.zeros(20), 0.7], 20)
        levelsup = 4

        def pin(T):
            assert np.all(T["word"] == 0) and np.all(T["nid"] == 16)
            assert n == 0 or (T["nw"] == T["nf"] == 1 and T["fn"][0] == 16)
    else:                               # a root with 4096 children
        leaves = random_descriptors(4096, 6)
        at = (np.arange(min(len(B), 600)) * 7) % 4096
        leaves[at] = B[:len(at)]
        V = flat(leaves, (1.0 + np.random.default_rng(6).permutation(4096)) / 4099.0)
        levelsup = 0

        def pin(T):
            m = min(n, 600)
            if n and len(distinct_rows(D[:m])) == m:
                assert np.array_equal(T["word"][:m], at[:m])
    return _scene(name, V, levelsup, D, which, pin)


def flags(name, D, which):
    B, n = base(D), len(D)
    r = (np.arange(3) * max(len(B) // 3, 1)) % len(B)
    if which == "childless_not_leaf":
        # node 2 has no children and no leaf flag: it ends a descent with
        # word 0, which is also node 1's word
        V = flat(B[r], np.array([0.25, 0.55, 0.35]))
        V["is_leaf"][2] = 0
        levelsup = 0

        def pin(T):
            assert set(np.unique(T["word"])) <= {0, 1}
            at2 = T["nid"] == 2
            assert np.all(T["word"][at2] == 0) and np.all(T["weight"][at2] == 0.55)
            assert T["nw"] <= 2 and (r[1] >= n or T["nid"][r[1]] == 2)
    else:
        # node 1 is flagged leaf and has children: it takes word 0 and is never terminal
        desc = np.concatenate([np.zeros((1, 32), np.uint8), B[r[[0, 1, 0, 2]]]])
        desc[4, 3] ^= 4
        V = tree(np.array([0, 0, 0, 1, 1], np.int32), desc, np.array([0.0, 0.9, 0.25, 0.55, 0.35]), 2,
                 is_leaf=np.array([0, 1, 1, 1, 1], np.uint8))
        levelsup = 1

        def pin(T):
            assert 0 not in T["word"] and set(np.unique(T["word"])) <= {1, 2, 3}
            assert n == 0 or (T["word"][r[0]] == 2 and T["nid"][r[0]] == 1)
    S = _scene(name, V, levelsup, D, which, pin)
    assert S["n_words"] == (2 if which == "childless_not_leaf" else 4)
    return S


BUILDERS = {
    "identity": (identity, {}),
    "identity_root": (identity, {"levelsup": 1}),
    "one_word": (few_words, {"n_leaders": 1}),
    "two_words": (few_words, {"n_leaders": 2}),
    "three_words": (few_words, {"n_leaders": 3}),
    "runs": (runs, {}),
    "stopped_all": (stopped, {"pattern": "all"}),
    "stopped_but_one": (stopped, {"pattern": "but_one"}),
    "stopped_alternate": (stopped, {"pattern": "alternate"}),
    "stopped_ends": (stopped, {"pattern": "ends"}),
    "tie_dup_0_1": (tie_dup, {"j1": 0, "j2": 1}),
    "tie_dup_first_last": (tie_dup, {"j1": 0, "j2": 129}),
    "tie_dup_63_64": (tie_dup, {"j1": 63, "j2": 64}),
    "tie_equal": (tie_equal, {}),
    "interleaved": (interleaved, {}),
    "levels_0": (levels, {"levelsup": 0}),
    "levels_1": (levels, {"levelsup": 1}),
    "levels_2": (levels, {"levelsup": 2}),
    "levels_L": (levels, {"levelsup": 3}),
    "levels_L_plus_2": (levels, {"levelsup": 5}),
    "depth1_k1": (shape, {"which": "depth1_k1"}),
    "chain20": (shape, {"which": "chain20"}),
    "root4096": (shape, {"which": "root4096"}),
    "childless_not_leaf": (flags, {"which": "childless_not_leaf"}),
    "leaf_with_children": (flags, {"which": "leaf_with_children"}),
}
NAMES = list(BUILDERS)


def scene(name, D):
    """The named vocabulary around D, with the restatement's result S["T"]
    and the pinned outcome S["pin"], already asserted on S["T"]."""
    fn, kw = BUILDERS[name]
    return fn(name, np.ascontiguousarray(D, np.uint8).reshape(-1, 32), **kw)


# Host-form sizes (tests/test_vocab_scenes_gpu.py) and the slot contexts:
# (nfeatures, nlevels) -> the count a 640 x 480 texture frame gives and the
# keys a thread of k_bow_build then holds.  64 and 65 need a four-level
# pyramid (with eight levels the top level has no cell at this frame size and
# the upload is refused); 96 is the smallest nfeatures an eight-level context
# accepts at 640 x 480.
HOST_SIZES = (0, 1, 255, 256, 257, 2048)
SLOT_SHAPES = ((64, 4), (65, 4), (96, 8), (1024, 8), (1025, 8), (2048, 8), (2049, 8), (4096, 8))
FRAME = (640, 480, 5)       # synth.texture_frame(w, h, seed)


def keys_per_thread(n):
    N = 1
    while N < n:
        N <<= 1
    return (N + 1023) // 1024
