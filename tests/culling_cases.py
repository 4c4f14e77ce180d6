"""Operation sequences for the culling tests: the operations of covis_cases
plus {"op": "octaves", "id", "oct"} | {"op": "cull_kf", "cur", "keep",
"max_culls", "cand"} | {"op": "cull_mp", "cur_kf", "ids", "found", "visible",
"first_kf"}; the runners that play a sequence on the restatement
(tests/culling_numpy.py) and on the device; hand-built cases with their
answers; the window scene with octaves; the array form of the golden file.

cull_kf yields cand, n_done, n_mps, n_redundant, decision, bad_points; cull_mp
yields action."""
import numpy as np

import covis_cases as cc
import culling_numpy as cu
from covis_cases import ORDERED, ALL, _ints, add, set_matches, erase_points, erase_kf, update, read, reference, read_all

FIELDS = dict(cc.FIELDS, cull_kf=("cand", "n_done", "n_mps", "n_redundant", "decision", "bad_points"),
              cull_mp=("action",))
# the lists of an operation, in the order the golden file stores them
LISTS = {"add": ("id", "row"), "set": ("id", "idx", "mp"), "erase_points": ("ids",), "erase_kf": ("id",),
         "update": ("ids", "th"), "read": ("id", "which"), "reference": ("frame",), "octaves": ("id", "oct"),
         "cull_kf": ("cur", "keep", "max_culls", "cand"), "cull_mp": ("cur_kf", "ids", "found", "visible", "first_kf")}
CODES = tuple(LISTS)


def octaves(i, octs):
    return dict(op="octaves", id=int(i), oct=_ints(octs))


def cull_kf(cur=-1, keep=(), max_culls=0, cand=None):
    """cand: the caller's list, with cur = -1."""
    assert (cur == -1) == (cand is not None)
    return dict(op="cull_kf", cur=int(cur), keep=_ints(keep), max_culls=int(max_culls),
                cand=_ints(cand if cand is not None else []))


def cull_mp(cur_kf, ids, found, visible, first_kf):
    return dict(op="cull_mp", cur_kf=int(cur_kf), ids=_ints(ids), found=_ints(found), visible=_ints(visible),
                first_kf=_ints(first_kf))


class OnRestatement:
    def __init__(self):
        self.w = cu.World()

    def add(self, i, key, row):
        self.w.add_keyframe(i, key, row)

    def octaves(self, i, o):
        self.w.set_octaves(i, o)

    def set(self, i, idx, mp):
        self.w.set_matches(i, idx, mp)

    def erase_points(self, ids):
        self.w.erase_points(ids)

    def erase_kf(self, i):
        self.w.erase_keyframe(i)

    def update(self, ids, th):
        return self.w.update_connections(ids, th)

    def read(self, i, which):
        return self.w.ordered_list(i) if which == ORDERED else self.w.all_list(i)

    def reference(self, frame):
        return self.w.update_reference(frame)

    def cull_kf(self, cur, keep, max_culls, cand):
        return self.w.KeyFrameCulling(cur, keep, max_culls, cand)

    def cull_mp(self, cur_kf, ids, found, visible, first_kf):
        return self.w.MapPointCulling(cur_kf, ids, found, visible, first_kf)

    def members(self):
        return sorted(i for i, kf in self.w.kfs.items() if not kf.isBad())


class OnDevice:
    def __init__(self, m):
        self.m = m

    def add(self, i, key, row):
        self.m.add_keyframe(i, key, row)

    def octaves(self, i, o):
        self.m.set_octaves(i, o)

    def set(self, i, idx, mp):
        self.m.set_matches(i, idx, mp)

    def erase_points(self, ids):
        self.m.erase_points(ids)

    def erase_kf(self, i):
        self.m.erase_keyframe(i)

    def update(self, ids, th):
        return self.m.update_connections(ids, th)

    def read(self, i, which):
        return self.m.connections(i, which)

    def reference(self, frame):
        r = self.m.update_reference(frame)
        assert r["n_local_kf"] == len(r["local_kf"]) and r["n_local_mp"] == len(r["local_mp"])
        return r

    def cull_kf(self, cur, keep, max_culls, cand):
        r = self.m.cull_keyframes(cur, keep, max_culls, cand)
        assert r["n_cand"] == len(r["cand"]) and r["n_bad"] == len(r["bad_points"]) and r["n_done"] == len(r["decision"])
        return r

    def cull_mp(self, cur_kf, ids, found, visible, first_kf):
        return self.m.cull_points(cur_kf, ids, found, visible, first_kf)


def step(b, o):
    """Plays one operation on a backend; its result, or None."""
    k = o["op"]
    if k == "add":
        b.add(o["id"], o["key"], o["row"])
    elif k == "octaves":
        b.octaves(o["id"], o["oct"])
    elif k == "set":
        b.set(o["id"], o["idx"], o["mp"])
    elif k == "erase_points":
        b.erase_points(o["ids"])
    elif k == "erase_kf":
        b.erase_kf(o["id"])
    elif k == "update":
        u, f = b.update(o["ids"], o["th"])
        return dict(kind=k, updated=_ints(u), front=_ints(f))
    elif k == "read":
        kfs, ws = b.read(o["id"], o["which"])
        return dict(kind=k, kfs=_ints(kfs), weights=_ints(ws))
    elif k == "reference":
        r = b.reference(o["frame"])
        return dict(kind=k, frame_erased=_ints(r["frame_erased"]), local_kf=_ints(r["local_kf"]),
                    local_mp=_ints(r["local_mp"]), head=_ints([r["n_voters"], r["ref_kf"]]))
    elif k == "cull_kf":
        r = b.cull_kf(o["cur"], o["keep"], o["max_culls"], o["cand"] if o["cur"] == -1 else None)
        return dict(kind=k, **{f: _ints(r[f]) for f in FIELDS[k]})
    else:
        return dict(kind=k, action=_ints(b.cull_mp(o["cur_kf"], o["ids"], o["found"], o["visible"], o["first_kf"])))
    return None


def run_restatement(ops):
    b = OnRestatement()
    out = [r for r in (step(b, o) for o in ops) if r is not None]
    return out, b.w


def sizes_of(ops):
    kf = mp = kp = 1
    for o in ops:
        for f in ("id", "cur"):
            if f in o:
                kf = max(kf, o[f] + 1)
        for f in ("cand", "keep"):
            if f in o and len(o[f]):
                kf = max(kf, int(np.max(o[f])) + 1, len(o[f]))     # a list may name a keyframe twice
        for f in ("row", "mp", "ids", "frame"):
            if f in o and o["op"] != "update" and len(o[f]):
                mp = max(mp, int(np.max(o[f])) + 1)
        for f in ("row", "frame"):
            if f in o:
                kp = max(kp, len(o[f]))
    return kf, mp, kp


def run_device(ox, ctx, ops, sizes=None, keep=None):
    kf, mp, kp = sizes or sizes_of(ops)
    m = ox.CovisibilityMap(ctx, kf, mp, kp)
    try:
        b = OnDevice(m)
        out = [r for r in (step(b, o) for o in ops) if r is not None]
        if keep:
            keep(m)
    finally:
        m.close()
    return out


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["kind"] == w["kind"], (k, g["kind"], w["kind"])
        for f in FIELDS[g["kind"]]:
            assert np.array_equal(g[f], w[f]), (k, g["kind"], f, g[f][:24], w[f][:24])


def state_reads(members, frame):
    """Every list of the state: both reads of every member and a frame."""
    return read_all(members) + [reference(frame)]


# ---- hand-built cases: name -> (ops, answers of the cull operations in order) ----
def _world(rows, octs=None, keys=None):
    """rows: id -> row; octaves 0 unless given; keys ascending in the id unless given."""
    ops = []
    for i, row in rows.items():
        ops.append(add(i, (keys or {}).get(i, 1000 + i), row))
        ops.append(octaves(i, (octs or {}).get(i, [0] * len(row))))
    return ops


def kf_answer(cand, n_mps, n_red, dec, bad=(), n_done=None):
    return dict(cand=cand, n_done=[len(dec) if n_done is None else n_done], n_mps=n_mps, n_redundant=n_red, decision=dec,
                bad_points=list(bad))


def ratio_case(n, r):
    """Keyframe 1 holds n points, the first r of them held by 2, 3 and 4 too."""
    pts = list(range(100, 100 + n))
    return _world({1: pts, 2: pts[:r], 3: pts[:r], 4: pts[:r]}) + [cull_kf(cand=[1])]


def rule_cases():
    c = {}
    # point 10 in 1 and in three others: redundant, 1 of 1 > 0.9: culled; three observers remain: not bad
    c["three_others"] = (_world({1: [10], 2: [10], 3: [10], 4: [10]}) + [cull_kf(cand=[1])],
                         [kf_answer([1], [1], [1], [1])])
    # two others: not redundant
    c["two_others"] = (_world({1: [10], 2: [10], 3: [10]}) + [cull_kf(cand=[1])], [kf_answer([1], [1], [0], [0])])
    # octave 2 in keyframe 1: observers at 3 (o + 1) count
    c["octave_plus_one"] = (_world({1: [10], 2: [10], 3: [10], 4: [10]}, {1: [2], 2: [3], 3: [3], 4: [0]})
                            + [cull_kf(cand=[1])], [kf_answer([1], [1], [1], [1])])
    # one of them at 4 (o + 2) does not: two in scale
    c["octave_plus_two"] = (_world({1: [10], 2: [10], 3: [10], 4: [10]}, {1: [2], 2: [3], 3: [4], 4: [0]})
                            + [cull_kf(cand=[1])], [kf_answer([1], [1], [0], [0])])
    # 0.9 * 10 = 9.0 and 0.9 * 20 = 18.0 in FP64: 9 > 9.0 and 18 > 18.0 are false
    c["ratio_9_of_10"] = (ratio_case(10, 9), [kf_answer([1], [10], [9], [0])])
    c["ratio_10_of_10"] = (ratio_case(10, 10), [kf_answer([1], [10], [10], [1])])
    c["ratio_18_of_20"] = (ratio_case(20, 18), [kf_answer([1], [20], [18], [0])])
    # the twentieth point is keyframe 1's alone: nobody holds it after the cull and it goes bad
    c["ratio_19_of_20"] = (ratio_case(20, 19), [kf_answer([1], [20], [19], [1], [119])])
    # no point at all: 0 > 0.0 is false
    c["ratio_0_of_0"] = (_world({1: [-1, -1], 2: [10]}) + [cull_kf(cand=[1])], [kf_answer([1], [0], [0], [0])])
    # order: 10 in 1, 2, 3, 4.  Keyframe 3's list holds 1, 2, 4 at weight 1, the larger key first.  The first of 1
    # and 2 sees three others and goes; the second is left with two others and stays, and so does 4.
    four = {1: [10], 2: [10], 3: [10], 4: [10]}
    for name, keys, first, second in (("order_a_first", {1: 900, 2: 800, 4: 700, 3: 100}, 1, 2),
                                      ("order_b_first", {1: 800, 2: 900, 4: 700, 3: 100}, 2, 1)):
        c[name] = (_world(four, keys=keys) + [update([3], 1), cull_kf(cur=3), read(3, ORDERED), read(second, ALL)],
                   [kf_answer([first, second, 4], [1, 1, 1], [1, 0, 0], [1, 0, 0])])
    # a point left with two observers.  Keyframe 1: a private point 90, point 50 (in 1, 2, 5) and twenty points that
    # 3, 4, 6 hold too: 20 of 22 > 19.8, culled; 90 (nobody left) and 50 (2 and 5 left) go bad, in index order.
    # Keyframe 2: 50 and nine points of 3, 4, 6: 9 of 10 is not > 9.0; without 50, 9 of 9 > 8.1: culled.
    r1 = [90] + list(range(70, 74)) + [50] + list(range(74, 90))
    r2 = [50] + list(range(60, 69))
    others = list(range(60, 69)) + list(range(70, 90))
    shrink = {1: r1, 2: r2, 3: others, 4: others, 5: [50], 6: others}
    c["two_left_flips_next"] = (_world(shrink) + [cull_kf(cand=[1, 2]), reference([50, 90, 60])],
                                [kf_answer([1, 2], [22, 9], [20, 9], [1, 1], [90, 50])])
    c["without_the_cull_before"] = (_world(shrink) + [cull_kf(cand=[2])], [kf_answer([2], [10], [9], [0])])
    # the limit: the same pair with max_culls = 1 stops behind keyframe 1
    c["max_culls_stops"] = (_world(shrink) + [cull_kf(cand=[1, 2], max_culls=1), cull_kf(cand=[2])],
                            [kf_answer([1, 2], [22], [20], [1], [90, 50]), kf_answer([2], [9], [9], [1])])
    # keyframe 0 is skipped; 1 is redundant but kept (mbNotErase): nothing changes; 7 was never added; 2 goes; 2
    # again names no member; 3 still sees 0, 1, 4 and goes; 4 is left with 0 and 1
    five = {k: [10] for k in range(5)}
    c["zero_kept_dangling"] = (_world(five) + [cull_kf(cand=[0, 1, 7, 2, 2, 3, 4], keep=[1, 6])] + read_all([0, 1, 4]),
                               [kf_answer([0, 1, 7, 2, 2, 3, 4], [0, 1, 0, 1, 0, 1, 1], [0, 1, 0, 1, 0, 1, 0],
                                          [-1, 2, -1, 1, -1, 1, 0])])
    # an erased point in a row is skipped: 11 is erased, then written back into row 1
    two = {k: [10, 11] for k in (1, 2, 3, 4)}
    c["erased_point_skipped"] = (_world(two) + [erase_points([11]), set_matches(1, [1], [11]), cull_kf(cand=[1])],
                                 [kf_answer([1], [1], [1], [1])])
    # MapPointCulling with cur_kf 10.  30: erased.  31: 1 / 5 < 0.25.  32: 1 / 4 is not, age 0.  33: 3 / 0 = inf,
    # age 2, two observers.  34: 0 / 0 = NaN, age 2, three observers, not yet 3 keyframes old.  35: age 3, three
    # observers.  36: age 2, no observer.  37: age 3 and two observers: the earlier branch.
    mp_rows = {1: [30, 31, 32, 33, 34, 35, 37], 2: [31, 32, 33, 34, 35, 37], 3: [31, 32, 34, 35]}
    c["map_point_culling"] = (_world(mp_rows) + [erase_points([30]),
                                                 cull_mp(10, [30, 31, 32, 33, 34, 35, 36, 37], [5, 1, 1, 3, 0, 9, 9, 9],
                                                         [5, 5, 4, 0, 0, 9, 9, 9], [10, 10, 10, 8, 8, 7, 8, 7]),
                                                 reference([30, 31, 32, 33, 34, 35, 36, 37])],
                              [dict(action=[1, 2, 0, 3, 0, 4, 3, 3])])
    return c


def check_answers(results, want):
    """The cull results of a run against the hand-worked answers, in order."""
    got = [r for r in results if r["kind"] in ("cull_kf", "cull_mp")]
    assert len(got) == len(want)
    for k, (r, a) in enumerate(zip(got, want)):
        for f, v in a.items():
            assert r[f].tolist() == list(v), (k, f, r[f].tolist(), v)


# ---- the window scene with octaves ----
def culling_scene(seed, members, th=15, draw=60, window=80, stride=10, coarse_every=2):
    """A window scene (every point in about six rows) with octaves drawn in
    0..7; every second keyframe is coarse (octaves 5..7, so that most of its
    points' observers are in scale) and carries two points that one neighbour
    shares.
    Grown as LocalMapping grows it; then KeyFrameCulling of the last keyframe
    with two kept keyframes, the state's lists, MapPointCulling of recent
    points, and the lists again.  Returns (ops, the keyframes alive at the end
    according to the restatement)."""
    rng = np.random.default_rng(seed)
    rows = cc.window_rows(rng, members, draw=draw, window=window, step=stride)
    top = int(max(r.max() for r in rows)) + 1
    octs = []
    for k in range(members):
        coarse = k % coarse_every == 1
        octs.append(rng.integers(5, 8, len(rows[k])) if coarse else rng.integers(0, 8, len(rows[k])))
        if coarse and k + 1 < members:      # two empty places get a point of two observers
            holes = np.flatnonzero(rows[k] < 0)[:2]
            for h in holes:
                rows[k][h] = top
                empty = np.flatnonzero(rows[k + 1] < 0)
                rows[k + 1][empty[int(rng.integers(len(empty)))]] = top
                top += 1
    keys = cc.rand_keys(rng, members)
    ids = rng.permutation(members + 3)[:members]
    ops = []
    for k in range(members):
        ops += [add(ids[k], keys[k], rows[k]), octaves(ids[k], octs[k]), update([ids[k]], th)]
    cur = int(ids[members // 2])
    b = OnRestatement()
    for o in ops:
        step(b, o)
    lst = b.read(cur, ORDERED)[0]
    keep = [int(lst[i]) for i in range(1, len(lst), 4)][:8]     # LoopClosing holds some
    ops.append(cull_kf(cur=cur, keep=keep))
    gone = step(b, ops[-1])["bad_points"]
    alive = b.members()
    frame = rows[members // 2 + 1]
    ops += state_reads(alive, frame)
    # the recent points: two rows, points the cull took, and three that nobody observes, found as often as seen and
    # two keyframes old (action 3 whatever else is drawn)
    fresh = np.arange(top + 5, top + 8)
    recent = np.unique(np.concatenate([rows[members // 2], rows[members // 2 - 1], gone[:3], fresh]))
    recent = recent[recent >= 0]
    n = len(recent)
    cur_kf = members + 10
    found, visible, first = rng.integers(0, 8, n), rng.integers(0, 9, n), cur_kf - rng.integers(0, 5, n)
    is_fresh = np.isin(recent, fresh)
    found[is_fresh], visible[is_fresh], first[is_fresh] = 5, 5, cur_kf - 2
    ops.append(cull_mp(cur_kf, recent, found, visible, first))
    ops += state_reads(alive, frame)
    return ops, alive


def scene_properties(ops):
    """What the restatement shows of a culling scene's first KeyFrameCulling: a
    cull, a deferred cull, a candidate that stays, a point gone bad through a
    cull, and a candidate whose decision differs from the one the state before
    the call gives it."""
    b = OnRestatement()
    p = dict(cull=False, deferred=False, stays=False, bad_point=False, depends=False, mp_actions=False)
    for o in ops:
        if o["op"] == "cull_kf" and not p["cull"]:
            alone = {}
            for c in b.read(o["cur"], ORDERED)[0]:
                kf = b.w.kfs[c]
                if c != 0 and not kf.isBad():
                    m, r = cu.predicate_counts(b.w, c)
                    alone[c] = r > 0.9 * m
            r = step(b, o)
            dec = dict(zip(r["cand"].tolist(), r["decision"].tolist()))
            p["cull"] = 1 in dec.values()
            p["deferred"] = 2 in dec.values()
            p["stays"] = 0 in dec.values()
            p["bad_point"] = len(r["bad_points"]) > 0
            p["depends"] = any(alone[c] != (d in (1, 2)) for c, d in dec.items() if d >= 0)
            continue
        r = step(b, o)
        if o["op"] == "cull_mp":
            p["mp_actions"] = set(r["action"].tolist()) == {0, 1, 2, 3, 4}
    return p


def random_ops(seed, members, row_len, th=3):
    """`members` keyframes whose rows are row_len of the same row_len + 2
    points, one entry in ten empty, so that from five keyframes on most points
    have three other observers; octaves in 0..7, every second keyframe at 7
    throughout (all its observers are in scale).  Both culls interleaved with set_matches, erase_points, updates and frames; after
    every cull both reads of every member and a frame."""
    rng = np.random.default_rng(seed)
    universe = row_len + 2
    keys = cc.rand_keys(rng, members)
    ids = [int(i) for i in rng.permutation(members + 2)[:members]]

    def row():
        r = rng.choice(universe, size=row_len, replace=False).astype(np.int32)
        r[rng.random(row_len) < 0.1] = -1
        return r

    b = OnRestatement()
    ops = []

    def play(new):
        for o in new:
            step(b, o)
        ops.extend(new)

    for n, (i, k) in enumerate(zip(ids, keys)):
        play([add(i, k, row()), octaves(i, np.full(row_len, 7) if n % 2 else rng.integers(0, 8, row_len))])
    play([reference(row())])
    if not members:
        play([cull_kf(cand=[0, 1]), cull_mp(3, [0, 1], [1, 0], [1, 9], [0, 3])])
        return ops
    play([update(ids, th), cull_kf(cur=ids[0], keep=ids[1:2])])
    play(state_reads(b.members(), row()))
    if row_len:
        a = b.members()[0]
        play([set_matches(a, [0], [-1]), set_matches(a, [0, row_len - 1, 0], [-1, -1, universe]),
              erase_points([universe, 0, 1]), update(b.members()[::-1], th)])
    pts = rng.choice(universe + 2, size=min(universe + 2, 40), replace=False)
    n = len(pts)
    play([cull_mp(7, pts, rng.integers(0, 6, n), rng.integers(0, 7, n), 7 - rng.integers(0, 5, n))])
    play(state_reads(b.members(), row()))
    play([update(b.members(), th), cull_kf(cand=ids[::-1] + ids[:1], max_culls=1)])
    play(state_reads(b.members(), row()))
    play([cull_kf(cand=ids)])
    play(state_reads(b.members(), row()))
    return ops


# ---- the array form of (ops, results): what tests/golden/culling_sequence.npz holds ----
def encode(ops, results):
    code, key, ptr, val = [], [], [0], []
    for o in ops:
        code.append(CODES.index(o["op"]))
        key.append(o.get("key", 0))
        for f in LISTS[o["op"]]:
            val += [int(x) for x in np.atleast_1d(o[f])]
            ptr.append(len(val))
    rkind, rptr, rval = [], [0], []
    for r in results:
        rkind.append(CODES.index(r["kind"]))
        for f in FIELDS[r["kind"]]:
            rval += [int(x) for x in r[f]]
            rptr.append(len(rval))
    return dict(code=np.array(code, np.int32), key=np.array(key, np.uint64), ptr=np.array(ptr, np.int64),
                val=np.array(val, np.int32), rkind=np.array(rkind, np.int32), rptr=np.array(rptr, np.int64),
                rval=np.array(rval, np.int32))


def decode(d):
    ops, results = [], []
    at = 0
    for k, c in enumerate(d["code"]):
        name = CODES[int(c)]
        o = dict(op=name)
        for f in LISTS[name]:
            v = d["val"][d["ptr"][at]:d["ptr"][at + 1]].astype(np.int32)
            at += 1
            o[f] = int(v[0]) if f in ("id", "th", "which", "cur", "max_culls", "cur_kf") else v
        if name == "add":
            o["key"] = int(d["key"][k])
        ops.append(o)
    at = 0
    for c in d["rkind"]:
        name = CODES[int(c)]
        r = dict(kind=name)
        for f in FIELDS[name]:
            r[f] = d["rval"][d["rptr"][at]:d["rptr"][at + 1]].astype(np.int32)
            at += 1
        results.append(r)
    return ops, results


def golden_ops():
    """The recorded sequence: the culling scene at 14 keyframes (rows of 66),
    with the lists after both culls, then a KeyFrameCulling over a given list
    that stops at its first cull, and the lists again."""
    ops, alive = culling_scene(2043, 14, draw=55, stride=5)
    ops += [update(alive, 15), cull_kf(cand=alive[::-1], max_culls=1)]
    b = OnRestatement()
    for o in ops:
        step(b, o)
    return ops + state_reads(b.members(), ops[0]["row"])


def write_golden(path):
    ops = golden_ops()
    res, _ = run_restatement(ops)
    np.savez_compressed(path, **encode(ops, res))
