"""Operation sequences for the covisibility tests: builders, the runner that
plays one on the restatement (tests/covis_numpy.py), the runner that plays it
on the device, and the array form the golden file stores.

An operation is a dict: {"op": "add", "id", "key", "row"} | {"op": "set",
"id", "idx", "mp"} | {"op": "erase_points", "ids"} | {"op": "erase_kf", "id"}
| {"op": "update", "ids", "th"} | {"op": "read", "id", "which"} | {"op":
"reference", "frame"}.  The last three yield a result each, a dict of integer
arrays: update -> updated, front; read -> kfs, weights; reference ->
frame_erased, local_kf, local_mp, head (n_voters, ref_kf).

Keys are 64-bit values unrelated to the ids and to the add order."""
import numpy as np

import covis_numpy as cn

ORDERED, ALL = 0, 1
CODES = ("add", "set", "erase_points", "erase_kf", "update", "read", "reference")
FIELDS = {"update": ("updated", "front"), "read": ("kfs", "weights"),
          "reference": ("frame_erased", "local_kf", "local_mp", "head")}


def _ints(x):
    return np.asarray(x, np.int32).reshape(-1)


def add(i, key, row):
    return dict(op="add", id=int(i), key=int(key), row=_ints(row))


def set_matches(i, idx, mp):
    return dict(op="set", id=int(i), idx=_ints(idx), mp=_ints(mp))


def erase_points(ids):
    return dict(op="erase_points", ids=_ints(ids))


def erase_kf(i):
    return dict(op="erase_kf", id=int(i))


def update(ids, th=15):
    return dict(op="update", ids=_ints(ids), th=int(th))


def read(i, which=ORDERED):
    return dict(op="read", id=int(i), which=int(which))


def reference(frame):
    return dict(op="reference", frame=_ints(frame))


def read_all(ids):
    """Both reads of every keyframe: the derived lists against the stored ones."""
    return [read(i, w) for i in ids for w in (ORDERED, ALL)]


def run_restatement(ops):
    w = cn.World()
    out = []
    for o in ops:
        k = o["op"]
        if k == "add":
            w.add_keyframe(o["id"], o["key"], o["row"])
        elif k == "set":
            w.set_matches(o["id"], o["idx"], o["mp"])
        elif k == "erase_points":
            w.erase_points(o["ids"])
        elif k == "erase_kf":
            w.erase_keyframe(o["id"])
        elif k == "update":
            u, f = w.update_connections(o["ids"], o["th"])
            out.append(dict(kind=k, updated=_ints(u), front=_ints(f)))
        elif k == "read":
            kfs, ws = w.ordered_list(o["id"]) if o["which"] == ORDERED else w.all_list(o["id"])
            out.append(dict(kind=k, kfs=_ints(kfs), weights=_ints(ws)))
        else:
            r = w.update_reference(o["frame"])
            out.append(dict(kind=k, frame_erased=_ints(r["frame_erased"]), local_kf=_ints(r["local_kf"]),
                            local_mp=_ints(r["local_mp"]), head=_ints([r["n_voters"], r["ref_kf"]])))
    return out, w


def sizes_of(ops):
    """(kf_capacity, mp_capacity, max_keypoints) that hold the sequence."""
    kf = mp = kp = 1
    for o in ops:
        if "id" in o:
            kf = max(kf, o["id"] + 1)
        for f in ("row", "mp", "ids", "frame"):
            if f in o and o["op"] != "update" and len(o[f]):
                mp = max(mp, int(np.max(o[f])) + 1)
        for f in ("row", "frame"):
            if f in o:
                kp = max(kp, len(o[f]))
    return kf, mp, kp


def run_device(ox, ctx, ops, sizes=None, keep=None):
    """Plays ops on an ox.CovisibilityMap; keep: a function called with the
    map before it is closed."""
    kf, mp, kp = sizes or sizes_of(ops)
    m = ox.CovisibilityMap(ctx, kf, mp, kp)
    out = []
    try:
        for o in ops:
            k = o["op"]
            if k == "add":
                m.add_keyframe(o["id"], o["key"], o["row"])
            elif k == "set":
                m.set_matches(o["id"], o["idx"], o["mp"])
            elif k == "erase_points":
                m.erase_points(o["ids"])
            elif k == "erase_kf":
                m.erase_keyframe(o["id"])
            elif k == "update":
                u, f = m.update_connections(o["ids"], o["th"])
                out.append(dict(kind=k, updated=_ints(u), front=_ints(f)))
            elif k == "read":
                kfs, ws = m.connections(o["id"], o["which"])
                out.append(dict(kind=k, kfs=_ints(kfs), weights=_ints(ws)))
            else:
                r = m.update_reference(o["frame"])
                assert r["n_local_kf"] == len(r["local_kf"]) and r["n_local_mp"] == len(r["local_mp"])
                out.append(dict(kind=k, frame_erased=_ints(r["frame_erased"]), local_kf=_ints(r["local_kf"]),
                                local_mp=_ints(r["local_mp"]), head=_ints([r["n_voters"], r["ref_kf"]])))
        if keep:
            keep(m)
    finally:
        m.close()
    return out


def assert_same(got, want):
    """Exact, field by field, lists in order."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["kind"] == w["kind"], (k, g["kind"], w["kind"])
        for f in FIELDS[g["kind"]]:
            assert np.array_equal(g[f], w[f]), (k, g["kind"], f, g[f][:24], w[f][:24])


# ---- random scenes ----
def rand_keys(rng, n):
    """n distinct 64-bit keys, some above 2^63, in no relation to anything."""
    keys = set()
    while len(keys) < n:
        keys.add(int(rng.integers(1, 2 ** 62)) * 4 + int(rng.integers(0, 4)))
    keys = list(keys)
    rng.shuffle(keys)
    return keys


def window_rows(rng, members, draw=60, window=150, step=12):
    """Row k: `draw` of the `window` consecutive point ids from k * step, in
    random order, one index in six empty."""
    rows = []
    for k in range(members):
        pts = rng.choice(window, size=draw, replace=False) + k * step
        row = []
        it = iter(pts)
        for i in range(draw + draw // 5):
            row.append(-1 if i % 6 == 5 else int(next(it)))
        rows.append(np.array(row, np.int32))
    return rows


def window_scene(seed, members, th=15, batch=65):
    """The window scene as LocalMapping grows it (add, then UpdateConnections
    of the new keyframe), then the edits that make a stale entry: keyframe e
    trades its row for private points and five points of a far keyframe, is
    updated (a fallback list; the far keyframe's list shows an entry below th)
    and erased.  Reads of every keyframe after each stage, frames that are one
    keyframe's points, a batched update in between."""
    rng = np.random.default_rng(seed)
    rows = window_rows(rng, members)
    keys = rand_keys(rng, members)
    ids = rng.permutation(members + 3)[:members]          # ids in no order either
    order = rng.permutation(members)                      # add order
    ops = []
    for k in order:
        ops += [add(ids[k], keys[k], rows[k]), update([ids[k]], th)]
    ops += read_all(ids)
    frame_of = members // 2
    ops.append(reference(rows[frame_of]))
    # keyframe e leaves its neighbourhood
    e, far = members // 2 + 1, 0
    n = len(rows[e])
    top = int(max(r.max() for r in rows)) + 1
    new = np.arange(top, top + n, dtype=np.int32)
    shared = rows[far][rows[far] >= 0][:5]
    new[:5] = shared
    ops += [set_matches(ids[e], np.arange(n), np.full(n, -1)), set_matches(ids[e], np.arange(n), new),
            update([ids[e]], th)]
    ops += read_all([ids[e], ids[far], ids[e - 1]])
    ops += [erase_kf(ids[e])]
    left = [ids[k] for k in range(members) if k != e]
    ops += read_all(left)
    ops.append(reference(rows[frame_of]))
    # some points turn bad, one of them in the frame; a batch of updates
    bad = rows[frame_of][rows[frame_of] >= 0][:3]
    ops += [erase_points(bad), reference(rows[frame_of])]
    ops += [update(left[:batch], th)] + read_all(left[:batch]) + [reference(rows[frame_of - 1])]
    return ops


def scene_properties(ops, th=15):
    """What the restatement's results show of a scene: an ordered list with
    entries below th, a fallback list, a weight tie, a stale entry, a
    neighbour pass that appends."""
    res, _ = run_restatement(ops)
    p = dict(below_th=False, fallback=False, tie=False, appends=False, stale=False)
    gone = set()
    it = iter(res)
    for o in ops:
        if o["op"] == "erase_kf":
            gone.add(o["id"])
        if o["op"] not in FIELDS:
            continue
        r = next(it)
        if o["op"] == "reference" and len(r["local_kf"]) > r["head"][0]:
            p["appends"] = True
        if o["op"] == "read" and o["which"] == ORDERED:
            ws = r["weights"]
            if len(ws) > 1 and ws.min() < th:
                p["below_th"] = True
            if len(ws) == 1 and ws[0] < th:
                p["fallback"] = True
            if np.any(ws[1:] == ws[:-1]):
                p["tie"] = True
            if gone & set(r["kfs"].tolist()):
                p["stale"] = True
    return p


def random_ops(seed, members, row_len, th=3):
    """`members` keyframes with rows of row_len entries over a small universe
    of points, so that most pairs share some; interleaved set_matches,
    erase_points, erase_keyframe and batched updates (1, 2, all) with reads
    and frames of row_len entries that hold a point twice."""
    rng = np.random.default_rng(seed)
    universe = max(3 * row_len // 2, 2)
    keys = rand_keys(rng, members)
    ids = [int(i) for i in rng.permutation(members + 2)[:members]]

    def row():
        k = min(row_len, universe)
        r = rng.choice(universe, size=k, replace=False).astype(np.int32)
        r[rng.random(k) < 1 / 6] = -1
        return r

    def frame():
        f = row()
        if len(f) >= 2 and f[0] >= 0:
            f[-1] = f[0]                                   # a point twice
        return f

    ops = [add(i, k, row()) for i, k in zip(ids, keys)]
    ops += [reference(frame())]
    if not members:
        return ops
    ops += [update(ids[:1], th), update(ids[:2], th), update(ids, th)] + read_all(ids) + [reference(frame())]
    if row_len:
        a = ids[0]
        ops += [set_matches(a, [0], [-1]), set_matches(a, [0, row_len - 1, 0], [-1, -1, universe]),
                erase_points([universe, 0, 1]), update(ids[::-1], th)] + read_all(ids) + [reference(frame())]
    if members >= 3:
        ops += [erase_kf(ids[1])]
        left = [i for i in ids if i != ids[1]]
        ops += read_all(left) + [reference(frame()), update(left, th)] + read_all(left) + [reference(frame())]
    return ops


# ---- the array form of (ops, results): what tests/golden/covis_sequence.npz holds ----
def encode(ops, results):
    code, ident, aux, key = [], [], [], []
    ptr, val = [0], []
    for o in ops:
        code.append(CODES.index(o["op"]))
        ident.append(o.get("id", -1))
        aux.append(o.get("th", o.get("which", 0)))
        key.append(o.get("key", 0))
        lists = {"add": ("row",), "set": ("idx", "mp"), "erase_points": ("ids",), "update": ("ids",),
                 "reference": ("frame",)}.get(o["op"], ())
        for j in range(2):                                  # two lists per op
            if j < len(lists):
                val += [int(x) for x in o[lists[j]]]
            ptr.append(len(val))
    rptr, rval, rkind = [0], [], []
    for r in results:
        rkind.append(CODES.index(r["kind"]))
        for j in range(4):                                  # four fields per result
            f = FIELDS[r["kind"]]
            if j < len(f):
                rval += [int(x) for x in r[f[j]]]
            rptr.append(len(rval))
    return dict(code=np.array(code, np.int32), id=np.array(ident, np.int32), aux=np.array(aux, np.int32),
                key=np.array(key, np.uint64), ptr=np.array(ptr, np.int64), val=np.array(val, np.int32),
                rkind=np.array(rkind, np.int32), rptr=np.array(rptr, np.int64), rval=np.array(rval, np.int32))


def decode(d):
    ops, results = [], []
    for k, c in enumerate(d["code"]):
        name = CODES[int(c)]
        l = [d["val"][d["ptr"][2 * k + j]:d["ptr"][2 * k + j + 1]].astype(np.int32) for j in range(2)]
        i, a = int(d["id"][k]), int(d["aux"][k])
        ops.append({"add": lambda: add(i, int(d["key"][k]), l[0]), "set": lambda: set_matches(i, l[0], l[1]),
                    "erase_points": lambda: erase_points(l[0]), "erase_kf": lambda: erase_kf(i),
                    "update": lambda: update(l[0], a), "read": lambda: read(i, a),
                    "reference": lambda: reference(l[0])}[name]())
    for k, c in enumerate(d["rkind"]):
        name = CODES[int(c)]
        r = dict(kind=name)
        for j, f in enumerate(FIELDS[name]):
            r[f] = d["rval"][d["rptr"][4 * k + j]:d["rptr"][4 * k + j + 1]].astype(np.int32)
        results.append(r)
    return ops, results


def golden_ops():
    """The recorded sequence: 14 keyframes of the window scene with rows of 72
    (windows 20 apart, so that a frame does not reach every keyframe), the
    stale-entry edits, a batch."""
    rng = np.random.default_rng(2024)
    members = 14
    rows = window_rows(rng, members, draw=60, window=150, step=20)
    keys = rand_keys(rng, members)
    ids = [int(i) for i in rng.permutation(16)[:members]]
    th = 15
    ops = []
    for k in rng.permutation(members):
        ops += [add(ids[k], keys[k], rows[k]), update([ids[k]], th)]
    ops += read_all(ids) + [reference(rows[3])]
    n = len(rows[7])
    new = np.arange(1000, 1000 + n, dtype=np.int32)
    new[:5] = rows[0][rows[0] >= 0][:5]
    ops += [set_matches(ids[7], np.arange(n), np.full(n, -1)), set_matches(ids[7], np.arange(n), new),
            update([ids[7]], th)] + read_all([ids[7], ids[0], ids[6]]) + [erase_kf(ids[7])]
    left = [i for i in ids if i != ids[7]]
    ops += read_all(left) + [reference(rows[6]), erase_points(rows[6][rows[6] >= 0][:4]), reference(rows[6]),
                             update(left, th)] + read_all(left) + [reference(rows[8])]
    return ops


# ---- hand-built cases, one per rule, with the answer worked out by hand ----
def limit_case(v):
    """v voters, each with one private partner of weight 15 outside the frame.
    Voter k holds frame point k and 15 points of its own, which its partner
    v + k holds too.  The voters' keys fall with k, so the key order is
    v - 1 ... 0.  Answer: (n_voters, local_kf)."""
    ops = []
    for k in range(v):
        own = 1000 + 15 * k + np.arange(15)
        ops += [add(k, 5000 - k, np.concatenate([[k], own])), add(v + k, 9000 + k, own)]
    ops += [update(list(range(v)), 15), reference(np.arange(v))]
    voters = list(range(v - 1, -1, -1))
    # before each voter: stop once the list holds more than 80
    appended = [v + k for k in voters[:max(0, 81 - v)]]
    return ops, (v, voters + appended)


def stale_case(all_listed):
    """Keyframe 0 (the smallest key) is connected to 1..11 with weights
    11..1.  Keyframe 1 then trades its row for keyframe 12's points, is
    updated and erased: W[0][1] stays, a stale entry at the head of 0's list.
    The frame sees 0, 2, 3 (or 0, 2..10 with all_listed)."""
    ops, row0 = [], [500]
    base = 100
    groups = {}
    for k in range(1, 12):
        groups[k] = list(range(base, base + 12 - k))
        base += 12 - k
        row0 += groups[k]
    ops.append(add(0, 5, row0))
    for k in range(1, 12):
        ops.append(add(k, 100 + k, groups[k] + [500 + k]))
    ops += [add(12, 7, [900, 901]), update([0], 1)]
    n1 = len(groups[1]) + 1
    ops += [set_matches(1, np.arange(n1), np.full(n1, -1)), set_matches(1, [0, 1], [900, 901]), update([1], 1),
            erase_kf(1), read(0, ORDERED)]
    seen = range(2, 11) if all_listed else (2, 3)
    ops.append(reference([500] + [500 + k for k in seen]))
    return ops


def rule_cases():
    """name -> (ops, the results every result-yielding op must give, in
    order).  update: (updated, front); read: (kfs, weights); reference: a dict
    of the fields that the rule fixes."""
    c = {}
    rows3 = [add(0, 50, [1, 2, 3, 4]), add(1, 90, [1, 2, 10]), add(2, 20, [3, 4, 11])]
    # 1: counts 2 and 2 below th 3: one fallback entry, the smaller key (keyframe 2) of the equal maxima
    c["fallback_smaller_key"] = (rows3 + [update([0], 3), read(0, ORDERED), read(0, ALL), read(2, ORDERED),
                                          read(1, ORDERED)],
                                 [([1], [2]), ([2], [2]), ([2, 1], [2, 2]), ([0], [2]), ([], [])])
    # 2: both reach th 2: equal weights, the larger key (keyframe 1) first
    c["tie_larger_key_first"] = (rows3 + [update([0], 2), read(0, ORDERED)], [([1], [1]), ([1, 2], [2, 2])])
    # 3: J = 0 (key 10) counts I = 1 three times and K = 2 once (below th 3); I's update adds the same weight
    # to J: `else return`, J's list stays filtered
    jik = [add(0, 10, [1, 2, 3, 4, 5]), add(1, 30, [1, 2, 3, 9]), add(2, 20, [4, 8])]
    same = jik + [update([0], 3), read(0, ORDERED), read(1, ORDERED), update([1], 3), read(0, ORDERED), read(0, ALL)]
    c["add_connection_same_weight"] = (same, [([1], [1]), ([1], [3]), ([0], [3]), ([1], [0]), ([1], [3]),
                                              ([2, 1], [1, 3])])
    # 4: I's row gains point 4: weight 4 differs from J's 3: J's list is rebuilt and shows K's 1
    c["add_connection_new_weight"] = (same + [set_matches(1, [3], [4]), update([1], 3), read(0, ORDERED),
                                              read(1, ORDERED), read(1, ALL), read(2, ORDERED)],
                                      [([1], [1]), ([1], [3]), ([0], [3]), ([1], [0]), ([1], [3]), ([2, 1], [1, 3]),
                                       ([1], [0]), ([1, 2], [4, 1]), ([0], [4]), ([0, 2], [4, 1]), ([], [])])
    # 5: every match of 0 gone: KFcounter is empty, the function returns, the old connection stays
    c["all_zero_unchanged"] = ([add(0, 9, [1, 2, 3]), add(1, 4, [1, 2, 3, 7]), update([0], 2),
                                set_matches(0, [0, 1, 2], [-1, -1, -1]), update([0], 2), read(0, ORDERED),
                                read(1, ORDERED)],
                               [([1], [1]), ([0], [-1]), ([1], [3]), ([0], [3])])
    # 6: point 3 three times in the frame: keyframe 1 collects 3 votes against 0's 2
    two = [add(0, 10, [1, 2, 5]), add(1, 20, [3, 6])]
    c["twice_votes_twice"] = (two + [reference([1, 2, 3]), reference([1, 2, 3, 3, 3])],
                              [dict(local_kf=[0, 1], head=[2, 0], local_mp=[1, 2, 5, 3, 6], frame_erased=[0, 0, 0]),
                               dict(local_kf=[0, 1], head=[2, 1], local_mp=[1, 2, 5, 3, 6],
                                    frame_erased=[0, 0, 0, 0, 0])])
    # 7: the 80 limit
    for v in (79, 80, 81, 82):
        ops, (nv, lk) = limit_case(v)
        assert len(lk) == (82 if v == 82 else 81)
        c["limit_%d" % v] = (ops, [([1] * v, [v + k for k in range(v)]), dict(local_kf=lk, head=[nv, v - 1])])
    # 8: 0's list is 1 (erased), 2, 3 (both listed), 4, ... 11: 4 is appended; with 2..10 listed nothing is,
    # 11 at place 11 is not reached.  The other voters' lists hold 0 alone.
    head0 = (list(range(1, 12)), list(range(11, 0, -1)))
    c["stale_then_listed"] = (stale_case(False), [([1], [1]), ([1], [12]), head0,
                                                  dict(local_kf=[0, 2, 3, 4], head=[3, 0])])
    c["place_11_not_reached"] = (stale_case(True), [([1], [1]), ([1], [12]), head0,
                                                    dict(local_kf=[0] + list(range(2, 11)), head=[10, 0])])
    # 9: first occurrence across keyframes; 6 is erased: flagged in the frame, no vote for 2 (which got it
    # back by a later edit), not a local point
    c["local_points_and_erased"] = ([add(0, 10, [5, -1, 6, 7]), add(1, 20, [7, 8, 5, 9]), add(2, 30, [-1, 20]),
                                     erase_points([6]), set_matches(2, [0], [6]), reference([5, 6, 9])],
                                    [dict(frame_erased=[0, 1, 0], local_kf=[0, 1], head=[2, 1], local_mp=[5, 7, 8, 9])])
    return c


def check_answers(results, want):
    assert len(results) == len(want)
    for k, (r, a) in enumerate(zip(results, want)):
        if isinstance(a, dict):
            for f, v in a.items():
                assert r[f].tolist() == list(v), (k, f, r[f].tolist(), v)
        else:
            f0, f1 = FIELDS[r["kind"]][:2]
            assert (r[f0].tolist(), r[f1].tolist()) == (list(a[0]), list(a[1])), (k, r[f0].tolist(), r[f1].tolist(), a)
