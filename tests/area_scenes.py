"""Hand-built scenes for the two-phase area searches (k_area_lists /
k_area_replay: WindowSearch and the pair, motion-model and local-map
SearchByProjection): numpy data, a mirror of the kernels' decisions, and the
call of one search on a scene (test data and checker only).

A scene is two sets of keypoints and descriptors on the 640 x 480 view grid
(64 x 48 cells of 10 px): the queries (F1 / the last frame / the map points)
and the searched keypoints (F2 / the current frame), plus validity flags,
already-assigned flags and angles.  Every scene is made of *groups*: queries
at one centre and their candidates within 8 px of it, at one octave.  Groups
stand 80 px apart, or share a centre at octaves that each search's level
filter separates, so a group's candidate lists hold its own candidates only
under all four searches at the base radius R0 = 10:

  window, pair   radius R0,            levels oct .. oct          octaves 0, 1, 2
  motion         radius R0 scale[oct], levels oct - 1 .. oct + 1  octaves 0, 3, 6
  local map      radius R0 scale[pred], levels pred - 1 .. pred   octaves 0, 2, 4

(the largest radius is R0 * 1.2^6 < 30 px).  The three octaves of a kind are
its *bands* 0, 1, 2.

Chains.  N queries with one position and the all-zero descriptor, N chain
candidates where candidate k has its first dist[k] bits set (default k + 1),
and fillers further than TH_HIGH = 100 that are never accepted and only set
the list length.  The reference's loop gives chain query k chain candidate
k; the parallel rounds settle one more member per round, N + 1 rounds in
all.  `expect` records what each query must take by construction.

Posed scenes.  Scene.posed(R, t) moves the query points to Rcw^T (xyz - tcw)
(float64, rounded to float32) and passes [Rcw | tcw] in place of the identity,
so the projection searches see a full rotation while every query still
projects to its centre within 1e-3 px; candidates stay 2 px inside or
outside every box, so `expect` is unchanged.  The posed local-map kind runs
through isInFrustum (orbx_search_local_map) with normals and distance ranges
rotated along; isInFrustum cannot predict level 0 away from ratio == 1, so
its band-0 queries predict level 1 (levels 0 .. 1, radius 12 px).

Also the white-box mirror of launch_area_search's LDS decisions and of the
replay's claim rounds (mirror()), shared by the CPU and the GPU tests, and
track_chain(): a chain of displacement among a tracked frame's natural
keypoints, for orbx_track_frame's motion search.
"""
import numpy as np

from oracle_lib import KEYPOINT
from test_match_numpy import COLS, ROWS, Grid, POP

F32 = np.float32
W, H = 640, 480
CAM = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
R0 = 10
TH_HIGH = 100
KINDS = ("window", "pair", "motion", "local")
BANDS = {"window": (0, 1, 2), "pair": (0, 1, 2), "motion": (0, 3, 6), "local": (0, 2, 4)}
T_IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)

# k_area_replay / launch_area_search (orbx_search.hip), mirrored
K_AREA_CAP = 128
K_REPLAY_THREADS = 1024
K_REPLAY_ENTRIES = 8192
K_MAX_ROUNDS = 24
K_AREA_QUERY_INTS = 5
K_LDS = 160 * 1024 - 1024
K_MAX_FEATURES = 4096

# centres of the special groups: columns 50 and 130 hold them in the large
# scenes (the filler spots start at x = 230), all columns in the small ones
SPOTS = [(50 + 80 * cx, 50 + 80 * cy) for cx in range(7) for cy in range(5)]
FILL_SPOTS = [(240 + 24 * ix, 24 + 24 * iy) for iy in range(19) for ix in range(16)]


def scale_factors(nlevels=8, scale=1.2):
    sf = float(F32(scale))
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(float(s[-1]) * sf))
    return np.array(s, np.float32)


def bits(n):
    """Descriptor with its first n bits set: n bits from the all-zero one."""
    d = np.zeros(32, np.uint8)
    d[:n // 8] = 255
    if n % 8:
        d[n // 8] = (1 << (n % 8)) - 1
    return d


def far(rng):
    """Descriptor of 149 .. 248 set bits: never accepted by an all-zero query."""
    d = np.full(32, 255, np.uint8)
    for b in rng.choice(np.arange(24, 256), int(rng.integers(8, 108)), replace=False):
        d[b // 8] &= ~np.uint8(1 << (b % 8))
    return d


class Builder:
    """Collects groups, then lays the queries and candidates out in index
    order: special queries keep their order at spread-out indices between the
    others, candidates are permuted."""

    def __init__(self, kind, seed):
        self.kind = kind
        self.rng = np.random.default_rng(seed)
        self.q = []        # dict(x, y, oct, desc, angle, valid, special, tag)
        self.c = []        # dict(x, y, oct, desc, angle, assigned)
        self.expect = []   # (query id, candidate id or -1)
        self.above = []    # (a, b): candidate a must get a larger index than b
        self.tags = {}     # tag -> query ids

    def band(self, b):
        return BANDS[self.kind][b]

    def query(self, centre, octave, desc, angle=0.0, valid=1, special=True, tag=None):
        self.q.append(dict(x=centre[0], y=centre[1], oct=octave, desc=desc, angle=angle, valid=valid,
                           special=special))
        if tag is not None:
            self.tags.setdefault(tag, []).append(len(self.q) - 1)
        return len(self.q) - 1

    def cand(self, centre, octave, desc, off=None, assigned=0, angle=0.0):
        if off is None:
            off = self.rng.integers(-8, 9, 2)
        self.c.append(dict(x=centre[0] + int(off[0]), y=centre[1] + int(off[1]), oct=octave, desc=desc, angle=angle,
                           assigned=assigned))
        return len(self.c) - 1

    def fillers(self, centre, octave, n):
        return [self.cand(centre, octave, far(self.rng)) for _ in range(n)]

    def chain(self, centre, band, n, fillers, dist=None, tag="chain", invalid=(), assigned=(), angles=None,
              odd=None):
        """n chain queries and n chain candidates at `centre`, `fillers`
        never-accepted candidates.  invalid: members whose q_valid is
        cleared; assigned: chain candidates already assigned; odd: (member
        position, descriptor) of one more query put before that member."""
        octave = self.band(band)
        if self.kind == "window":
            assigned = ()      # WindowSearch has no such input
        dist = list(dist) if dist is not None else list(range(1, n + 1))
        cs = [self.cand(centre, octave, bits(dist[k]), assigned=int(k in assigned)) for k in range(n)]
        self.fillers(centre, octave, fillers)
        free = [c for k, c in enumerate(cs) if k not in assigned]
        for k in range(n):
            if odd is not None and odd[0] == k:
                self.expect.append((self.query(centre, octave, odd[1], tag=tag + "_odd"), -1))
            q = self.query(centre, octave, np.zeros(32, np.uint8), angle=0.0 if angles is None else angles[k],
                           valid=int(k not in invalid), tag=tag)
            if k in invalid:
                self.expect.append((q, -1))
            else:
                self.expect.append((q, free.pop(0) if free else -1))
        return cs

    def fill(self, nq, n2, per_spot=16, spots=None):
        """Unrelated queries and candidates at octave band 0: spots of
        per_spot candidates with random descriptors; the queries go round the
        spots, each with the descriptor of one candidate of its spot with up
        to three bits changed (so two queries can want one candidate)."""
        spots = FILL_SPOTS if spots is None else spots
        octave = self.band(0)
        ns = max(1, -(-n2 // per_spot))
        assert ns <= len(spots), (n2, per_spot)
        per = [[] for _ in range(ns)]
        for j in range(n2):
            d = self.rng.integers(0, 256, 32, dtype=np.uint8)
            per[j % ns].append(self.cand(spots[j % ns], octave, d))
        for i in range(nq):
            s = i % ns
            if per[s]:
                d = self.c[per[s][(i // ns) % len(per[s])]]["desc"].copy()
                for b in self.rng.integers(0, 256, int(self.rng.integers(0, 4))):
                    d[b // 8] ^= np.uint8(1 << (b % 8))
            else:
                d = self.rng.integers(0, 256, 32, dtype=np.uint8)
            self.query(spots[s], octave, d, special=False, tag="fill")

    def finish(self, name, nnratio=1.0, check_ori=0, slots=None):
        """slots: the special queries' final indices (ascending), else drawn."""
        rng = self.rng
        nq, n2 = len(self.q), len(self.c)
        special = [i for i, q in enumerate(self.q) if q["special"]]
        others = [i for i, q in enumerate(self.q) if not q["special"]]
        if slots is None:
            slots = np.sort(rng.choice(nq, len(special), replace=False)) if special else np.array([], np.int64)
        slots = np.asarray(slots, np.int64)
        assert len(slots) == len(special) and (np.diff(slots) > 0).all()
        order = np.full(nq, -1, np.int64)          # final index -> query id
        order[slots] = special
        order[order < 0] = others
        qpos = np.empty(nq, np.int64)
        qpos[order] = np.arange(nq)
        cpos = rng.permutation(n2)                 # candidate id -> final index
        for a, b in self.above:
            if cpos[a] < cpos[b]:
                cpos[a], cpos[b] = cpos[b], cpos[a]
        corder = np.empty(n2, np.int64)
        corder[cpos] = np.arange(n2)
        k1, k2 = np.zeros(nq, KEYPOINT), np.zeros(n2, KEYPOINT)
        for arr, items, idx in ((k1, self.q, order), (k2, self.c, corder)):
            for f, key in (("x", "x"), ("y", "y"), ("angle", "angle"), ("octave", "oct")):
                arr[f] = [items[i][key] for i in idx]
            arr["size"] = 31.0
        d1 = np.ascontiguousarray(np.array([self.q[i]["desc"] for i in order], np.uint8).reshape(nq, 32))
        d2 = np.ascontiguousarray(np.array([self.c[i]["desc"] for i in corder], np.uint8).reshape(n2, 32))
        valid = np.array([self.q[i]["valid"] for i in order], np.uint8)
        assigned = np.array([self.c[i]["assigned"] for i in corder], np.uint8)
        expect = {int(qpos[q]): (int(cpos[c]) if c >= 0 else -1) for q, c in self.expect}
        tags = {t: sorted(int(qpos[i]) for i in ids) for t, ids in self.tags.items()}
        return Scene(name, self.kind, k1, d1, k2, d2, valid, assigned, F32(nnratio), int(check_ori), expect, tags)


class Scene:
    def __init__(self, name, kind, k1, d1, k2, d2, valid, assigned, nnratio, check_ori, expect, tags):
        self.name, self.kind = name, kind
        self.k1, self.d1, self.k2, self.d2 = k1, d1, k2, d2
        self.valid, self.assigned = valid, assigned
        self.nnratio, self.check_ori = nnratio, check_ori
        self.expect, self.tags = expect, tags
        self.nq, self.n2 = len(k1), len(k2)
        # the projection kinds' inputs: points at depth 1 under the identity pose
        self.xyz = np.ascontiguousarray(np.stack([(k1["x"] - CAM[2]) / CAM[0], (k1["y"] - CAM[3]) / CAM[1],
                                                  np.ones(self.nq, np.float32)], 1).astype(np.float32))
        self.proj = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
        self.pred = np.ascontiguousarray(k1["octave"].astype(np.int32))
        self.vcos = np.full(self.nq, 0.9, np.float32)    # <= 0.998: RadiusByViewingCos gives 4.0
        self.th_local = F32(R0 / 4.0)
        self.th_motion = F32(R0)
        self.T, self.pose = T_IDENTITY, None

    def posed(self, R, t):
        """The same scene seen from the pose Xc = R Xw + t."""
        import copy
        s = copy.copy(self)
        R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
        Xc = self.xyz.astype(np.float64)
        s.xyz = np.ascontiguousarray(((Xc - t) @ R).astype(np.float32))       # rows of R^T (Xc - t)
        s.T = np.ascontiguousarray(np.concatenate([R, t[:, None]], 1).astype(np.float32).reshape(-1))
        s.pose, s.name = (R, t), self.name + "-posed"
        if self.kind == "local":
            s.pred = np.ascontiguousarray(np.maximum(self.pred, 1))
            dist = np.linalg.norm(Xc, axis=1)
            e = Xc / dist[:, None]
            o = np.cross(e, [0.3, -0.5, 0.8])
            o /= np.linalg.norm(o, axis=1, keepdims=True)
            s.normal = np.ascontiguousarray(((0.9 * e + np.sqrt(1 - 0.81) * o) @ R).astype(np.float32))
            ratio = scale_factors()[s.pred].astype(np.float64) * 0.93          # between scale[pred - 1] and scale[pred]
            s.mp_dist = np.ascontiguousarray(np.stack([dist / ratio, dist * 1.5], 1).astype(np.float32))
            s.Ow = (-(R.T @ t)).astype(np.float32)
        return s

    def centres(self):
        """Search centre and radius of every query, as the search computes them."""
        sf = scale_factors()
        k1 = self.k1
        if self.kind == "window":
            return k1["x"].copy(), k1["y"].copy(), np.full(self.nq, F32(R0))
        if self.kind == "local":
            r = F32(F32(4.0) * self.th_local) * sf[self.pred]
            return self.proj[:, 0].copy(), self.proj[:, 1].copy(), r.astype(np.float32)
        T, X = self.T.reshape(3, 4), self.xyz     # as the searches project (unposed: xc = x, invz = 1)
        c = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
        inv = (1.0 / c[2].astype(np.float64)).astype(np.float32)
        u = (CAM[0] * c[0]) * inv + CAM[2]
        v = (CAM[1] * c[1]) * inv + CAM[3]
        r = np.full(self.nq, F32(R0)) if self.kind == "pair" else self.th_motion * sf[k1["octave"]]
        return u.astype(np.float32), v.astype(np.float32), r.astype(np.float32)

    def levels(self):
        o = self.k1["octave"].astype(np.int64)
        if self.kind in ("window", "pair"):
            return o, o
        if self.kind == "motion":
            return o - 1, o + 1
        p = self.pred.astype(np.int64)
        return p - 1, p


# ---------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------
def chain_scene(kind, n, seed=1, fillers=20, extra=60, **kw):
    """One chain of n in a list of n + fillers (<= 64) at band 0, between
    unrelated queries."""
    b = Builder(kind, seed)
    b.chain(SPOTS[0], 0, n, fillers, **kw)
    b.fill(extra, extra, per_spot=4, spots=SPOTS[10:])
    return b.finish(f"chain{n}")


def three_chains(kind, n, seed=2):
    """Chains of n at one centre in lists of 50 (sorted, a thread per query),
    100 (index order, a wave per query) and 150 (over kAreaCap: the replay
    rescans the frame), in the three bands."""
    b = Builder(kind, seed)
    for band, total in ((0, 50), (1, 100), (2, 150)):
        b.chain(SPOTS[0], band, n, total - n, tag=f"chain{band}")
    b.fill(40, 40, per_spot=4, spots=SPOTS[10:])
    return b.finish(f"chain{n}x3")


def _tie(b, centre, band, fillers, hi_first, third=False, tag="tie"):
    """Two queries, two candidates at equal distance 5 in different cells
    (cell x differs: cell order puts `first` first); hi_first: the candidate
    of the earlier cell has the larger index.  third: a nearer candidate
    (distance 2) makes the tie one between second and third."""
    octave = b.band(band)
    first = b.cand(centre, octave, np.array([0b11111] + [0] * 31, np.uint8), off=(-7, 3))
    second = b.cand(centre, octave, np.array([0, 0b11111] + [0] * 30, np.uint8), off=(7, -3))
    b.above.append((first, second) if hi_first else (second, first))
    order = [first, second]
    if third:
        order.insert(0, b.cand(centre, octave, bits(2), off=(0, 0)))
    b.fillers(centre, octave, fillers)
    for c in order:
        b.expect.append((b.query(centre, octave, np.zeros(32, np.uint8), tag=tag), c))


def ties(kind, seed=3):
    b = Builder(kind, seed)
    _tie(b, SPOTS[0], 0, 6, hi_first=True)
    _tie(b, SPOTS[1], 0, 6, hi_first=False)
    _tie(b, SPOTS[2], 0, 10, hi_first=True, third=True)
    _tie(b, SPOTS[3], 1, 70, hi_first=True, tag="tie_mid")
    _tie(b, SPOTS[4], 2, 140, hi_first=True, tag="tie_long")
    _tie(b, SPOTS[5], 1, 70, hi_first=False, tag="tie_mid")
    _tie(b, SPOTS[6], 2, 140, hi_first=False, tag="tie_long")
    return b.finish("ties")


BOUNDARY_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129)


def boundaries(kind, seed=4):
    """Single queries with exactly 0, 1, 2, 63, 64, 65, 127, 128, 129
    admissible candidates; the one acceptable candidate is 3 bits away."""
    b = Builder(kind, seed)
    for s, c in enumerate(BOUNDARY_COUNTS):
        octave = b.band(0)
        want = b.cand(SPOTS[s], octave, bits(3)) if c else -1
        b.fillers(SPOTS[s], octave, max(c - 1, 0))
        b.expect.append((b.query(SPOTS[s], octave, np.zeros(32, np.uint8), tag=f"count{c}"), want))
    return b.finish("boundaries")


def budget(kind, nq=1000, n2=1000, per_query=10, seed=5):
    """Queries of per_query candidates each (spots of per_query candidates
    and as many queries): the short lists sum past the LDS entry budget.  Two
    chains of 6 stand among them: one at indices on both sides of the place
    where the budget runs out (about 8192 / per_query), one past it."""
    b = Builder(kind, seed)
    b.chain(SPOTS[0], 0, 6, 4, tag="chain_a")
    b.chain(SPOTS[1], 0, 6, 4, tag="chain_b")
    b.fill(nq - 12, n2 - 20, per_spot=per_query)
    at = [int(nq * f) for f in (.70, .76, .80, .84, .88, .92, .93, .94, .95, .96, .97, .98)]
    return b.finish("budget", slots=at)


def extras(kind, seed=6):
    """A chain of 12 with two candidates already assigned and two members'
    q_valid cleared."""
    b = Builder(kind, seed)
    b.chain(SPOTS[0], 0, 12, 20, invalid=(3, 7), assigned=(2, 5))
    b.fill(30, 30, per_spot=4, spots=SPOTS[10:])
    return b.finish("extras")


def rotation(kind, seed=7):
    """A chain of 23 whose matches fall into rotation bins 0 (17), 3 (3), 6
    (2) and 9 (one): the three-maxima rule removes that one (window and
    motion, check_ori on)."""
    assert kind in ("window", "motion")
    angles = [0.0] * 23
    for k, a in ((2, 90.0), (9, 90.0), (20, 90.0), (5, 180.0), (14, 180.0), (11, 270.0)):
        angles[k] = a
    b = Builder(kind, seed)
    b.chain(SPOTS[0], 0, 23, 20, angles=angles)
    s = b.finish("rotation", check_ori=1)
    removed = s.tags["chain"][11]
    s.expect[removed] = -1
    return s


RATIO_DIST = (1, 2, 4, 7, 12, 21, 36, 61)


def ratio_chain(seed=8):
    """Pair search at nnratio 0.6: a chain whose distances pass the ratio
    (each at most 0.6 of the next), with one more query before member 2 that
    is 20 bits further from every candidate, so its best and second are too
    close and it is rejected; the members behind it still move up."""
    b = Builder("pair", seed)
    b.chain(SPOTS[0], 0, len(RATIO_DIST), 12, dist=RATIO_DIST, odd=(2, np.array([0] * 28 + [255, 255, 15, 0], np.uint8)))
    b.fill(30, 30, per_spot=4, spots=SPOTS[10:])
    return b.finish("ratio", nnratio=0.6)


def large(kind, nq, n2, seed=9, name="large"):
    """nq queries, n2 searched keypoints: a chain of 12 in a short list, one
    of 5 in a list of 100 and one of 5 in a list of 150, ties in lists of all
    three forms, the rest spots of 16."""
    b = Builder(kind, seed)
    b.chain(SPOTS[0], 0, 12, 20, tag="chain0")
    b.chain(SPOTS[0], 1, 5, 95, tag="chain1")
    b.chain(SPOTS[0], 2, 5, 145, tag="chain2")
    _tie(b, SPOTS[1], 0, 6, hi_first=True)
    _tie(b, SPOTS[2], 1, 70, hi_first=False, tag="tie_mid")
    _tie(b, SPOTS[3], 2, 140, hi_first=True, tag="tie_long")
    b.fill(nq - len(b.q), n2 - len(b.c), per_spot=16)
    s = b.finish(name)
    assert (s.nq, s.n2) == (nq, n2)
    return s


def edge(kind, nq, n2, seed=10, per_spot=4):
    """nq queries and n2 searched keypoints in spots of per_spot."""
    b = Builder(kind, seed + nq + n2)
    b.fill(nq, n2, per_spot=per_spot)
    return b.finish(f"edge{nq}x{n2}")


def lds_limit():
    """The largest n with the per-query arrays still in LDS at nq = n2 = n."""
    n = 1
    while lds_plan(n + 1, n + 1)[0]:
        n += 1
    return n


# ---------------------------------------------------------------------------
# white-box mirror of launch_area_search / k_area_replay
# ---------------------------------------------------------------------------
def area_replay_lds(n2, nq_lds, ent_cap):
    return n2 * 16 + ((n2 + 15) & ~15) + n2 * 4 + 48 * 4 + n2 * 4 + n2 * 8 + nq_lds * K_AREA_QUERY_INTS * 4 + ent_cap * 4


def lds_plan(nq, n2):
    """(q_lds, ent_cap), or None where the fixed part does not fit."""
    cap_q, n2 = max(nq, 1), max(n2, 1)
    q_lds = int(area_replay_lds(n2, cap_q, K_REPLAY_ENTRIES) <= K_LDS)
    fixed = area_replay_lds(n2, cap_q if q_lds else 0, 0)
    if fixed > K_LDS:
        return None
    return q_lds, min(K_REPLAY_ENTRIES, (K_LDS - fixed) // 4)


def candidate_lists(s):
    """Per query: None when the search skips it, else its admissible
    candidates (before `taken`) in the reference's order -- distance, then
    GetFeaturesInArea order (cell x, cell y, index) -- as (indices,
    distances).  Cells are the numpy Grid's."""
    g = Grid(s.k2, W, H)
    cell = np.full(s.n2, -1, np.int64)
    for cx in range(COLS):
        for cy in range(ROWS):
            for j in g.cells[cx][cy]:
                cell[j] = cx * ROWS + cy
    ccx, ccy = cell // ROWS, cell % ROWS
    qx, qy, r = s.centres()
    lo, hi = s.levels()
    x0 = np.maximum(0, np.floor(((qx - g.minx) - r) * g.winv).astype(np.int64))
    x1 = np.minimum(COLS - 1, np.ceil(((qx - g.minx) + r) * g.winv).astype(np.int64))
    y0 = np.maximum(0, np.floor(((qy - g.miny) - r) * g.hinv).astype(np.int64))
    y1 = np.minimum(ROWS - 1, np.ceil(((qy - g.miny) + r) * g.hinv).astype(np.int64))
    empty = (x0 >= COLS) | (x1 < 0) | (y0 >= ROWS) | (y1 < 0)
    x2, y2, o2 = s.k2["x"], s.k2["y"], s.k2["octave"].astype(np.int64)
    out = []
    for i in range(s.nq):
        active = bool(s.valid[i]) and not empty[i]
        if s.kind == "motion" and (qx[i] < 0 or qx[i] > W or qy[i] < 0 or qy[i] > H):
            active = False
        if not active:
            out.append(None)
            continue
        m = (cell >= 0) & (ccx >= x0[i]) & (ccx <= x1[i]) & (ccy >= y0[i]) & (ccy <= y1[i])
        m &= (o2 >= lo[i]) & (o2 <= hi[i])
        m &= ~(np.abs(x2 - qx[i]) > r[i]) & ~(np.abs(y2 - qy[i]) > r[i])
        idx = np.nonzero(m)[0]
        dist = POP[np.bitwise_xor(s.d1[i][None, :], s.d2[idx])].sum(axis=1)
        o = np.lexsort((idx, cell[idx], dist))
        out.append((idx[o], dist[o]))
    return out


def _decide(s, lst, free):
    """The acceptance rule over the first two free candidates of a list."""
    idx, dist = lst
    best = second = -1
    for k in range(len(idx)):
        if free(int(idx[k])):
            if best < 0:
                best = k
            else:
                second = k
                break
    if best < 0:
        return -1
    bd = int(dist[best])
    bd2 = int(dist[second]) if second >= 0 else 0x7fffffff
    if bd > TH_HIGH:
        return -1
    if s.kind in ("window", "pair"):
        if not F32(bd) <= F32(F32(bd2) * s.nnratio):
            return -1
    elif s.kind == "local" and second >= 0:
        o2 = s.k2["octave"]
        if o2[idx[best]] == o2[idx[second]] and F32(bd) > F32(s.nnratio * F32(bd2)):
            return -1
    return int(idx[best])


def sequential(s, lists):
    """The reference's greedy loop over the lists: state per query, and the
    match vector before the rotation filter."""
    taken = np.where(s.assigned != 0, -2, -1).astype(np.int64)
    state = np.full(s.nq, -1, np.int64)
    for i, lst in enumerate(lists):
        if lst is None or len(lst[0]) == 0:
            continue
        st = _decide(s, lst, lambda j: taken[j] == -1)
        state[i] = st
        if st >= 0:
            taken[st] = i
    return state


def rounds(s, lists):
    """The replay's parallel claim rounds: (rounds used, fell back)."""
    big = 0x7fffffff
    assigned = s.assigned != 0
    state = np.full(s.nq, -2, np.int64)
    prev = np.full(s.n2, big, np.int64)
    for rnd in range(K_MAX_ROUNDS):
        nxt = np.full(s.n2, big, np.int64)
        changed = False
        for i, lst in enumerate(lists):
            st = -1
            if lst is not None and len(lst[0]):
                st = _decide(s, lst, lambda j: not assigned[j] and prev[j] >= i)
            changed |= st != state[i]
            state[i] = st
            if st >= 0:
                nxt[st] = min(nxt[st], i)
        if not changed:
            return rnd + 1, 0, state
        prev = nxt
    return K_MAX_ROUNDS, 1, None


def entry_offsets(cnt, ent_cap):
    """q_off of the replay's staging scan: the short lists' LDS offsets in
    chunks of the block, -1 where the budget is spent."""
    off = np.full(len(cnt), -1, np.int64)
    used = 0
    for q0 in range(0, len(cnt), K_REPLAY_THREADS):
        run = used
        for i in range(q0, min(q0 + K_REPLAY_THREADS, len(cnt))):
            w = cnt[i] if 0 < cnt[i] <= 64 else 0
            if w > 0 and run + w <= ent_cap:
                off[i] = run
            run += w
        used = min(run, ent_cap)
    return off


def mirror(s):
    """What the kernels will do with scene s, from the sizes and lists alone."""
    lists = candidate_lists(s)
    cnt = np.array([-1 if l is None else len(l[0]) for l in lists], np.int64)
    plan = lds_plan(s.nq, s.n2)
    q_lds, ent_cap = plan
    off = entry_offsets(cnt, ent_cap)
    nrounds, fell_back, state = rounds(s, lists)
    seq = sequential(s, lists)
    if state is not None:
        assert np.array_equal(state, seq), "the rounds' fixed point is the sequential result"
    return dict(lists=lists, cnt=cnt, q_lds=q_lds, ent_cap=ent_cap, off=off, rounds=nrounds, fallback=fell_back,
                state=seq, in_lds=(off >= 0), short=(cnt > 0) & (cnt <= 64))


def expected_matches(s, state):
    """Match vector and count from the queries' states, with the rotation
    filter of WindowSearch / the motion search (check_ori on)."""
    from test_match_numpy import HISTO, three_maxima
    from test_proj_numpy import rot_bin
    m = np.full(s.n2, -1, np.int64)
    hist = [[] for _ in range(HISTO)]
    for i, st in enumerate(state):
        if st >= 0:
            m[st] = i
            hist[rot_bin(s.k1["angle"][i], s.k2["angle"][st])].append(st)
    if s.check_ori and s.kind in ("window", "motion"):
        keep = three_maxima(hist)
        for b in range(HISTO):
            if b not in keep:
                for j in hist[b]:
                    m[j] = -1
    return m, int((m >= 0).sum())


# ---------------------------------------------------------------------------
# a chain inside orbx_track_frame's motion search, among natural keypoints
# ---------------------------------------------------------------------------
TRACK_TH = 15.0    # Tracking::TrackWithMotionModel: SearchByProjection(cur, last, 15)
TRACK_CASE = (1, 6, 1.5)   # seed, shift, prediction error of the track_data images used


class TrackMotion(Scene):
    """The motion search of one tracked frame as a scene for the mirror: the
    last frame's keypoints with a usable map point against the current
    frame's, projected with the predicted pose."""

    def __init__(self, kl, dl, kc, dc, scene, Tpred):
        lmp = scene["last_mp"]
        valid = ((lmp >= 0) & (scene["last_outlier"] == 0)).astype(np.uint8)
        Scene.__init__(self, "track", "motion", kl, dl, kc, dc, valid, np.zeros(len(kc), np.uint8), F32(1.0), 1, {}, {})
        self.X = scene["pos"][np.maximum(lmp, 0)].astype(np.float32)
        self.T = np.asarray(Tpred, np.float32).reshape(3, 4)

    def centres(self):
        T, X = self.T, self.X
        c = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
        inv = (1.0 / c[2].astype(np.float64)).astype(np.float32)
        u = (CAM[0] * c[0]) * inv + CAM[2]
        v = (CAM[1] * c[1]) * inv + CAM[3]
        return u.astype(np.float32), v.astype(np.float32), (F32(TRACK_TH) * scale_factors()[self.k1["octave"]])


def track_chain(kl, dl, kc, dc, scene, Tpred, n=24, octave=1, depth=4.0):
    """Puts n chain queries in front of the last frame (kl, dl) of a
    track_data scene, among the current frame's natural keypoints (kc, dc).

    The chain is one of displacement: candidates c_0 .. c_{n-1} are current
    keypoints each within reach of the next; query 0 stands on c_0 with its
    descriptor, query k between c_{k-1} and c_k with a descriptor that is
    nearest to c_{k-1}, then c_k, and further from everything else in its
    window.  Query k - 1 takes c_{k-1}, so query k takes c_k: n + 1 rounds.
    Each query observes a new map point that the predicted pose projects to
    its position.  Returns (kl, dl, scene, candidates) or None when the
    keypoints hold no such path."""
    sf = scale_factors()
    r = float(F32(TRACK_TH) * sf[octave])
    o = kc["octave"]
    ok = np.nonzero((o >= octave - 1) & (o <= octave + 1) & (kc["x"] > 40) & (kc["x"] < W - 40) & (kc["y"] > 40) &
                    (kc["y"] < H - 40))[0]
    x, y = kc["x"].astype(np.float64), kc["y"].astype(np.float64)

    def link(a, b):
        """Descriptor of the query between a and b, or None."""
        if max(abs(x[a] - x[b]), abs(y[a] - y[b])) > 2 * (r - 1.5):
            return None
        diff = [i for i in range(256) if (dc[a][i // 8] ^ dc[b][i // 8]) >> (i % 8) & 1]
        t = -(-len(diff) * 35 // 100)
        if t < 1 or len(diff) - t > 95 or t >= len(diff) - t:
            return None
        d = dc[a].copy()
        for i in diff[:t]:
            d[i // 8] ^= np.uint8(1 << (i % 8))
        mx, my = (x[a] + x[b]) / 2, (y[a] + y[b]) / 2
        near = ok[(np.abs(x[ok] - mx) <= r + 1.5) & (np.abs(y[ok] - my) <= r + 1.5) & (ok != a) & (ok != b)]
        if len(near) and POP[np.bitwise_xor(d[None, :], dc[near])].sum(axis=1).min() <= len(diff) - t + 4:
            return None
        return d

    budget = [20000]   # links tried, so that a frame without a path ends the search

    def extend(path, descs):
        if len(path) == n:
            return True
        budget[0] -= 1
        if budget[0] < 0:
            return False
        a = path[-1]
        nb = ok[(np.abs(x[ok] - x[a]) <= 2 * r) & (np.abs(y[ok] - y[a]) <= 2 * r)]
        for b in nb:
            if int(b) in path:
                continue
            d = link(a, int(b))
            if d is None:
                continue
            path.append(int(b))
            descs.append(d)
            if extend(path, descs):
                return True
            path.pop()
            descs.pop()
        return False

    for start in ok:
        path, descs = [int(start)], [dc[start].copy()]
        if extend(path, descs):
            break
        if budget[0] < 0:
            return None
    else:
        return None
    q = np.zeros(n, KEYPOINT)
    for k in range(n):
        a = path[max(k - 1, 0)]
        q["x"][k], q["y"][k] = (x[a] + x[path[k]]) / 2, (y[a] + y[path[k]]) / 2
        q["angle"][k] = kc["angle"][path[k]]
    q["octave"], q["size"] = octave, 31.0 * float(sf[octave])
    cam_x = -float(np.asarray(Tpred, np.float32)[3])
    P = np.stack([(q["x"].astype(np.float64) - CAM[2]) / CAM[0] * depth + cam_x,
                  (q["y"].astype(np.float64) - CAM[3]) / CAM[1] * depth, np.full(n, depth)], 1)
    dist = np.linalg.norm(P, axis=1)
    dmax = dist * float(sf[octave])
    m = len(scene["pos"])
    out = dict(scene)
    out["pos"] = np.ascontiguousarray(np.concatenate([scene["pos"], P.astype(np.float32)]))
    out["normal"] = np.ascontiguousarray(np.concatenate([scene["normal"], (P / dist[:, None]).astype(np.float32)]))
    out["dist"] = np.ascontiguousarray(np.concatenate([scene["dist"],
                                                       np.stack([dmax / float(sf[-1]), dmax], 1).astype(np.float32)]))
    out["desc"] = np.ascontiguousarray(np.concatenate([scene["desc"], np.array(descs, np.uint8)]))
    out["skip"] = np.concatenate([scene["skip"], np.zeros(n, np.uint8)])
    out["last_mp"] = np.concatenate([np.arange(m, m + n), scene["last_mp"]]).astype(np.int32)
    out["last_outlier"] = np.concatenate([np.zeros(n, np.uint8), scene["last_outlier"]])
    return (np.concatenate([q, kl]), np.ascontiguousarray(np.concatenate([np.array(descs, np.uint8), dl])), out, path)


# ---------------------------------------------------------------------------
# the catalogue both test files walk, and the call of one search on a scene
# ---------------------------------------------------------------------------
EDGES = ((0, 40), (1, 40), (17, 40), (1025, 300), (40, 1), (40, 65))
WM = ("window", "motion")
CATALOGUE = {
    "chain10x3": (KINDS, lambda k: three_chains(k, 10)),
    "chain23": (KINDS, lambda k: chain_scene(k, 23)),
    "chain24": (KINDS, lambda k: chain_scene(k, 24)),
    "chain24x3": (KINDS, lambda k: three_chains(k, 24)),
    "chain40x3": (KINDS, lambda k: three_chains(k, 40)),
    "ties": (KINDS, ties),
    "boundaries": (KINDS, boundaries),
    "budget": (KINDS, budget),
    "extras": (KINDS, extras),
    "rotation": (WM, rotation),
    "ratio": (("pair",), lambda k: ratio_chain()),
    "qglob_full": (KINDS, lambda k: large(k, 4096, 1536, name="qglob_full")),
    "qglob_shrunk": (KINDS, lambda k: large(k, K_MAX_FEATURES, K_MAX_FEATURES, name="qglob_shrunk")),
    "lds_max": (KINDS, lambda k: large(k, lds_limit(), lds_limit(), name="lds_max")),
}
CATALOGUE.update({f"edge{nq}x{n2}": (KINDS, (lambda nq, n2: lambda k: edge(k, nq, n2))(nq, n2)) for nq, n2 in EDGES})
CASES = [(name, kind) for name, (kinds, _) in CATALOGUE.items() for kind in kinds]
_built = {}


def scene(name, kind):
    """The scene and its mirror, built once."""
    if (name, kind) not in _built:
        s = CATALOGUE[name][1](kind)
        _built[name, kind] = (s, mirror(s))
    return _built[name, kind]


def search(s, fns, handle=None):
    """One search over scene s: fns maps the kind to the oracle's function,
    or with a context handle to the library's; (return code, matches, n)."""
    import ctypes

    import orb_slam_amd as ox
    from oracle_lib import ptr
    F1, F2 = ox.frame_view(s.k1, s.d1, W, H), ox.frame_view(s.k2, s.d2, W, H)
    m = np.full(max(s.n2, 1), -9, np.int32)
    n = ctypes.c_int(-9)
    head = () if handle is None else (handle,)
    r1, r2 = ctypes.byref(F1), ctypes.byref(F2)
    if s.kind == "window":
        a = (r1, r2, ptr(s.valid), R0, 0, -1, s.nnratio, s.check_ori)
    elif s.kind == "pair":
        a = (r1, r2, ptr(s.xyz), ptr(s.valid), ptr(s.assigned), ptr(s.T), ptr(CAM), R0, s.nnratio)
    elif s.kind == "motion":
        a = (r2, r1, ptr(s.xyz), ptr(s.valid), ptr(s.assigned), ptr(s.T), ptr(CAM), s.th_motion, s.check_ori)
    elif s.pose is not None:
        # the posed local-map kind: isInFrustum of the map points, then the search (fns["local_map"])
        from local_map_data import LocalMapQuery
        T = s.T.reshape(3, 4)
        keep = dict(Rcw=np.ascontiguousarray(T[:, :3]).reshape(-1), tcw=np.ascontiguousarray(T[:, 3]), Ow=s.Ow,
                    cam=CAM, mp_pos=s.xyz, mp_normal=s.normal, mp_dist=s.mp_dist,
                    mp_skip=(s.valid == 0).astype(np.uint8), mp_desc=s.d1, f_assigned=s.assigned,
                    in_view=np.zeros(max(s.nq, 1), np.uint8), proj_xy=np.zeros((max(s.nq, 1), 2), np.float32),
                    pred_level=np.zeros(max(s.nq, 1), np.int32), view_cos=np.zeros(max(s.nq, 1), np.float32), matches_f=m)
        q = LocalMapQuery()
        q.frame = ctypes.addressof(F2)
        for field, arr in keep.items():
            setattr(q, field, arr.ctypes.data)
        q.n_mp, q.view_cos_limit, q.th, q.nnratio = s.nq, 0.5, float(s.th_local), float(s.nnratio)
        rc = fns["local_map"](*head, ctypes.byref(q))
        s.frustum = (keep["in_view"], keep["proj_xy"], keep["pred_level"])
        return rc, m[:s.n2].astype(np.int64), q.n_matches
    else:
        a = (r2, s.nq, ptr(s.valid), ptr(s.proj), ptr(s.pred), ptr(s.vcos), ptr(s.d1), ptr(s.assigned), s.th_local,
             s.nnratio)
    rc = fns[s.kind](*head, *a, ptr(m), ctypes.byref(n))
    return rc, m[:s.n2].astype(np.int64), n.value
