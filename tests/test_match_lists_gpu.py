"""k_match_prev's candidate lists on inputs that extraction never produces.

The batch SearchForInitialization kernel orders its candidate slots by grid
column and scans, per query, only the slots of the query's cell columns.  The
features are written into the slots through Context.write_features, so the
cases below control what the ordering and the column ranges meet: candidates
in descending x, ties on distance inside a cell and across cells, positions
exactly at the window's edge, queries at the image corners, candidates
outside the grid, empty and full slots, one column, one position, lists
longer than a wave whose keys exceed the key space, a steal, both settings of
the rotation check, a cyclic sequence, octave-0 queries that are no prefix.

The comparator is the oracle's SearchForInitialization
(src/ORBmatcher.cc:598-713) on the same arrays.  Where a case depends on a
property of its input, the property is asserted on the CPU first.
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
from oracle_lib import load, ptr

pytestmark = pytest.mark.gpu

W, H = 160, 128
NF = 500
GRID_COLS, GRID_ROWS = 64, 48
LDS_BUDGET = 44 * 1024


def init_lds_bytes(cap_c, cap1, cap_keys):
    """orbx_match_common.h's init_lds_bytes, restated."""
    return cap_c * (7 * 4 + 32 + 16) + cap1 * 8 + ((cap1 + 15) & ~15) + 257 * 4 + 36 * 4 + cap_keys * 4 + \
        256 * (32 + 8 + 16) + 64


def cap_keys_of(cap_c, nfeatures):
    fixed = init_lds_bytes(cap_c, nfeatures, 0)
    return max(cap_c, (LDS_BUDGET - min(fixed, LDS_BUDGET)) // 4)


def keypoints(x, y, octave=0, angle=0.0):
    k = np.zeros(len(x), ox.KEYPOINT)
    k["x"], k["y"] = np.asarray(x, np.float32), np.asarray(y, np.float32)
    k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = 31.0, angle, 50.0, octave, -1
    return k


def descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(rng, d, nbits):
    """d with nbits distinct bits flipped."""
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


def cells(k, bounds=(0.0, W, 0.0, H)):
    """Frame::PosInGrid in float, (cx, cy) or (-1, -1)."""
    b = np.asarray(bounds, np.float32)
    gw, gh = np.float32(GRID_COLS) / (b[1] - b[0]), np.float32(GRID_ROWS) / (b[3] - b[2])
    rnd = lambda v: np.where(v >= 0, np.floor(v + np.float32(0.5)), np.ceil(v - np.float32(0.5))).astype(np.int64)
    cx, cy = rnd((k["x"] - b[0]) * gw), rnd((k["y"] - b[2]) * gh)
    out = (cx < 0) | (cx >= GRID_COLS) | (cy < 0) | (cy >= GRID_ROWS)
    return np.where(out, -1, cx), np.where(out, -1, cy)


def pair(rng, n1, n2, n_hi=20, jitter=3.0, bits=20, shuffle=True):
    """Two frames: n1 / n2 octave-0 keypoints (the second frame's are jittered
    copies of the first's with some descriptor bits flipped, the rest
    random), then n_hi keypoints of higher octaves."""
    def frame(n0):
        x, y = rng.uniform(0, W - 0.01, n0 + n_hi), rng.uniform(0, H - 0.01, n0 + n_hi)
        octv = np.r_[np.zeros(n0, np.int32), rng.integers(1, 8, n_hi)]
        return keypoints(x, y, octv, rng.uniform(0, 360, n0 + n_hi).astype(np.float32)), descriptors(rng, n0 + n_hi)
    (k1, d1), (k2, d2) = frame(n1), frame(n2)
    m = min(n1, n2)
    src = rng.permutation(n1)[:m] if shuffle else np.arange(m)
    for j, i in enumerate(src):
        k2["x"][j] = np.clip(k1["x"][i] + rng.uniform(-jitter, jitter), 0, W - 0.01)
        k2["y"][j] = np.clip(k1["y"][i] + rng.uniform(-jitter, jitter), 0, H - 0.01)
        k2["angle"][j] = (k1["angle"][i] + rng.choice([0.0, 0.0, 0.0, 3.0, 90.0])) % 360
        d2[j] = flip(rng, d1[i], int(rng.integers(0, bits + 1)))
    return (k1, d1), (k2, d2)


def oracle(f1, f2, window, nnratio, check_ori, bounds=None):
    (k1, d1), (k2, d2) = f1, f2
    F1, F2 = ox.frame_view(k1, d1, W, H), ox.frame_view(k2, d2, W, H)
    if bounds is not None:
        for F in (F1, F2):
            F.min_x, F.max_x, F.min_y, F.max_y = (float(v) for v in bounds)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32).copy()
    m12 = np.full(max(len(k1), 1), -1, np.int32)
    nm = ctypes.c_int()
    assert load().orbx_ref_search_for_initialization(ctypes.byref(F1), ctypes.byref(F2), ptr(prev), ptr(m12), window,
                                                     nnratio, int(check_ori), ctypes.byref(nm)) == 0
    return m12[:len(k1)], nm.value


def make_ctx(nfeatures, slots):
    ctx = ox.Context(nfeatures=nfeatures, max_w=W, max_h=H, slots=slots)
    ctx.upload(np.zeros((slots, H, W), np.uint8))   # sets the frame size the matcher's grid uses
    ctx.sync()
    return ctx


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx(NF, 3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def quota(ctx):
    q = int(ctx.features_per_level()[0])
    assert 65 < q < 256 and q + 20 <= NF
    return q


def check(ctx, frames, window=100, nnratio=0.9, check_ori=True, bounds=None, only=None):
    """frames into slots 0 .. n-1, every slot (or slot `only`) against its
    cyclic predecessor, each compared with the oracle.  -> oracle results"""
    n = len(frames)
    ctx.set_image_bounds(bounds)
    try:
        for s, (k, d) in enumerate(frames):
            ctx.write_features(s, k, d)
        if only is None:
            ctx.match_prev(0, n, n, window=window, nnratio=nnratio, check_ori=check_ori)
        else:
            ctx.match_prev(only, 1, n, window=window, nnratio=nnratio, check_ori=check_ori)
        ctx.sync()
        out = {}
        for s in (range(n) if only is None else [only]):
            p = s - 1 if s else n - 1
            rm, rn = oracle(frames[p], frames[s], window, nnratio, check_ori, bounds)
            gm, gn = ctx.matches(s)
            n1 = len(frames[p][0])
            print(f"slot {s}: {rn} matches of {n1} queries")
            assert gn == rn, (s, gn, rn)
            assert np.array_equal(gm[:n1], rm), (s, np.nonzero(gm[:n1] != rm)[0][:8])
            out[s] = (rm, rn)
        return out
    finally:
        ctx.set_image_bounds(None)


def test_write_features_round_trip(ctx):
    rng = np.random.default_rng(1)
    (k, d), _ = pair(rng, 30, 30)
    ctx.write_features(2, k, d)
    gk, gd = ctx.features(2)
    assert np.array_equal(gk.view(np.uint8), k.view(np.uint8)) and np.array_equal(gd, d)
    ctx.write_features(2, k[:0], d[:0])
    assert len(ctx.features(2)[0]) == 0


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("window", [100, 12])
def test_descending_x_candidates(ctx, quota, window, check_ori):
    """Candidates in descending-x index order: the column order is the
    reverse of the index order, the reorder is far from the identity."""
    rng = np.random.default_rng(2)
    f1, (k2, d2) = pair(rng, quota, quota, shuffle=False)
    o = np.argsort(-k2["x"][:quota], kind="stable")
    k2[:quota], d2[:quota] = k2[:quota][o], d2[:quota][o]
    assert np.all(np.diff(k2["x"][:quota]) <= 0) and len(np.unique(cells(k2[:quota])[0])) > 20
    res = check(ctx, [f1, (k2, d2)], window=window, check_ori=check_ori)
    assert res[1][1] > 10


def test_duplicated_descriptors_first_in_area_order_wins(ctx, quota):
    """Candidates that tie on distance inside one grid cell and across
    cells: the reference keeps the first in GetFeaturesInArea order (cell
    column, cell row, index).  nnratio 1.5 accepts a best equal to the second."""
    rng = np.random.default_rng(3)
    n = 25
    assert 4 * n <= quota
    qx, qy = rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)
    d1 = descriptors(rng, n)
    xs, ys, ds = [], [], []
    for i in range(n):
        dd = flip(rng, d1[i], 4)
        # index order against cell order: a later cell column first, then two
        # in one cell, then an earlier cell row of the first column
        for dx, dy in ((6.0, 0.0), (0.1, 0.1), (0.3, 0.2), (0.0, -6.0)):
            xs.append(qx[i] + dx)
            ys.append(qy[i] + dy)
            ds.append(dd)
    k1, k2 = keypoints(qx, qy), keypoints(xs, ys)
    d2 = np.array(ds, np.uint8)
    cx, cy = cells(k2)
    same = sum(1 for i in range(n) if (cx[4 * i + 1], cy[4 * i + 1]) == (cx[4 * i + 2], cy[4 * i + 2]))
    across = sum(1 for i in range(n) if cx[4 * i] != cx[4 * i + 1] and cy[4 * i + 3] != cy[4 * i + 1])
    assert same > 5 and across == n
    res = check(ctx, [(k1, d1), (k2, d2)], window=10, nnratio=1.5, check_ori=False, only=1)
    rm, rn = res[1]
    assert rn > 12
    # the winner is never the first of the four by index (its column is later)
    assert np.all(rm[rm >= 0] % 4 != 0)


def test_positions_at_the_window_edge(ctx):
    """|dx| and |dy| exactly the window, one float above and one below."""
    rng = np.random.default_rng(4)
    win = 20
    q = [(50.0, 60.0), (90.5, 40.25), (120.0, 100.0)]
    xs, ys = [], []
    for x, y in q:
        for sgn in (-1.0, 1.0):
            e = np.float32(x + sgn * win)
            for v in (e, np.nextafter(e, np.float32(1e9)), np.nextafter(e, np.float32(-1e9))):
                xs.append(v); ys.append(np.float32(y))
            e = np.float32(y + sgn * win)
            for v in (e, np.nextafter(e, np.float32(1e9)), np.nextafter(e, np.float32(-1e9))):
                xs.append(np.float32(x)); ys.append(v)
    k1, k2 = keypoints([p[0] for p in q], [p[1] for p in q]), keypoints(xs, ys)
    assert np.float32(50.0 + 20) in k2["x"] and np.nextafter(np.float32(70), np.float32(1e9)) in k2["x"]
    d1 = descriptors(rng, len(k1))
    # every candidate a distinct near copy of its query: the nearest one in
    # the window wins, so a wrong edge decision changes the match
    d2 = np.array([flip(rng, d1[i // 12], 1 + (i % 12)) for i in range(len(k2))], np.uint8)
    o = rng.permutation(len(k2))
    res = check(ctx, [(k1, d1), (k2[o], d2[o])], window=win, nnratio=1.5, check_ori=False, only=1)
    assert res[1][1] == len(q)


@pytest.mark.parametrize("window", [100, 7])
def test_queries_at_the_image_corners(ctx, quota, window):
    rng = np.random.default_rng(5)
    (k1, d1), (k2, d2) = pair(rng, quota, quota)
    eps = np.float32(0.01)
    corners = [(0.0, 0.0), (W - eps, 0.0), (0.0, H - eps), (W - eps, H - eps)]
    for i, (x, y) in enumerate(corners):
        k1["x"][i], k1["y"][i] = x, y
        k2["x"][i], k2["y"][i] = np.clip(x + 1.5 * (1 if x == 0 else -1), 0, W), np.clip(y + 1.0 * (1 if y == 0 else -1), 0, H)
        d2[i] = flip(rng, d1[i], 3)
    check(ctx, [(k1, d1), (k2, d2)], window=window)


def test_candidates_outside_the_grid(ctx, quota):
    rng = np.random.default_rng(6)
    f1, f2 = pair(rng, quota, quota)
    bounds = (12.0, 150.0, 9.0, 117.0)
    for k, _ in (f1, f2):
        cx, _ = cells(k[:quota], bounds)
        assert 5 < np.count_nonzero(cx < 0) < quota - 20
    res = check(ctx, [f1, f2], bounds=bounds)
    assert res[1][1] > 5


def test_candidate_and_query_counts(ctx, quota):
    rng = np.random.default_rng(7)
    for nq in (0, 1, quota):
        for ncand in (0, 1, 63, 64, 65, quota):
            f1, f2 = pair(rng, nq, ncand, n_hi=5)
            assert np.count_nonzero(f2[0]["octave"] == 0) == ncand and np.count_nonzero(f1[0]["octave"] == 0) == nq
            check(ctx, [f1, f2], only=1)
    # no keypoints at all in either slot
    check(ctx, [pair(rng, 0, 0, n_hi=0)[0], pair(rng, 5, 5, n_hi=0)[0]])


def test_all_candidates_in_one_grid_column(ctx, quota):
    rng = np.random.default_rng(8)
    f1, f2 = pair(rng, quota, quota, jitter=0.0)
    for k, _ in (f1, f2):
        k["x"][:quota] = rng.uniform(40.1, 40.9, quota).astype(np.float32)
        cx, _ = cells(k[:quota])   # (a y that rounds to row 48 is outside the grid)
        assert set(np.unique(cx)) <= {16, -1} and np.count_nonzero(cx == 16) > quota - 10
    res = check(ctx, [f1, f2], window=30)
    assert res[1][1] > 5


def test_all_candidates_at_one_position(ctx, quota):
    rng = np.random.default_rng(9)
    f1, f2 = pair(rng, quota, quota)
    for k, _ in (f1, f2):
        k["x"][:quota], k["y"][:quota] = 77.5, 33.25
    res = check(ctx, [f1, f2], window=5)
    assert res[1][1] > 5


def test_cluster_lists_longer_than_a_wave(ctx, quota):
    """Every candidate in every query's window: lists of `quota` > 64 keys,
    more keys in a group than the key space holds (several chunks)."""
    rng = np.random.default_rng(10)
    f1, f2 = pair(rng, quota, quota)
    cap_keys = cap_keys_of(quota, NF)
    assert quota > 64 and quota * quota > cap_keys > quota
    res = check(ctx, [f1, f2], window=200)
    assert res[1][1] > 5


def test_lists_longer_than_a_wave_2000_features():
    """nfeatures 2000: the key space holds one list at a time."""
    rng = np.random.default_rng(11)
    c = make_ctx(2000, 2)
    try:
        q = int(c.features_per_level()[0])
        cap_keys = cap_keys_of(q, 2000)
        f1, f2 = pair(rng, q, q, n_hi=50)
        # the longest list is every candidate (the window covers the image)
        assert q > 64 and q * q > cap_keys
        res = check(c, [f1, f2], window=200)
        assert res[1][1] > 20
    finally:
        c.close()


def test_a_later_query_steals_a_slot(ctx):
    rng = np.random.default_rng(12)
    D = descriptors(rng, 1)[0]
    k1 = keypoints([60.0, 61.0, 100.0], [50.0, 51.0, 90.0], angle=10.0)
    d1 = np.array([flip(rng, D, 12), flip(rng, D, 2), descriptors(rng, 1)[0]], np.uint8)
    k2 = keypoints([60.5, 100.5, 20.0], [50.5, 90.0, 20.0], angle=10.0)
    d2 = np.array([D, flip(rng, d1[2], 5), descriptors(rng, 1)[0]], np.uint8)
    assert hamming(d1[0], D) == 12 and hamming(d1[1], D) == 2
    res = check(ctx, [(k1, d1), (k2, d2)], window=10, only=1)
    rm, rn = res[1]
    assert list(rm) == [-1, 0, 1] and rn == 2


def test_three_pair_cyclic_sequence(ctx, quota):
    rng = np.random.default_rng(13)
    f1, f2 = pair(rng, quota, quota)
    _, f3 = pair(rng, quota, quota - 7)
    f3[0]["x"][:50], f3[0]["y"][:50], f3[1][:50] = f2[0]["x"][:50], f2[0]["y"][:50], f2[1][:50]
    res = check(ctx, [f1, f2, f3], window=40)
    assert res[1][1] > 5 and res[2][1] > 5


def test_octave0_queries_that_are_no_prefix_and_exceed_the_quota(ctx, quota):
    """Extraction writes octave 0 first and at most the quota of it; the
    matcher does not depend on either for its queries (frame 1)."""
    rng = np.random.default_rng(14)
    n1 = quota + 40
    (k1, d1), f2 = pair(rng, n1, quota, n_hi=60)
    o = rng.permutation(len(k1))
    k1, d1 = k1[o], d1[o]
    oct0 = np.nonzero(k1["octave"] == 0)[0]
    assert len(oct0) == n1 > quota and not np.array_equal(oct0, np.arange(n1)) and len(k1) <= NF
    res = check(ctx, [(k1, d1), f2], only=1)
    assert res[1][1] > 5
