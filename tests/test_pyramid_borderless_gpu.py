"""The batch pyramid keeps level interiors only: k_pyr_resize_lds writes no
border row, border word or row padding of levels >= 1, and k_describe stages
every window that leaves a level's interior from its REFLECT_101 sources
inside the level.  The padded levels' borders are filled on demand for the
readers of a whole level (Context.level).  Everything here is exact, against
the oracle, and every extraction starts from raw-pyramid areas poisoned with
one byte value (Context.fill_pyramid), so a result that depended on a byte the
extraction does not write would differ.

1. nothing reads a border: keypoints, descriptors and counts of a batch, both
   contraction modes, three sizes (level 0 direct and copied), two poisons;
2. every edge centre: the describe kernel's patch and moments at each window
   position next to a level's four sides and corners;
3. borders on demand: Context.level raw and blurred, in any order, repeated,
   and after the slot is reused;
4. the pipeline's parts: a batch split over three streams with asynchronous
   matching against one stream with synchronous matching, and a part's levels;
5. the other pyramid forms: the single-frame cascade, Harris scores, a level
   narrower than 32 pixels, the wide-level fallback k_pyr_resize, levels with
   scalar-tail columns;
6. the interior of every level, apart from its border.
"""
import ctypes
import functools

import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor, load, ptr
from test_cv24_numpy import _vec_cols, level_sizes

pytestmark = pytest.mark.gpu

E = 16          # padded border = EDGE_THRESHOLD
R = 18          # pattern reach: the blurred patch is rows / columns -18 .. 18
WIN_R = 21      # k_describe's window: rows Y - 21 .. Y + 21 ...
WIN_BYTES = 48  # ... and 48 bytes from (X - 21) & ~3
N = 300
SIZES = [(160, 128), (192, 144), (181, 120)]   # w % 16 == 0: level 0 direct; 181: level 0 copied
RES_ROWS = 16
RESIZE_LDS = 96 * 1024


def edge_sides(x, y, lw, lh):
    """describe_stage_window's predicate for a keypoint at level position
    (x, y): which sides of the level's interior its window leaves (top,
    bottom, left, right)."""
    X, Y = E + x, E + y
    x0 = (X - WIN_R) & ~3
    return (Y - WIN_R < E, Y + WIN_R >= E + lh, x0 < E, x0 + WIN_BYTES > E + lw)


def assert_kps_equal(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in ox.KEYPOINT.names:
        assert np.array_equal(a[f], b[f]), f


def noise_frames(w, h, count=3):
    return np.stack([synth.noise_frame(w, h, 7 + s) for s in range(count)])


@functools.lru_cache(maxsize=None)
def oracle(w, h, slot, variant="iso", nlevels=8, score_type=1, nfeatures=N):
    """Oracle results for noise frame `slot` of size w x h, computed once:
    keypoints, descriptors, the padded raw levels, the blurred levels and the
    per-level keypoints (level coordinates, output order)."""
    ref = RefExtractor(nfeatures, nlevels=nlevels, score_type=score_type, variant=variant)
    kps, desc = ref(noise_frames(w, h)[slot])
    levels = [ref.level(l) for l in range(nlevels)]
    blurred = [ref.level(l, blurred=True) for l in range(nlevels)]
    keys = [ref.level_keys(l) for l in range(nlevels)]
    for a in (kps, desc, *levels, *blurred):
        a.setflags(write=False)
    return kps, desc, levels, blurred, keys


def poisoned_batch(w, h, byte, contract=0, **kw):
    """A context whose slots' pyramids were poisoned before the three noise
    frames were extracted as one batch."""
    ctx = ox.Context(nfeatures=N, max_w=w, max_h=h, slots=3, **kw)
    ctx.set_fp_contract(contract)
    ctx.upload(noise_frames(w, h))
    ctx.fill_pyramid(0, 3, byte)
    ctx.extract(0, 3)
    ctx.sync()
    return ctx


# --- 1. nothing reads a border ---------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_noise_frames_have_edge_keypoints(w, h):
    """The precondition of the tests below, on the oracle's per-level
    keypoints: edge-band keypoints on every level that has keypoints, each of
    the four sides on at least two levels >= 1, and waves (keypoints 2i,
    2i + 1) with two, one and no edge keypoint."""
    sizes = level_sizes(w, h, 8, 1.2)
    for slot in range(3):
        keys = oracle(w, h, slot)[4]
        flags, side_levels = [], np.zeros(4, int)
        for l, (lw, lh) in enumerate(sizes):
            sides = np.array([edge_sides(int(k["x"]), int(k["y"]), lw, lh) for k in keys[l]]).reshape(-1, 4)
            if len(keys[l]):
                assert sides.any(), (slot, l)
            if l >= 1:
                side_levels += sides.any(0)
            flags += list(sides.any(1))
        assert (side_levels >= 2).all(), (slot, side_levels)
        waves = {int(flags[i]) + int(flags[i + 1]) for i in range(0, len(flags) - 1, 2)}
        assert waves == {0, 1, 2}, (slot, waves)


@pytest.mark.parametrize("byte", [0x5A, 0xFF])
@pytest.mark.parametrize("w,h", SIZES)
def test_batch_ignores_poisoned_borders(w, h, byte):
    for contract, variant in ((0, "iso"), (1, "contract")):
        ctx = poisoned_batch(w, h, byte, contract)
        assert ctx.level0_direct() == (w % 16 == 0)
        for s in range(3):
            rk, rd = oracle(w, h, s, variant)[:2]
            gk, gd = ctx.features(s)
            assert len(rk) > 100
            assert_kps_equal(gk, rk)
            assert np.array_equal(gd, rd), (contract, s)
        ctx.close()


# --- 2. every edge centre ----------------------------------------------------
def edge_centres(lw, lh):
    """Window centres next to each side and corner; on a level too small for
    all of them, those outside the range a keypoint can have are left out."""
    xs = list(range(16, 28)) + list(range(lw - 28, lw - 16))
    ys = list(range(16, 22)) + list(range(lh - 22, lh - 16))
    cs = [(x, lh // 2) for x in xs] + [(lw // 2, y) for y in ys]
    corners = [(16, 16), (lw - 17, 16), (16, lh - 17), (lw - 17, lh - 17)]
    legal = lambda c: 16 <= c[0] < lw - 16 and 16 <= c[1] < lh - 16
    return sorted(set(filter(legal, cs + corners))), corners


def moments_np(padded, x, y, umax):
    """IC_Angle's m01, m10 on the padded raw level."""
    m01 = m10 = 0
    for v in range(-15, 16):
        u = np.arange(-umax[abs(v)], umax[abs(v)] + 1)
        row = padded[E + y + v, E + x + u].astype(np.int64)
        m01 += v * int(row.sum())
        m10 += int((u * row).sum())
    return m01, m10


@pytest.mark.parametrize("w,h", [(160, 128), (181, 120)])
def test_describe_windows_at_every_edge_centre(w, h):
    sizes = level_sizes(w, h, 8, 1.2)
    last = max(l for l, (lw, lh) in enumerate(sizes) if lw > 32 and lh > 32)
    assert last > 2
    _, _, levels, blurred, _ = oracle(w, h, 1)
    umax = RefExtractor(N).umax()
    ctx = poisoned_batch(w, h, 0x5A)
    for l in (1, 2, last):
        lw, lh = sizes[l]
        centres, corners = edge_centres(lw, lh)
        assert set(corners) <= set(centres) and len(centres) >= 12
        # the centres straddle the predicate: most windows leave the interior,
        # the innermost ones are the first that do not
        assert {any(edge_sides(x, y, lw, lh)) for (x, y) in centres} == ({True, False} if l < last else {True})
        want = blurred[l]
        for (x, y) in centres:
            got = ctx.describe_patch(1, l, x, y)
            exp = want[E + y - R:E + y + R + 1, E + x - R:E + x + R + 1]
            assert np.array_equal(got, exp), (l, x, y, np.argwhere(got != exp)[:4])
        for (x, y) in corners:
            lo, hi = ctx.describe_moments(1, l, x, y)
            assert lo == hi == moments_np(levels[l], x, y, umax), (l, x, y)
    ctx.close()


# --- 3. borders on demand, 6. interiors --------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_levels_on_demand(w, h):
    ctx = poisoned_batch(w, h, 0xFF)
    order = [5, 1, 7, 0, 2, 3, 4, 6]
    for s in (2, 0):
        levels, blurred = oracle(w, h, s)[2:4]
        for l in order:
            for _ in range(2):
                assert np.array_equal(ctx.level(s, l), levels[l]), (s, l)
        for l in (1, 3):
            assert np.array_equal(ctx.level(s, l, blurred=True), blurred[l]), (s, l)
    # another frame into slot 0: no stale border survives
    ctx.upload(noise_frames(w, h)[1], first=0)
    ctx.extract(0, 1)
    ctx.sync()
    levels, blurred = oracle(w, h, 1)[2:4]
    for l in order:
        assert np.array_equal(ctx.level(0, l), levels[l]), l
    assert np.array_equal(ctx.level(0, 3, blurred=True), blurred[3])
    ctx.close()


def nfast(lw):
    """Interior words of the packed form (k_pyr_resize_lds)."""
    return max(E // 4, (E + min(lw, _vec_cols(lw, True))) >> 2) - E // 4


def test_sizes_cover_the_remainder_wave():
    """Levels whose last nfast % 64 packed words share one wave as row groups
    (remainder 1 .. 32) and levels whose remainder stays in the sliding form."""
    rems = {nfast(lw) % 64 for (w, h) in SIZES for (lw, _) in level_sizes(w, h, 8, 1.2)[1:]}
    assert any(0 < r <= 32 for r in rems) and any(r > 32 or r == 0 for r in rems), rems


@pytest.mark.parametrize("w,h", SIZES)
def test_level_interiors(w, h):
    ctx = poisoned_batch(w, h, 0x5A)
    for s in range(3):
        levels = oracle(w, h, s)[2]
        for l, (lw, lh) in enumerate(level_sizes(w, h, 8, 1.2)):
            got = ctx.level(s, l)[E:E + lh, E:E + lw]
            bad = np.argwhere(got != levels[l][E:E + lh, E:E + lw])
            assert len(bad) == 0, f"slot {s} level {l}: {len(bad)} interior bytes differ, first at {tuple(bad[0])}"
    ctx.close()


# --- 4. the pipeline's parts -------------------------------------------------
def test_split_batch_parts():
    w, h, n, count = 160, 128, N, 48
    frames = synth.sequence(w, h, count, seed=11)
    ctx = ox.Context(nfeatures=n, max_w=w, max_h=h, slots=count)
    ctx.upload(frames)

    def run(split, async_match):
        ctx.set_split(split)
        ctx.set_async_match(async_match)
        ctx.fill_pyramid(0, count, 0x5A)
        ctx.extract_match(0, count, count)
        ctx.sync()
        return [ctx.features(s) for s in range(count)], [ctx.matches(s) for s in range(count)]

    feats, matches = run(1, 1)     # three parts of 16 on their own streams
    # a slot of the middle part, read after sync()
    ref = RefExtractor(n)
    ref(frames[20])
    for l in (3, 0, 7, 1):
        assert np.array_equal(ctx.level(20, l), ref.level(l)), l
    feats1, matches1 = run(0, 0)   # one stream, synchronous matching
    for s in range(count):
        assert_kps_equal(feats[s][0], feats1[s][0])
        assert np.array_equal(feats[s][1], feats1[s][1]), s
        assert matches[s][1] == matches1[s][1] and np.array_equal(matches[s][0], matches1[s][0]), s
    L = load()
    prev = lambda s: s - 1 if s else count - 1
    want = {s: ref(frames[s]) for s in {0, 15, 16, 31, 32, 47} | {prev(s) for s in (0, 15, 16, 31, 32, 47)}}
    for s in (0, 15, 16, 31, 32, 47):
        assert_kps_equal(feats[s][0], want[s][0])
        assert np.array_equal(feats[s][1], want[s][1]), s
        (k1, d1), (k2, d2) = want[prev(s)], want[s]
        F1, F2 = ox.frame_view(k1, d1, w, h), ox.frame_view(k2, d2, w, h)
        pm = np.stack([k1["x"], k1["y"]], 1).astype(np.float32).copy()
        m = np.zeros(len(k1), np.int32)
        nm = ctypes.c_int()
        L.orbx_ref_search_for_initialization(ctypes.byref(F1), ctypes.byref(F2), ptr(pm), ptr(m), 100, 0.9, 1,
                                             ctypes.byref(nm))
        gm, gn = matches[s]
        assert gn == nm.value and np.array_equal(gm[:len(k1)], m), s
    ctx.close()


# --- 5. the other pyramid forms ----------------------------------------------
@pytest.mark.parametrize("w,h", [(160, 128), (181, 120)])
def test_single_frame_extract(w, h):
    """orbx_extract: the captured graph (the cascade where w % 16 == 0) and
    stream launches, on a poisoned slot."""
    ctx = ox.Context(nfeatures=N, max_w=w, max_h=h, slots=1)
    frames = noise_frames(w, h)
    for mode in (1, 0):
        ctx.set_launch_mode(mode)
        for s in range(3):
            ctx.fill_pyramid(0, 1, 0xFF)
            gk, gd = ctx(frames[s])
            rk, rd = oracle(w, h, s)[:2]
            assert_kps_equal(gk, rk)
            assert np.array_equal(gd, rd), (mode, s)
    ctx.close()


def test_harris_scores():
    w, h = 160, 128
    ctx = poisoned_batch(w, h, 0x5A, score_type=0)
    rk, rd = oracle(w, h, 0, score_type=0)[:2]
    gk, gd = ctx.features(0)
    assert len(rk) > 100
    assert_kps_equal(gk, rk)
    assert np.array_equal(gd, rd)
    ctx.close()


def test_level_narrower_than_two_borders():
    w, h, nl = 160, 128, 10
    sizes = level_sizes(w, h, nl, 1.2)
    assert sizes[-1][0] < 32 <= sizes[-2][0], sizes
    ctx = poisoned_batch(w, h, 0xFF, nlevels=nl)
    for s in range(3):
        rk, rd, levels = oracle(w, h, s, nlevels=nl)[:3]
        gk, gd = ctx.features(s)
        assert_kps_equal(gk, rk)
        assert np.array_equal(gd, rd), s
        for l in (nl - 1, nl - 2, 1):
            assert np.array_equal(ctx.level(s, l), levels[l]), (s, l)
    ctx.close()


def staged_resize_lds(w, h, nlevels, l):
    """launch_extract's LDS bytes of level l's staged strip: the most parent
    rows feeding a strip of 16 interior rows (the row table of cv::resize),
    times the staged row pitch, plus the level's column table."""
    (pw, ph), (lw, lh) = level_sizes(w, h, nlevels, 1.2)[l - 1:l + 1]
    f = ((np.arange(lh) + 0.5) * (float(ph) / lh) - 0.5).astype(np.float32)
    ys = np.floor(f).astype(np.int64)
    s0, s1 = np.clip(ys, 0, ph - 1), np.clip(ys + 1, 0, ph - 1)
    span = max(int(s1[y:y + RES_ROWS].max() - s0[y:y + RES_ROWS].min()) + 1 for y in range(0, lh, RES_ROWS))
    return span * ((pw + 15) & ~15) + 8 * lw


def test_wide_level_fallback():
    """One wide, low frame of two levels whose staged strip exceeds the LDS
    budget, so level 1 takes k_pyr_resize (per-pixel gathers, which still
    writes the border).  3681 is the smallest width that crosses the limit;
    no read-back tells the two kernels apart, so the path is asserted from
    launch_extract's formula, restated in staged_resize_lds."""
    w, h, nl, n = 3681, 128, 2, 1000
    assert staged_resize_lds(w, h, nl, 1) > RESIZE_LDS >= staged_resize_lds(w - 1, h, nl, 1)
    img = synth.noise_frame(w, h, 5)
    ref = RefExtractor(n, nlevels=nl)
    rk, rd = ref(img)
    ctx = ox.Context(nfeatures=n, nlevels=nl, max_w=w, max_h=h, slots=2)
    ctx.upload(np.stack([img, img]))
    ctx.fill_pyramid(0, 2, 0x5A)
    ctx.extract(0, 2)
    ctx.sync()
    for s in range(2):
        gk, gd = ctx.features(s)
        assert len(rk) > 500
        assert_kps_equal(gk, rk)
        assert np.array_equal(gd, rd), s
    for l in (1, 0):
        assert np.array_equal(ctx.level(1, l), ref.level(l)), l
    ctx.close()


def test_scalar_tail_columns_present():
    """181 x 120 has levels whose last columns are off the SSE2 path
    (nvec_resize < w): the general-form words of the staged resize."""
    sizes = level_sizes(181, 120, 8, 1.2)
    assert sum(_vec_cols(lw, True) < lw for lw, _ in sizes[1:]) >= 3, sizes
    # widths that are no multiple of 4: the last interior word straddles the
    # level's edge, in the resize and in describe's reflected staging
    assert {lw % 4 for lw, _ in sizes[1:]} >= {1, 2, 3}
