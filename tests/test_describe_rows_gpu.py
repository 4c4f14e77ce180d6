"""k_describe's IC_Angle by rows: one patch row per lane, v_dot4_u32_u8 against
a host-built table of the circle.  The moments are integers, so every check
is exact.

1. every mask byte and weight: one bright pixel seen from every centre around
   it (Context.describe_moments: the kernel's own staging and IC_Angle code);
2. magnitude: saturated half-planes and a saturated frame;
3. general data, including the level's corner positions (on the frame whose
   level 0 is read from the frame store these take the reflecting staging);
4. the blurred patch at the positions where its three row strips meet, where
   the raw-byte rule switches and where the tail columns are;
5. extraction end to end in both contraction modes.

The comparator is tests/test_ic_moments_numpy.py's moments_np, which is pinned
against the oracle there, over the level as the context reads it back.

Legal centres lie at least 16 rows inside a level and the patch reaches 18, so
the raw-byte rule can switch only in the patch's first two and last two rows:
inside the first and the last strip.  The seam rows are asserted on their own
at every position.
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor
import test_describe_shared_gpu as shared
from test_cv24_numpy import _vec_cols, level_sizes
from test_describe_fused_gpu import crop
from test_ic_moments_numpy import HP, moments_np
from test_orb_numpy import umax_np

pytestmark = pytest.mark.gpu

N = shared.N
E = 16
DIRECT, COPY = shared.DIRECT, shared.COPY
SIZES = (DIRECT, COPY)

_ctx = {}


def context(size, img, key):
    """One context per (size, key), its slot 0 extracted from img once."""
    if (size, key) not in _ctx:
        ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1)
        ctx.upload(img)
        ctx.extract(0, 1)
        ctx.sync()
        assert ctx.level0_direct() is (size == DIRECT)
        _ctx[(size, key)] = ctx
    return _ctx[(size, key)]


def both_halves(ctx, level, x, y):
    lo, hi = ctx.describe_moments(0, level, int(x), int(y))
    assert lo == hi, (level, x, y, lo, hi)
    return lo


def legal(size, level):
    lw, lh = level_sizes(size[0], size[1], 8, 1.2)[level]
    return lw, lh, (E, lw - E - 1), (E, lh - E - 1)


@pytest.mark.parametrize("size", SIZES)
def test_every_mask_byte_and_weight(size):
    w, h = size
    px, py = w // 2, h // 2
    umax = umax_np()
    offs = range(-17, 18)
    assert {(px - u) & 3 for u in offs} == {0, 1, 2, 3}
    assert px - 17 >= E and px + 17 < w - E and py - 17 >= E and py + 17 < h - E
    img = np.zeros((h, w), np.uint8)
    img[py, px] = 255
    ctx = context(size, img, "pixel")
    bad = []
    for v in offs:
        for u in offs:
            inside = abs(v) <= HP and abs(u) <= umax[min(abs(v), HP)]
            want = (255 * v, 255 * u) if inside else (0, 0)
            got = both_halves(ctx, 0, px - u, py - v)
            if got != want:
                bad.append((u, v, got, want))
    assert not bad, (len(bad), bad[:6])


def spread(lo, hi, offsets):
    """Positions around the middle of [lo, hi], clipped to it, without repeats."""
    mid = (lo + hi) // 2
    return sorted({min(max(mid + o, lo), hi) for o in offsets})


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", ["vertical", "horizontal", "full"])
def test_magnitude(size, kind):
    w, h = size
    img = np.zeros((h, w), np.uint8)
    if kind == "vertical":
        img[:, :w // 2] = 255
    elif kind == "horizontal":
        img[:h // 2] = 255
    else:
        img[:] = 255
    ctx = context(size, img, kind)
    umax = umax_np()
    largest = 0
    for level in (0, 1, 7):
        lw, lh, (x_lo, x_hi), (y_lo, y_hi) = legal(size, level)
        raw = ctx.level(0, level)
        assert raw.shape == (lh + 2 * E, lw + 2 * E)
        offsets = (-16, -9, -2, -1, 0, 1, 3, 8, 15)
        for y in spread(y_lo, y_hi, offsets):
            for x in spread(x_lo, x_hi, offsets):
                want = moments_np(raw, x, y, umax)
                assert both_halves(ctx, level, x, y) == want, (level, x, y)
                largest = max(largest, abs(want[0]), abs(want[1]))
    # a saturated half-plane that ends at the centre (level 0's positions
    # include it) gives the largest moment there is: 255 * sum |u| over half
    # the circle
    if kind != "full":
        half_circle = int((umax * (umax + 1) // 2).sum() * 2 - umax[0] * (umax[0] + 1) // 2)
        assert largest == 255 * half_circle, (largest, 255 * half_circle)


@pytest.mark.parametrize("size", SIZES)
def test_general_data(size):
    w, h = size
    img = shared.image(size, 21)
    ctx = context(size, img, "noise21")
    umax = umax_np()
    rng = np.random.default_rng(1900 + w)
    for level in (0, 1, 3, 7):
        lw, lh, (x_lo, x_hi), (y_lo, y_hi) = legal(size, level)
        raw = ctx.level(0, level)
        # exactly kEdge from each level edge; on the frame-store level 0 the
        # window of each crosses the image edge
        pos = [(x_lo, y_lo), (x_hi, y_lo), (x_lo, y_hi), (x_hi, y_hi),
               (x_lo, (y_lo + y_hi) // 2), (x_hi, (y_lo + y_hi) // 2),
               ((x_lo + x_hi) // 2, y_lo), ((x_lo + x_hi) // 2, y_hi)]
        while len(pos) < 64:
            pos.append((int(rng.integers(x_lo, x_hi + 1)), int(rng.integers(y_lo, y_hi + 1))))
        if level == 0:
            assert {x & 3 for x, _ in pos} == {0, 1, 2, 3}
        for x, y in pos:
            assert both_halves(ctx, level, x, y) == moments_np(raw, x, y, umax), (level, x, y)


@pytest.mark.parametrize("size", SIZES)
def test_blurred_patch_seams_and_edges(size):
    w, h = size
    img = shared.image(size, 22)
    ref = RefExtractor(N)
    ref(img)
    ctx = context(size, img, "noise22")
    for level in (0, 2):
        lw, lh, (x_lo, x_hi), (y_lo, y_hi) = legal(size, level)
        want = ref.level(level, blurred=True)
        assert np.array_equal(ctx.level(0, level), ref.level(level)), level
        xm = (x_lo + x_hi) // 2
        xs = [xm, xm + 1, xm + 2, xm + 3]
        assert {x & 3 for x in xs} == {0, 1, 2, 3}
        # the patch reaches 18 rows: the first two (last two) rows of the
        # patch at y_lo, y_lo + 1 (y_hi, y_hi - 1) lie outside the level
        ys = [y_lo, y_lo + 1, y_lo + 2, y_lo + 9, (y_lo + y_hi) // 2, y_hi - 9, y_hi - 2, y_hi - 1, y_hi]
        pos = [(x, y) for x in xs for y in ys]
        if size == COPY and level == 0:
            # tail columns: 181 = 180 vectorised columns + 1
            assert _vec_cols(lw, False) == lw - 1
            pos += [(x, y) for x in (x_hi, x_hi - 1, x_hi - 2, x_hi - 3, x_hi - 10, x_hi - 17)
                    for y in (y_lo, (y_lo + y_hi) // 2, y_hi)]
        for x, y in pos:
            got, exp = ctx.describe_patch(0, level, x, y), crop(want, x, y)
            assert np.array_equal(got[11:14], exp[11:14]), (level, x, y, "rows 11-13")
            assert np.array_equal(got[23:26], exp[23:26]), (level, x, y, "rows 23-25")
            assert np.array_equal(got, exp), (level, x, y, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_single_frame(size, contract):
    shared.check_inputs()
    o = shared.oracle(size, 21, "contract" if contract else "iso")
    ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1)
    ctx.set_fp_contract(contract)
    ctx.upload(shared.image(size, 21))
    ctx.extract(0, 1)
    ctx.sync()
    shared.assert_features(ctx.features(0), o, (size, contract))
    ctx.close()


@pytest.mark.parametrize("contract", [0, 1])
def test_batch_of_three(contract):
    shared.check_inputs()
    seeds = (21, 22, 23)
    ctx = ox.Context(nfeatures=N, max_w=DIRECT[0], max_h=DIRECT[1], slots=3)
    ctx.set_fp_contract(contract)
    ctx.upload(np.stack([shared.image(DIRECT, s) for s in seeds]))
    ctx.extract(0, 3)
    ctx.sync()
    for slot, s in enumerate(seeds):
        shared.assert_features(ctx.features(slot), shared.oracle(DIRECT, s, "contract" if contract else "iso"),
                               ("batch", s, contract))
    ctx.close()


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_single_call(size, contract):
    """orbx_extract: k_describe also writes the page-locked result block."""
    shared.check_inputs()
    ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1)
    ctx.set_fp_contract(contract)
    for seed in (22, 23):
        got = ctx(shared.image(size, seed))
        shared.assert_features(got, shared.oracle(size, seed, "contract" if contract else "iso"),
                               ("single call", size, seed, contract))
    ctx.close()


@pytest.mark.parametrize("contract", [0, 1])
def test_harris_score(contract):
    shared.check_inputs()
    o = shared.oracle(DIRECT, 21, "contract" if contract else "iso", score_type=0)
    assert len(o["kps"]) > 50
    ctx = ox.Context(nfeatures=N, score_type=0, max_w=DIRECT[0], max_h=DIRECT[1], slots=1)
    ctx.set_fp_contract(contract)
    ctx.upload(shared.image(DIRECT, 21))
    ctx.extract(0, 1)
    ctx.sync()
    shared.assert_features(ctx.features(0), o, ("harris", contract))
    got = ctx(shared.image(DIRECT, 21))
    shared.assert_features(got, o, ("harris single call", contract))
    ctx.close()
