"""The describe kernel blurs each keypoint's 37x37 patch itself (separable
7x7 on the raw window it stages in LDS) instead of reading a whole-level
blurred pyramid.  Checked bit for bit:

1. the patch (Context.describe_patch, the kernel's own staging + blur device
   functions) against the oracle's blurred level at the extreme legal keypoint
   positions of every level: border bytes that stay raw, taps that read the
   border, tail columns (level widths with w % 4 of 1, 2 and 3);
2. constructed exact .5 ties, where the float (round half to even) and tail
   (+2^15 >> 16) column rules differ;
3. extraction end to end on small frames with and without a tail column, and
   the descriptors recomputed in numpy from the on-demand blurred level getter;
4. the getter after a slot is re-extracted with another image.
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor
from test_cv24_numpy import _reflect101, _vec_cols, blur_np, level_sizes
from test_orb_numpy import describe_np, pattern

pytestmark = pytest.mark.gpu

E = 16    # padded border = EDGE_THRESHOLD: legal keypoints lie in [16, w - 16) x [16, h - 16)
R = 18    # pattern reach: the patch is rows / columns -18 .. 18


def crop(padded, x, y):
    """The 37x37 window around level position (x, y) of a padded level."""
    return padded[E + y - R:E + y + R + 1, E + x - R:E + x + R + 1]


def assert_kps_equal(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in ox.KEYPOINT.names:
        assert np.array_equal(a[f], b[f]), f


def pyramid_only(ctx, img, slot=0):
    ctx.upload(img, first=slot)
    ctx.extract(slot, 1)
    ctx.sync()


def test_patch_matches_oracle_blurred_level():
    # 161 x 120 gives lower-level widths with w % 4 in {0, 1, 2} only; 181 has
    # the tail column at level 0 (181 % 4 = 1, 180 vectorised columns) and
    # w % 4 = 1, 2 and 3 below it
    w, h = 181, 120
    sizes = level_sizes(w, h, 8, 1.2)
    assert sizes[0][0] % 4 == 1 and _vec_cols(w, False) == w - 1
    assert {1, 2, 3} <= {lw % 4 for lw, _ in sizes[1:]}, sizes
    img = synth.noise_frame(w, h, 21)
    ref = RefExtractor(300)
    ref(img)
    ctx = ox.Context(nfeatures=300, max_w=w, max_h=h, slots=1)
    pyramid_only(ctx, img)
    for l, (lw, lh) in enumerate(sizes):
        assert lw - 17 >= 16 and lh - 17 >= 16, (l, lw, lh)
        want = ref.level(l, blurred=True)
        assert np.array_equal(ctx.level(0, l), ref.level(l)), l
        for (x, y) in [(16, 16), (lw - 17, 16), (16, lh - 17), (lw - 17, lh - 17), (lw // 2, lh // 2)]:
            got = ctx.describe_patch(0, l, x, y)
            assert np.array_equal(got, crop(want, x, y)), (l, x, y, np.argwhere(got != crop(want, x, y))[:4])
    ctx.close()


def test_rounding_ties():
    """All rows identical: the vertical pass multiplies the horizontal sum by
    257, so a horizontal sum of 32768 is exactly 128.5.  At the tail column
    160 the result is 129, at a vectorised column 128."""
    w, h = 161, 120
    assert _vec_cols(w, False) == 160
    row = np.random.default_rng(3).integers(0, 256, w).astype(np.uint8)
    row[157:161] = (136, 104, 100, 200)     # REFLECT_101: columns 161, 162, 163 repeat 159, 158, 157
    sym_c = 80
    row[sym_c - 3:sym_c + 4] = (136, 104, 100, 200, 100, 104, 136)
    img = np.repeat(row[None], h, 0)
    taps = np.array([18, 34, 49, 55, 49, 34, 18])
    assert int((taps * np.array([136, 104, 100, 200, 100, 104, 136])).sum()) == 32768
    # CPU pre-check with the numpy restatement, before any GPU call
    padded = np.repeat(row[_reflect101(np.arange(-E, w + E), w)][None], h + 2 * E, 0)
    b = blur_np(padded, w, h)
    assert b[E + 60, E + 160] == 129 and b[E + 60, E + sym_c] == 128
    ref = RefExtractor(300)
    ref(img)
    want = ref.level(0, blurred=True)
    assert np.array_equal(ref.level(0), padded) and np.array_equal(want, b)
    ctx = ox.Context(nfeatures=300, max_w=w, max_h=h, slots=1)
    pyramid_only(ctx, img)
    for (x, y) in [(w - 17, 60), (sym_c, 60), (sym_c - 18, 16), (sym_c + 18, h - 17)]:
        got = ctx.describe_patch(0, 0, x, y)
        assert np.array_equal(got, crop(want, x, y)), (x, y)
    right, mid = ctx.describe_patch(0, 0, w - 17, 60), ctx.describe_patch(0, 0, sym_c, 60)
    assert right[R, R + 16] == 129 and mid[R, R] == 128
    ctx.close()


@pytest.mark.parametrize("w,h,seed", [(161, 120, 1), (160, 120, 1)])
def test_extract_end_to_end_small(w, h, seed):
    n = 300
    frames = synth.sequence(w, h, 2, seed=seed)
    sizes = level_sizes(w, h, 8, 1.2)
    refs = {0: RefExtractor(n), 1: RefExtractor(n, variant="contract")}
    # precondition, on the oracle: keypoints whose patch reaches the tail columns
    if w % 4:
        refs[0](frames[0])
        near = sum(int((refs[0].level_keys(l)["x"] >= lw - 19).sum()) for l, (lw, _) in enumerate(sizes) if lw % 4)
        assert near >= 1
    pat = pattern()
    for contract in (0, 1):
        ref = refs[contract]
        ctx = ox.Context(nfeatures=n, max_w=w, max_h=h, slots=2)
        ctx.set_fp_contract(contract)
        ctx.upload(frames)
        ctx.extract(0, 2)
        ctx.sync()
        feats = [ctx.features(s) for s in range(2)]
        for s in range(2):
            rk, rd = ref(frames[s])
            assert len(rk) > 100
            assert_kps_equal(feats[s][0], rk)
            assert np.array_equal(feats[s][1], rd), (contract, s)
            if contract == 0:
                # descriptors from the getter's blurred levels (ISO arithmetic)
                gk, gd = feats[s]
                blurred = [ctx.level(s, l, blurred=True) for l in range(8)]
                for l in range(8):
                    assert np.array_equal(blurred[l], ref.level(l, blurred=True)), (s, l)
                at = 0
                for l in range(8):
                    lk = ref.level_keys(l)
                    for k in range(0, len(lk), max(1, len(lk) // 12)):
                        d = describe_np(blurred[l], lk["x"][k], lk["y"][k], lk["angle"][k], pat)
                        assert np.array_equal(d, gd[at + k]), (s, l, k)
                    at += len(lk)
                assert at == len(gk)
        # orbx_extract: the captured graph (1) and stream launches (0)
        for mode in (1, 0):
            ctx.set_launch_mode(mode)
            for s in range(2):
                gk, gd = ctx(frames[s])
                rk, rd = ref(frames[s])
                assert_kps_equal(gk, rk)
                assert np.array_equal(gd, rd), (contract, mode, s)
        ctx.close()


def test_blurred_getter_is_fresh():
    w, h, n = 161, 120, 300
    a, b, c = synth.noise_frame(w, h, 31), synth.texture_frame(w, h, 32), synth.noise_frame(w, h, 33)
    ref = RefExtractor(n)
    ctx = ox.Context(nfeatures=n, max_w=w, max_h=h, slots=2)
    ctx.upload(np.stack([a, b]))
    ctx.extract(0, 2)
    ctx.sync()

    def check(slot, img, levels):
        ref(img)
        for l in levels:
            assert np.array_equal(ctx.level(slot, l, blurred=True), ref.level(l, blurred=True)), (slot, l)

    check(1, b, (2,))
    check(0, a, (2, 0))
    ctx.upload(c, first=0)
    ctx.extract(0, 1)
    ctx.sync()
    check(0, c, (2, 0))
    check(1, b, (2,))
    ctx.close()
