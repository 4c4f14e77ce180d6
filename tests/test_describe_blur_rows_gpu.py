"""The blur's row pass on aligned words: the seven taps of each of a dword's
four bytes read fixed bytes of the left, centre and right words (the shift is
in the weight constants), the sums are accumulated onto the bits of the float
2^23 and leave as floats by one exact subtraction.  The cases also pin the
raw-byte select (bytes outside the level keep the border's value) at every
position where it switches, alone and inside waves whose two keypoints differ
in it: a wave-uniform instance of the blur without the select was built and
measured with the row pass and would be checked by the
same cases.  Every comparison is exact.

1. every tap at every byte position: one bright pixel seen from every centre
   whose window holds it, at all four alignments of the window origin;
2. magnitude: frames whose row sums reach the top of the accumulator's range
   (255 * 257 = 65,535, asserted on the numpy restatement of the row pass);
3. the raw-byte select's switch: two, one and no rows or columns outside the
   level, the corners, and the tail columns;
4. waves whose two keypoints lie on different sides of that switch (the debug
   hook puts one keypoint in both halves of its wave): whole extractions, with
   the mix asserted on the oracle's keypoints first;
5. k_blur, which shares the row pass: whole blurred levels.

The comparator is the oracle's blurred level (RefExtractor.level(l,
blurred=True)), cropped as test_describe_fused_gpu.crop does, against
Context.describe_patch: the kernel's own staging and blur code.
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from oracle_lib import RefExtractor
import test_describe_shared_gpu as shared
from test_cv24_numpy import _vec_cols, level_sizes
from test_describe_fused_gpu import crop

pytestmark = pytest.mark.gpu

N = shared.N
E = 16        # padded border; legal centres lie in [16, w - 16) x [16, h - 16)
R = 18        # the patch reaches 18 rows / columns
WIN_R = 21    # the staged window starts at (E + x - 21) & ~3
DIRECT, COPY = shared.DIRECT, shared.COPY
SIZES = (DIRECT, COPY)
TAPS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)

_ctx = {}
_ref = {}


def staged(size, img, key):
    """(context with img extracted in slot 0, the oracle's blurred levels, its
    raw levels); one context per size, the oracle once per (size, key)."""
    if size not in _ctx:
        _ctx[size] = [ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1), None]
    ctx, have = _ctx[size]
    if have != key:
        ctx.upload(img)
        ctx.extract(0, 1)
        ctx.sync()
        assert ctx.level0_direct() is (size == DIRECT)
        _ctx[size][1] = key
    if (size, key) not in _ref:
        ref = RefExtractor(N)
        ref(img)
        _ref[(size, key)] = ([ref.level(l, blurred=True) for l in range(8)], [ref.level(l) for l in range(8)])
    return (ctx,) + _ref[(size, key)]


def legal(size, level):
    lw, lh = level_sizes(size[0], size[1], 8, 1.2)[level]
    return lw, lh, (E, lw - E - 1), (E, lh - E - 1)


def assert_patches(ctx, want, level, positions, what):
    bad = []
    for x, y in positions:
        got, exp = ctx.describe_patch(0, level, int(x), int(y)), crop(want[level], x, y)
        if not np.array_equal(got, exp):
            bad.append((x, y, np.argwhere(got != exp)[:3].tolist()))
    assert not bad, (what, level, len(bad), bad[:4])


def weights(c):
    return np.array([(c >> (8 * i)) & 255 for i in range(4)], np.int64)


def row_sums_np(padded):
    """The row pass as the kernels compute it, on every aligned dword of a
    padded level that has a dword on either side: the four sums per dword from
    the three aligned words, accumulated onto the bits of 2^23, and the floats
    after the subtraction.  Returns (float sums, plain seven-tap sums)."""
    p = padded.astype(np.int64)
    nd = p.shape[1] // 4
    dw = p[:, :4 * nd].reshape(p.shape[0], nd, 4)
    wl, wc, wr = dw[:, :-2], dw[:, 1:-1], dw[:, 2:]
    e = np.stack([wl[..., 2], wl[..., 3], wr[..., 0], wr[..., 1]], -1)
    h = np.stack([wl @ weights(0x31221200) + wc @ weights(0x12223137),
                  e @ weights(0x00122212) + wc @ weights(0x22313731),
                  e @ weights(0x12221200) + wc @ weights(0x31373122),
                  wr @ weights(0x00122231) + wc @ weights(0x37312212)], -1)
    assert h.max() < 1 << 23
    f = (h.astype(np.uint32) + np.uint32(0x4B000000)).view(np.float32) - np.float32(8388608.0)
    flat = p[:, :4 * nd]
    plain = sum(TAPS[t] * flat[:, 1 + t:1 + t + 4 * (nd - 2)] for t in range(7))
    return f.reshape(p.shape[0], -1), plain


@pytest.mark.parametrize("size", SIZES)
def test_every_tap_at_every_byte_position(size):
    w, h = size
    px, py = w // 2, h // 2
    us = range(-WIN_R, WIN_R + 1)
    vs = (-21, -18, -4, -3, 0, 3, 4, 18, 21)
    assert {(E + px - u - WIN_R) & 3 for u in us} == {0, 1, 2, 3}
    assert {((E + px - u - WIN_R) & ~3) % 16 for u in us} == {0, 4, 8, 12}
    assert px - WIN_R >= E and px + WIN_R < w - E and py - WIN_R >= E and py + WIN_R < h - E
    img = np.zeros((h, w), np.uint8)
    img[py, px] = 255
    ctx, want, raw = staged(size, img, "pixel")
    # the oracle's blurred level is the kernel's outer product around the pixel
    # (no product is a tie) and zero elsewhere
    spot = np.rint(255.0 * np.outer(TAPS, TAPS) / 65536.0).astype(np.uint8)
    exp0 = np.zeros_like(want[0])
    exp0[E + py - 3:E + py + 4, E + px - 3:E + px + 4] = spot
    assert not np.any((255 * np.outer(TAPS, TAPS)) % 65536 == 32768)
    assert np.array_equal(want[0], exp0)
    assert_patches(ctx, want, 0, [(px - u, py - v) for v in vs for u in us], "pixel")


def magnitude_frames(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    frames = {"full": np.full((h, w), 255, np.uint8),
              "vertical": np.where(xx < w // 2, 255, 0).astype(np.uint8),
              "horizontal": np.where(yy < h // 2, 255, 0).astype(np.uint8),
              "checker": (((xx + yy) & 1) * 255).astype(np.uint8)}
    for p in range(2, 9):
        frames[f"stripes{p}"] = np.where(xx % p == 0, 255, 0).astype(np.uint8)
    return frames


def spread(lo, hi, offsets):
    """Positions around the middle of [lo, hi], clipped to it, without repeats."""
    mid = (lo + hi) // 2
    return sorted({min(max(mid + o, lo), hi) for o in offsets})


@pytest.mark.parametrize("size", SIZES)
def test_magnitude(size):
    w, h = size
    for kind, img in magnitude_frames(w, h).items():
        ctx, want, raw = staged(size, img, kind)
        # CPU: the regrouped, biased row sums equal the plain ones, and the
        # saturated frame takes them to the top of the range
        top = 0
        for level in (0, 2):
            f, plain = row_sums_np(raw[level])
            assert np.array_equal(f, plain.astype(np.float32)), (kind, level)
            top = max(top, int(plain.max()))
        if kind == "full":
            assert top == 65535 == 255 * int(TAPS.sum()), top
        for level in (0, 2):
            lw, lh, (x_lo, x_hi), (y_lo, y_hi) = legal(size, level)
            xs = spread(x_lo, x_hi, (-1000, -2, -1, 0, 1, 1000))
            assert {x & 3 for x in xs} == {0, 1, 2, 3}
            ys = spread(y_lo, y_hi, (-1000, 0, 1000))
            assert_patches(ctx, want, level, [(x, y) for y in ys for x in xs], kind)


@pytest.mark.parametrize("size", SIZES)
def test_raw_byte_switch(size):
    ctx, want, raw = staged(size, shared.image(size, 23), "noise23")
    for level in (0, 2):
        lw, lh, (x_lo, x_hi), (y_lo, y_hi) = legal(size, level)
        assert np.array_equal(ctx.level(0, level), raw[level]), level
        xm, ym = (x_lo + x_hi) // 2, (y_lo + y_hi) // 2
        # the middle's whole ten dword columns and 37 rows lie inside the level
        assert ((E + xm - WIN_R) & ~3) - E >= 0 and ((E + xm - WIN_R) & ~3) - E + 48 <= lw
        assert ym - R >= 0 and ym + R < lh
        # two, one and no rows (columns) of the patch outside the level; up to
        # x_lo + 6 the dword columns still reach outside it
        ys = [y_lo, y_lo + 1, y_lo + 2, y_hi - 2, y_hi - 1, y_hi]
        xs = [x_lo + o for o in range(7)] + [x_hi - o for o in range(7)]
        assert [max(0, R - y) for y in ys[:3]] == [2, 1, 0] and [max(0, y + R - lh + 1) for y in ys[3:]] == [0, 1, 2]
        assert [max(0, R - x) for x in xs[:3]] == [2, 1, 0] and [max(0, x + R - lw + 1) for x in xs[7:10]] == [2, 1, 0]
        pos = [(xm + a, y) for y in ys for a in range(4)] + [(x, ym) for x in xs]
        pos += [(x, y) for x in (x_lo, x_hi) for y in (y_lo, y_hi)]
        pos += [(xm + a, ym) for a in range(4)]
        if size == COPY and level == 0:
            # tail columns: 181 = 180 vectorised columns + 1
            assert _vec_cols(lw, False) == lw - 1
            pos += [(x, y) for x in (x_hi, x_hi - 1, x_hi - 2, x_hi - 3, x_hi - 10, x_hi - 17)
                    for y in (y_lo, ym, y_hi)]
        assert_patches(ctx, want, level, pos, "noise23")


def patch_classes(size, o):
    """Per keypoint of the oracle's output, in output order: "out" when its
    37x37 patch leaves its level, "in" when the patch's ten dword columns and
    37 rows lie inside it (no lane has a raw byte), else "mid"."""
    sizes = level_sizes(size[0], size[1], 8, 1.2)
    cls, octave = [], []
    for l, keys in enumerate(o["keys"]):
        lw, lh = sizes[l]
        for x, y in zip(keys["x"].astype(np.int64).tolist(), keys["y"].astype(np.int64).tolist()):
            x0 = (E + x - WIN_R) & ~3
            c0 = x0 + 4 * ((E + x - x0 - R) >> 2) - E      # level column of the first of the 40
            rows_in = y - R >= 0 and y + R < lh
            if not (rows_in and x - R >= 0 and x + R < lw):
                cls.append("out")
            elif c0 >= 0 and c0 + 40 <= lw:
                cls.append("in")
            else:
                cls.append("mid")
            octave.append(l)
    assert np.array_equal(np.array(octave), o["kps"]["octave"])
    return cls


def assert_mixed_pairs(size, seed, variant):
    """Keypoints 2i and 2i + 1 share a wave: some wave has exactly one patch
    that leaves its level, some both, some neither."""
    cls = patch_classes(size, shared.oracle(size, seed, variant))
    pairs = {tuple(sorted(cls[i:i + 2])) for i in range(0, len(cls) - 1, 2)}
    assert {("in", "out"), ("out", "out"), ("in", "in")} <= pairs, (size, seed, pairs)


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_mixed_waves_single_frames(size, contract):
    shared.check_inputs()
    variant = "contract" if contract else "iso"
    for seed in (21, 22, 23):
        assert_mixed_pairs(size, seed, variant)
    ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1)
    ctx.set_fp_contract(contract)
    for seed in (21, 22, 23):
        ctx.upload(shared.image(size, seed))
        ctx.extract(0, 1)
        ctx.sync()
        shared.assert_features(ctx.features(0), shared.oracle(size, seed, variant), (size, seed, contract))
    ctx.close()


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_mixed_waves_batch_of_three(size, contract):
    shared.check_inputs()
    variant = "contract" if contract else "iso"
    seeds = (21, 22, 23)
    for seed in seeds:
        assert_mixed_pairs(size, seed, variant)
    ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=3)
    ctx.set_fp_contract(contract)
    ctx.upload(np.stack([shared.image(size, s) for s in seeds]))
    ctx.extract(0, 3)
    ctx.sync()
    for slot, s in enumerate(seeds):
        shared.assert_features(ctx.features(slot), shared.oracle(size, s, variant), ("batch", size, s, contract))
    ctx.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", ["full", "checker"])
def test_k_blur_whole_levels(size, kind):
    ctx, want, raw = staged(size, magnitude_frames(*size)[kind], kind)
    for level in range(8):
        assert np.array_equal(ctx.level(0, level, blurred=True), want[level]), (kind, level)
