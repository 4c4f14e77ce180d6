"""Pyramid level 0 read from the frame store (direct mode): batches of frames
whose width is a multiple of 16 run without the padded level-0 copy.  FAST,
the level-1 resize, the Harris score and the describe kernel read the frame
itself; only the describe window of a level-0 keypoint within 21 pixels of an
image edge needs border bytes, which it reflects on the fly (BORDER_REFLECT_101).
Everything is bit-exact against the oracle:

1. which calls select the mode;
2. keypoints whose describe window reaches over each of the four edges;
3. the patch getter at the corners and edge midpoints of the legal range;
4. neighbouring slots (a row that wrapped into the next row or frame would show);
5. the padded level 0 built on demand for the level getters;
6. the Harris score;
7. the pipelined extract_match with its part streams.
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor, load, ptr

pytestmark = pytest.mark.gpu

W, H, N = 160, 128, 300
E = 16    # padded border: legal keypoints lie in [16, w - 16) x [16, h - 16)
R = 18    # the blurred patch is rows / columns -18 .. 18
SPLIT_MIN_FRAMES = 16   # kSplitMinFrames (orbx_extract.hip): frames per pipeline part, at least


def assert_kps_equal(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in ox.KEYPOINT.names:
        assert np.array_equal(a[f], b[f]), (what, f)


def crop(padded, x, y):
    return padded[E + y - R:E + y + R + 1, E + x - R:E + x + R + 1]


_cache = {}


def images():
    """Three different 160x128 images: noise seeds 21 and 22, and the inverse of the first."""
    if "img" not in _cache:
        a = synth.noise_frame(W, H, 21)
        _cache["img"] = [a, synth.noise_frame(W, H, 22), (255 - a).astype(np.uint8)]
    return _cache["img"]


def oracle(i, variant="iso", score_type=1):
    """Oracle output of images()[i], computed once: features, per-level keys, padded levels."""
    key = (i, variant, score_type)
    if key not in _cache:
        ref = RefExtractor(N, variant=variant, score_type=score_type)
        k, d = ref(images()[i])
        _cache[key] = dict(kps=k, desc=d, keys0=ref.level_keys(0), raw=[ref.level(l) for l in range(8)],
                           blur=[ref.level(l, blurred=True) for l in range(8)])
    return _cache[key]


def test_mode_selection():
    ctx = ox.Context(nfeatures=N, max_w=192, max_h=128, slots=1)
    ctx.upload(images()[0])
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct() is True
    ctx.upload(synth.noise_frame(181, 120, 21))     # rows of 181 bytes: the copy stays
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct() is False
    ctx.upload(images()[0])
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct() is True
    assert ctx.launch_mode() == 1
    k, d = ctx(images()[0])                         # orbx_extract's captured graph: the cascade
    assert ctx.level0_direct() is False
    o = oracle(0)
    assert_kps_equal(k, o["kps"])
    assert np.array_equal(d, o["desc"])
    ctx.close()


@pytest.mark.parametrize("contract", [0, 1])
def test_edge_keypoints(contract):
    o = oracle(0, "contract" if contract else "iso")
    k0 = o["keys0"]
    bands = [int((k0["x"] < 21).sum()), int((k0["x"] >= W - 27).sum()), int((k0["y"] < 21).sum()),
             int((k0["y"] >= H - 21).sum())]
    # on the oracle's own output, before any GPU call: windows over every edge (4, 7, 3, 5 of 65)
    assert min(bands) >= 3, (bands, len(k0))
    ctx = ox.Context(nfeatures=N, max_w=W, max_h=H, slots=1)
    ctx.set_fp_contract(contract)
    ctx.upload(images()[0])
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct()
    gk, gd = ctx.features(0)
    assert_kps_equal(gk, o["kps"])
    assert np.array_equal(gd, o["desc"])
    ctx.close()


def test_patch_getter_direct():
    o = oracle(0)
    ctx = ox.Context(nfeatures=N, max_w=W, max_h=H, slots=1)
    ctx.upload(images()[0])
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct()
    want = o["blur"][0]
    for (x, y) in [(16, 16), (W - 17, 16), (16, H - 17), (W - 17, H - 17), (W // 2, 16), (W // 2, H - 17),
                   (16, H // 2), (W - 17, H // 2), (W // 2, H // 2)]:
        got = ctx.describe_patch(0, 0, x, y)
        assert np.array_equal(got, crop(want, x, y)), (x, y, np.argwhere(got != crop(want, x, y))[:4])
    ctx.close()


def test_neighbouring_slots_and_level_getter():
    imgs = images()
    ctx = ox.Context(nfeatures=N, max_w=W, max_h=H, slots=3)
    ctx.upload(np.stack(imgs))

    def check_features(slots, what):
        for s in slots:
            gk, gd = ctx.features(s)
            assert_kps_equal(gk, oracle(s)["kps"], (what, s))
            assert np.array_equal(gd, oracle(s)["desc"]), (what, s)

    for s in range(3):                      # each slot alone
        ctx.extract(s, 1)
        ctx.sync()
        assert ctx.level0_direct()
        check_features([s], "alone")
    ctx.extract(0, 3)                       # one batch of three
    ctx.sync()
    assert ctx.level0_direct()
    check_features(range(3), "batch")
    # the padded level 0 is built on demand; levels 1-7 come from the extraction
    for s in range(3):
        o = oracle(s)
        assert np.array_equal(ctx.level(s, 0), o["raw"][0]), s
        assert np.array_equal(ctx.level(s, 0, blurred=True), o["blur"][0]), s
        for l in range(1, 8):
            assert np.array_equal(ctx.level(s, l), o["raw"][l]), (s, l)
            assert np.array_equal(ctx.level(s, l, blurred=True), o["blur"][l]), (s, l)
    # another image into slot 1: the getter follows, the neighbours keep theirs
    ctx.upload(imgs[0], first=1)
    ctx.extract(1, 1)
    ctx.sync()
    for s, i in ((1, 0), (0, 0), (2, 2)):
        assert np.array_equal(ctx.level(s, 0), oracle(i)["raw"][0]), s
        assert np.array_equal(ctx.level(s, 0, blurred=True), oracle(i)["blur"][0]), s
    assert np.array_equal(ctx.level(1, 1), oracle(0)["raw"][1])
    gk, gd = ctx.features(1)
    assert_kps_equal(gk, oracle(0)["kps"])
    assert np.array_equal(gd, oracle(0)["desc"])
    ctx.close()


def test_harris_score_direct():
    o = oracle(0, score_type=0)
    ctx = ox.Context(nfeatures=N, score_type=0, max_w=W, max_h=H, slots=1)
    ctx.upload(images()[0])
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct()
    gk, gd = ctx.features(0)
    assert len(gk) > 50
    assert_kps_equal(gk, o["kps"])
    assert np.array_equal(gd, o["desc"])
    ctx.close()


def test_pipeline_parts():
    """One extract_match call, asynchronous matching, three pipeline parts
    (three parts take 3 x kSplitMinFrames frames; 2 x would run as two)."""
    B = 3 * SPLIT_MIN_FRAMES
    frames = np.stack(synth.sequence(W, H, B, seed=9))
    ctx = ox.Context(nfeatures=N, max_w=W, max_h=H, slots=B)
    ctx.upload(frames)
    ctx.set_split(3)
    ctx.set_async_match(True)
    ctx.extract_match(0, B, B, mode="init", window=100, nnratio=0.9, check_ori=True)
    ctx.sync()
    assert ctx.level0_direct()
    ref = RefExtractor(N)
    L = load()
    for s in (0, B // 2, B - 1):
        p = (s - 1) % B                      # the sequence is cyclic
        (k1, d1), (k2, d2) = ref(frames[p]), ref(frames[s])
        for slot, (rk, rd) in ((p, (k1, d1)), (s, (k2, d2))):
            gk, gd = ctx.features(slot)
            assert_kps_equal(gk, rk, slot)
            assert np.array_equal(gd, rd), slot
        F1, F2 = ox.frame_view(k1, d1, W, H), ox.frame_view(k2, d2, W, H)
        prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32).copy()
        m = np.zeros(len(k1), np.int32)
        nm = ctypes.c_int()
        L.orbx_ref_search_for_initialization(ctypes.byref(F1), ctypes.byref(F2), ptr(prev), ptr(m), 100, 0.9, 1,
                                             ctypes.byref(nm))
        gm, gn = ctx.matches(s)
        assert gn == nm.value and np.array_equal(gm[:len(k1)], m), s
    ctx.close()
