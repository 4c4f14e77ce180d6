"""Staged pyramid resize (k_pyr_resize_lds): every byte of every padded level
>= 1 against the CPU restatement, on frame sizes chosen so that the levels
cover each path of the kernel's packed row loop.

A level's interior words on the SSE2 column path (nfast of them) run one
thread per word sliding down a 16-row strip, in whole waves; the last
R = nfast % 64 words (R <= 32) share one wave as (row group, word) items.
The widths below were picked on the CPU from the level sizes
(ORBextractor::ComputePyramid, src/ORBextractor.cc:781-822) and the SSE2
column count of cv::resize's VResizeLinearVec_32s8u:

  1328 x 200  level 1 nfast 276 (> 256: a second trip of the workgroup,
              R 20), level 3 nfast 192 (R 0), level 4 w 640 (no scalar-tail
              column, R 32: two row groups), levels 2 and 6 R 38 and 47 (more
              than half a wave: they stay in the sliding form), levels 5 and
              7 R 5 and 28; w % 16 == 0: level 0 read from the frame store
              (staged rows without the left pad)
  918 x 150   level 1 nfast 191 (R 63), level 3 R 4 (sixteen groups),
              level 7 w 256 nfast 64 (R 0, no tail); w % 16 != 0: level 0
              copied, padded parent rows
  928 x 150   level 1 nfast 193 (R 1: one word, sixteen row groups),
              level 4 w 448 (no tail), level 7 nfast 64
  333 x 100   three slots; levels 2 .. 7 have fewer than 64 interior words
              (23 .. 57), level 1 nfast 69 (R 5)
  333 x 120   scale factor 2.01, 3 levels: the source step is over 2, so an
              interior word's taps do not fit 8 bytes and the level takes
              the general (not packed) form

Nearly every padded level height here is no multiple of 16, so the last strip
of a level is short (the first test prints each level's).  The reflected
border words and the scalar-tail words are part of every compared level.  Texture and noise images: with noise any wrong byte shows.
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor
from test_cv24_numpy import level_sizes

pytestmark = pytest.mark.gpu

K_EDGE = 16
STRIP = 16


def vec_count(w):
    """Columns on the SSE2 vertical path of an 8-bit linear resize of width w
    (VResizeLinearVec_32s8u: 16 at a time, then 4 at a time while x < w - 4)."""
    x = 0
    while x <= w - 16:
        x += 16
    while x < w - 4:
        x += 4
    return x


def nfast(w):
    """Interior 4-byte words of a padded row whose columns are all < vec_count."""
    return max(K_EDGE // 4, (K_EDGE + min(w, vec_count(w))) >> 2) - K_EDGE // 4


# name, w, h, nfeatures, scale, nlevels, slots
FRAMES = [
    ("wide-direct", 1328, 200, 1000, 1.2, 8, 1),
    ("r63-copied", 918, 150, 1000, 1.2, 8, 1),
    ("r1-direct", 928, 150, 1000, 1.2, 8, 1),
    ("small-batch", 333, 100, 300, 1.2, 8, 3),
    ("over-2x", 333, 120, 300, 2.01, 3, 1),
]


def frames_of(kind, w, h, slots, seed):
    make = synth.texture_frame if kind == "texture" else synth.noise_frame
    return np.stack([make(w, h, seed + s) for s in range(slots)])


def test_chosen_widths_cover_the_paths():
    """The coverage the frame list claims, recomputed from the widths: the
    remainders, a level under 64 words, one over 256, both level-0 modes,
    levels with and without scalar-tail columns, short last strips."""
    rems, words, tails, short = set(), [], set(), set()
    for name, w, h, _, scale, nlev, _ in FRAMES:
        if nlev != 8:
            continue
        for lvl, (lw, lh) in enumerate(level_sizes(w, h, nlev, scale)):
            if lvl == 0:
                continue
            n = nfast(lw)
            print(f"{name}: level {lvl} {lw} x {lh}: nfast {n}, R {n % 64}, tail columns {lw - min(lw, vec_count(lw))}, "
                  f"last strip {(lh + 2 * K_EDGE) % STRIP or STRIP} rows")
            words.append(n)
            if n >= 64:
                rems.add(n % 64)
            tails.add(lw > vec_count(lw))
            short.add((lh + 2 * K_EDGE) % STRIP != 0)
    assert {0, 1, 63} <= rems and any(1 < r <= 32 for r in rems) and any(32 < r < 63 for r in rems)
    assert min(words) < 64 and max(words) > 256
    assert tails == {True, False} and True in short
    assert {w % 16 == 0 for _, w, *_ in FRAMES} == {True, False}


@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("name,w,h,nf,scale,nlev,slots", FRAMES)
def test_levels_match_oracle(name, w, h, nf, scale, nlev, slots, kind):
    frames = frames_of(kind, w, h, slots, seed=len(name) + w)
    ctx = ox.Context(nfeatures=nf, scale_factor=scale, nlevels=nlev, max_w=w, max_h=h, slots=slots)
    ctx.upload(frames)
    ctx.extract(0, slots)
    ctx.sync()
    assert ctx.level0_direct() == (w % 16 == 0)
    ref = RefExtractor(nf, scale=scale, nlevels=nlev)
    sizes = level_sizes(w, h, nlev, scale)
    for s in range(slots):
        ref(frames[s])
        for lvl in range(1, nlev):
            g, r = ctx.level(s, lvl), ref.level(lvl)
            print(f"{name}/{kind} slot {s} level {lvl}: {sizes[lvl][0]} x {sizes[lvl][1]}, nfast {nfast(sizes[lvl][0])}")
            assert g.shape == r.shape == (sizes[lvl][1] + 2 * K_EDGE, sizes[lvl][0] + 2 * K_EDGE)
            bad = np.argwhere(g != r)
            assert len(bad) == 0, f"slot {s} level {lvl}: {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}"
    ctx.close()
