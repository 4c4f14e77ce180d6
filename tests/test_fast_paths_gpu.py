"""k_fast_cells, every path: FAST's per-cell output before retainBest (the
debug read-back Context.fast_lists) against the oracle's FAST on each cell's
ROI, and the final keypoints and descriptors against RefExtractor, all by
exact equality, on frames and extractor settings chosen on the CPU so that
together they run

* all five kernel instances (tile pitch 96, 144, 208, banded 336, banded
  runtime pitch), one banded case with >= 3 bands and a short last band;
* interior row widths (nqe dwords) of 1, 2, divisors and non-divisors of 256,
  64 < nqe <= 84 at pitch 336 and nqe > 256 at the runtime pitch;
* every first / last pixel position (j_lo, j_hi in 0..3) of a row's partial
  dwords, cells with one interior dword, cells with 1 and 2 interior rows and
  cells with none (hy <= 6);
* survivor densities from noise at fastTh 5 and 7 (nearly every pixel passes
  the compass test, so every loop iteration crosses the 128-entry scoring
  threshold) over texture at 20 and 35 to a flat frame (no survivor, the
  threshold-7 fallback, no keypoint) and a frame flat but for one textured
  cell (the fallback on most cells); fastTh 5 < 7 makes the fallback the
  higher threshold, where compaction compares every byte;
* a 3-slot batch and one Harris-score case (which reads the cell lists);
* hand-built rings of known score (an isolated 200-on-50 pixel: 149; the
  8- versus 9-pixel arc; dark and bright scores of 1, 254 and 255, the ends of
  the range that the scoring code holds as fp16 subnormals) in the first and
  last interior column and row of a cell.

The cell lists are read back after the whole extraction.  retainBest selects
from a list of more than 512 corners in place in global memory (shorter ones
in LDS), which permutes it: such a list (the wide cells of the banded
instances) is put back into raster order, (y, x) ascending, before it is
compared, entry for entry like the others, whose device order is compared as
it is.

test_frames_cover_the_paths recomputes the cell geometry, the instance choice
and the band plan from the sizes alone (ORBextractor's grid,
src/ORBextractor.cc:560-606, and the launcher's rules) and asserts the list
above; the GPU tests assert that the device reports the same geometry and
instance (Context.fast_instance).
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor
from test_cv24_numpy import level_sizes
from test_fast_numpy import RING, oracle_fast

pytestmark = pytest.mark.gpu

K_EDGE = 16
F32 = np.float32
LDS_TARGET = 40 * 1024          # kFastLdsTarget: four workgroups per CU
STATIC_U16 = 4 * 384 * 2 + 64   # fast_static_lds(false): u16 survivor queues
STATIC_U32 = 4 * 384 * 4 + 64   # fast_static_lds(true)
RETAIN_LDS_CAP = 512            # kRetainCellCap: longer cell lists are selected in place

# name, w, h, nfeatures, scale, nlevels, fastTh, score type, slots, image kind
FRAMES = [
    ("p96-noise5", 100, 87, 500, 1.2, 8, 5, 1, 1, "noise"),
    ("p96-noise7", 107, 101, 500, 1.2, 8, 7, 1, 1, "noise"),
    ("p144-texture20-batch", 333, 250, 500, 1.2, 8, 20, 1, 3, "texture"),
    ("p144-harris", 320, 240, 500, 1.2, 8, 20, 0, 1, "texture"),
    ("p144-one-cell", 333, 250, 500, 1.2, 8, 20, 1, 1, "one-cell"),
    ("p144-rings20", 333, 250, 500, 1.2, 8, 20, 1, 1, "rings"),
    ("p144-rings1", 333, 250, 500, 1.2, 8, 1, 1, 1, "rings"),
    ("p208-texture35", 200, 100, 30, 1.5, 2, 35, 1, 1, "texture"),
    ("p208-flat", 200, 100, 30, 1.5, 2, 20, 1, 1, "flat"),
    ("p336-texture20", 340, 189, 30, 1.5, 2, 20, 1, 1, "texture"),
    ("p336-noise5", 340, 189, 30, 1.5, 2, 5, 1, 1, "noise"),
    ("runtime-texture20", 1100, 140, 120, 1.5, 2, 20, 1, 1, "texture"),
    ("runtime-noise7", 1100, 140, 120, 1.5, 2, 7, 1, 1, "noise"),
]


# ---------------------------------------------------------------------------
# CPU restatement of the cell grid, the instance choice and the band plan
# ---------------------------------------------------------------------------
def cells_of(w, h, nf, scale, nlev):
    """ORBextractor's cell grid per level (src/ORBextractor.cc:560-606), as
    dicts of level, ini_x, ini_y, hx, hy, valid, in the device's cell order."""
    fpl = RefExtractor(nf, scale=scale, nlevels=nlev).features_per_level()
    ratio = F32(F32(w) / F32(h))
    out = []
    for lvl, (lw, lh) in enumerate(level_sizes(w, h, nlev, scale)):
        cols = int(np.sqrt(F32(F32(int(fpl[lvl])) / F32(F32(5) * ratio))))
        rows = int(F32(ratio * F32(cols)))
        assert cols > 0 and rows > 0
        min_x = min_y = K_EDGE
        max_x, max_y = lw - K_EDGE, lh - K_EDGE
        cell_w = int(np.ceil(F32(max_x - min_x) / F32(cols)))
        cell_h = int(np.ceil(F32(max_y - min_y) / F32(rows)))
        h_y = cell_h + 6
        for i in range(rows):
            ini_y = min_y + i * cell_h - 3
            row_valid = True
            if i == rows - 1:
                h_y = max_y + 3 - ini_y
                row_valid = h_y > 0
            h_x = cell_w + 6
            for j in range(cols):
                ini_x = min_x + j * cell_w - 3 if row_valid else 0
                valid = row_valid
                if row_valid and j == cols - 1:
                    h_x = max_x + 3 - ini_x
                    valid = h_x > 0
                out.append(dict(level=lvl, ini_x=ini_x, ini_y=ini_y, hx=h_x if valid else 0, hy=h_y if valid else 0,
                                valid=valid))
    return out


def tile_bytes(hy, pitch):
    return (hy * pitch + 511) & ~511


def lds_bytes(tile):
    return 2 * tile + tile // 32


def band_plan(hmax, pitch, static):
    """(tile bytes, band rows) of the launcher's plan(): whole cells when the
    workgroup's LDS stays within the target, else the fewest equal row bands."""
    whole = tile_bytes(hmax, pitch)
    if lds_bytes(whole) + static <= LDS_TARGET or hmax <= 9:
        return whole, 0
    wh = hmax
    while wh > 9 and lds_bytes(tile_bytes(wh, pitch)) + static > LDS_TARGET:
        wh -= 1
    nint, bmax = hmax - 6, wh - 8
    nbands = (nint + bmax - 1) // bmax
    rows = (nint + nbands - 1) // nbands
    return tile_bytes(min(hmax, rows + 8), pitch), rows


def instance_of(cells):
    """(tile pitch or 0, workgroup threads, band rows) the launcher picks."""
    valid = [c for c in cells if c["valid"]]
    wmax = max((15 + c["hx"] + 15) & ~15 for c in valid)
    hmax = max(c["hy"] for c in valid)
    for pitch in (96, 144, 208):
        if wmax <= pitch and tile_bytes(hmax, pitch) <= 65536:
            return pitch, 256, 0
    if wmax <= 336:
        tile, rows = band_plan(hmax, 336, STATIC_U16)
        if tile <= 65536:
            return 336, 256, rows
    return 0, 256, band_plan(hmax, wmax, STATIC_U32)[1]


def row_shape(c):
    """(nqe, j_lo, j_hi, interior rows) of a valid cell: the interior columns
    3 .. hx - 4 of its 16-byte aligned tile rows, as dwords."""
    sh = (K_EDGE + c["ini_x"]) & 15
    c_lo, c_hi = 3 + sh, c["hx"] - 4 + sh
    nqe = (c_hi >> 2) - (c_lo >> 2) + 1 if c_hi >= c_lo else 0
    return nqe, c_lo & 3, c_hi & 3, max(c["hy"] - 6, 0)


def test_frames_cover_the_paths():
    """The coverage the frame list claims, recomputed from the sizes."""
    instances, nqes, jlo, jhi, rows, bands = set(), {}, set(), set(), set(), []
    for name, w, h, nf, scale, nlev, th, score, slots, kind in FRAMES:
        cells = cells_of(w, h, nf, scale, nlev)
        inst = instance_of(cells)
        instances.add(inst[0])
        hmax = max(c["hy"] for c in cells if c["valid"])
        if inst[2]:
            nint = hmax - 6
            bands.append(((nint + inst[2] - 1) // inst[2], nint % inst[2]))
        shapes = [row_shape(c) for c in cells if c["valid"]]
        print(f"{name}: {w} x {h}, {len(cells)} cells, instance {inst}, tallest cell {hmax}, nqe "
              f"{sorted({s[0] for s in shapes})}, interior rows {sorted({s[3] for s in shapes})}")
        for nqe, a, b, r in shapes:
            rows.add(r)
            if nqe > 0 and r > 0:
                nqes.setdefault(inst[0], set()).add(nqe)
                jlo.add(a)
                jhi.add(b)
    every = set().union(*nqes.values())
    assert instances == {96, 144, 208, 336, 0}
    assert any(n >= 3 and 0 < last for n, last in bands), bands        # >= 3 bands, the last one short
    assert {1, 2} <= every                                               # one dword: q0 == q_last
    assert any(256 % n == 0 and n > 2 for n in every) and any(256 % n != 0 for n in every)
    assert any(64 < n <= 84 for n in nqes[336]) and any(n > 256 for n in nqes[0])
    assert jlo == {0, 1, 2, 3} and jhi == {0, 1, 2, 3}
    assert {0, 1, 2} <= rows                                             # hy <= 6, and 1 and 2 interior rows
    kinds = {(f[9], f[6]) for f in FRAMES}
    assert {("noise", 5), ("noise", 7), ("texture", 20), ("texture", 35), ("flat", 20), ("one-cell", 20),
            ("rings", 20), ("rings", 1)} <= kinds
    assert any(f[8] == 3 for f in FRAMES) and any(f[7] == 0 for f in FRAMES)


# ---------------------------------------------------------------------------
# Frames
# ---------------------------------------------------------------------------
def ring_patch(v, ring_value, first, count):
    """A 7 x 7 patch of value v whose ring pixels first .. first + count - 1
    (mod 16, OpenCV order) are ring_value: the centre's arc of `count`
    contiguous pixels differs from it by |v - ring_value|."""
    p = np.full((7, 7), v, np.uint8)
    for k in range(first, first + count):
        dx, dy = RING[k % 16]
        p[3 + dy, 3 + dx] = ring_value
    return p


def ring_patches():
    pixel = np.full((7, 7), 50, np.uint8)
    pixel[3, 3] = 200                       # 16 ring pixels darker by 150: score 149
    return [
        pixel,
        ring_patch(100, 60, 3, 9),          # a 9-arc darker by 40: score 39
        ring_patch(100, 60, 3, 8),          # 8 only: no corner
        ring_patch(100, 140, 14, 9),        # the bright arc, across the ring's wrap
        ring_patch(100, 140, 14, 8),
        ring_patch(100, 99, 0, 16),         # arc value 1: score 0, never a corner
        ring_patch(100, 98, 5, 9),          # arc value 2: score 1 (a corner at fastTh 1 only)
        ring_patch(100, 101, 0, 16),
        ring_patch(100, 102, 11, 9),
        ring_patch(255, 0, 0, 16),          # arc value 255: score 254, the largest
        ring_patch(254, 0, 2, 10),          # 254: score 253
        ring_patch(0, 255, 0, 16),
        ring_patch(0, 254, 9, 9),
        ring_patch(255, 1, 7, 9),           # 254 again, from the other end of the pixel range
    ]


def frames_of(kind, w, h, slots, seed, cells):
    if kind == "texture":
        return np.stack([synth.texture_frame(w, h, seed + s) for s in range(slots)])
    if kind == "noise":
        return np.stack([synth.noise_frame(w, h, seed + s) for s in range(slots)])
    if kind == "flat":
        return np.stack([synth.flat_frame(w, h) for _ in range(slots)])
    level0 = [c for c in cells if c["level"] == 0 and c["valid"]]
    if kind == "one-cell":      # flat but for the interior of one level-0 cell
        c = level0[len(level0) // 2]
        img = synth.flat_frame(w, h, 120)
        tex = synth.texture_frame(w, h, seed)
        ys, xs = slice(c["ini_y"] + 3, c["ini_y"] + c["hy"] - 3), slice(c["ini_x"] + 3, c["ini_x"] + c["hx"] - 3)
        img[ys, xs] = tex[ys, xs]
        return img[None]
    assert kind == "rings"
    # the patches centred on the four corners of the interior (columns 3 and
    # hx - 4, rows 3 and hy - 4) of the first, a middle and the last cell of
    # level 0 and of their right-hand neighbours' first column
    img = np.full((h, w), 50, np.uint8)
    patches, k = ring_patches(), 0
    for c in (level0[0], level0[len(level0) // 2], level0[-1], level0[1]):
        for cy in (c["ini_y"] + 3, c["ini_y"] + c["hy"] - 4):
            for cx in (c["ini_x"] + 3, c["ini_x"] + c["hx"] - 4):
                img[cy - 3:cy + 4, cx - 3:cx + 4] = patches[k % len(patches)]
                k += 1
    assert k >= len(patches)
    return img[None]


def test_ring_patches_have_the_scores_claimed():
    """The hand-built rings through the oracle's FAST at threshold 1: scores
    149, 39, none, 39, none, none, 1, none, 1, 254, 253, 254, 253, 253."""
    want = [149, 39, None, 39, None, None, 1, None, 1, 254, 253, 254, 253, 253]
    for p, s in zip(ring_patches(), want):
        img = np.full((21, 21), p[0, 0], np.uint8)
        img[7:14, 7:14] = p
        got = [int(k["response"]) for k in oracle_fast(img, 1) if (k["x"], k["y"]) == (10, 10)]
        assert got == ([] if s is None else [s]), (p, s, got)


# ---------------------------------------------------------------------------
# GPU: every cell's list, the instance, the final keypoints
# ---------------------------------------------------------------------------
def expected_cell(level_img, c, fast_th):
    """ORBextractor's cell (src/ORBextractor.cc:599-614): FAST(fastTh) on the
    cell's ROI, FAST(7) when that finds <= 3 corners; (level x, level y, score)
    in raster order."""
    if not c["valid"]:
        return np.zeros((0, 3), np.int64)
    y0, x0 = K_EDGE + c["ini_y"], K_EDGE + c["ini_x"]
    roi = level_img[y0:y0 + c["hy"], x0:x0 + c["hx"]]
    k = oracle_fast(roi, fast_th)
    if len(k) <= 3:
        k = oracle_fast(roi, 7)
    return np.stack([k["x"].astype(np.int64) + c["ini_x"], k["y"].astype(np.int64) + c["ini_y"],
                     k["response"].astype(np.int64)], axis=1).reshape(-1, 3)


@pytest.mark.parametrize("name,w,h,nf,scale,nlev,th,score,slots,kind", FRAMES, ids=[f[0] for f in FRAMES])
def test_cells_and_keypoints_match_oracle(name, w, h, nf, scale, nlev, th, score, slots, kind):
    cells = cells_of(w, h, nf, scale, nlev)
    frames = frames_of(kind, w, h, slots, seed=len(name) + w, cells=cells)
    ctx = ox.Context(nfeatures=nf, scale_factor=scale, nlevels=nlev, score_type=score, fast_th=th, max_w=w, max_h=h,
                     slots=slots)
    ctx.upload(frames)
    ctx.extract(0, slots)
    ctx.sync()
    assert ctx.fast_instance() == instance_of(cells)
    ref = RefExtractor(nf, scale=scale, nlevels=nlev, fast_th=th, score_type=score)
    for s in range(slots):
        rk, rd = ref(frames[s])
        levels = [ref.level(lvl) for lvl in range(nlev)]
        got = ctx.fast_lists(s)
        assert len(got) == len(cells)
        ncorners = 0
        for idx, (c, g) in enumerate(zip(cells, got)):
            assert g[:6] == (c["level"], c["ini_x"], c["ini_y"], c["hx"], c["hy"], c["valid"]), (idx, c, g[:6])
            want = expected_cell(levels[c["level"]], c, th)
            ncorners += len(want)
            dev = g[6]
            if len(dev) > RETAIN_LDS_CAP:   # permuted by retainBest: back into raster order
                dev = dev[np.lexsort((dev[:, 0], dev[:, 1]))]
            assert dev.shape == want.shape and np.array_equal(dev, want), (
                f"{name} slot {s} cell {idx} (level {c['level']}, {c['hx']} x {c['hy']} at {c['ini_x']}, {c['ini_y']}): "
                f"{len(dev)} corners, oracle {len(want)}")
        gk, gd = ctx.features(s)
        print(f"{name} slot {s}: {ncorners} FAST corners in {len(cells)} cells, {len(gk)} keypoints")
        assert len(gk) == len(rk)
        for f in ox.KEYPOINT.names:
            assert np.array_equal(gk[f], rk[f]), (name, s, f)
        assert np.array_equal(gd, rd)
        if kind == "flat":
            assert ncorners == 0 and len(gk) == 0
    ctx.close()
