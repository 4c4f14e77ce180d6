"""k_fast_cells' tail: non-max suppression from the list of scored pixels and
ranked emission, against the dword path and the oracle.

The method is test_fast_paths_gpu's: FAST's per-cell output before retainBest
(Context.fast_lists) against the oracle's FAST on each cell's ROI, device
order as it is, and the final keypoints and descriptors against RefExtractor,
all by exact equality.  Here the list's capacity is set per case
(Context.set_fast_list_cap) and the path that every cell took is read back
(Context.fast_paths) and compared with the path predicted on the CPU from the
S' map (score_map, a numpy restatement checked against the oracle's FAST):
a band of a cell takes the list path when the launch has a list and the band's
scored pixels (S >= the pass's threshold, halo rows of a band included) number
at most its capacity.

test_cases_cover_the_tail asserts on the CPU, from the score maps, that the
frames contain what the case list claims (see there); it needs no GPU.

Not among the cases: a list longer than its cell's list_cap.  The geometry
sets list_cap = ceil(iw / 2) * ceil(ih / 2) for an interior of iw x ih pixels,
the largest number of strict 8-neighbour maxima it can hold (no two in one
2 x 2 block), so no frame reaches the guard; it and the error flag are the
shared code of both paths' emission.
"""
import functools

import numpy as np
import pytest

import orb_slam_amd as ox
from oracle_lib import RefExtractor
from test_fast_numpy import RING, oracle_fast
from test_fast_paths_gpu import (K_EDGE, LDS_TARGET, RETAIN_LDS_CAP, STATIC_U16, STATIC_U32, cells_of, expected_cell,
                                 frames_of, instance_of, lds_bytes, tile_bytes)

DEFAULT_CAP = 1536   # kFastListCap
LOW = 7              # the fallback threshold


# ---------------------------------------------------------------------------
# CPU: S' map, NMS, the launcher's capacity rule, the path of every cell
# ---------------------------------------------------------------------------
def score_map(roi, t):
    """S' of a cell's ROI at threshold t (test_fast_numpy.fast_np's
    definitions): the FAST score where it is >= t, else 0; 0 outside the
    interior (rows / columns 3 .. n - 4)."""
    img = np.asarray(roi, np.int32)
    rows, cols = img.shape
    S = np.zeros((rows, cols), np.int32)
    if rows < 7 or cols < 7:
        return S
    v = img[3:rows - 3, 3:cols - 3]
    d = np.stack([v - img[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] for dx, dy in RING])
    dd = np.concatenate([d, d[:8]])
    A = np.stack([dd[k:k + 9].min(axis=0) for k in range(16)]).max(axis=0)
    B = np.stack([(-dd[k:k + 9]).min(axis=0) for k in range(16)]).max(axis=0)
    m = np.maximum(A, B)
    S[3:rows - 3, 3:cols - 3] = np.where(m > t, np.maximum(m, t) - 1, 0)
    return S


def nms(S):
    """Kept pixels of an S' map: strictly greater than all 8 neighbours."""
    P = np.pad(S, 1)
    keep = S > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                keep &= S > P[dy:dy + S.shape[0], dx:dx + S.shape[1]]
    return keep


def effective_cap(inst, hmax, wmax, cap):
    """The capacity the launcher runs with: `cap` where the list and its kept
    bitmap fit behind the planned LDS within the 40 KB target, else 0."""
    pitch, _, rows = inst
    tile = tile_bytes(min(hmax, rows + 8) if rows else hmax, pitch if pitch else wmax)
    entry, static = (2, STATIC_U16) if pitch else (4, STATIC_U32)
    extra = tile // 8 + (((cap + 1) * entry + 15) & ~15)   # + the spare entry
    return cap if cap > 0 and lds_bytes(tile) + static + extra <= LDS_TARGET and tile // 32 <= 1536 else 0


def cell_paths(roi, c, th, cap, band_rows):
    """(path mask, S' map of the final pass, its threshold) of a valid cell:
    bit 0 where a band's scored pixels fit the list, bit 1 where not."""
    hy = c["hy"]
    if hy <= 6:
        return 0, score_map(roi, th), th

    def bands_mask(S):
        mask, brows = 0, band_rows if band_rows > 0 else hy
        for b0 in range(3, hy - 3, brows):
            b1 = min(b0 + brows, hy - 3)
            s0, s1 = max(3, b0 - 1), min(hy - 4, b1)
            n = int(np.count_nonzero(S[s0:s1 + 1])) if th > 0 else 0
            mask |= 1 if 0 < cap and n <= cap else 2
        return mask

    S = score_map(roi, th)
    mask = bands_mask(S)
    if int(np.count_nonzero(nms(S))) <= 3:   # the threshold-7 fallback
        if th > LOW or band_rows > 0:        # (whole cells at fastTh <= 7 only filter)
            S = score_map(roi, min(th, LOW))
            mask |= bands_mask(S)
        return mask, S, LOW
    return mask, S, th


CASES = [
    # name, w, h, nfeatures, scale, nlevels, fastTh, score type, slots, image kind, list capacity (None: default,
    # "edge": a cell's own count, see edge_cap)
    ("p96-noise5", 100, 87, 500, 1.2, 8, 5, 1, 1, "noise", None),
    ("p96-noise5-cap0", 100, 87, 500, 1.2, 8, 5, 1, 1, "noise", 0),
    ("p96-noise7-cap64", 107, 101, 500, 1.2, 8, 7, 1, 1, "noise", 64),
    ("p144-texture20-batch", 333, 250, 500, 1.2, 8, 20, 1, 3, "texture", None),
    ("p144-texture20-cap0", 333, 250, 500, 1.2, 8, 20, 1, 1, "texture", 0),
    ("p144-texture20-edge", 333, 250, 500, 1.2, 8, 20, 1, 1, "texture", "edge"),
    ("p144-texture5", 333, 250, 500, 1.2, 8, 5, 1, 1, "texture", None),
    ("p144-harris", 320, 240, 500, 1.2, 8, 20, 0, 1, "texture", None),
    ("p144-one-cell", 333, 250, 500, 1.2, 8, 20, 1, 1, "one-cell", None),
    ("p144-one-cell-cap0", 333, 250, 500, 1.2, 8, 20, 1, 1, "one-cell", 0),
    ("p144-rings20", 333, 250, 500, 1.2, 8, 20, 1, 1, "rings", None),
    ("p144-rings1", 333, 250, 500, 1.2, 8, 1, 1, 1, "rings", None),
    ("p144-dots20", 333, 250, 500, 1.2, 8, 20, 1, 1, "dots", None),
    ("p144-dots20-cap0", 333, 250, 500, 1.2, 8, 20, 1, 1, "dots", 0),
    ("p144-dots5", 333, 250, 500, 1.2, 8, 5, 1, 1, "dots", None),
    ("p144-dots5-cap0", 333, 250, 500, 1.2, 8, 5, 1, 1, "dots", 0),
    ("p144-noise7", 333, 250, 500, 1.2, 8, 7, 1, 1, "noise", None),
    ("p208-texture35", 200, 100, 30, 1.5, 2, 35, 1, 1, "texture", None),
    ("p208-flat", 200, 100, 30, 1.5, 2, 20, 1, 1, "flat", None),
    ("p336-texture20-cap1200", 340, 189, 30, 1.5, 2, 20, 1, 1, "texture", 1200),
    ("p336-texture20-cap0", 340, 189, 30, 1.5, 2, 20, 1, 1, "texture", 0),
    ("p336-speckle-cap96", 340, 189, 30, 1.5, 2, 20, 1, 1, "speckle", 96),
    ("runtime-speckle-cap128", 1100, 140, 120, 1.5, 2, 20, 1, 1, "speckle", 128),
    ("runtime-speckle-cap0", 1100, 140, 120, 1.5, 2, 20, 1, 1, "speckle", 0),
]


def dots_frame(w, h, cells):
    """Isolated pixels on a flat background of 50 in level-0 cells (a pixel of
    value 50 + d alone scores d - 1; at level 0 pixel x lies in byte x & 3 of
    its tile dword):
    cell A: one pixel (the cell's only scored pixel);
    cell B: pairs in one dword, pixels 0/2, 0/3 and 1/3, all kept;
    cell C: two equal adjacent pixels and a 2 x 2 plateau: scored, none kept;
    cell D: a pixel of score 5 before one of score 149 in the same 32-byte
    bitmap word, and one more of score 6 (fastTh 5: three kept corners, the
    fallback to 7 emits one and its rank skips the others)."""
    img = np.full((h, w), 50, np.uint8)
    level0 = [c for c in cells if c["level"] == 0 and c["valid"]]
    a, b, c, d = level0[0], level0[1], level0[len(level0) // 2], level0[-2]

    def at(cell, row, x4, k):   # interior row `row`, the dword at or after interior column x4, pixel k
        x = (cell["ini_x"] + 3 + x4 + 3) & ~3
        return cell["ini_y"] + 3 + row, x + k

    img[at(a, 8, 12, 1)] = 200
    for row, (k0, k1) in zip((6, 14, 22), ((0, 2), (0, 3), (1, 3))):
        img[at(b, row, 12, k0)] = 200
        img[at(b, row, 12, k1)] = 190
    y, x = at(c, 6, 8, 1)
    img[y, x:x + 2] = 200
    y, x = at(c, 16, 16, 3)
    img[y:y + 2, x:x + 2] = 200
    # (pitch 144: a row's tile bytes start at bit 0 or 16 of a bitmap word, and a column that is a multiple of 32
    # at one that is a multiple of 16, so columns + 4 and + 12 share a word)
    y, x = d["ini_y"] + 3 + 7, (d["ini_x"] + 3 + 31) & ~31
    img[y, x + 4] = 56
    img[y, x + 12] = 200
    img[y + 9, x + 8] = 57
    return img[None]


def speckle_frame(w, h, seed):
    """One pixel in about 150 of a flat frame set to a random value: few scored
    pixels per band, so that the small lists that fit beside the banded
    instances' tiles hold most bands."""
    r = np.random.default_rng(seed)
    img = np.full((h, w), 120, np.uint8)
    on = r.random((h, w)) < 1.0 / 150
    img[on] = r.integers(0, 256, int(on.sum()), dtype=np.uint8)
    return img[None]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Frames, cells, instance and, per slot and cell, the expected path mask,
    the final S' map and threshold (computed once per case)."""
    _, w, h, nf, scale, nlev, th, score, slots, kind, cap = next(c for c in CASES if c[0] == name)
    cells = cells_of(w, h, nf, scale, nlev)
    if kind == "dots":
        frames = dots_frame(w, h, cells)
    elif kind == "speckle":
        frames = speckle_frame(w, h, w)
    else:
        frames = frames_of(kind, w, h, slots, seed=len(name.split("-cap")[0].split("-edge")[0]) + w, cells=cells)
    inst = instance_of(cells)
    valid = [c for c in cells if c["valid"]]
    hmax, wmax = max(c["hy"] for c in valid), max((15 + c["hx"] + 15) & ~15 for c in valid)
    ref = RefExtractor(nf, scale=scale, nlevels=nlev, fast_th=th, score_type=score)
    rois = []
    for s in range(slots):
        ref(frames[s])
        levels = [ref.level(lvl).copy() for lvl in range(nlev)]
        rois.append([levels[c["level"]][K_EDGE + c["ini_y"]:K_EDGE + c["ini_y"] + c["hy"],
                                        K_EDGE + c["ini_x"]:K_EDGE + c["ini_x"] + c["hx"]] if c["valid"] else None
                     for c in cells])
    if cap == "edge":
        cap = edge_cap(rois[0], cells, th)
    cap_eff = effective_cap(inst, hmax, wmax, DEFAULT_CAP if cap is None else cap)
    paths = [[cell_paths(r, c, th, cap_eff, inst[2]) if c["valid"] else (0, None, th) for r, c in zip(rois[s], cells)]
             for s in range(slots)]
    return frames, cells, inst, cap, cap_eff, rois, paths


def edge_cap(rois, cells, th):
    """A capacity n such that one whole cell has exactly n scored pixels and
    another n + 1 (the smallest such n over 30)."""
    counts = sorted({int(np.count_nonzero(score_map(r, th))) for r, c in zip(rois, cells) if c["valid"]})
    for n in counts:
        if n > 30 and n + 1 in counts:
            return n
    raise AssertionError(f"no two cells with consecutive counts: {counts}")


def test_score_map_matches_oracle():
    """score_map + nms against the oracle's FAST on cell ROIs of three cases."""
    for name in ("p144-dots5", "p96-noise5", "p208-texture35"):
        _, w, h, nf, scale, nlev, th, *_ = next(c for c in CASES if c[0] == name)
        _, cells, _, _, _, rois, _ = case_data(name)
        for c, roi in zip(cells, rois[0]):
            if not c["valid"]:
                continue
            S = score_map(roi, th)
            yy, xx = np.nonzero(nms(S))
            k = oracle_fast(roi, th)
            assert np.array_equal(k["x"], xx) and np.array_equal(k["y"], yy) and np.array_equal(k["response"], S[yy, xx])


def test_cases_cover_the_tail():
    """What the case list claims, from the score maps."""
    D = {c[0]: case_data(c[0]) for c in CASES}
    masks = {n: [p[0] for p in d[6][0]] for n, d in D.items()}
    insts = {n: d[2] for n, d in D.items()}
    for n, d in D.items():
        print(f"{n}: instance {d[2]}, capacity {d[3]} -> {d[4]}, cells by path "
              f"{ {m: masks[n].count(m) for m in sorted(set(masks[n]))} }")
    # count == capacity on the list path, capacity + 1 on the dword path, on one frame
    _, cells, _, cap, cap_eff, rois, paths = D["p144-texture20-edge"]
    assert cap == cap_eff
    cnt = [int(np.count_nonzero(score_map(r, 20))) if c["valid"] else -1 for r, c in zip(rois[0], cells)]
    assert masks["p144-texture20-edge"][cnt.index(cap)] & 1 and masks["p144-texture20-edge"][cnt.index(cap + 1)] & 2
    # capacity 0: the dword path everywhere; the default: the list wherever a cell has interior rows
    for n in ("p96-noise5-cap0", "p144-texture20-cap0", "p144-dots20-cap0", "p336-texture20-cap0", "runtime-speckle-cap0"):
        assert D[n][4] == 0 and set(masks[n]) <= {0, 2}
    for n in ("p144-texture20-batch", "p144-dots20", "p144-dots5", "p144-rings20", "p144-harris", "p208-texture35"):
        assert D[n][4] == DEFAULT_CAP and set(masks[n]) <= {0, 1} and 1 in masks[n]
    # noise: nearly every pixel is scored, cells overflow the default capacity and a small one
    assert 2 in masks["p144-noise7"] and D["p144-noise7"][4] == DEFAULT_CAP
    assert 3 in masks["p96-noise7-cap64"] or 2 in masks["p96-noise7-cap64"]
    assert 1 in masks["p96-noise5"]          # small cells of noise still fit the default list
    # the dots frame: cells with no scored pixel, with exactly one; pairs in one dword; plateaus
    _, cells, _, _, _, rois, paths = D["p144-dots20"]
    level0 = [i for i, c in enumerate(cells) if c["level"] == 0 and c["valid"]]
    nsc = {i: int(np.count_nonzero(score_map(rois[0][i], 20))) for i in level0}
    assert 0 in nsc.values() and nsc[level0[0]] == 1
    b, c, d = level0[1], level0[len(level0) // 2], level0[-2]
    Sb = score_map(rois[0][b], 20)
    yy, xx = np.nonzero(nms(Sb))
    pairs = {(int(x0 + cells[b]["ini_x"]) & 3, int(x1 + cells[b]["ini_x"]) & 3)
             for (y0, x0), (y1, x1) in zip(zip(yy[:-1], xx[:-1]), zip(yy[1:], xx[1:]))
             if y0 == y1 and (x0 + cells[b]["ini_x"]) >> 2 == (x1 + cells[b]["ini_x"]) >> 2}
    assert pairs == {(0, 2), (0, 3), (1, 3)}, pairs
    Sc = score_map(rois[0][c], 20)
    assert np.count_nonzero(Sc) == 6 and not nms(Sc).any() and len(set(Sc[Sc > 0])) == 1
    # fastTh 5: cell D keeps three corners, of scores 5, 149, 6 in raster order, and emits the 149 alone
    _, cells5, _, _, _, rois5, paths5 = D["p144-dots5"]
    mask, Sd, t = paths5[0][d]
    yy, xx = np.nonzero(nms(Sd))
    assert mask == 1 and t == LOW and list(Sd[yy, xx]) == [5, 149, 6]
    pos = [int(y) * 144 + K_EDGE + cells5[d]["ini_x"] + int(x) - ((K_EDGE + cells5[d]["ini_x"]) & ~15) for y, x in zip(yy, xx)]
    assert D["p144-dots5"][2][0] == 144 and pos[0] >> 5 == pos[1] >> 5   # the same word of the kept bitmap
    # kept corners in the first and last interior row and column (the rings frames)
    _, cellsr, _, _, _, roisr, _ = D["p144-rings20"]
    seen = set()
    for cc, roi in zip(cellsr, roisr[0]):
        if cc["valid"] and cc["level"] == 0 and cc["hy"] > 6:
            yy, xx = np.nonzero(nms(score_map(roi, 20)))
            seen |= {("row", 0)} if 3 in yy else set()
            seen |= {("row", 1)} if cc["hy"] - 4 in yy else set()
            seen |= {("col", 0)} if 3 in xx else set()
            seen |= {("col", 1)} if cc["hx"] - 4 in xx else set()
    assert len(seen) == 4
    # flat but for one cell: the fallback's second pass on most cells; flat: nothing
    assert masks["p144-one-cell"].count(1) > len(masks["p144-one-cell"]) // 2 and set(masks["p208-flat"]) <= {0, 1}
    # a banded instance with >= 3 bands whose halo rows hold scored pixels, on both paths; the runtime pitch
    pitch, _, rows = insts["p336-texture20-cap1200"]
    hmax = max(cc["hy"] for cc in D["p336-texture20-cap1200"][1] if cc["valid"])
    assert pitch == 336 and rows > 0 and (hmax - 6 + rows - 1) // rows >= 3
    assert D["p336-texture20-cap1200"][4] == 1200 and 3 in masks["p336-texture20-cap1200"]   # a cell with bands on both paths
    assert D["p336-speckle-cap96"][4] == 96 and 1 in masks["p336-speckle-cap96"]
    halo = False
    for cc, roi in zip(D["p336-texture20-cap1200"][1], D["p336-texture20-cap1200"][5][0]):
        if cc["valid"] and cc["hy"] > 6 + rows:
            S = score_map(roi, 20)
            halo |= bool(S[3 + rows - 1].any() and S[3 + rows].any())   # rows on both sides of the first band's end
    assert halo
    assert insts["runtime-speckle-cap128"][0] == 0 and D["runtime-speckle-cap128"][4] == 128
    assert 1 in masks["runtime-speckle-cap128"]
    assert any(c[8] == 3 for c in CASES) and any(c[7] == 0 for c in CASES)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_lists_paths_and_keypoints(name):
    _, w, h, nf, scale, nlev, th, score, slots, kind, _ = next(c for c in CASES if c[0] == name)
    frames, cells, inst, cap, cap_eff, rois, paths = case_data(name)
    ctx = ox.Context(nfeatures=nf, scale_factor=scale, nlevels=nlev, score_type=score, fast_th=th, max_w=w, max_h=h,
                     slots=slots)
    if cap is not None:
        ctx.set_fast_list_cap(cap)
    ctx.upload(frames)
    ctx.extract(0, slots)
    ctx.sync()
    assert ctx.fast_instance() == inst
    ref = RefExtractor(nf, scale=scale, nlevels=nlev, fast_th=th, score_type=score)
    for s in range(slots):
        rk, rd = ref(frames[s])
        levels = [ref.level(lvl) for lvl in range(nlev)]
        got_paths, got_cap = ctx.fast_paths(s)
        assert got_cap == cap_eff
        assert list(got_paths) == [p[0] for p in paths[s]], name
        got = ctx.fast_lists(s)
        assert len(got) == len(cells)
        for idx, (c, g) in enumerate(zip(cells, got)):
            assert g[:6] == (c["level"], c["ini_x"], c["ini_y"], c["hx"], c["hy"], c["valid"]), (idx, c, g[:6])
            want = expected_cell(levels[c["level"]], c, th)
            dev = g[6]
            if len(dev) > RETAIN_LDS_CAP:   # permuted by retainBest: back into raster order
                dev = dev[np.lexsort((dev[:, 0], dev[:, 1]))]
            assert dev.shape == want.shape and np.array_equal(dev, want), (
                f"{name} slot {s} cell {idx} (level {c['level']}, {c['hx']} x {c['hy']} at {c['ini_x']}, {c['ini_y']}, "
                f"path {got_paths[idx]}): {len(dev)} corners, oracle {len(want)}")
        gk, gd = ctx.features(s)
        assert len(gk) == len(rk)
        for f in ox.KEYPOINT.names:
            assert np.array_equal(gk[f], rk[f]), (name, s, f)
        assert np.array_equal(gd, rd)
    ctx.close()
