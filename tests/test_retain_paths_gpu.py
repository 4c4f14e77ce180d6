"""Every path of retainBest on the device (k_retain_cells, k_retain_levels
and the introselect replay under them, wave_nth_element): rounds that partition in
memory (ranges of more than 64 entries), the hand-off into registers, the
register rounds, the final insertion sort, the heap_select fallback, for u32
(FAST score) and u64 (Harris key) entries in both pivot eras; then whole
extractions that put the two kernels through each of their cell and level
branches.  All comparisons are exact.

The lists are picked on the CPU with a Python restatement of libstdc++'s
introselect (below) that records every round; the restatement itself is held
to the oracle's (orbx_ref_nth_element_perm), and the chosen cases are asserted
to cover each situation, so a case that stops covering one fails here and is
not skipped silently.

Depth exhaustion: ascending responses under the GCC 4.8 pivot run out of
depth while the range is still longer than 64 (the memory phase) at n = 200
and 512, and inside the register phase at n = 128 and 129; the organ-pipe
lists reach it in the register phase under both pivots.  Both fallbacks are
covered.
"""
import ctypes
import functools

import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor, load, ptr

REG = 64   # ranges of at most this many entries are held in registers


def debug_lib():
    """The library with the two diagnostic entries' signatures set."""
    L = ox.lib()
    vp, i = ctypes.c_void_p, ctypes.c_int
    for fn in (L.orbx_debug_nth_pivot, L.orbx_debug_nth64):
        fn.argtypes, fn.restype = [vp, i, i, i, vp, vp], i
    return L


# ---------------------------------------------------------------------------
# libstdc++ introselect with the comparator "response greater", restated
# ---------------------------------------------------------------------------
def _heap_push(a, base, hole, top, value, key):
    parent = (hole - 1) // 2
    while hole > top and key[a[base + parent]] > key[value]:
        a[base + hole] = a[base + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[base + hole] = value


def _heap_adjust(a, base, hole, length, value, key):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if key[a[base + second]] > key[a[base + second - 1]]:
            second -= 1
        a[base + hole] = a[base + second]
        hole = second
    if length % 2 == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        a[base + hole] = a[base + second - 1]
        hole = second - 1
    _heap_push(a, base, hole, top, value, key)


def _heap_select(a, base, middle, last, key):
    if middle >= 2:
        parent = (middle - 2) // 2
        while True:
            _heap_adjust(a, base, parent, middle, a[base + parent], key)
            if parent == 0:
                break
            parent -= 1
    for i in range(middle, last):
        if key[a[base + i]] > key[a[base]]:
            value = a[base + i]
            a[base + i] = a[base]
            _heap_adjust(a, base, 0, middle, value, key)


def introselect(keys, nth, mode):
    """std::nth_element(first, first + nth, last, greater) on indices
    0..n-1 with the given keys.  mode 0: libstdc++ >= 4.9's pivot, 1: GCC
    4.6..4.8's.  Returns (permutation, rounds, info): rounds = [(first, last,
    m, cut, depth before the round)], m the number of swaps of the round's
    unguarded partition; info = dict(heap=(first, last) or None, final=length
    of the range left to the insertion sort or None)."""
    key = [int(k) for k in keys]
    n = len(key)
    a = list(range(n))
    rounds = []
    info = dict(heap=None, final=None)
    if n == 0 or nth == n:
        return a, rounds, info
    first, last = 0, n
    depth = 2 * (n.bit_length() - 1)
    while last - first > 3:
        if depth == 0:
            info["heap"] = (first, last)
            _heap_select(a, first, nth + 1 - first, last - first, key)
            a[first], a[nth] = a[nth], a[first]
            return a, rounds, info
        d0 = depth
        depth -= 1
        mid = first + (last - first) // 2
        x, y, z = (first if mode == 1 else first + 1), mid, last - 1
        kx, ky, kz = key[a[x]], key[a[y]], key[a[z]]
        if kx > ky:
            t = y if ky > kz else (z if kx > kz else x)
        else:
            t = x if kx > kz else (z if ky > kz else y)
        a[first], a[t] = a[t], a[first]
        p = key[a[first]]
        i, j, m = first + 1, last, 0
        while True:
            while key[a[i]] > p:
                i += 1
            j -= 1
            while p > key[a[j]]:
                j -= 1
            if not i < j:
                break
            a[i], a[j] = a[j], a[i]
            m += 1
            i += 1
        cut = i
        rounds.append((first, last, m, cut, d0))
        if cut <= nth:
            first = cut
        else:
            last = cut
    info["final"] = last - first
    for i in range(first + 1, last):
        val = a[i]
        k = i
        while k > first and key[val] > key[a[k - 1]]:
            a[k] = a[k - 1]
            k -= 1
        a[k] = val
    return a, rounds, info


def situations(n, nth, rounds, info):
    """Names of the situations (WANTED below) that this run meets."""
    s = set()
    if n == 0 or nth == n:
        s.add("final0")   # nothing to select: the list stays as it is
    handoff = next(((f, l) for f, l, *_ in rounds if l - f <= REG), None)
    if n > REG and handoff:
        f, l = handoff
        if l - f == 64:
            s.add("handoff64")
        if f > 0:
            s.add("handoff_first>0")
        if l < n:
            s.add("handoff_last<n")
    if n == 65 and rounds and rounds[0][1] - rounds[0][0] == 65:
        s.add("range65")   # one memory round on 65 entries, then the hand-off
    for f, l, m, cut, _ in rounds:
        if l - f <= REG:
            if m == 0:
                s.add("reg_m0")
            if cut == nth:
                s.add("reg_cut==nth")
    if info["final"] is not None:
        s.add(f"final{info['final']}")
    if info["heap"]:
        f, l = info["heap"]
        s.add("heap_reg" if l - f <= REG else "heap_mem")
    return s


def m3killer(n, mode):
    """A median-of-three killer for the era's pivot choice, as response
    ranks (descending order is the comparator's 'sorted')."""
    k = np.zeros(n, np.int64)
    h = n // 2
    for i in range(h):
        k[2 * i] = i + 1
        k[2 * i + 1] = h + i + 1
    if n % 2:
        k[n - 1] = n
    return k


def key_lists():
    r = np.random.default_rng(11)
    out = []
    for n in (4, 63, 64, 65, 66, 127, 128, 129, 200, 512):
        out += [("scores", r.integers(7, 60, n)), ("equal", np.full(n, 20)), ("binary", r.integers(0, 2, n)),
                ("wide", r.integers(0, 256, n)), ("ascending", np.arange(n) * 255 // max(n - 1, 1)),
                ("descending", (n - 1 - np.arange(n)) * 255 // max(n - 1, 1)),
                ("organ", np.minimum(np.arange(n), n - 1 - np.arange(n)) % 256),
                ("killer", m3killer(n, 0) * 255 // n), ("rkiller", (n + 1 - m3killer(n, 0)) * 255 // n)]
    return out


def nths(n):
    """Small, middle and last positions, and n itself: introselect keeps nth inside
    [first, last), so its final range is never empty; the 0-entry case is
    nth == n, where nth_element returns at once."""
    return sorted({v for v in (1, 2, 3, 8, n // 2, n - 2, n - 1) if 0 < v < n}) + [n]


WANTED = {"handoff64", "range65", "handoff_first>0", "handoff_last<n", "reg_m0", "reg_cut==nth", "final0", "final1",
          "final2", "final3", "heap_reg", "heap_mem"}


@functools.lru_cache(maxsize=None)
def u32_cases():
    """(kind, keys, nth, mode, situations) for every list, nth and era."""
    cases = []
    for kind, keys in key_lists():
        for nth in nths(len(keys)):
            for mode in (0, 1):
                _, rounds, info = introselect(keys, nth, mode)
                cases.append((kind, keys, nth, mode, situations(len(keys), nth, rounds, info)))
    return cases


def test_cases_cover_every_situation():
    seen = set()
    kinds = set()
    for kind, keys, nth, mode, sit in u32_cases():
        seen |= sit
        kinds.add(kind)
    assert WANTED <= seen, sorted(WANTED - seen)
    assert {"equal", "binary"} <= kinds


def test_restatement_matches_oracle():
    R = load()
    for kind, keys, nth, mode, _ in u32_cases():
        n = len(keys)
        perm, _, _ = introselect(keys, nth, mode)
        want = np.zeros(n, np.int32)
        resp = np.asarray(keys, np.float32)
        assert R.orbx_ref_nth_element_perm(ptr(resp), n, nth, mode, 0, ptr(want)) == 0
        assert np.array_equal(np.asarray(perm, np.int32), want), (kind, n, nth, mode)


@pytest.mark.gpu
def test_replay_u32():
    """LDS and global replays, whole permutation, against the oracle."""
    L, R = debug_lib(), load()
    for kind, keys, nth, mode, _ in u32_cases():
        n = len(keys)
        entries = ((np.asarray(keys).astype(np.uint32) & 0xFF) << 24 | np.arange(n, dtype=np.uint32)).astype(np.uint32)
        glb = np.zeros(n, np.uint32)
        lds = np.zeros(n, np.uint32)
        assert L.orbx_debug_nth_pivot(entries.ctypes.data, n, nth, mode, glb.ctypes.data, lds.ctypes.data) == 0
        want = np.zeros(n, np.int32)
        resp = (entries >> 24).astype(np.float32)
        assert R.orbx_ref_nth_element_perm(ptr(resp), n, nth, mode, 0, ptr(want)) == 0
        assert np.array_equal(lds & 0xFFFFFF, want), (kind, n, nth, mode)
        assert np.array_equal(glb, lds), (kind, n, nth, mode)
        assert np.array_equal(lds >> 24, entries[want] >> 24), (kind, n, nth, mode)


# ---------------------------------------------------------------------------
# u64 entries: Harris keys
# ---------------------------------------------------------------------------
def harris_key(r):
    u = (np.asarray(r, np.float32) + np.float32(0)).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def responses_of(keys):
    """The u32 case's keys as float responses: negative and positive values
    with the same ties, the middle key as zeros of both signs."""
    k = np.asarray(keys, np.int64)
    mid = int(np.sort(k)[len(k) // 2])
    r = ((k - mid).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    zeros = np.flatnonzero(k == mid)
    r[zeros[::2]] = np.float32(-0.0)
    return r


@functools.lru_cache(maxsize=None)
def u64_cases():
    out = []
    for kind, keys, nth, mode, sit in u32_cases():
        if len(keys) in (64, 65, 200):
            out.append((kind, responses_of(keys), nth, mode, sit))
    return out


def test_u64_cases_keep_the_situations():
    """The float responses order exactly as the u32 keys they come from, so
    the rounds, and the situations met, are those of the u32 case."""
    seen, signs = set(), set()
    for kind, resp, nth, mode, sit in u64_cases():
        n = len(resp)
        _, rounds, info = introselect(harris_key(resp), nth, mode)
        assert situations(n, nth, rounds, info) == sit, (kind, n, nth, mode)
        seen |= sit
        signs |= {"neg"} if (resp < 0).any() else set()
        signs |= {"-0"} if (np.signbit(resp) & (resp == 0)).any() else set()
        signs |= {"+0"} if (~np.signbit(resp) & (resp == 0)).any() else set()
        signs |= {"ties"} if len(np.unique(resp)) < n else set()
    assert WANTED - {"range65"} <= seen | {"range65"} and {"neg", "-0", "+0", "ties"} <= signs
    assert {"handoff64", "handoff_first>0", "handoff_last<n", "reg_m0", "reg_cut==nth", "final0", "final1", "final2",
            "final3", "heap_reg", "heap_mem"} <= seen, sorted(seen)


@pytest.mark.gpu
def test_replay_u64():
    L, R = debug_lib(), load()
    for kind, resp, nth, mode, _ in u64_cases():
        n = len(resp)
        glb = np.zeros(n, np.uint64)
        lds = np.zeros(n, np.uint64)
        assert L.orbx_debug_nth64(resp.ctypes.data, n, nth, mode, glb.ctypes.data, lds.ctypes.data) == 0
        want = np.zeros(n, np.int32)
        assert R.orbx_ref_nth_element_perm(ptr(resp), n, nth, mode, 0, ptr(want)) == 0
        assert np.array_equal((lds & np.uint64(0xFFFFFFFF)).astype(np.int32), want), (kind, n, nth, mode)
        assert np.array_equal((lds >> np.uint64(32)).astype(np.uint32), harris_key(resp)[want]), (kind, n, nth, mode)
        assert np.array_equal(glb, lds), (kind, n, nth, mode)


# ---------------------------------------------------------------------------
# The retain kernels: whole extractions
# ---------------------------------------------------------------------------
from test_fast_paths_gpu import cells_of, expected_cell   # noqa: E402

W = 4   # cell waves per workgroup of k_retain_cells (cwaves)

# name, w, h, nfeatures, fastTh, score type (0 Harris, 1 FAST), slots, image kind, single-frame context
SCENES = [
    ("noise-96x80-n100", 96, 80, 100, 7, 1, 1, "noise", False),
    ("texture-320x240-n500-batch3", 320, 240, 500, 20, 1, 3, "texture", False),
    ("texture-200x150-n300-batch9", 200, 150, 300, 20, 1, 9, "texture", False),
    ("texture-320x240-n500-harris", 320, 240, 500, 20, 0, 1, "texture", False),
    ("noise-160x120-n200-harris-batch9", 160, 120, 200, 7, 0, 9, "noise", False),
    ("texture-250x187-n400-single", 250, 187, 400, 20, 1, 1, "texture", True),
    ("sparse-320x240-n500", 320, 240, 500, 20, 1, 1, "sparse", False),
    ("graded-320x240-n500", 320, 240, 500, 20, 1, 1, "graded", False),
]


def scene_frames(kind, w, h, slots, seed):
    if kind == "texture":
        return np.stack([synth.texture_frame(w, h, seed + s) for s in range(slots)])
    if kind == "noise":
        return np.stack([synth.noise_frame(w, h, seed + s) for s in range(slots)])
    if kind == "graded":   # contrast fading to nothing from left to right: cells from rich to empty
        alpha = np.linspace(1.0, 0.0, w, dtype=np.float32)[None, :] ** 2
        return np.stack([(120 + (synth.texture_frame(w, h, seed + s).astype(np.float32) - 120) * alpha).astype(np.uint8)
                         for s in range(slots)])
    assert kind == "sparse"   # texture in the left third only: most cells are empty, the rest are rich
    f = np.stack([synth.flat_frame(w, h, 120) for _ in range(slots)])
    for s in range(slots):
        f[s][:, :w // 3] = synth.texture_frame(w, h, seed + s)[:, :w // 3]
    return f


def quota(tot, valid, nfc):
    """The redistribution of src/ORBextractor.cc:622-670 as level_quota runs
    it: per-cell quota and the number of passes of its while loop."""
    n = len(tot)
    ret, nomore = [0] * n, [False] * n
    to_dist = n_nomore = 0
    for c in range(n):
        if valid[c]:
            if tot[c] > nfc:
                ret[c] = nfc
            else:
                ret[c] = tot[c]
                to_dist += nfc - tot[c]
                nomore[c] = True
                n_nomore += 1
    passes = 0
    while to_dist > 0 and n_nomore < n:
        passes += 1
        n_new = nfc + int(np.ceil(np.float32(to_dist) / np.float32(n - n_nomore)))
        to_dist = 0
        for c in range(n):
            if not nomore[c]:
                if tot[c] > n_new:
                    ret[c] = n_new
                else:
                    ret[c] = tot[c]
                    to_dist += n_new - tot[c]
                    nomore[c] = True
                    n_nomore += 1
    return ret, passes


@functools.lru_cache(maxsize=None)
def scene(name):
    """Frames, oracle results and the situations each (level, slot) meets."""
    _, w, h, nf, th, score, slots, kind, single = next(s for s in SCENES if s[0] == name)
    frames = scene_frames(kind, w, h, slots, seed=w + nf)
    cells = cells_of(w, h, nf, 1.2, 8)
    ref = RefExtractor(nf, fast_th=th, score_type=score)
    fpl = [int(v) for v in ref.features_per_level()]
    want, sit = [], set()
    for s in range(slots):
        want.append(ref(frames[s]))
        levels = [ref.level(lvl) for lvl in range(8)]
        for lvl in range(8):
            cl = [c for c in cells if c["level"] == lvl]
            tot = [len(expected_cell(levels[lvl], c, th)) for c in cl]
            valid = [c["valid"] for c in cl]
            nfc = int(np.ceil(np.float32(fpl[lvl]) / np.float32(len(cl))))
            keep, passes = quota(tot, valid, nfc)
            total = sum(min(t, k) for t, k in zip(tot, keep))
            sit.add("cells<W" if len(cl) < W else "cells>2W" if len(cl) > 2 * W else "cells>=W")
            sit |= {"n=0" for t in tot if t == 0}
            sit |= {"0<n<=k" for t, k in zip(tot, keep) if 0 < t <= k}
            sit |= {"n>k" for t, k in zip(tot, keep) if t > k > 0}
            sit |= {"n>k, n<=64" for t, k in zip(tot, keep) if 64 >= t > k > 0}
            sit |= {"n>k, n>64" for t, k in zip(tot, keep) if t > 64 and t > k > 0}
            sit.add("level replay" if total > fpl[lvl] else "no level replay")
            if passes > 1:
                sit.add("quota passes>1")
            if not all(valid):
                sit.add("invalid cells")
    return frames, want, sit


SCENE_WANTED = {"cells<W", "cells>2W", "n=0", "0<n<=k", "n>k", "n>k, n<=64", "n>k, n>64",
                "level replay", "no level replay", "quota passes>1", "invalid cells"}


def test_scenes_cover_every_situation():
    """Levels of fewer cells than a workgroup has waves and of more than
    twice as many (a workgroup's four cells then span two levels, or lie
    inside one), every cell branch, both level branches, a quota that
    redistributes more than once, invalid cells, a 3-slot and two 9-slot
    batches, Harris scores, the single-frame call."""
    seen = set()
    for sc in SCENES:
        seen |= scene(sc[0])[2]
    assert SCENE_WANTED <= seen, sorted(SCENE_WANTED - seen)
    assert any(sc[6] == 3 for sc in SCENES) and any(sc[5] == 0 for sc in SCENES) and any(sc[8] for sc in SCENES)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["gcc49", "gcc48"])
@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_extraction_matches_oracle(name, mode):
    _, w, h, nf, th, score, slots, kind, single = next(s for s in SCENES if s[0] == name)
    frames, want, _ = scene(name)
    if mode != 1:   # scene() holds the default era's (GCC 4.8)
        ref = RefExtractor(nf, fast_th=th, score_type=score, nth_pivot=mode)
        want = [ref(f) for f in frames]
    ctx = ox.Context(nfeatures=nf, score_type=score, fast_th=th, max_w=w, max_h=h, slots=slots)
    ctx.set_nth_pivot(mode)
    if not single:
        ctx.upload(frames)
        ctx.extract(0, slots)
        ctx.sync()
    for s in range(slots):
        gk, gd = ctx(frames[s]) if single else ctx.features(s)   # single: orbx_extract, one host image per call
        rk, rd = want[s]
        assert len(gk) == len(rk) and len(gk) > 0, (name, s)
        for f in ox.KEYPOINT.names:
            assert np.array_equal(gk[f], rk[f]), (name, s, f)
        assert np.array_equal(gd, rd), (name, s)
    ctx.close()
