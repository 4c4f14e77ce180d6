"""Trip counts of retainBest on the c2 sequence, per frame, from the CPU:
the oracle's FAST on every cell (the lists k_retain_cells receives), the
level quota, and libstdc++'s introselect restated in Python
(tests/test_retain_paths_gpu.py) on each cell list and each level list.

Reports cells by list length against the quota and the 64-entry register
window, introselect rounds by the length of the range they partition, the
quota's redistribution passes, and the level lists that are replayed.

usage: python tools/retain_rounds.py [frames (8)] [W H nfeatures (640 480 1000)] [pivot mode (1)]
"""
import sys
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from orb_slam_amd import synth  # noqa: E402
from oracle_lib import RefExtractor  # noqa: E402
from test_fast_paths_gpu import cells_of, expected_cell  # noqa: E402
from test_retain_paths_gpu import introselect, quota  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
frames_n = a[0] if a else 8
w, h, nf = a[1:4] if len(a) >= 4 else (640, 480, 1000)
mode = a[4] if len(a) >= 5 else 1
frames = synth.sequence(w, h, frames_n, seed=2000)
cells = cells_of(w, h, nf, 1.2, 8)
ref = RefExtractor(nf)
fpl = [int(v) for v in ref.features_per_level()]
c = Counter()


def bucket(n):
    return ">128" if n > 128 else "65-128" if n > 64 else "33-64" if n > 32 else "<=32"


def replay(keys, nth, what):
    _, rounds, info = introselect(keys, nth, mode)
    for f, l, *_ in rounds:
        c[f"{what} rounds on {bucket(l - f)}"] += 1
    c[f"{what} rounds"] += len(rounds)
    if info["heap"]:
        c[f"{what} heap fallbacks"] += 1
    if rounds and rounds[0][1] - rounds[0][0] > 64:
        c[f"{what} lists that hand off to registers"] += any(l - f <= 64 for f, l, *_ in rounds) or info["final"] is not None


for fr in frames:
    ref(fr)
    levels = [ref.level(lvl) for lvl in range(8)]
    for lvl in range(8):
        cl = [x for x in cells if x["level"] == lvl]
        lists = [expected_cell(levels[lvl], x, 20) for x in cl]
        tot = [len(x) for x in lists]
        nfc = int(np.ceil(np.float32(fpl[lvl]) / np.float32(len(cl))))
        keep, passes = quota(tot, [x["valid"] for x in cl], nfc)
        c["quota passes"] += passes
        c["cells"] += len(cl)
        level_keys = []
        for e, n, k in zip(lists, tot, keep):
            c["corners"] += n
            if n == 0 or k == 0:
                c["cells with n = 0 or k = 0"] += 1
                continue
            keys = e[:, 2]
            if n <= k:
                c["cells with n <= k (copy)"] += 1
                level_keys += list(keys)
                continue
            c["cells with k < n <= 64" if n <= 64 else "cells with 64 < n <= 512" if n <= 512 else "cells with n > 512"] += 1
            c["quota sum over replayed cells"] += k
            perm, _, _ = introselect(keys, k, mode)
            replay(keys, k, "cell")
            level_keys += [keys[i] for i in perm[:k]]
        if len(level_keys) > fpl[lvl]:
            c["levels replayed"] += 1
            c["level entries replayed"] += len(level_keys)
            replay(level_keys, fpl[lvl], "level")
print(f"# {frames_n} frames {w}x{h}, {nf} keypoints, pivot mode {mode}; per frame")
for k in sorted(c):
    print(f"{k:45s} {c[k] / frames_n:10.2f}")
