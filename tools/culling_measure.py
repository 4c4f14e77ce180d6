"""Times LocalMapping's culling on the device covisibility graph
(orbx_covis_cull_keyframes, orbx_covis_cull_points in orbx_covis.hip) on the
GPU and writes one JSON file.

The map: 500 keyframes with rows of 2400 entries (2000 points, one index in
six empty); keyframe k draws its points from the 5000 consecutive ids from
125 k on, so that the middle keyframe's ordered list holds about 80
keyframes.  Octaves are drawn in 0..7, every fourth keyframe's in 5..7.  All
keyframes are added, given their octaves, and updated in id order.

  cull_keyframes_kept    one orbx_covis_cull_keyframes of the middle keyframe
                         with every candidate in `keep`: the whole call, no
                         cull, so the state stays and the call repeats.
  cull_keyframes_walked  the same call without `keep` and with cand_cap = 0:
                         the walk culls as it would (the counts come back),
                         the commit is withheld (ORBX_ERR_CAPACITY), so the
                         state stays as well.  It lacks the commit kernels'
                         work and the shadow's update.
  cull_keyframes_once    one committed call on the fresh map (a single wall
                         time: it changes the map).
  cull_points            one orbx_covis_cull_points over 2000 recent points
                         that all stay (found = visible, one keyframe old).
  mirror                 --mirror: what a caller with a host copy pays per
                         cull without the feature: orbx_covis_erase_keyframe
                         plus orbx_covis_erase_points of 30 of its points, for
                         40 keyframes one after the other (five before them
                         warm the calls up).  Only calls of ABI
                         14, so that it runs on the commit before the culling
                         (--tree PATH picks the package to import).

Every entry: the median, minimum, 90th percentile and maximum of the wall time
over --reps calls after warm-up, and the kernel timer of the call measured in
a pass of its own.

usage: python tools/culling_measure.py OUT.json [--reps 40] [--members 500] [--mirror] [--tree PATH]
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
args = sys.argv[1:]
tree = Path(args[args.index("--tree") + 1]).resolve() if "--tree" in args else ROOT
sys.path.insert(0, str(tree))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam_amd as ox  # noqa: E402
import covis_cases as cc  # noqa: E402

out_path = Path(args[0])
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 40
members = int(args[args.index("--members") + 1]) if "--members" in args else 500
DRAW, WINDOW, STEP = 2000, 5000, 125


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), p90_ms=float(ms[int(0.9 * (len(ms) - 1))]),
                max_ms=float(ms[-1]), n=len(ms))


def measure(ctx, call, timer):
    for _ in range(5):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.timing(True, only=timer)
    n0 = ctx.kernel_time(timer)[0]
    for _ in range(reps):
        call()
    k, avg, _ = ctx.kernel_time(timer)
    ctx.timing(False)
    return {"wall": stats(wall), timer + "_timer": dict(regions=int(k - n0), avg_ms=float(avg))}


rng = np.random.default_rng(members)
rows = cc.window_rows(rng, members, draw=DRAW, window=WINDOW, step=STEP)
keys = cc.rand_keys(rng, members)
octs = [rng.integers(5, 8, len(r)) if k % 4 == 1 else rng.integers(0, 8, len(r)) for k, r in enumerate(rows)]
n_points = STEP * members + WINDOW
res = {"parameters": dict(members=members, draw=DRAW, window=WINDOW, step=STEP, row=len(rows[0]), reps=reps,
                          package=str(Path(ox.__file__).resolve().parent), abi=int(ox.lib().orbx_abi_version()))}
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)


def fresh_map(with_octaves):
    m = ox.CovisibilityMap(ctx, members, n_points, len(rows[0]))
    for i in range(members):
        m.add_keyframe(i, keys[i], rows[i])
        if with_octaves:
            m.set_octaves(i, octs[i])
    for i0 in range(0, members, 256):
        m.update_connections(np.arange(i0, min(i0 + 256, members)))
    return m


mid = members // 2
if "--mirror" in args:
    m = fresh_map(False)
    wall = []
    victims = [k for k in range(members) if k % 4 == 1][5:50]
    for n, k in enumerate(victims):           # the first five warm the two calls up
        pts = rows[k][rows[k] >= 0][:30]
        t0 = time.perf_counter()
        m.erase_keyframe(k)
        m.erase_points(pts)
        ctx.sync()
        if n >= 5:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["mirror"] = dict(erase_keyframe_plus_erase_points_30=stats(wall))
    m.close()
else:
    m = fresh_map(True)
    cand = m.connections(mid)[0]
    last = {}

    def kept():
        last["kept"] = m.cull_keyframes(mid, keep=cand)

    def walked():
        last["walked"] = m.cull_keyframes(mid, cand_cap=0)

    recent = np.unique(np.concatenate([rows[mid], rows[mid - 1]]))
    recent = recent[recent >= 0][:2000]
    ones = np.ones(len(recent), np.int32)

    def points():
        last["points"] = m.cull_points(mid, recent, ones, ones, ones * (mid - 1))

    e = dict(cull_keyframes_kept=measure(ctx, kept, "covis_cull_kf"))
    r = last["kept"]
    e["cull_keyframes_kept"].update(n_cand=int(r["n_cand"]), decisions={str(d): int((r["decision"] == d).sum())
                                                                       for d in (-1, 0, 1, 2)})
    e["cull_keyframes_walked"] = measure(ctx, walked, "covis_cull_kf")
    r = last["walked"]
    e["cull_keyframes_walked"].update(code=int(r["code"]), n_cand=int(r["n_cand"]), n_done=int(r["n_done"]),
                                      n_bad=int(r["n_bad"]))
    e["cull_points"] = measure(ctx, points, "covis_cull_mp")
    e["cull_points"].update(n=int(len(recent)), kept=int((last["points"] == 0).sum()))
    t0 = time.perf_counter()
    r = m.cull_keyframes(mid)
    e["cull_keyframes_once"] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, n_cand=int(r["n_cand"]),
                                    decisions={str(d): int((r["decision"] == d).sum()) for d in (-1, 0, 1, 2)},
                                    n_bad=int(r["n_bad"]), members_after=len(m))
    res["culling"] = e
    m.close()
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res))
print("written", out_path)
