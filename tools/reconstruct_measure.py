"""Times the end of map initialisation on the device (orbx_reconstruct.hip) on
the GPU and writes one JSON file:

  host   orbx_init_reconstruct as one call (upload, three launches, read-back)
         on the 300-match cloud (ReconstructF) and plane (ReconstructH) of
         tests/reconstruct_numpy.py, the two alternating
  dev    orbx_dev_init_reconstruct over the pairs of `--slots` device-resident
         frames at bench c2's shape (640x480, 1000 keypoints, one sequence),
         after extraction + SearchForInitialization and orbx_dev_init_models:
         the "reconstruct" kernel timer and the wall time to the
         synchronisation, with the models' own choice and with ReconstructF
         forced on every pair (rh_threshold above 1)

usage: python tools/reconstruct_measure.py OUT.json [--slots 1024] [--reps 30]
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam_amd as ox  # noqa: E402
import reconstruct_numpy as rn  # noqa: E402
from orb_slam_amd import synth  # noqa: E402

args = sys.argv[1:]
out_path = Path(args[0])
slots = int(args[args.index("--slots") + 1]) if "--slots" in args else 1024
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 30


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), p90_ms=float(ms[int(0.9 * (len(ms) - 1))]))


res = {}
# --- host form ---------------------------------------------------------------
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
qs = {name: ox.reconstruct_query(*rn.case(name)[0][:7]) for name in ("F-300", "H-300")}
L = ox.lib()
import ctypes  # noqa: E402
for _ in range(5):
    for q, keep in qs.values():
        assert L.orbx_init_reconstruct(ctx.handle, ctypes.byref(q)) == 0
t = {name: [] for name in qs}
for _ in range(reps):
    for name, (q, keep) in qs.items():
        t0 = time.perf_counter()
        L.orbx_init_reconstruct(ctx.handle, ctypes.byref(q))
        t[name].append((time.perf_counter() - t0) * 1e3)
res["host"] = {name: dict(stats(t[name]), ok=int(qs[name][0].ok), n_hyp=int(qs[name][0].n_hyp)) for name in qs}
ctx.close()

# --- device-resident form ------------------------------------------------------
w, h, nf, M = 640, 480, 1000, 200
frames = synth.sequence(w, h, slots, seed=2000)
ctx = ox.Context(nfeatures=nf, max_w=w, max_h=h, slots=slots)
ctx.upload(frames, first=0)
ctx.extract_match(0, slots, slots, mode="init", window=100, nnratio=0.9, check_ori=True)
draws = np.random.RandomState(5).randint(0, 2**31, size=(slots, M, 8), dtype=np.int64).astype(np.int32)
ctx.dev_init_models(0, slots, slots, draws, max_iter=M)
ctx.sync()
cam = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
res["dev"] = dict(slots=slots, pairs=slots - 1)
for tag, thr in (("as_chosen", 0.40), ("forced_F", 2.0)):
    for _ in range(3):
        ctx.dev_init_reconstruct(0, slots, slots, cam, rh_threshold=thr)
    ctx.sync()
    ctx.timing(True, only="reconstruct")
    wall = []
    for _ in range(max(reps // 3, 5)):
        t0 = time.perf_counter()
        ctx.dev_init_reconstruct(0, slots, slots, cam, rh_threshold=thr)
        ctx.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    n, avg, tot = ctx.kernel_time("reconstruct")
    ctx.timing(False)
    sample = [ctx.read_init_reconstruct(s) for s in range(1, min(slots, 33))]
    ninl = [r["n_inliers"] for r in sample]
    good = [int(r["n_good"].max()) for r in sample]
    res["dev"][tag] = dict(wall=stats(wall), timer_regions=int(n), timer_avg_ms=float(avg), sampled_pairs=len(sample),
                           model_h=sum(r["model"] == 0 for r in sample), model_f=sum(r["model"] == 1 for r in sample),
                           ok=sum(r["ok"] for r in sample), n_inliers=[min(ninl), max(ninl)],
                           max_good=[min(good), max(good)])
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res, indent=1))
