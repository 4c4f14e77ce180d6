"""Times the Sim3 solver on the device (orbx_sim3.hip) on the GPU and writes
one JSON file:

  host    orbx_sim3_ransac as one call (upload, three launches, read-back):
          N = 100 correspondences, 300 iterations
  batch   orbx_sim3_ransac_batch over 8 such candidates
  dev     orbx_dev_sim3_candidates: the keyframe of one device-resident slot
          (640x480, 1000 keypoints) against 8 others -- SearchByBoW and the
          solver behind it, one synchronisation; beside it the search alone
          (orbx_dev_search_by_bow_kf), so that the solver's share is the
          difference
  numpy   the restatement of tests/sim3_numpy.py on the host case, for
          orientation only

Every entry: the median, minimum and 90th percentile of the wall time to the
synchronisation over --reps calls after warm-up, and the "sim3" kernel timer
(the three kernels of a call) and each kernel's own timer, measured in passes
of their own (the timers' events cost wall time).

usage: python tools/sim3_measure.py OUT.json [--reps 30]
"""
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam_amd as ox  # noqa: E402
import sim3_numpy as s3  # noqa: E402
from orb_slam_amd import synth  # noqa: E402

args = sys.argv[1:]
out_path = Path(args[0])
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 30
M = 300


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), p90_ms=float(ms[int(0.9 * (len(ms) - 1))]),
                max_ms=float(ms[-1]), n=len(ms))


def measure(ctx, call):
    for _ in range(5):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    out = dict(wall=stats(wall))
    for name in ("sim3", "sim3.prepare", "sim3.solve", "sim3.check"):   # a pass each: one pair of events per call
        ctx.timing(True, only=name)
        for _ in range(reps):
            call()
        n, avg, tot = ctx.kernel_time(name)
        ctx.timing(False)
        out[name.replace(".", "_") + "_timer"] = dict(regions=int(n), avg_ms=float(avg))
    return out


res = {"iterations": M}
L = ox.lib()
# --- host arrays ---------------------------------------------------------------
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
scenes = [s3.scene(500 + k, 100) for k in range(8)]
built = [ox.sim3_query(kf1, kf2, m, s3.make_draws(600 + k, M), idx1=idx1) for k, (kf1, kf2, m, idx1) in enumerate(scenes)]
q0 = built[0][0]
res["host"] = measure(ctx, lambda: L.orbx_sim3_ransac(ctx.handle, ctypes.byref(q0)))
res["host"].update(N=int(q0.N), found_iter=int(q0.found_iter), n_inliers=int(q0.n_inliers))
arr = (ox.Sim3Query * 8)(*[b[0] for b in built])
res["batch8"] = measure(ctx, lambda: L.orbx_sim3_ransac_batch(ctx.handle, 8, arr))
res["batch8"].update(N=[int(arr[k].N) for k in range(8)])
kf1, kf2, m, idx1 = scenes[0]
d0 = s3.make_draws(600, M)
t = []
for _ in range(5):
    t0 = time.perf_counter()
    s3.sim3_ransac(kf1, kf2, m, d0, idx1=idx1)
    t.append((time.perf_counter() - t0) * 1e3)
res["numpy_restatement_host_case"] = stats(t)
ctx.close()

# --- device-resident frames -------------------------------------------------------
from vocab_data import make_vocab  # noqa: E402
w, h, nf, ncand = 640, 480, 1000, 8
ctx = ox.Context(nfeatures=nf, max_w=w, max_h=h, slots=ncand + 1)
ctx.upload(np.stack(synth.sequence(w, h, ncand + 1, seed=2100)), 0)
ctx.extract(0, ncand + 1)
ctx.sync()
V = make_vocab(k=10, L=4, seed=3)
voc = ox.Vocabulary(ctx, V["k"], V["L"], V["parent"], V["is_leaf"], V["desc"], V["weight"])
ctx.compute_bow(voc, 0, ncand + 1, 2)
cam = np.array([520.0, 520.0, 320.0, 240.0], np.float32)
rng = np.random.default_rng(1)
kfs = []
for s in range(ncand + 1):
    keys = ctx.features(s)[0]
    n = len(keys)
    depth = rng.uniform(3.0, 8.0, n)
    pos = np.stack([(keys["x"] - cam[2]) / cam[0] * depth, (keys["y"] - cam[3]) / cam[1] * depth, depth], 1)
    kfs.append(dict(mp=np.ones(n, np.uint8), pos=pos.astype(np.float32), Tcw=np.eye(4, dtype=np.float32), cam=cam,
                    sigma2=s3.SIGMA2))
slots2 = list(range(1, ncand + 1))
draws = np.stack([s3.make_draws(700 + k, M) for k in range(ncand)])
last = {}


def dev_call():
    last["r"] = ctx.dev_sim3_candidates(0, kfs[0], slots2, [kfs[s] for s in slots2], draws, min_inliers=20)


res["dev8"] = measure(ctx, dev_call)
r = last["r"]
res["dev8"].update(n_matches=r["n_matches"].tolist(), N=[x["N"] for x in r["results"]],
                   discarded=r["discarded"].tolist())
mps = [k["mp"] for k in kfs]
outs = [np.zeros(nf, np.int32) for _ in slots2]
ptrs = (ctypes.c_void_p * ncand)(*[o.ctypes.data for o in outs])
mpp = (ctypes.c_void_p * ncand)(*[mps[s].ctypes.data for s in slots2])
s2 = np.ascontiguousarray(slots2, np.int32)
nm = np.zeros(ncand, np.int32)


def search_call():
    assert L.orbx_dev_search_by_bow_kf(ctx.handle, 0, ox._ptr(mps[0]), ncand, ox._ptr(s2), mpp, 0.75, 1, ptrs, nf,
                                       ox._ptr(nm)) == 0


for _ in range(5):
    search_call()
t = []
for _ in range(reps):
    t0 = time.perf_counter()
    search_call()
    t.append((time.perf_counter() - t0) * 1e3)
res["dev8_search_alone"] = dict(wall=stats(t))
voc.close()
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res, indent=1))
