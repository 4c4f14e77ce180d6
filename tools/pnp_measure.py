"""Times the PnP solver on the device (orbx_pnp.hip) on the GPU and writes one
JSON file:

  host    orbx_pnp_ransac as one call (upload, five launches, read-back): N =
          100 correspondences, Relocalisation's parameters, a fresh solver's
          iterate(5) (which can run 35 iterations)
  batch   orbx_pnp_ransac_batch over 8 such candidates
  dev     orbx_dev_pnp_candidates: the frame of one device-resident slot
          (640x480, 1000 keypoints) against 8 keyframe views -- SearchByBoW
          and the solver behind it, one synchronisation; beside it the search
          alone (orbx_dev_search_by_bow), so that the solver's share is the
          difference
  numpy   the restatement of tests/pnp_numpy.py on the host case on one core:
          the number to beat

Every entry: the median, minimum and 90th percentile of the wall time to the
synchronisation over --reps calls after warm-up, and the "pnp" kernel timer
(the kernels of a call) and each part's own timer, measured in passes of
their own (the timers' events cost wall time).  "kernels" holds the compiler's
register, scratch, LDS and occupancy figures of the five kernels, "bound_by"
what the timers show to bound a call.

usage: python tools/pnp_measure.py OUT.json [--reps 30]
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
import pnp_numpy as pn  # noqa: E402
from orb_slam_amd import synth  # noqa: E402

args = sys.argv[1:]
out_path = Path(args[0])
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 30
PAR = dict(pn.RELOC, n_iter=5)
TIMERS = ("pnp", "pnp.prepare", "pnp.solve", "pnp.check", "pnp.refine")


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
    for name in TIMERS:   # a pass each: one pair of events per call
        ctx.timing(True, only=name)
        n0 = ctx.kernel_time(name)[0]
        for _ in range(reps):
            call()
        n, avg, tot = ctx.kernel_time(name)
        ctx.timing(False)
        out[name.replace(".", "_") + "_timer"] = dict(regions=int(n - n0), avg_ms=float(avg))
    return out


def kernel_resources():
    """Registers, scratch, LDS and occupancy of the kernels of orbx_pnp.hip, from the compiler's report for the
    gfx950 code object (the flags of orb_slam_amd/build.py)."""
    import re
    import subprocess
    import tempfile
    from orb_slam_amd import build as b
    src = b.CSRC / "orbx_pnp.hip"
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b.hipcc(), "-x", "hip", f"--offload-arch={b.ARCH}", *b.COMMON,
                            "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(Path(tmp) / "pnp.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_pnp_[a-z]+", m.group(1))
            name = k.group(0) if k else None
            if name:
                out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


res = {"parameters": {k: PAR[k] for k in sorted(PAR)}, "kernels": kernel_resources(),
       "bound_by": "one lane's dependent FP64 chain: the 12x12 Jacobi (k_pnp_solve takes the same time for 35 and 280 "
                   "hypotheses) and, larger and growing with the inlier set, the sequential sums over the points of a "
                   "refit in k_pnp_refine"}
L = ox.lib()
# --- host arrays ---------------------------------------------------------------
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
scenes = [pn.scene(100, seed=500 + k, noise=0.5) for k in range(8)]
built = [ox.pnp_query(pn.frame_of(sc), pn.draws_for(600 + k, 300), **PAR) for k, sc in enumerate(scenes)]


def fresh(q):
    q.iter_done = q.best_inliers = 0     # the calls are timed on a fresh solver each


def host_call():
    fresh(built[0][0])
    L.orbx_pnp_ransac(ctx.handle, ctypes.byref(built[0][0]))


res["host"] = measure(ctx, host_call)
q0 = built[0][0]
res["host"].update(N=int(q0.N), can_run=int(max(5, q0.ransac_max_its)), iters_run=int(q0.iters_run),
                   n_inliers=int(q0.n_inliers), n_records=int(q0.n_records))
arr = (ox.PnpQuery * 8)(*[b[0] for b in built])


def batch_call():
    for k in range(8):
        fresh(arr[k])
    L.orbx_pnp_ransac_batch(ctx.handle, 8, arr)


res["batch8"] = measure(ctx, batch_call)
res["batch8"].update(N=[int(arr[k].N) for k in range(8)], iters_run=[int(arr[k].iters_run) for k in range(8)])
t = []
for _ in range(5):
    s = pn.solver_of(scenes[0], PAR)
    d0 = pn.draws_for(600, 300)
    t0 = time.perf_counter()
    r = s.iterate(5, d0)
    t.append((time.perf_counter() - t0) * 1e3)
res["numpy_restatement_host_case"] = dict(stats(t), iters_run=int(r["iters_run"]))
# the restatement evaluating everything the device evaluates: all iterations the call can run
t = []
for _ in range(3):
    s = pn.solver_of(scenes[0], PAR)
    t0 = time.perf_counter()
    for it in range(s.max_its):
        st = pn.draw_set(s.N, d0[it])
        rec = pn.compute_pose(s.c["p3d"][st].astype(np.float64), s.c["p2d"][st].astype(np.float64), s.epnp_cam, s.decomp)
        pn.check_inliers(s.c, s.cam, rec[pn.O_R:pn.O_R + 9], rec[pn.O_T:pn.O_T + 3])
    t.append((time.perf_counter() - t0) * 1e3)
res["numpy_restatement_all_iterations"] = dict(stats(t), iterations=int(s.max_its))
ctx.close()

# --- device-resident frame --------------------------------------------------------
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
fk = ctx.features(0)[0]
views, keep = [], []
for s in range(1, ncand + 1):
    keys, desc = ctx.features(s)
    _, (ids, ptr, feat), _ = ctx.read_bow(s)
    a = dict(keys=np.ascontiguousarray(keys), desc=np.ascontiguousarray(desc, np.uint8), mp=np.ones(len(keys), np.uint8),
             ids=np.ascontiguousarray(ids, np.uint32), ptr=np.ascontiguousarray(ptr, np.int32),
             feat=np.ascontiguousarray(feat if len(feat) else np.zeros(1), np.int32))
    v = ox.BowView()
    v.keys, v.desc, v.n, v.mp = a["keys"].ctypes.data, a["desc"].ctypes.data, len(keys), a["mp"].ctypes.data
    v.n_nodes, v.node_id, v.node_ptr, v.feat_idx = len(ids), a["ids"].ctypes.data, a["ptr"].ctypes.data, a["feat"].ctypes.data
    views.append(v)
    keep.append(a)
m_f, nm = ctx.search_by_bow(0, views)
pos = []
for k in range(ncand):       # map points that make the matches a scene seen from the identity pose
    p = rng.normal(size=(views[k].n, 3)).astype(np.float32) + np.float32([0, 0, 5])
    i = np.flatnonzero(m_f[k][:len(fk)] >= 0)
    z = rng.uniform(3.0, 8.0, len(i))
    good = np.stack([(fk["x"][i] - cam[2]) / cam[0] * z, (fk["y"][i] - cam[3]) / cam[1] * z, z], 1)
    ok = rng.random(len(i)) > 0.2
    p[m_f[k][i][ok]] = good[ok]
    pos.append(p)
draws = [pn.draws_for(700 + k, 300) for k in range(ncand)]
last = {}


def dev_call():
    last["r"] = ctx.dev_pnp_candidates(0, views, pos, cam, pn.SIGMA2, draws, **PAR)


res["dev8"] = measure(ctx, dev_call)
r = last["r"]
res["dev8"].update(n_matches=r["n_matches"].tolist(), N=[x["N"] for x in r["results"]],
                   iters_run=[x["iters_run"] for x in r["results"]], found=[x["found"] for x in r["results"]],
                   discarded=r["discarded"].tolist())
for _ in range(5):
    ctx.search_by_bow(0, views)
t = []
for _ in range(reps):
    t0 = time.perf_counter()
    ctx.search_by_bow(0, views)
    t.append((time.perf_counter() - t0) * 1e3)
res["dev8_search_alone"] = dict(wall=stats(t))
voc.close()
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res, indent=1))
