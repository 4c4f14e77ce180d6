"""Times the covisibility map on the device (orbx_covis.hip) on the GPU and
writes one JSON file.

For 256, 1024 and 4096 keyframes with rows of 1200 entries (1000 points, one
index in six empty): keyframe k draws its points from the 2500 consecutive
ids from 250 k on, so that a keyframe shares points with about ten keyframes
on either side and a frame that holds one keyframe's 1000 points is seen by
about 20 keyframes.  All keyframes are added, then updated in id order.

  update_reference     one orbx_covis_update_reference: the frame's upload,
                       the mark, count, select, top, pass and the three point
                       kernels, the header's and the lists' read-back
  update_connections   one orbx_covis_update_connections for one keyframe: the
                       mark, count and connect kernels and the read-back
  restatement          tests/covis_numpy.py on one core for the same two
                       calls.  It is Python over dicts, not the reference's
                       C++ over std::map: a yardstick for the work, not a
                       competitor.  Its world holds every row, and the
                       connections of the keyframes within 40 of the frame's
                       (the state the two calls read is the same: an update
                       reaches the keyframes that share a point, ten away)

Every entry: the median, minimum, 90th percentile and maximum of the wall time
over --reps calls after warm-up, and the four kernel timers, measured in
passes of their own (the timers' events cost wall time).  "kernels" holds the
compiler's register, scratch and LDS figures.

usage: python tools/covis_measure.py OUT.json [--reps 40] [--sizes 256,1024,4096]
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
import covis_cases as cc  # noqa: E402
import covis_numpy as cn  # noqa: E402

args = sys.argv[1:]
out_path = Path(args[0])
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 40
sizes = [int(x) for x in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else [256, 1024, 4096]
DRAW, WINDOW, STEP, NEAR = 1000, 2500, 250, 40
TIMERS = ("covis_count", "covis_select", "covis_points", "covis_connect")


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), p90_ms=float(ms[int(0.9 * (len(ms) - 1))]),
                max_ms=float(ms[-1]), n=len(ms))


def measure(ctx, call, timers):
    for _ in range(5):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    out = dict(wall=stats(wall))
    for name in timers:   # a pass each: one pair of events per call
        ctx.timing(True, only=name)
        n0 = ctx.kernel_time(name)[0]
        for _ in range(reps):
            call()
        k, avg, _ = ctx.kernel_time(name)
        ctx.timing(False)
        out[name + "_timer"] = dict(regions=int(k - n0), avg_ms=float(avg))
    return out


def kernel_resources():
    """Registers, scratch and LDS of the kernels of orbx_covis.hip, from the compiler's report for the gfx950 code
    object (the flags of orb_slam_amd/build.py).  k_covis_select and k_covis_list size their LDS at launch: 4 bytes
    per keyframe ever added, and 4 bytes per id below the largest, rounded up to a power of two."""
    import re
    import subprocess
    import tempfile
    from orb_slam_amd import build as b
    src = b.CSRC / "orbx_covis.hip"
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b.hipcc(), "-x", "hip", f"--offload-arch={b.ARCH}", *b.COMMON,
                            "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(Path(tmp) / "covis.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_covis_[a-z_]+?(?=E|$)", m.group(1))
            name = k.group(0) if k else None
            if name:
                out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("static_lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


res = {"parameters": dict(draw=DRAW, window=WINDOW, step=STEP, row=DRAW + DRAW // 5, reps=reps)}
if "--no-resources" not in args:
    res["kernels"] = kernel_resources()
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
for members in sizes:
    rng = np.random.default_rng(members)
    rows = cc.window_rows(rng, members, draw=DRAW, window=WINDOW, step=STEP)
    keys = cc.rand_keys(rng, members)
    n_points = STEP * members + WINDOW
    t0 = time.perf_counter()
    m = ox.CovisibilityMap(ctx, members, n_points, len(rows[0]))
    for i in range(members):
        m.add_keyframe(i, keys[i], rows[i])
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i0 in range(0, members, 256):
        m.update_connections(np.arange(i0, min(i0 + 256, members)))
    t_build = time.perf_counter() - t0
    mid = members // 2
    frame = rows[mid]
    last = {}

    def reference_call():
        last["ref"] = m.update_reference(frame)

    def update_call():
        last["upd"] = m.update_connections([mid])

    e = dict(build=dict(add_ms_per_keyframe=t_add * 1e3 / members, update_ms_per_keyframe=t_build * 1e3 / members),
             update_reference=measure(ctx, reference_call, TIMERS[:3]),
             update_connections=measure(ctx, update_call, (TIMERS[0], TIMERS[3])))
    r = last["ref"]
    e["update_reference"].update(n_voters=int(r["n_voters"]), n_local_kf=int(r["n_local_kf"]),
                                 n_local_mp=int(r["n_local_mp"]), ref_kf=int(r["ref_kf"]))
    # the restatement on one core, and that it agrees
    w = cn.World()
    for i in range(members):
        w.add_keyframe(i, keys[i], rows[i])
    near = list(range(max(0, mid - NEAR), min(members, mid + NEAR + 1)))
    w.update_connections(near)
    t_r, t_u = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        want = w.update_reference(frame)
        t_r.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want_u = w.update_connections([mid])
        t_u.append((time.perf_counter() - t0) * 1e3)
    e["restatement"] = dict(update_reference=stats(t_r), update_connections=stats(t_u),
                            same_reference=(want["local_kf"] == r["local_kf"].tolist()
                                            and want["local_mp"] == r["local_mp"].tolist()
                                            and want["ref_kf"] == r["ref_kf"] and want["n_voters"] == r["n_voters"]),
                            same_update=(want_u[0] == last["upd"][0].tolist() and want_u[1] == last["upd"][1].tolist()))
    res[str(members)] = e
    m.close()
    print(members, json.dumps(e), flush=True)
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print("written", out_path)
