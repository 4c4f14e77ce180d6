"""Times the keyframe database on the device (orbx_kfdb.hip) on the GPU and
writes one JSON file.

For 256, 1024 and 4096 members of about 1000 words each (words drawn from a
universe of 5000, so that two BowVectors share about 200 words -- the length
of the scan's sequential FP64 chain) and every member given ten neighbours:

  reloc   one orbx_kfdb_query in relocalisation mode, host query arrays: one
          upload, the scan and select kernels, one read-back
  loop    the same in loop mode with 20 covisible and 20 connected keyframes
  score20 (4096 only) orbx_kfdb_score for 20 ids: the scan alone with its
          upload and read-back
  numpy   the restatement of tests/kfdb_numpy.py on one core for the same two
          queries.  It is Python over an inverted file, not the reference's
          C++: a yardstick for the work, not a competitor

Every entry: the median, minimum and 90th percentile of the wall time over
--reps calls after warm-up, and the "kfdb_scan" and "kfdb_select" kernel
timers, measured in passes of their own (the timers' events cost wall time).
"kernels" holds the compiler's register, scratch and LDS figures.

usage: python tools/kfdb_measure.py OUT.json [--reps 40]
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
import kfdb_cases as kc  # noqa: E402
import kfdb_numpy as kn  # noqa: E402

args = sys.argv[1:]
out_path = Path(args[0])
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 40
WORDS, UNIVERSE, MAX_WORDS = 1000, 5000, 1024
TIMERS = ("kfdb_scan", "kfdb_select")


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), p90_ms=float(ms[int(0.9 * (len(ms) - 1))]),
                max_ms=float(ms[-1]), n=len(ms))


def measure(ctx, call, n=None):
    n = n or reps
    for _ in range(5):
        call()
    wall = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    out = dict(wall=stats(wall))
    for name in TIMERS:   # a pass each: one pair of events per call
        ctx.timing(True, only=name)
        n0 = ctx.kernel_time(name)[0]
        for _ in range(n):
            call()
        k, avg, _ = ctx.kernel_time(name)
        ctx.timing(False)
        out[name + "_timer"] = dict(regions=int(k - n0), avg_ms=float(avg))
    return out


def kernel_resources():
    """Registers, scratch and LDS of the kernels of orbx_kfdb.hip, from the compiler's report for the gfx950 code
    object (the flags of orb_slam_amd/build.py).  Both kernels size their LDS at launch: the query for the scan
    (12 bytes a word), the sort keys for the select (8 bytes a member, rounded up to a power of two)."""
    import re
    import subprocess
    import tempfile
    from orb_slam_amd import build as b
    src = b.CSRC / "orbx_kfdb.hip"
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b.hipcc(), "-x", "hip", f"--offload-arch={b.ARCH}", *b.COMMON,
                            "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(Path(tmp) / "kfdb.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_kfdb_[a-z_]+?(?=E|$)", m.group(1))
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


res = {"parameters": dict(words=WORDS, universe=UNIVERSE, max_words=MAX_WORDS, reps=reps), "kernels": kernel_resources()}
ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
rng = np.random.default_rng(11)
for members in (256, 1024, 4096):
    db = ox.KeyFrameDatabase(ctx, members, MAX_WORDS)
    ref_db = kn.KeyFrameDatabase()
    for i in range(members):
        b = kc.rand_bow(rng, int(rng.integers(WORDS - 100, WORDS + 1)), UNIVERSE)
        db.add(i, *b)
        kf = kn.KeyFrame(i, *b)
        kf.neighbours = [int(x) for x in rng.choice(members, 10, replace=False)]
        ref_db.add(kf)
    ids = np.arange(members, dtype=np.int32)
    db.set_neighbours(ids, [ref_db.kfs[i].neighbours for i in range(members)])
    q = kc.rand_bow(rng, WORDS, UNIVERSE)
    covis = [int(x) for x in rng.choice(members, 20, replace=False)]
    conn = [int(x) for x in rng.choice(members, 20, replace=False)]
    last = {}

    def reloc_call():
        last["reloc"] = db.detect_relocalisation_candidates(q, info=True)

    def loop_call():
        last["loop"] = db.detect_loop_candidates(q, 1.0, ref=covis, exclude=conn, info=True)

    e = dict(reloc=measure(ctx, reloc_call), loop=measure(ctx, loop_call))
    for k in ("reloc", "loop"):
        c, info = last[k]
        e[k].update(n_candidates=len(c), max_common_words=int(info["max_common_words"]),
                    n_sharing=int(info["n_sharing"]), n_scored=int(info["n_scored"]))
    if members == 4096:
        e["score20"] = measure(ctx, lambda: db.score(q, covis))
    # the restatement on one core, and that it agrees
    t_r, t_l = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        want_r = ref_db.DetectRelocalisationCandidates(ref_db.new_query(*q))
        t_r.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pq = ref_db.new_query(*q)
        ms = ref_db.detect_loop_min_score(pq, [ref_db.kfs[i] for i in covis])
        want_l = ref_db.DetectLoopCandidates(pq, ms, [ref_db.kfs[i] for i in conn])
        t_l.append((time.perf_counter() - t0) * 1e3)
    e["numpy_restatement"] = dict(reloc=stats(t_r), loop=stats(t_l),
                                  same_reloc=[k.mnId for k in want_r] == last["reloc"][0].tolist(),
                                  same_loop=[k.mnId for k in want_l] == last["loop"][0].tolist())
    res[str(members)] = e
    db.close()
ctx.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res, indent=1))
