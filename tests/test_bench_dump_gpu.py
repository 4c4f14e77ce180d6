"""`bench.py --dump-outputs` on the GPU: the files hold what the timed path
computed in its last step, checked against the oracle on the same seeded
inputs (small batches; the bench's own shapes are tests/test_bench_shape_gpu.py)."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import orb_slam_amd as ox
from orb_slam_amd import synth, synth_pose as sp

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu


def _bench(args):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout
    return json.loads(lines[0])


def _load(d):
    out = {p.stem: np.load(p) for p in sorted(d.iterdir())}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64e6
    return out


def test_c2_dump_is_the_last_steps_output(tmp_path):
    B, nf, w, h = 5, 1000, 640, 480
    line = _bench(["--steps", "3", "--warmup", "1", "--batch", str(B), "--dump-outputs", str(tmp_path)])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    got = _load(tmp_path)
    assert sorted(got) == ["descriptor_frames", "descriptors", "keypoints", "matches", "n_keypoints", "n_matches"]
    assert list(got["descriptor_frames"]) == list(range(B))
    frames = synth.sequence(w, h, B, seed=2000)
    ex = oracle_lib.RefExtractor(nf)
    L = oracle_lib.load()
    ref = [ex(f) for f in frames]
    for f in range(B):
        k, d = ref[f]
        pk, pd = ref[(f - 1) % B]
        assert got["n_keypoints"][f] == len(k) > 0
        assert np.array_equal(got["keypoints"][f, :len(k)],
                              np.stack([k[n] for n in k.dtype.names], 1).astype(np.float32))
        assert not got["keypoints"][f, len(k):].any()
        assert np.array_equal(got["descriptors"][f, :len(k)], d)
        F1, F2 = ox.frame_view(pk, pd, w, h), ox.frame_view(k, d, w, h)
        pm = np.stack([pk["x"], pk["y"]], 1).astype(np.float32).copy()
        want = np.zeros(len(pk), np.int32)
        nm = ctypes.c_int()
        L.orbx_ref_search_for_initialization(ctypes.byref(F1), ctypes.byref(F2), oracle_lib.ptr(pm),
                                             oracle_lib.ptr(want), 100, 0.9, 1, ctypes.byref(nm))
        assert got["n_matches"][f] == nm.value > 0
        assert np.array_equal(got["matches"][f, :len(pk)], want)
        assert not got["matches"][f, len(pk):].any()


def test_pose_dump_is_the_last_steps_output(tmp_path):
    P = 4
    _bench(["--workload", "pose", "--steps", "2", "--warmup", "1", "--batch", str(P), "--dump-outputs",
            str(tmp_path)])
    got = _load(tmp_path)
    assert sorted(got) == ["Tcw", "n_inliers", "outlier"]
    assert got["Tcw"].shape == (P, 16) and got["outlier"].shape == (P, 1000)
    L = oracle_lib.load()
    L.orbx_ref_pose_optimization.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.orbx_ref_pose_optimization.restype = ctypes.c_int
    for i in range(P):
        p, arrs = sp.to_ctypes(sp.make_frame(n_kp=1000, seed=7000 * 1000 + i))
        ni = ctypes.c_int()
        assert L.orbx_ref_pose_optimization(ctypes.byref(p), ctypes.byref(ni), None) == 0
        # the pose tolerance of bench.parity_pose; inlier count and flags identical
        assert np.abs(got["Tcw"][i] - np.ctypeslib.as_array(p.Tcw)).max() <= 1e-5
        assert got["n_inliers"][i] == ni.value
        assert np.array_equal(got["outlier"][i], arrs["outlier"])
