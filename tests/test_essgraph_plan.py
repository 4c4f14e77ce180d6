"""orbx_essgraph_plan, the symbolic part of the essential-graph solve (host
only, no GPU): against a numpy envelope computation for every case of
tests/essgraph_numpy.py, against the pattern of a dense Cholesky factor, its
refusals, and the stand-alone C++ checks of the planner and of the adapter's
edge rules (tests/essgraph_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import essgraph_numpy as en
import orb_slam_amd as ox
from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


@pytest.mark.parametrize("name", list(en.CASES))
def test_plan_equals_the_numpy_envelope(name):
    g = en.CASES[name]()
    want = en.plan(g["ids"], g["loop_kf"], g["edges"])
    got = ox.essgraph_plan(g["ids"], g["loop_kf"], g["edges"])
    for key in ("n_free", "n_blocks", "max_row_blocks"):
        assert got[key] == want[key], key
    for key in ("free_index", "first", "row_off"):
        assert np.array_equal(got[key], want[key]), key
    fr = got["free_index"]
    assert fr[g["loop_kf"]] == -1                                   # the fixed vertex is removed
    free = np.nonzero(fr >= 0)[0]
    assert np.array_equal(np.sort(fr[free]), np.arange(got["n_free"]))
    assert np.all(np.diff(g["ids"][free[np.argsort(fr[free])]]) > 0)   # the order is by id


def test_envelope_contains_the_cholesky_factor_of_a_random_pattern():
    rng = np.random.RandomState(11)
    for trial in range(5):
        n = 40
        edges = [(k, k - 1, 1) for k in range(1, n)]
        edges += [(int(a), int(b), 1) for a, b in rng.randint(0, n, (12, 2)) if a != b]
        ids = rng.permutation(1000)[:n]
        pl = ox.essgraph_plan(ids, -1, edges)
        fr = pl["free_index"]
        assert pl["n_free"] == n
        A = np.zeros((n, n))
        for i, j, _ in edges:
            A[fr[i], fr[j]] = A[fr[j], fr[i]] = rng.uniform(0.5, 1.0)
        A += np.diag(np.abs(A).sum(1) + 1.0)
        L = np.linalg.cholesky(A)
        inside = np.zeros((n, n), bool)
        for r in range(n):
            inside[r, pl["first"][r]:r + 1] = True
        assert not np.any((np.abs(L) > 0) & ~inside)
        assert np.count_nonzero(np.abs(L) > 1e-14) > np.count_nonzero(np.tril(A))      # there is fill, and it is inside
        assert pl["n_blocks"] == inside.sum() == pl["row_off"][-1]


def test_plan_refusals():
    lib = ox.lib()

    def code(ids, fixed, edges):
        try:
            ox.essgraph_plan(ids, fixed, edges)
        except ox.OrbxError as e:
            return e.code
        return 0
    assert code([1, 2, 3], 0, [(1, 0, 1)]) == 0
    assert code([1, 2, 1], 0, [(1, 0, 1)]) == -1          # duplicate ids
    assert code([1, 2, 3], 0, [(1, 1, 1)]) == -1          # i == j
    assert code([1, 2, 3], 0, [(1, 3, 1)]) == -1          # an index outside the array
    assert code([1, 2, 3], 0, [(-1, 0, 0)]) == -1
    assert code([1, 2, 3], 3, [(1, 0, 1)]) == -1
    assert code([1, 2, 3], 0, [(1, 0, 2)]) == -1          # kind
    assert lib.orbx_essgraph_plan(3, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert lib.orbx_essgraph_plan(-1, None, 0, 0, None, None, None, None, None, None, None) == -1
    empty = ox.essgraph_plan([4, 5], 0, np.zeros((0, 3), np.int64))
    assert empty["n_free"] == 0 and empty["n_blocks"] == 0 and list(empty["free_index"]) == [-1, -1]


def test_planner_and_edge_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    exe = tmp_path / "essgraph_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}", str(HERE / "essgraph_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "essgraph_check: ok" in r.stdout, r.stdout + r.stderr
