"""The numpy restatement of the initialisation models (tests/init_numpy.py)
checked on its own: hand-worked set selection, the geometry of noise-free
scenes, the committed fixture that pins it, and the new C symbols (no GPU)."""
import re
from pathlib import Path

import numpy as np
import pytest

import init_numpy as inp
import orb_slam_amd as ox

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "init_models.npz"
RAND_MAX = 2**31 - 1
NEW_FUNCTIONS = ["orbx_init_models", "orbx_init_models_batch", "orbx_dev_init_models", "orbx_dev_read_init_models"]


def test_set_selection_by_hand():
    """10 matches, 2 iterations.  RandomInt(0, size - 1) = int(r / 2^31 * size);
    the picked entry is overwritten by the back of the list, which is popped.
    Iteration 0, draws (RAND_MAX, 0, 2^30, 0, RAND_MAX, 2^30, 0, 0):
      [0..9]            size 10 randi 9 -> 9   list [0 1 2 3 4 5 6 7 8]
      size 9  randi 0 -> 0                     list [8 1 2 3 4 5 6 7]
      size 8  randi 4 -> 4                     list [8 1 2 3 7 5 6]
      size 7  randi 0 -> 8                     list [6 1 2 3 7 5]
      size 6  randi 5 -> 5                     list [6 1 2 3 7]
      size 5  randi 2 -> 2                     list [6 1 7 3]
      size 4  randi 0 -> 6                     list [3 1 7]
      size 3  randi 0 -> 3
    Iteration 1, every draw 2^30 (r / 2^31 = 0.5):
      size 10 randi 5 -> 5                     list [0 1 2 3 4 9 6 7 8]
      size 9  randi 4 -> 4                     list [0 1 2 3 8 9 6 7]
      size 8  randi 4 -> 8                     list [0 1 2 3 7 9 6]
      size 7  randi 3 -> 3                     list [0 1 2 6 7 9]
      size 6  randi 3 -> 6                     list [0 1 2 9 7]
      size 5  randi 2 -> 2                     list [0 1 7 9]
      size 4  randi 2 -> 7                     list [0 1 9]
      size 3  randi 1 -> 1"""
    h = 2**30
    draws = np.array([[RAND_MAX, 0, h, 0, RAND_MAX, h, 0, 0], [h] * 8], np.int32)
    sets = inp.make_sets(10, draws)
    assert sets.tolist() == [[9, 0, 4, 8, 5, 2, 6, 3], [5, 4, 8, 3, 6, 2, 7, 1]]
    # N = 8: every set is a permutation of all matches
    s8 = inp.make_sets(8, inp.make_draws(4, 16))
    assert all(sorted(r) == list(range(8)) for r in s8.tolist())


def test_compaction_and_normalize_by_hand():
    m = np.array([-1, 3, -1, 0, 2, -7], np.int32)
    assert inp.compact(m).tolist() == [[1, 3], [3, 0], [4, 2]]
    keys = inp.make_keys(np.array([[1, 10], [3, 30], [8, 20]], np.float32))
    pn, T = inp.normalize(keys)
    # mean (4, 20); mean |dev| (8/3, 20/3)
    sx, sy = np.float32(1.0 / np.float64(np.float32(8) / np.float32(3))), np.float32(1.0 / np.float64(np.float32(20) / np.float32(3)))
    assert T.tolist() == [sx, 0, np.float32(-4) * sx, 0, sy, np.float32(-20) * sy, 0, 0, 1]
    assert pn[:, 0].tolist() == [np.float32(-3) * sx, np.float32(-1) * sx, np.float32(4) * sx]


def test_noise_free_plane_gives_the_homography():
    k1, k2, m = inp.scene(11, 150, planar=True, noise=0.0, outliers=0.0)
    r = inp.init_models(k1, k2, m, inp.make_draws(2, 50), max_iter=50)
    assert r["n_matches"] == 150 and r["best_h"] >= 0
    H = r["H21"].astype(np.float64).reshape(3, 3)
    x1 = np.stack([r["xy"][:, 0], r["xy"][:, 1], np.ones(150)], 0).astype(np.float64)
    p = H @ x1
    err = np.hypot(p[0] / p[2] - r["xy"][:, 2], p[1] / p[2] - r["xy"][:, 3])
    assert err.max() < 1e-3, err.max()
    assert r["inliers_h"].all()
    assert r["RH"] > 0.40   # the branch Initialize takes for a plane (:113)


def test_noise_free_cloud_gives_the_fundamental_matrix():
    k1, k2, m = inp.scene(12, 150, planar=False, noise=0.0, outliers=0.0)
    r = inp.init_models(k1, k2, m, inp.make_draws(3, 50), max_iter=50)
    assert r["best_f"] >= 0 and r["inliers_f"].all()
    F = r["F21"].astype(np.float64).reshape(3, 3)
    x1 = np.stack([r["xy"][:, 0], r["xy"][:, 1], np.ones(150)], 0).astype(np.float64)
    x2 = np.stack([r["xy"][:, 2], r["xy"][:, 3], np.ones(150)], 0).astype(np.float64)
    l2 = F @ x1
    # distance of x2 from the epipolar line of x1: float32 coordinates (2^-24
    # x 640 px) through an 8-point solve of condition <= 1e4
    dist = np.abs((x2 * l2).sum(0)) / np.hypot(l2[0], l2[1])
    assert dist.max() < 1e-2, dist.max()
    # rank 2 was set in float64 on Fn and rounded to float32; T2t Fn T1 keeps
    # it to float32 rounding of the entries
    assert abs(np.linalg.det(F / np.linalg.norm(F))) < 1e-6
    assert r["RH"] < 0.40


def test_header_and_library_have_the_new_entry_points():
    """Fails on the parent commit: the functions do not exist there."""
    text = (ROOT / "include" / "orbx.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\}\s*orbx_init_query\s*;", code)
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 6
    lib = ox.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    import ctypes
    q = ctypes.byref(ox.InitQuery())
    assert lib.orbx_init_models(None, q) == -1
    assert lib.orbx_init_models_batch(None, 1, q) == -1
    assert lib.orbx_dev_init_models(None, 0, 1, 1, 1.0, 200, None) == -1
    assert lib.orbx_dev_read_init_models(None, 0, q) == -1


def test_query_layout_matches_the_header():
    """The ctypes view lists the header's fields in the header's order."""
    text = (ROOT / "include" / "orbx.h").read_text()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*orbx_init_query\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            mm = re.search(r"(\w+)\s*(\[\d+\])?\s*$", part.strip())
            if mm and part.strip():
                names.append(mm.group(1))
    assert names == [f[0] for f in ox.InitQuery._fields_]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_reproduces_the_fixture(golden, s):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith(f"s{s}_")}
    M = int(g["max_iter"])
    r = inp.init_models(g["keys1"], g["keys2"], g["matches12"], g["draws"], sigma=1.0, max_iter=M)
    # the bit-exact layer, independent of the linear-algebra library
    assert r["n_matches"] == int(g["n_matches"])
    assert r["sets"].tobytes() == g["sets"].tobytes()
    assert r["T1"].tobytes() == g["T1"].tobytes() and r["T2"].tobytes() == g["T2"].tobytes()
    H21, H12 = inp.denorm_h(g["Hn"], g["T1"], g["T2"])
    F21 = inp.denorm_f(g["Fn"], g["T1"], g["T2"])
    sh, _ = inp.check_homography(H21, H12, r["xy"], 1.0)
    sf, _ = inp.check_fundamental(F21, r["xy"], 1.0)
    assert sh.tobytes() == g["score_h"].tobytes() and sf.tobytes() == g["score_f"].tobytes()
    # the solves: well-conditioned iterations agree to a float32 ulp of the
    # largest entry, and their end-to-end scores are mostly the same bits
    for name, ok, score in (("Hn", g["gap_h"] >= 1e-4, "score_h"),
                            ("Fn", (g["c8_f"] >= 1e-4) & (g["gap_f"] >= 1e-4), "score_f")):
        assert ok.mean() >= 0.95
        a, b = r[name][ok], g[name][ok]
        b = b * np.sign((a * b).sum(1, keepdims=True))
        ulp = np.spacing(np.abs(b).max(1, keepdims=True).astype(np.float32))
        assert (np.abs(a - b) <= ulp).all(), name
        assert (r[score][ok].view(np.uint32) == g[score][ok].view(np.uint32)).mean() >= 0.9, score


@pytest.mark.parametrize("i", range(len(inp.CASES)), ids=[f"N{c[0]}-it{c[1]}" for c in inp.CASES])
def test_gpu_cases_stay_inside_the_conditioning_cap(i):
    """The cases of tests/test_init_gpu.py: the cut of the solve comparison
    excludes at most 5 % of the iterations per model, by the restatement."""
    (k1, k2, m, d, M), r = inp.case(i)
    assert r["n_matches"] == inp.CASES[i][0] and len(k1) != len(k2)
    for ok in inp.considered(r):
        assert (~ok).sum() <= 0.05 * M
