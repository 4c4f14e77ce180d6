"""The numpy restatement of Sim3Solver (tests/sim3_numpy.py) checked on its
own: the draw quirk by hand and by enumeration, RandomInt's ends, the size_t
limits, the iteration cap, Horn on exact points, the sign of q, iterate's
return rule, the committed fixture that pins it, and the new C symbols (no
GPU)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import sim3_numpy as s3

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "sim3_ransac.npz"
RAND_MAX = 2**31 - 1
NEW_FUNCTIONS = ["orbx_sim3_ransac", "orbx_sim3_ransac_batch", "orbx_dev_sim3_candidates"]
F32 = np.float32


def at(pos, size):
    """A rand() value that RandomInt maps to `pos` of `size`."""
    r = int((pos + 0.5) / size * 2**31)
    assert s3.random_int(r, size) == pos
    return r


def test_draw_quirk_by_hand():
    """10 correspondences.  The removal is buf[idx] = back; pop_back with the
    drawn value idx as the position.
    Iteration 0, positions 5, 5, 5:
      [0..9] size 10  randi 5 -> 5   buf[5] = 9       buf [0 1 2 3 4 9 6 7 8 | 9]
      size 9          randi 5 -> 9   buf[9] = buf[8]  buf [0 1 2 3 4 9 6 7 | 8 8]
        (the write lands at place 9, past the new size 8; place 5 keeps its 9)
      size 8          randi 5 -> 9   the same correspondence again
    Iteration 1, positions 2, 7, 2 (an ordinary removal while value == place):
      size 10 randi 2 -> 2  buf[2] = 9    [0 1 9 3 4 5 6 7 8]
      size 9  randi 7 -> 7  buf[7] = 8    [0 1 9 3 4 5 6 8]
      size 8  randi 2 -> 9  buf[9] = 8    [0 1 9 3 4 5 6] -- place 2 still holds 9
    Iteration 2, positions 9, 8, 7: the back each time, nothing moves."""
    draws = [[at(5, 10), at(5, 9), at(5, 8)], [at(2, 10), at(7, 9), at(2, 8)], [at(9, 10), at(8, 9), at(7, 8)]]
    assert s3.make_sets(10, draws).tolist() == [[5, 9, 9], [2, 7, 9], [9, 8, 7]]
    # with the usual removal (at the drawn position) iteration 0 would be 5, 9, 8
    assert s3.make_sets(2, draws).tolist() == [[0, 0, 0]] * 3   # fewer than three: no sets


@pytest.mark.parametrize("N", [3, 4, 5, 8, 11])
def test_draw_quirk_by_enumeration(N):
    """Every outcome of the three positions: a correspondence repeats in
    N - 2 of the N (N - 1) (N - 2) sets, never more than twice, and always as
    the back of the list picked by the second and third draw."""
    repeats = 0
    for r1 in range(N):
        for r2 in range(N - 1):
            for r3 in range(N - 2):
                st = s3.make_sets(N, [[at(r1, N), at(r2, N - 1), at(r3, N - 2)]])[0].tolist()
                assert all(0 <= x < N for x in st)
                if len(set(st)) < 3:
                    repeats += 1
                    assert st[1] == st[2] == N - 1 and st[0] == r1 == r2 == r3
    assert repeats == N - 2


def test_random_int_ends():
    for size in (1, 3, 300, 4096):
        assert s3.random_int(0, size) == 0
        assert s3.random_int(RAND_MAX, size) == size - 1
    assert s3.random_int(2**30, 9) == 4


def test_size_t_truncation_of_the_limits():
    assert s3.max_error(1.0) == 9
    assert s3.max_error(1.44) == 13          # 9.210 * 1.44f = 13.26...
    assert s3.max_error(F32(1.2) ** 14) == int(9.210 * float(F32(1.2) ** 14))
    # the comparison is float < float(limit): 8.9999 passes the limit 9, 9.0 does not
    assert F32(8.9999) < F32(s3.max_error(1.0)) and not F32(9.0) < F32(s3.max_error(1.0))


def test_ransac_max_its():
    assert s3.ransac_max_its(20, 20) == 1
    for N in (21, 300):
        eps = float(F32(20) / F32(N))
        direct = int(np.ceil(np.log(1 - 0.99) / np.log(1 - eps ** 3)))
        assert s3.ransac_max_its(N, 20) == max(1, min(direct, 300))
    assert s3.ransac_max_its(21, 20) == 3 and s3.ransac_max_its(300, 20) == 300
    assert s3.ransac_max_its(300, 20, max_iterations=100000) == 15541
    assert s3.ransac_max_its(19, 20) == 0


def _exact_case():
    rng = np.random.RandomState(3)
    X2 = rng.uniform(-2, 2, (3, 3))
    R, t, s = s3._rot([0.3, -0.5, 0.2]), np.array([0.5, -1.0, 2.0]), 1.7
    X1 = s * X2 @ R.T + t                    # x1 = s R x2 + t: T12 maps camera 2 to camera 1
    c = dict(x3dc1=X1.astype(F32), x3dc2=X2.astype(F32))
    return c, R, t, s


def test_horn_on_three_exact_points():
    c, R, t, s = _exact_case()
    r = s3.compute_t(c, [[0, 1, 2]])
    T12 = r["T12_all"].reshape(4, 4).astype(np.float64)
    assert np.abs(r["R"].reshape(3, 3) - R).max() < 4e-6
    assert abs(float(r["scale"][0]) - s) < 1e-5
    assert np.abs(T12[:3, 3] - t).max() < 2e-5
    T21 = r["T21_all"].reshape(4, 4).astype(np.float64)
    assert np.abs(T12 @ T21 - np.eye(4)).max() < 1e-5
    assert r["gap"][0] > 0.1 and r["q"][0, 0] > 0


def test_q_and_minus_q_are_one_rotation():
    c, R, t, s = _exact_case()
    q = s3.compute_t(c, [[0, 1, 2]])["q"]
    Rp, Rm = s3.rotation(q), s3.rotation(-q)
    assert np.abs(Rp.astype(np.float64) - Rm.astype(np.float64)).max() < 1e-6
    assert s3.fix_sign(-q.astype(np.float64))[0].tolist() == q[0].astype(np.float64).tolist()
    assert s3.fix_sign([[0.0, -0.6, 0.0, 0.8]])[0].tolist() == [0.0, 0.6, 0.0, -0.8]


def test_iterate_return_rule():
    sel = s3.iterate_select
    # the first count above min_inliers that reaches the running best
    r = sel([3, 20, 21, 50], N=100, min_inliers=20, max_its=300)
    assert (r["found_iter"], r["iters_run"], r["n_inliers"], r["best_inliers_out"], r["best_iter"]) == (2, 3, 21, 21, 2)
    # count == min_inliers updates the best but does not return
    r = sel([20, 20, 5], N=100, min_inliers=20, max_its=300)
    assert (r["found"], r["found_iter"], r["iters_run"], r["best_inliers_out"], r["best_iter"], r["no_more"]) == \
        (0, -1, 3, 20, 1, 0)
    # a carried-in best: 30 does not return, an equal 40 does
    r = sel([30, 40, 45], N=100, min_inliers=20, max_its=300, iter_done=7, best_inliers=40)
    assert (r["found_iter"], r["n_inliers"], r["best_inliers_out"]) == (1, 40, 40)
    r = sel([30, 39], N=100, min_inliers=20, max_its=300, iter_done=7, best_inliers=40)
    assert (r["found"], r["best_iter"], r["best_inliers_out"], r["iters_run"]) == (0, -1, 40, 2)
    # the cap: iterations past mRansacMaxIts are not run, and bNoMore is set at it
    r = sel([0, 0, 0, 99], N=21, min_inliers=20, max_its=3)
    assert (r["found"], r["iters_run"], r["no_more"]) == (0, 3, 1)
    r = sel([0, 99], N=21, min_inliers=20, max_its=3, iter_done=2)
    assert (r["found"], r["iters_run"], r["no_more"]) == (0, 1, 1)
    r = sel([99], N=21, min_inliers=20, max_its=3, iter_done=2)
    assert (r["found"], r["iters_run"], r["no_more"]) == (1, 1, 0)      # a return leaves bNoMore false
    # too few correspondences (:146-150)
    r = sel([50], N=19, min_inliers=20, max_its=0)
    assert (r["found"], r["iters_run"], r["no_more"]) == (0, 0, 1)


def test_noise_free_scene_recovers_the_similarity():
    kf1, kf2, m, idx1 = s3.scene(9, 80, outliers=0.0, noise=0.0, use_idx1=True)
    r = s3.sim3_ransac(kf1, kf2, m, s3.make_draws(2, 20), idx1=idx1)
    assert r["N"] == 80 and r["found"] and r["found_iter"] == 0 and r["n_inliers"] == 80
    assert r["inliers"].sum() == 80 and (r["inliers"][r["indices1"]] == 1).all()
    assert abs(float(r["s12"]) - 1 / 1.1) < 1e-4
    # no correspondence through a missing or bad map point, an unmatched keypoint or a negative index
    assert len(m) - 80 == 5 + 3 + 3 + 2 and (m >= 0).sum() == 88


def test_header_and_library_have_the_new_entry_points():
    """Fails on the parent commit: the functions do not exist there."""
    text = (ROOT / "include" / "orbx.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\}\s*orbx_sim3_query\s*;", code) and re.search(r"\}\s*orbx_sim3_kf\s*;", code)
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 9
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 9
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    q = ctypes.byref(ox.Sim3Query())
    assert lib.orbx_sim3_ransac(None, q) == -1
    assert lib.orbx_sim3_ransac_batch(None, 1, q) == -1
    assert lib.orbx_dev_sim3_candidates(None, 0, None, 1, None, None, 0.75, 1, 20, 0.99, 20, 300, 5, None, None, 0,
                                        None, None, None) == -1
    assert '"sim3"' in text


def _fields(text, name):
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            mm = re.search(r"(\w+)\s*(\[\d+\])?\s*$", part.strip())
            if mm and part.strip():
                names.append(mm.group(1))
    return names


def test_query_layout_matches_the_header():
    """The ctypes views list the header's fields in the header's order."""
    text = (ROOT / "include" / "orbx.h").read_text()
    assert _fields(text, "orbx_sim3_query") == [f[0] for f in ox.Sim3Query._fields_]
    assert _fields(text, "orbx_sim3_kf") == [f[0] for f in ox.Sim3Kf._fields_]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_reproduces_the_fixture(golden, s):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith(f"s{s}_")}
    kf1 = {k[4:]: g[k] for k in g if k.startswith("kf1_")}
    kf2 = {k[4:]: g[k] for k in g if k.startswith("kf2_")}
    idx1 = g["idx1"] if len(g["idx1"]) else None
    r = s3.sim3_ransac(kf1, kf2, g["matches12"], g["draws"], idx1=idx1)
    # the bit-exact layer, independent of the linear-algebra and maths libraries
    assert r["N"] == int(g["N"]) == 120
    assert r["sets"].tobytes() == g["sets"].tobytes()
    c = s3.construct(kf1, kf2, g["matches12"], idx1)
    t = s3.compute_t(c, g["sets"], q=g["q"], R=g["R"])
    assert t["T12_all"].tobytes() == g["T12_all"].tobytes() and t["T21_all"].tobytes() == g["T21_all"].tobytes()
    count, _ = s3.check_inliers(c, kf1, kf2, g["T12_all"], g["T21_all"])
    assert count.tobytes() == g["count"].tobytes()
    assert r["found_iter"] == int(g["found_iter"]) >= 0
    # the solve and the rotation: a float32 ulp
    ok = g["gap"] >= s3.CUT
    assert ok.mean() >= 0.95
    a, b = r["q"][ok], g["q"][ok]
    assert (np.abs(a - b) <= np.spacing(np.abs(b).max(1, keepdims=True).astype(F32))).all()
    assert np.abs(s3.rotation(g["q"]).astype(np.float64) - g["R"]).max() <= np.spacing(F32(1))
    assert (r["count"][ok] == g["count"][ok]).mean() >= 0.9


@pytest.mark.parametrize("i", range(len(s3.CASES)), ids=[f"N{c[0]}-it{c[1]}" for c in s3.CASES])
def test_gpu_cases_stay_inside_the_eigen_gap_cap(i):
    """The cases of tests/test_sim3_gpu.py: the cut of the solve comparison
    excludes at most 5 % of a case's iterations, by the restatement."""
    (kf1, kf2, m, d, kw), r = s3.case(i)
    N, M = s3.CASES[i][:2]
    assert r["N"] == N and len(d) == M and len(kf1["keys"]) != len(kf2["keys"])
    assert (~s3.considered(r)).sum() <= 0.05 * M
    assert len(set(kf1["keys"]["octave"])) > 1 or N < 8
