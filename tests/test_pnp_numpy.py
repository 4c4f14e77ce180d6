"""The numpy restatement of PnPsolver (tests/pnp_numpy.py) checked on its
own: SetRansacParameters' values, the draw quirk by hand and by enumeration,
the loop's or, resumption after a returned pose, a noise-free scene, the
committed fixture that pins it, and the new C symbols (no GPU)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import pnp_numpy as pn

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "pnp_ransac.npz"
NEW_FUNCTIONS = ["orbx_pnp_ransac", "orbx_pnp_ransac_batch", "orbx_dev_pnp_candidates"]
# A noise-free scene: the largest |Tcw - ground truth| entry the restatement
# gives on the eight scenes of test_noise_free_scene_returns_the_ground_truth
# is 2.7e-8 (rotation) and 1.55e-7 (translation): float32 inputs through an
# FP64 solve, the pose rounded to float32.  The bounds are four times that
# (the rotation's is one float32 ulp of 1).
TOL_R, TOL_T = 1.2e-7, 6.2e-7


def at(pos, size):
    """A rand() value that RandomInt maps to `pos` of `size`."""
    r = int((pos + 0.5) / size * 2**31)
    assert int((float(r) / 2147483648.0) * size) == pos
    return r


def draws_at(N, picks):
    return [at(p, N - j) for j, p in enumerate(picks)]


def test_set_ransac_parameters_values():
    """Relocalisation's call (Tracking.cc:923) at N = 20: 10 and 35."""
    assert pn.ransac_parameters(20, 0.99, 10, 300, 4, 0.5) == (10, 35)
    assert pn.ransac_parameters(20) == (8, 70)                    # the defaults: epsilon 0.4 -> ceil(69.6)
    assert pn.ransac_parameters(100, 0.99, 10, 300, 4, 0.5) == (50, 35)
    assert pn.ransac_parameters(10, 0.99, 10, 300, 4, 0.5) == (10, 1)     # min == N: one iteration
    assert pn.ransac_parameters(9, 0.99, 10, 300, 4, 0.5) == (10, 0)      # N < min: nothing runs
    assert pn.ransac_parameters(30, 0.99, 2, 300, 4, 0.0) == (4, 300)     # min_set bounds it below; the cap above
    assert pn.ransac_parameters(7, 0.99, 1, 300, 4, 0.99)[0] == 6         # float 7 * 0.99f = 6.93 truncated


def test_draw_quirk_by_hand():
    """10 correspondences.  The removal is buf[idx] = back; pop_back with the
    drawn value idx as the position.
    Places 5, 5, 5, 0:
      size 10  randi 5 -> 5   buf[5] = 9        [0 1 2 3 4 9 6 7 8]
      size 9   randi 5 -> 9   buf[9] = buf[8]   the write lands past the live part; place 5 keeps its 9
      size 8   randi 5 -> 9   the same correspondence again
      size 7   randi 0 -> 0
    Places 9, 8, 7, 6: the back each time, nothing moves."""
    assert pn.draw_set(10, draws_at(10, (5, 5, 5, 0))) == [5, 9, 9, 0]
    assert pn.draw_set(10, draws_at(10, (5, 5, 5, 5))) == [5, 9, 9, 9]
    assert pn.draw_set(10, draws_at(10, (9, 8, 7, 6))) == [9, 8, 7, 6]
    assert pn.draw_set(10, draws_at(10, (2, 7, 2, 2))) == [2, 7, 9, 9]


def quirk_counts(N):
    """(sets with a repeated correspondence, sets with one three times, all sets)."""
    twice = thrice = total = 0
    for r1 in range(N):
        for r2 in range(N - 1):
            for r3 in range(N - 2):
                for r4 in range(N - 3):
                    st = pn.draw_set(N, draws_at(N, (r1, r2, r3, r4)))
                    assert all(0 <= x < N for x in st)
                    top = max(st.count(x) for x in st)
                    total += 1
                    twice += top >= 2
                    thrice += top >= 3
                    assert top <= 3 and len(set(st)) >= 2
    return twice, thrice, total


@pytest.mark.parametrize("N", [4, 5, 6, 8, 11])
def test_draw_quirk_by_enumeration(N):
    """Every outcome of the four positions: of the N (N - 1) (N - 2) (N - 3)
    outcomes (4 N - 7) (N - 3) repeat a correspondence (9 of 24 at N = 4, 26
    of 120 at 5, 125 of 1680 at 8, 296 of 7920 at 11), N - 3 of them hold one
    three times, none four times."""
    assert quirk_counts(N) == ((4 * N - 7) * (N - 3), N - 3, N * (N - 1) * (N - 2) * (N - 3))


def test_the_loop_is_an_or():
    """A fresh iterate(5) with no success runs ransac_max_its iterations,
    not five; on the exhausted solver a further iterate(5) runs five more."""
    sc = pn.scene(30, seed=3, noise=0.5, outliers=1.0)          # every partner unrelated
    s = pn.solver_of(sc, pn.RELOC)
    assert (s.min_inliers, s.max_its) == (15, 35)
    d = pn.draws_for(3, 60)
    r = s.iterate(5, d)
    assert r["iters_run"] == 35 and r["no_more"] == 1 and not r["found"] and r["iter_done"] == 35
    r = s.iterate(5, d[35:])
    assert r["iters_run"] == 5 and r["no_more"] == 1 and r["iter_done"] == 40


def test_resumption_returns_the_same_pose_again():
    """After a returned pose (whose PoseOptimization, say, failed) the next
    call refits the set it came in with: the same pose at the next iteration
    with count >= min, whatever that iteration's own count."""
    sc = pn.scene(100, seed=5, noise=0.5)
    s = pn.solver_of(sc, pn.RELOC)
    d = pn.draws_for(5, 400)
    a = s.iterate(5, d)
    assert a["found"] and a["refined"] and a["no_more"] == 0
    b = s.iterate(5, d[a["iters_run"]:])
    assert b["found"] and b["refined"]
    counts = s.taps["count"]
    assert counts[b["found_iter"]] >= s.min_inliers and all(c < s.min_inliers for c in counts[:b["found_iter"]])
    if b["best_slot"] == 0:                                     # no new record: the incoming set was refitted
        assert b["Tcw"].tobytes() == a["Tcw"].tobytes() and b["inliers"].tobytes() == a["inliers"].tobytes()
    # driven like Relocalisation until bNoMore
    o, calls = a["iters_run"] + b["iters_run"], 2
    while not b["no_more"]:
        b = s.iterate(5, d[o:])
        o += b["iters_run"]
        calls += 1
        assert calls < 100
    assert b["iter_done"] == o >= s.max_its


@pytest.mark.parametrize("seed", range(8))
def test_noise_free_scene_returns_the_ground_truth(seed):
    """Without pixel noise the call returns the ground-truth pose with every
    true correspondence as an inlier, from a set without an unrelated
    partner: the first one that EPnP *solves*.  Four exact points do not
    always do (the four-dimensional null space leaves gauss_newton's five
    steps in a wrong minimum, reprojection errors of tens of pixels: the first
    clean set of seeds 0, 3, 5 and 6 here); such a set
    counts below min_inliers and returns nothing, like a set with an
    unrelated partner."""
    sc = pn.scene(60, seed=40 + seed, noise=0.0, outliers=0.3)
    s = pn.solver_of(sc, pn.RELOC)
    r = s.iterate(5, pn.draws_for(40 + seed, 300))
    assert r["found"] and r["refined"]
    good = np.ones(len(sc["keys"]), bool)
    good[sc["bad"]] = False
    n_good = int(good[s.c["kp_index"]].sum())
    clean = [all(good[s.c["kp_index"][i]] for i in st) and len(set(st)) == 4 for st in s.taps["sets"]]
    counts = s.taps["count"]
    assert clean[r["found_iter"]] and counts[r["found_iter"]] >= s.min_inliers
    assert all(c < s.min_inliers for c in counts[:r["found_iter"]])
    T = r["Tcw"].reshape(4, 4).astype(np.float64)
    eR, et = np.abs(T[:3, :3] - sc["R"]).max(), np.abs(T[:3, 3] - sc["t"]).max()
    print(f"seed {seed}: first clean set {clean.index(True)}, returned at {r['found_iter']}, |dR| {eR:.2e} |dt| {et:.2e}")
    assert eR <= TOL_R and et <= TOL_T
    assert r["n_inliers"] == n_good


def test_header_and_library_have_the_new_entry_points():
    """Fails on the parent commit: the functions do not exist there."""
    text = (ROOT / "include" / "orbx.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\}\s*orbx_pnp_query\s*;", code)
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 10
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 10
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    q = ctypes.byref(ox.PnpQuery())
    assert lib.orbx_pnp_ransac(None, q) == -1
    assert lib.orbx_pnp_ransac_batch(None, 1, q) == -1
    assert lib.orbx_dev_pnp_candidates(None, 0, 1, None, None, None, None, 8, 0.75, 1, 15, None, 0, None, None,
                                       None) == -1
    assert '"pnp"' in text
    assert int(re.search(r"#define ORBX_PNP_REC (\d+)", text).group(1)) == pn.REC == ox.PNP_REC
    assert int(re.search(r"#define ORBX_PNP_DEC (\d+)", text).group(1)) == pn.DEC


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
    """The ctypes view lists the header's fields in the header's order."""
    text = (ROOT / "include" / "orbx.h").read_text()
    assert _fields(text, "orbx_pnp_query") == [f[0] for f in ox.PnpQuery._fields_]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("s", range(len(pn.GOLDEN_SCENES)))
def test_restatement_reproduces_the_fixture(golden, s):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith(f"s{s}_")}
    sc = {k: g[k] for k in ("keys", "pos", "valid", "cam", "sigma2")}
    # the bit-exact layer, independent of the linear-algebra library: fed the fixture's decompositions
    records = {("it", i): g["rec"][i] for i in range(len(g["rec"]))}
    records.update({("refit", int(k)): g["refit_rec"][j] for j, k in enumerate(g["refit_slots"])})
    sol = pn.solver_of(sc, pn.RELOC, pn.TapDecomp(records))
    out = sol.iterate(5, g["draws"])
    assert np.array(sol.taps["sets"], np.int32).tobytes() == g["sets"].tobytes()
    assert np.array(sol.taps["rec"]).tobytes() == g["rec"].tobytes()
    assert np.array(sol.taps["count"], np.int32).tobytes() == g["count"].tobytes()
    for j, k in enumerate(g["refit_slots"]):
        rec, cnt = sol.taps["refits"][int(k)]
        assert rec.tobytes() == g["refit_rec"][j].tobytes() and cnt == g["refit_count"][j]
    for k in ("N", "ransac_min_inliers", "ransac_max_its", "iters_run", "no_more", "found", "found_iter", "n_inliers",
              "refined", "iter_done", "best_inliers", "best_slot"):
        assert out[k] == int(g[k]), k
    for k in ("Tcw", "inliers", "best_mask", "best_Tcw"):
        assert np.asarray(out[k]).tobytes() == g[k].tobytes(), k
    assert out["found"] and out["refined"]
    # with this machine's np.linalg: the same decisions, the pose within float32 round-off of the fixture's
    _, _, sol2, out2 = pn.golden_run(s)
    assert out2["found_iter"] == out["found_iter"] and out2["n_inliers"] == out["n_inliers"]
    assert np.abs(out2["Tcw"] - g["Tcw"]).max() <= 1e-4
