"""The numpy restatement of Optimizer::OptimizeSim3 (tests/sim3opt_numpy.py)
checked on its own, since the reference cannot be built next to the tests: the
exponential map against a matrix exponential, the numeric Jacobian against an
analytic one, convergence on a noiseless scene, the sigma2 oddity of e21, the
early exit, the decision margin of every GPU case, the committed fixtures that
pin it, and the new C symbols (no GPU)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import sim3opt_numpy as so
from test_lba_numpy import quat_matrix

ROOT = Path(__file__).resolve().parents[1]
NEW_FUNCTIONS = ["orbx_optimize_sim3", "orbx_optimize_sim3_batch", "orbx_dev_optimize_sim3"]


# --- the exponential map ----------------------------------------------------------------
def series_exp(u):
    """exp of the 4 x 4 similarity generator [[Omega + sigma I, upsilon], [0, 0]]
    by its power series."""
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 40):
        term = term @ G / k
        out = out + term
    return out


# The small-sigma branches put C = 1, A and B at their sigma -> 0 limits: exact
# to first order in sigma only, so a sigma far below 1e-12 tests them to 1e-12;
# the small-theta branches drop the higher orders in theta (measured: about
# 3e-6 theta |upsilon| in t where sigma is large): theta ~ 1e-7, and a few 1e-8
# there.
@pytest.mark.parametrize("u", [
    [2e-7, -1e-7, 3e-7, 0.3, -0.2, 0.1, 1e-14],      # |sigma| < eps, theta < eps
    [0.2, -0.3, 0.15, 0.3, -0.2, 0.1, -1e-14],       # |sigma| < eps, theta >= eps
    [2e-8, -1e-8, 3e-8, 0.3, -0.2, 0.1, 0.25],       # |sigma| >= eps, theta < eps
    [0.2, -0.3, 0.15, 0.3, -0.2, 0.1, -0.4],         # the general branch
], ids=["small-small", "small-sigma", "small-theta", "general"])
def test_exp_map_against_the_matrix_exponential(u):
    u = np.array(u)
    e = so.sim3_exp(u)
    M = np.eye(4)
    M[:3, :3] = e[7] * quat_matrix(e[:4])
    M[:3, 3] = e[4:7]
    assert np.abs(M - series_exp(u)).max() <= 1e-12
    # the constants of the Jacobian path are the exponentials
    assert abs(so.EXP_P - np.exp(1e-9)) <= np.spacing(1.0) and abs(so.EXP_M - np.exp(-1e-9)) <= np.spacing(1.0)
    assert so.EXP_P == 1.000000001 and so.EXP_M == 0.999999999   # 1 + x + x^2 / 2 rounds to these


# --- the numeric Jacobian -----------------------------------------------------------------
def analytic_jacobians(est, pb):
    """d e12 / d u and d e21 / d u for the left update S <- exp(u) S, written
    from p' = p + omega x p + upsilon + sigma p (p = S.map(P2c)) and
    q' = q - R^T (omega x P1c + upsilon + sigma P1c) / s (q = S^-1.map(P1c))."""
    R, s = quat_matrix(est[:4]), est[7]

    def dproj(cam, p):
        x, y, z = p
        return np.array([[cam[0] / z, 0, -cam[0] * x / (z * z)], [0, cam[1] / z, -cam[1] * y / (z * z)]])

    def gen(p):
        skew = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        return np.concatenate([-skew, np.eye(3), p[:, None]], 1)
    J12, J21 = [], []
    inv = so.sim3_inverse(est)
    for k in range(len(pb["idx"])):
        p = so.sim3_map(est, pb["P2"][k:k + 1])[0]
        q = so.sim3_map(inv, pb["P1"][k:k + 1])[0]
        J12.append(-dproj(pb["cam1"], p) @ gen(p))
        J21.append(dproj(pb["cam2"], q) @ (R.T @ gen(pb["P1"][k])) / s)
    return np.array(J12), np.array(J21)


def test_numeric_jacobian_against_the_analytic_one():
    kf1, kf2, m, init = so.scene(seed=77, N=50, noise=0.3)
    pb = so.build_problem(kf1, kf2, m)
    est = so.sim3_from_float(*init)
    _, _, _, err, J = so.linearize(est, pb)
    J = J.reshape(-1, 2, 2, 7)
    A12, A21 = analytic_jacobians(est, pb)
    # the projected coordinate carries a rounding error of about an ulp; the
    # central difference divides two of them by 2 delta
    coord = max(np.abs(pb["obs1"]).max(), np.abs(pb["obs2"]).max(), np.abs(err).max())
    bound = 8 * np.spacing(coord) / (2 * so.DELTA)
    worst = max(np.abs(J[:, 0] - A12).max(), np.abs(J[:, 1] - A21).max())
    print(f"numeric - analytic: worst {worst:.3e}, bound {bound:.3e}, largest entry {np.abs(A12).max():.1f}")
    assert worst <= bound
    assert np.abs(A12).max() > 100 and np.abs(A21).max() > 100


# --- whole runs -----------------------------------------------------------------------------
def test_noiseless_scene_converges_to_the_true_sim3():
    kf1, kf2, m, init = so.scene(seed=78, N=60, noise=0.0, start=0.03)
    r = so.optimize_sim3(kf1, kf2, m, *init)
    true = so.true_sim3()
    assert np.abs(so.sim3_from_float(*init) - true).max() > 1e-2
    err = np.abs(r["est"] - true).max()
    print(f"|estimate - truth| {err:.2e} after {r['iterations']} iterations")
    assert err <= 1e-6
    assert r["n_corr"] == 60 and r["n_bad"] == 0 and r["n_in"] == 60 and not r["returned_early"]
    assert np.array_equal(r["matches12"], m)


def test_e21_information_is_sigma2_not_its_inverse():
    """A pair at the top octave whose KF2 observation is a pixel off: under
    sigma2 (what src/Optimizer.cc:912 reads) its e21 chi2 is about 1.2^14 > 10
    and the pair is removed; under the inverse it would be about 0.08 and kept."""
    kf1, kf2, m, init = so.scene(seed=79, N=30, noise=0.0, start=0.01, octaves=so.NLEVELS - 1)
    pb = so.build_problem(kf1, kf2, m)
    i = int(pb["idx"][4])
    kf2["keys"]["x"][m[i]] += 1.0
    r = so.optimize_sim3(kf1, kf2, m, *init)
    k = int(np.nonzero(r["problem"]["idx"] == i)[0][0])
    assert r["matches12"][i] == -1 and r["n_bad"] == 1 and r["n_in"] == 29
    assert 10 < r["chi2"][0][k][1] < 1.3 * so.SIGMA2[-1] and r["chi2"][0][k][0] < 1
    inv = so.optimize_sim3(kf1, kf2, m, *init, sigma_inverse=True)
    assert inv["matches12"][i] == m[i] and inv["n_bad"] == 0 and inv["n_in"] == 30
    assert inv["chi2"][1][k][1] < 1.3 / so.SIGMA2[-1]


def test_early_exit_returns_zero_and_leaves_the_sim3():
    (kf1, kf2, m, init), r = so.case("n12_gross3")
    assert r["n_corr"] == 12 and r["n_bad"] == 3 and r["returned_early"] == 1 and r["n_in"] == 0
    assert r["iterations"][1] == 0
    assert np.array_equal(r["est"], so.sim3_from_float(*init))
    cleared = np.nonzero(r["matches12"] != m)[0]
    assert len(cleared) == 3 and (r["matches12"][cleared] == -1).all() and (m[cleared] >= 0).all()
    # skipped entries are left set: invalid on either side, not observed
    skipped = np.setdiff1d(np.nonzero(m != -1)[0], r["problem"]["idx"])
    assert len(skipped) == 3 + 3 + 2 and np.array_equal(r["matches12"][skipped], m[skipped])
    assert (m[skipped] <= so.NOT_OBSERVED).sum() == 2


EXPECT = {   # name: (returned_early, n_bad > 0, a second round ran)
    "n0": (1, False, False), "n9": (1, False, False), "n10": (0, False, True), "n12_gross3": (1, True, False),
    "n40_gross": (0, True, True), "n64": (0, True, True), "n65": (0, True, True), "n130_clean": (0, False, True),
    "n257": (0, True, True), "n4000": (0, True, True), "behind": (0, True, True)}


@pytest.mark.parametrize("name", list(so.CASES))
def test_gpu_cases_take_their_paths_with_a_decision_margin(name):
    """Every case of tests/test_sim3opt_gpu.py takes the path it is there for,
    and every stored chi2 at both checks lies outside th2 (1 +- 1e-3): a
    condition on the inputs (the seeds), not on the code under test."""
    (kf1, kf2, m, init), r = so.case(name)
    early, bad, second = EXPECT[name]
    assert r["n_corr"] == so.CASES[name][0]
    assert r["returned_early"] == early and (r["n_bad"] > 0) == bad and (r["iterations"][1] > 0) == second
    assert len(kf1["keys"]) != len(kf2["keys"]) and len(kf1["keys"]) <= 4096
    assert so.MARGIN == 1e-3 and so.margin_ok(r)
    if name == "behind":   # a mapped depth is negative, and g2o projects it all the same
        z = so.sim3_map(so.sim3_from_float(*init), r["problem"]["P2"])[:, 2]
        assert (z < 0).sum() == 2
    if name == "n4000":
        assert len(kf1["keys"]) > 4000
    if second and bad:
        assert r["iterations"][1] <= 10
    elif second:
        assert r["iterations"][1] <= 5


# --- the fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", so.GOLDEN)
def test_restatement_reproduces_the_fixture(name):
    path = ROOT / "tests" / "golden" / f"sim3opt_{name}.npz"
    assert path.stat().st_size < 1 << 20
    g = np.load(path)
    kf1 = {k[4:]: g[k] for k in g.files if k.startswith("kf1_")}
    kf2 = {k[4:]: g[k] for k in g.files if k.startswith("kf2_")}
    # the bit-exact layer: every linearisation at the recorded estimate
    pb = so.build_problem(kf1, kf2, g["matches12"])
    bad = np.zeros(len(pb["idx"]), bool)
    for k in range(len(g["log_est"])):
        if k == int(g["iterations"][0]):
            c = g["chi2"][0]
            bad = (c[:, 0] > so.TH2) | (c[:, 1] > so.TH2)
        pb["active"] = ~bad
        chi, h, b, _, _ = so.linearize(g["log_est"][k], pb)
        assert np.float64(chi).tobytes() == g["log_chi2"][k].tobytes()
        assert h.tobytes() == g["log_H"][k].tobytes() and b.tobytes() == g["log_b"][k].tobytes()
    # the whole run
    r = so.optimize_sim3(kf1, kf2, g["matches12"], g["R12"], g["t12"], g["s12"])
    for k in ("n_in", "n_corr", "n_bad", "returned_early"):
        assert r[k] == int(g[k]), k
    assert r["matches12"].tobytes() == g["out_matches12"].tobytes()
    assert list(r["iterations"]) == g["iterations"].tolist() and list(r["trials"]) == g["trials"].tolist()
    assert r["est"].tobytes() == g["est"].tobytes()
    assert r["chi2"].tobytes() == g["chi2"].tobytes()


# --- the C side -----------------------------------------------------------------------------------
def test_header_and_library_have_the_new_entry_points():
    """Fails on the parent commit: the functions do not exist there."""
    text = (ROOT / "include" / "orbx.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\}\s*orbx_sim3_opt_query\s*;", code)
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 11
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 11
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    assert '"sim3opt"' in text


def test_argument_refusals_need_no_device():
    lib = ox.lib()
    q = ox.Sim3OptQuery()
    assert lib.orbx_optimize_sim3(None, ctypes.byref(q)) == -1
    assert lib.orbx_optimize_sim3_batch(None, 1, ctypes.byref(q)) == -1
    assert lib.orbx_dev_optimize_sim3(None, 0, None, None, 1, None, None, None) == -1


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
    assert _fields(text, "orbx_sim3_opt_query") == [f[0] for f in ox.Sim3OptQuery._fields_]
    assert f"#define ORBX_SIM3_OPT_MAX_LM {ox.SIM3_OPT_MAX_LM}" in text
    assert f"#define ORBX_SIM3_OPT_MAX_TRIALS {ox.SIM3_OPT_MAX_TRIALS}" in text
