"""The numpy restatement of ReconstructF / ReconstructH
(tests/reconstruct_numpy.py) checked on its own: known motions, every accept
and reject branch, the invariance to the SVD's unspecified signs, the
committed fixture, the constructed match on which the fp-contract modes
differ, the conditioning cut of the GPU test, and the new C symbols (no GPU)."""
import re
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import reconstruct_numpy as rn

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "init_reconstruct.npz"
NEW_FUNCTIONS = ["orbx_init_reconstruct", "orbx_init_reconstruct_batch", "orbx_dev_init_reconstruct",
                 "orbx_dev_read_init_reconstruct"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def angle_deg(a, b):
    c = np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


def rotation_angle_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("name", ["F-300", "F-65", "H-300", "H-65"])
def test_known_motion_is_recovered(name):
    """R within 1 degree, t up to scale within 3 degrees of direction, the
    points in front of both cameras and on the scene's rays."""
    a, r = rn.case(name)
    truth = a[7]
    assert r["ok"] == 1 and r["best"] >= 0
    R = r["R21"].astype(np.float64).reshape(3, 3)
    t = r["t21"].astype(np.float64)
    assert rotation_angle_deg(R, truth["R"]) < 1.0
    assert angle_deg(t, truth["t"]) < 3.0
    tri = r["triangulated"].astype(bool)
    assert tri.sum() >= 0.9 * r["N"]
    X = r["p3d"][tri].astype(np.float64)
    assert np.all(X[:, 2] > 0) and np.all((X @ R.T + t)[:, 2] > 0)
    scale = np.linalg.norm(truth["t"])      # |t21| = 1
    rel = np.linalg.norm(X * scale - truth["X"][tri], axis=1) / np.linalg.norm(truth["X"][tri], axis=1)
    assert np.median(rel) < 0.1
    # untouched keypoints
    unmatched = a[2] < 0
    assert not r["p3d"][unmatched].any() and not r["triangulated"][unmatched].any()


@pytest.mark.parametrize("name", sorted(rn.CASES))
def test_every_case_decides_as_pinned(name):
    """Each accept and reject branch has a case, confirmed by the float32
    restatement."""
    a, r = rn.case(name)
    assert r["ok"] == rn.CASES[name]["ok"], (r["n_good"], r["parallax"])
    assert (r["best"] >= 0) == bool(r["ok"])
    if not r["ok"]:
        assert r["R21"] is None and not r["p3d"].any() and not r["triangulated"].any()


def test_reject_branches_are_the_intended_ones():
    g = {n: rn.case(n)[1] for n in rn.CASES}
    nh = lambda r: r["n_good"][:r["n_hyp"]]
    # F: pure rotation -- two hypotheses alike (nsimilar > 1, :515)
    r = g["F-rotation"]
    assert np.count_nonzero(nh(r) > 0.7 * nh(r).max()) > 1
    # F: a clear winner with every point but too little parallax (:523)
    r = g["F-parallax"]
    assert np.count_nonzero(nh(r) > 0.7 * nh(r).max()) == 1 and nh(r).max() == r["n_inliers"] >= 50
    assert 0 < r["parallax"][int(np.argmax(nh(r)))] <= 1.0
    # F: fewer than 50 good points; fewer than 0.9 N
    assert g["F-few"]["n_good"].max() < 50 and g["F-few"]["parallax"].max() > 1.0
    r = g["F-noisy"]
    assert 50 <= nh(r).max() < int(0.9 * r["n_inliers"])
    # H: the second-best rule (:719), on init_numpy.scene's plane
    for n in ("H-ambiguous", "H-ambiguous-65"):
        s = np.sort(nh(g[n]))[::-1]
        assert s[1] >= 0.75 * s[0] and s[0] > 50 and s[0] > 0.9 * g[n]["n_inliers"]
    s = np.sort(nh(g["H-300"]))[::-1]
    assert (s[0], s[1]) == (300, 206)
    s = np.sort(nh(g["H-65"]))[::-1]
    assert s[0] == 65 and s[1] < 0.75 * 65
    # H: parallax below the caller's minimum; fewer than 50; the d1/d2 return
    r = g["H-parallax"]
    s = np.sort(nh(r))[::-1]
    assert s[1] < 0.75 * s[0] and r["parallax"][int(np.argmax(nh(r)))] < 8.0
    assert g["H-few"]["n_good"].max() == 40
    assert g["H-rotation"]["n_hyp"] == 0
    # identity homography: the early return
    a = rn.case_inputs("H-65")
    r = rn.reconstruct(*a[:4], 0, np.eye(3, dtype=np.float32).reshape(9), rn.CAM)
    assert r["n_hyp"] == 0 and r["ok"] == 0


@pytest.mark.parametrize("name", ["F-65", "H-65", "H-ambiguous-65", "F-noisy"])
def test_svd_sign_invariance(name):
    """Negating singular pairs (a column of U with the row of Vt) permutes
    the hypotheses and leaves the outcome unchanged."""
    a, r = rn.case(name)
    S = r["svd"]
    for flip in ((0,), (1,), (2,), (0, 1), (0, 2), (0, 1, 2)):
        T = S.copy()
        for k in flip:
            T[k:9:3] = -T[k:9:3]
            T[12 + 3 * k:15 + 3 * k] = -T[12 + 3 * k:15 + 3 * k]
        q = rn.reconstruct(*a[:7], svd=T, **a[8])
        assert q["ok"] == r["ok"] and q["n_hyp"] == r["n_hyp"]
        assert sorted(q["n_good"].tolist()) == sorted(r["n_good"].tolist())
        assert q["p3d"].tobytes() == r["p3d"].tobytes() and q["triangulated"].tobytes() == r["triangulated"].tobytes()
        if r["ok"]:
            assert q["R21"].tobytes() == r["R21"].tobytes() and q["t21"].tobytes() == r["t21"].tobytes()


@pytest.mark.parametrize("contract", [0, 1])
def test_restatement_reproduces_the_fixture(golden, contract):
    """Fed the recorded decompositions, the restatement gives the recorded
    bytes; on its own (np.linalg.svd) the recorded decisions."""
    G = golden
    for tag, model, *_ in rn.GOLDEN_CASES:
        args = (G[f"{tag}_keys1"], G[f"{tag}_keys2"], G[f"{tag}_matches12"], G[f"{tag}_inliers"], int(G[f"{tag}_model"]),
                G[f"{tag}_M21"], G["cam"])
        c = contract
        r = rn.reconstruct(*args, svd=G[f"{tag}_svd{c}"], v4=G[f"{tag}_v4{c}"], contract=c)
        assert G[f"{tag}_ok{c}"] == 1
        for name in ("ok", "n_inliers", "n_hyp", "best"):
            assert r[name] == int(G[f"{tag}_{name}{c}"]), name
        for name in ("n_good", "parallax", "p3d", "triangulated", "R_all", "t_all", "cos_parallax"):
            assert np.asarray(r[name]).tobytes() == G[f"{tag}_{name}{c}"].tobytes(), (tag, name)
        assert r["R21"].tobytes() == G[f"{tag}_R21{c}"].tobytes() and r["t21"].tobytes() == G[f"{tag}_t21{c}"].tobytes()
        # non-inlier matches: no null vector, no point
        out = G[f"{tag}_inliers"] == 0
        assert out.any() and not r["v4"][:, out].any() and np.isnan(r["cos_parallax"][:, out]).all()
        free = rn.reconstruct(*args, contract=c)
        assert free["ok"] == r["ok"] and free["n_hyp"] == r["n_hyp"]
        assert sorted(free["n_good"].tolist()) == sorted(r["n_good"].tolist())


def test_contract_modes_differ_on_the_constructed_match(golden):
    """One match whose frame-2 keypoint sits where the reprojection error as
    written and as fma(fy*y, invZ, cy), fma(ex, ex, ey*ey) fall on different
    sides of th2: the winning hypothesis counts it in one mode only."""
    G = golden
    args = (G["f_keys1"], G["f_keys2"], G["f_matches12"], G["f_inliers"], 1, G["f_M21"], G["cam"])
    built = rn.contract_case()
    assert built[1].tobytes() == G["f_keys2"].tobytes() and built[3].tobytes() == G["f_inliers"].tobytes()
    got = []
    for c in (0, 1):
        r = rn.reconstruct(*args, svd=G["f_svd"], v4=G[f"f_v4{c}"], contract=c)
        assert r["n_good"].tobytes() == G[f"f_n_good{c}"].tobytes()
        assert r["cos_parallax"].tobytes() == G[f"f_cos_parallax{c}"].tobytes()
        got.append(r["n_good"])
    assert G["f_inliers"].sum() == 1
    assert got[0].sum() != got[1].sum() and {int(got[0].max()), int(got[1].max())} == {0, 1}


def test_conditioning_cut_leaves_out_few_solves():
    """The GPU test compares the device's null vectors with a float64 SVD
    where (s3 - s4) / s1 >= CUT; that leaves out at most 5 % of a case's
    solves."""
    for name in rn.CASES:
        _, r = rn.case(name)
        gap = r["gap"][~np.isnan(r["gap"])] if r["n_hyp"] else np.zeros(0)
        if len(gap):
            assert np.count_nonzero(gap < rn.CUT) <= 0.05 * len(gap), name


def test_fmaf_is_exact_elementwise():
    from fractions import Fraction
    rng = np.random.default_rng(2)
    a = rng.normal(0, 3, 300).astype(np.float32)
    b = rng.normal(0, 3, 300).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(0, 1e-7, 300))).astype(np.float32)
    got = rn.fmaf(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        err = abs(Fraction(float(g)) - exact)
        for other in (np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))):
            assert err <= abs(Fraction(float(other)) - exact)


def test_header_declares_abi_8():
    text = (ROOT / "include" / "orbx.h").read_text()
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 8
    assert "orbx_reconstruct_query" in text
    for fn in NEW_FUNCTIONS:
        assert re.search(rf"\bint {fn}\(orbx_ctx\* ctx,", text), fn
        assert hasattr(ox.lib(), fn), fn
    assert ox.lib().orbx_abi_version() >= 8
    # argument rules that need no device
    assert ox.lib().orbx_init_reconstruct(None, None) == -1
    assert ox.lib().orbx_dev_init_reconstruct(None, 0, 1, 1, None, 0.4, 1.0, 50) == -1
    assert ox.lib().orbx_dev_read_init_reconstruct(None, 0, None, None) == -1
