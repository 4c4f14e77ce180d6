"""The numpy restatement of CreateNewMapPoints' triangulation and loop
(tests/newpoints_numpy.py) checked on its own: the committed fixture that pins
it, the coverage of that fixture, the geometry of a noise-free scene, and the
new C symbols and adapter (no GPU)."""
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import newpoints_numpy as npn
import orb_slam_amd as ox

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "new_points.npz"
NEW_FUNCTIONS = ["orbx_triangulate_matches", "orbx_create_new_map_points", "orbx_dev_create_new_map_points"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def gates_case(golden):
    return npn.unpack(golden, "g_", npn.GATES_CASE["n"])


@pytest.fixture(scope="module")
def chain_case(golden):
    return npn.unpack(golden, "c_", npn.CHAIN_CASE["n"])


def ulp_of_largest(v):
    return np.spacing(np.abs(v).max(axis=-1).astype(np.float32))


def assert_solves_agree(v_a, v_b):
    """Two accurate null vectors of a well-separated A differ in the final
    rounding only: after sign alignment, within one float32 ulp of the
    vector's largest entry."""
    sign = np.sign(np.sum(v_a.astype(np.float64) * v_b.astype(np.float64), axis=-1, keepdims=True))
    d = np.abs(v_a.astype(np.float64) - sign * v_b.astype(np.float64)).max(axis=-1)
    assert np.all(d <= ulp_of_largest(v_b)), d.max()


@pytest.mark.parametrize("contract", [0, 1])
def test_gates_reproduce_the_fixture(golden, gates_case, contract):
    """Fed the recorded null vectors, the gates give the recorded status and
    xyz bytes in both fp-contract modes.  (No match of these scenes decides
    differently in the two modes; test_contract_modes_differ_on_the_edited_
    matches has matches that do.)"""
    S = gates_case
    for k in range(npn.GATES_CASE["n"]):
        r = npn.triangulate(S["keys1"], S["g1"], S["keys2"][k], S["g2"][k], S["truth"][k], v4=golden[f"g_v4_{k}"],
                            contract=contract)
        assert r["status"].tobytes() == golden[f"g_status{contract}_{k}"].tobytes()
        assert r["xyz"].tobytes() == golden[f"g_xyz{contract}_{k}"].tobytes()


def test_svd_agrees_with_the_recorded_null_vectors(golden, gates_case):
    S = gates_case
    for k in range(npn.GATES_CASE["n"]):
        r = npn.triangulate(S["keys1"], S["g1"], S["keys2"][k], S["g2"][k], S["truth"][k])
        ran = ~np.isnan(r["gap"])
        assert np.array_equal(ran, (r["status"] != 0) & (r["status"] != 2))
        assert np.all(r["gap"][ran] >= 1e-4)      # every solve of the fixture is above the GPU test's cut
        assert_solves_agree(r["v4"][ran], golden[f"g_v4_{k}"][ran])


def test_fixture_holds_every_reachable_status(golden):
    """Status 3 and 8 need an exact zero out of the solve; every other value
    occurs, and no other does."""
    st = np.concatenate([golden[f"g_status0_{k}"] for k in range(npn.GATES_CASE["n"])])
    assert set(np.unique(st).tolist()) == {0, 1, 2, 4, 5, 6, 7, 9}


@pytest.mark.parametrize("chain", [0, 1])
def test_loop_reproduces_the_fixture(golden, chain_case, chain):
    n = npn.CHAIN_CASE["n"]
    res = npn.replay(chain_case, chain, v4s=[golden[f"c_v4{chain}_{k}"] for k in range(n)])
    for k, r in enumerate(res):
        assert r["matches12"].tobytes() == golden[f"c_matches12{chain}_{k}"].tobytes(), k
        assert r["status"].tobytes() == golden[f"c_status{chain}_{k}"].tobytes(), k
        assert r["xyz"].tobytes() == golden[f"c_xyz{chain}_{k}"].tobytes(), k


def test_chained_loop_differs_from_the_unchained_one(golden):
    """Neighbour 0 is the same; later neighbours lose the keypoints that got
    a point, and some of the candidates they leave go to other keypoints,
    which become points too."""
    n = npn.CHAIN_CASE["n"]
    m0 = [golden[f"c_matches120_{k}"] for k in range(n)]
    m1 = [golden[f"c_matches121_{k}"] for k in range(n)]
    assert np.array_equal(m0[0], m1[0])
    created = golden["c_status1_0"] == 1
    assert created.sum() > 50
    assert np.all(m1[1][created] == -1) and np.any(m0[1][created] >= 0)
    freed = (m1[1] >= 0) & (m1[1] != m0[1])
    assert freed.sum() >= 3
    assert np.count_nonzero(golden["c_status1_1"][freed] == 1) >= 1


def test_contract_modes_differ_on_the_edited_matches(golden):
    """Three matches whose KF2 keypoint sits where fx*x*invz+cx and
    errX*errX+errY*errY as written and as fma(fx*x, invz, cx),
    fma(errX, errX, errY*errY) fall on different sides of 5.991 sigma2: every
    one has another status in mode 1 than in mode 0, and a created point
    occurs in either mode."""
    keys1, g1, keys2, g2, m = npn.unpack_contract(golden)
    st = []
    for c in (0, 1):
        r = npn.triangulate(keys1, g1, keys2, g2, m, v4=golden["f_v4"], contract=c)
        assert r["status"].tobytes() == golden[f"f_status{c}"].tobytes()
        assert r["xyz"].tobytes() == golden[f"f_xyz{c}"].tobytes()
        st.append(r["status"])
    assert np.all(st[0] != st[1]) and 1 in st[0] and 1 in st[1]
    assert set(st[0].tolist()) | set(st[1].tolist()) <= {1, 6, 7}
    r = npn.triangulate(keys1, g1, keys2, g2, m)
    assert_solves_agree(r["v4"], golden["f_v4"])


def test_fmaf_is_exact():
    rng = np.random.default_rng(1)
    a = rng.normal(0, 3, 400).astype(np.float32)
    b = rng.normal(0, 3, 400).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(0, 1e-7, 400))).astype(np.float32)
    c[::3] = rng.normal(0, 3, len(c[::3])).astype(np.float32)
    for x, y, z in zip(a, b, c):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        got = npn.fmaf(x, y, z)
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)


def test_noise_free_scene_triangulates_the_points():
    S = npn.scene(21, 120, 2, noise=0.0, dup_frac=0.0, far_frac=0.0, bad_octave=0.0, wrong_frac=0.0, outlier_frac=0.0)
    for k in range(2):
        r = npn.triangulate(S["keys1"], S["g1"], S["keys2"][k], S["g2"][k], S["truth"][k])
        m = S["truth"][k] >= 0
        assert m.sum() > 50 and np.all(r["status"][m] == 1) and np.all(r["status"][~m] == 0)
        # both projections of the point land on the keypoints
        for g, keys, idx in ((S["g1"], S["keys1"], np.flatnonzero(m)), (S["g2"][k], S["keys2"][k], S["truth"][k][m])):
            uv, z = npn._project(g, r["xyz"][m].astype(np.float64))
            assert np.all(z > 0)
            assert np.abs(uv - np.stack([keys["x"][idx], keys["y"][idx]], 1)).max() < 2e-2


def test_a_point_behind_the_first_camera_is_status_4():
    """Hand-made: two cameras 1 m apart along x looking down z; the keypoint
    pair has the disparity of a point at z = -4 (u2 > u1 where a point in
    front gives u2 < u1)."""
    g1 = npn.make_geom(np.eye(3), [0, 0, 0])
    g2 = npn.make_geom(np.eye(3), [-1.0, 0, 0])
    k1 = npn.make_keys(np.array([[320.0, 240.0]], np.float32), [0])
    k2 = npn.make_keys(np.array([[320.0 + 125.0, 240.0]], np.float32), [0])
    st, x, v4, gap = npn.gates(g1, g2, k1[0], k2[0])
    assert st == 4
    k2["x"] = 320.0 - 125.0
    st, x, v4, gap = npn.gates(g1, g2, k1[0], k2[0])
    assert st == 1 and np.allclose(x, [0, 0, 4], atol=1e-4)
    k2["octave"] = 4          # 1.2^4 > 1.5 * 1.2: the scale gate
    assert npn.gates(g1, g2, k1[0], k2[0])[0] == 9
    k2["octave"], k2["y"] = 0, 240.0 + 8.0
    assert npn.gates(g1, g2, k1[0], k2[0])[0] == 6
    k2["x"], k2["y"] = 320.0 - 0.01, 240.0   # a point 50 km away: no parallax
    assert npn.gates(g1, g2, k1[0], k2[0])[0] == 2


def test_header_declares_abi_7():
    text = (ROOT / "include" / "orbx.h").read_text()
    assert int(re.search(r"#define ORBX_ABI_VERSION (\d+)", text).group(1)) >= 7
    for fn in NEW_FUNCTIONS:
        assert re.search(rf"\bint {fn}\(orbx_ctx\* ctx,", text), fn
    assert "orbx_kf_geom" in text
    for fn in NEW_FUNCTIONS:
        assert hasattr(ox.lib(), fn), fn
    assert ox.lib().orbx_abi_version() >= 7


ADAPTER_PROGRAM = r"""
#include <cstdio>
#include "orbx_adapters.hpp"
using namespace ORB_SLAM_AMD;
int main()
{
    const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Ow[3] = {0, 0, 0};
    std::vector<float> sf = {1.f, 1.2f}, s2 = {1.f, 1.44f};
    KeyFrameGeom g(R, t, Ow, 500.f, 500.f, 320.f, 240.f, sf, s2);
    const orbx_kf_geom v = g.view();
    if (v.nlevels != 2 || v.cam[2] != 320.f || v.Rcw != g.Rcw) return 1;
    // no neighbours: no device work, no context needed
    LocalMapping lm(nullptr);
    orbx_bow_view KF1{};
    if (!lm.CreateNewMapPoints(KF1, g, {}, {}, {}).empty()) return 2;
    std::vector<std::vector<NewPoint>> (LocalMapping::*fn)(const orbx_bow_view&, const KeyFrameGeom&,
        const std::vector<orbx_bow_view>&, const std::vector<KeyFrameGeom>&, const std::vector<float>&, bool) =
        &LocalMapping::CreateNewMapPoints;
    std::printf("ok %d\n", fn != nullptr);
    return 0;
}
"""


def test_adapter_compiles_into_a_standalone_program(tmp_path):
    """KeyFrameGeom fills orbx_kf_geom from the reference's getters and
    LocalMapping::CreateNewMapPoints returns the per-neighbour triples; the
    header builds into a program of its own against liborbx."""
    pkg = Path(ox.__file__).resolve().parent
    src = tmp_path / "newpoints_adapter.cpp"
    src.write_text(ADAPTER_PROGRAM)
    exe = tmp_path / "newpoints_adapter"
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{pkg / 'adapters'}", str(src), "-o", str(exe),
                        f"-L{pkg}", "-lorbx", f"-Wl,-rpath,{pkg}"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    text = (pkg / "adapters" / "orbx_adapters.hpp").read_text()
    assert "orbx_create_new_map_points(" in text and "struct KeyFrameGeom" in text
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 1", (r.returncode, r.stdout, r.stderr)
