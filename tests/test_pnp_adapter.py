"""The adapter's PnPsolver mirror (orb_slam_amd/adapters/orbx_adapters.hpp):
iterate draws four rand() values for every iteration the call can run and
makes one orbx_pnp_ransac call, carrying mnIterations, mnBestInliers,
mvbBestInliers and mBestTcw between calls.  The demo program runs iterate(5)
after srand(1) until it returns, beside the C call fed the same rand()
sequence."""
import json
import re
import subprocess
from pathlib import Path

import pytest

import orb_slam_amd as ox

ADAPTERS = Path(ox.__file__).resolve().parent / "adapters"
DEMO = ADAPTERS / "adapter_demo"


@pytest.fixture(scope="module")
def demo():
    if not DEMO.exists():
        from orb_slam_amd import build
        build.build()
    assert DEMO.exists()
    return DEMO


def test_adapter_mirrors_the_reference_signatures(demo):
    """The header compiles (the demo was built from it) and keeps the
    reference's public members (include/PnPsolver.h:36-47)."""
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    body = text[text.index("class PnPsolver {"):]
    assert re.search(r"PnPsolver\(const PnPFrame& F, const std::vector<float>& vMapPointPos,", body)
    assert re.search(r"void SetRansacParameters\(double probability = 0\.99, int minInliers = 8, int maxIterations = 300, "
                     r"int minSet = 4,\s*float epsilon = 0\.4, float th2 = 5\.991\)", body)
    assert re.search(r"iterate\(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers\)", body)
    assert re.search(r"find\(std::vector<bool>& vbInliers, int& nInliers\)", body)
    assert "orbx_pnp_ransac(" in body and "std::rand()" in body
    assert re.search(r"return iterate\(mRansacMaxIts, bFlag, vbInliers, nInliers\);", body)
    assert "mRansacMaxIts = std::max(1, std::min(nIterations, maxIterations));" in body
    demo_text = (ADAPTERS / "adapter_demo.cpp").read_text()
    assert "pnp.iterate(5," in demo_text and "orbx_pnp_ransac(" in demo_text


@pytest.mark.gpu
def test_iterate_equals_the_c_call(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["pnp_same"] == 1
    # 80 correspondences, every fifth partner unrelated, no noise: a set of
    # four true partners that EPnP solves returns, refined, with the 64 true ones
    assert r["pnp_n"] == 80 and r["pnp_found"] == 1 and r["pnp_refined"] == 1 and r["pnp_inliers"] == 64
    assert 1 <= r["pnp_iterations"] <= 300 and r["pnp_calls"] >= 1
    assert r["pnp_pose_error"] < 1e-5
    assert r["pnp_max_its"] == 35                  # the adapter's adjusted mRansacMaxIts is the device's
    assert "sim3_same" in r and "n1" in r          # the earlier keys stay


@pytest.mark.gpu
def test_find_runs_the_adjusted_iteration_count(demo):
    """find() is iterate(mRansacMaxIts) with the value SetRansacParameters
    adjusted (35 at Relocalisation's parameters and N = 80), not the 300
    passed in: on a scene where no Refine returns it runs exactly that many
    iterations and takes the exit at :213-227."""
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["pnp_find_max_its"] == 35
    assert r["pnp_find_iterations"] == r["pnp_find_max_its"]
    assert r["pnp_find_found"] == 0 and r["pnp_find_best"] == 0
