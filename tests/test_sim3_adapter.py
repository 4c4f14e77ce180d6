"""The adapter's Sim3Solver mirror (orb_slam_amd/adapters/orbx_adapters.hpp):
iterate draws 3 * nIterations values from rand() and makes one
orbx_sim3_ransac call, carrying mnIterations and mnBestInliers between calls.
The demo program runs iterate(5) after srand(1) until it returns, beside the C
call fed the same rand() sequence."""
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
    reference's member functions (include/Sim3Solver.h:36-48)."""
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    body = text[text.index("class Sim3Solver {"):]
    assert re.search(r"Sim3Solver\(const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2, const std::vector<int>& vMatches12,", body)
    assert re.search(r"void SetRansacParameters\(double probability = 0\.99, int minInliers = 6, int maxIterations = 300\)", body)
    assert re.search(r"iterate\(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers\)", body)
    assert re.search(r"find\(std::vector<bool>& vbInliers12, int& nInliers\)", body)
    for name in ("GetEstimatedRotation", "GetEstimatedTranslation", "GetEstimatedScale"):
        assert re.search(name + r"\(\) const", body), name
    assert "orbx_sim3_ransac(" in body and "std::rand()" in body
    demo_text = (ADAPTERS / "adapter_demo.cpp").read_text()
    assert "solver.iterate(5," in demo_text and "orbx_sim3_ransac(" in demo_text


@pytest.mark.gpu
def test_iterate_equals_the_c_call(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["sim3_same"] == 1
    # 80 correspondences, every fifth partner unrelated, no noise: the first
    # set of three true partners returns with the 64 true ones as inliers
    assert r["sim3_n"] == 80 and r["sim3_found"] == 1 and r["sim3_inliers"] == 64
    assert 1 <= r["sim3_iterations"] <= 300
    assert abs(r["sim3_scale"] - 1.25) < 1e-3
