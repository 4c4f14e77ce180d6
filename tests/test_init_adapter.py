"""The adapter's Initializer mirror (orb_slam_amd/adapters/orbx_adapters.hpp):
FindModels draws from rand() as the reference's set loop does and makes one
orbx_init_models call.  The demo program runs it after srand(1) beside the C
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
    reference's constructor and the model search's outputs."""
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    assert re.search(r"Initializer\(const std::vector<KeyPoint>& keys1, float sigma = 1\.0f, int iterations = 200", text)
    assert re.search(r"FindModels\(const std::vector<KeyPoint>& keys2, const std::vector<int>& vMatches12,\s*"
                     r"std::vector<bool>& vbMatchesInliersH, float& SH, float H\[9\],\s*"
                     r"std::vector<bool>& vbMatchesInliersF, float& SF, float F\[9\]\)", text)
    assert "orbx_init_models(" in text


@pytest.mark.gpu
def test_find_models_equals_the_c_call(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["init_n"] == r["init_matches"] > 50
    assert r["init_same"] == 1
    # the demo's second frame is the first shifted by two columns: both
    # models explain it, and most matches are inliers of the winner
    assert min(r["init_best"]) >= 0
    assert r["init_inliers"][0] > 0.5 * r["init_n"]
