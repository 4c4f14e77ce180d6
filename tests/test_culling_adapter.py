"""The adapter's KeyFrameCulling and MapPointCulling (orb_slam_amd/adapters/
orbx_adapters.hpp): the reference's names over orbx_covis_cull_keyframes and
orbx_covis_cull_points, with the tree part of KeyFrame::SetBadFlag written
out between the calls.  The demo program's scene and every answer below are
worked out by hand from src/LocalMapping.cc:190-218, :539-593 and
src/KeyFrame.cc:497-581."""
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


def test_adapter_mirrors_the_reference_names():
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    body = text[text.index("class CovisibilityGraph {"):]
    for sig in (r"void SetOctaves\(int mnId, const std::vector<int>& vOctaves\)",
                r"Culling KeyFrameCulling\(int mpCurrentKeyFrame, const std::vector<int>& vpNotErase",
                r"std::vector<int> MapPointCulling\(int nCurrentKFid, std::list<RecentMapPoint>& mlpRecentAddedMapPoints\)",
                r"void ChangeParent\(int mnId, int pKF\)", r"std::vector<int> GetChilds\(int mnId\) const",
                r"void UpdateSpanningTree\(int mnId\)"):
        assert re.search(sig, body), sig
    for fn in ("orbx_covis_set_octaves(", "orbx_covis_cull_keyframes(", "orbx_covis_cull_points("):
        assert fn in body, fn
    # the tree loop: one cull per call, the tree repaired, the call resumed with the rest of the list
    loop = body[body.index("Culling KeyFrameCulling("):body.index("std::vector<int> MapPointCulling(")]
    assert "q.max_culls = 1;" in loop and "UpdateSpanningTree(pKF);" in loop and "cur = -1;" in loop
    assert "first += q.n_done;" in loop
    tree = body[body.index("void UpdateSpanningTree(int mnId)"):]
    assert "if (w > max) {" in tree and "sParentCandidates.push_back(pC);" in tree
    demo_text = (ADAPTERS / "adapter_demo.cpp").read_text()
    assert "lm.KeyFrameCulling(5, {4})" in demo_text and "lm.MapPointCulling(5, lm_recent)" in demo_text


@pytest.mark.gpu
def test_demo_culling_answers(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    # 5 shares eleven points with 4 and 2, ten with 3 and 0; the larger key first among equals
    assert r["cull_list5"] == 4230
    # 4 and 2: ten of eleven points have three other observers in scale, 10 > 0.9 * 11; 4 is held, 2 goes.  3: its
    # ten points are still seen by 0, 4 and 5: it goes.  0 is never culled.
    assert r["cull_culled"] == 23 and r["cull_to_be_erased"] == 4
    assert r["cull_bad_points"] == 50                  # left with 4 and 5 when 2 went
    # 2's children 3 and 4: 3 finds the parent candidate 0 at weight 10 first, 4 then finds 3 at 10 before 0 at 10;
    # when 3 goes, 4 finds 0.  3 has no parent any more, 5 keeps 4.
    assert r["cull_parents"] == [-1, 0, 4] and r["cull_childs0"] == 4 and r["cull_size"] == 3
    # 10: found 5 of 5, two keyframes old, observers 0, 4, 5: stays.  60: 1 / 5 < 0.25.  50: bad already.
    assert r["cull_mp_bad"] == 60 and r["cull_mp_left"] == 10 and r["cull_mp_left_n"] == 1
    assert "covis_size" in r and "kfdb_reloc" in r and "n1" in r      # the earlier keys stay
