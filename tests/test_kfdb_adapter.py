"""The adapter's KeyFrameDatabase mirror (orb_slam_amd/adapters/
orbx_adapters.hpp): the reference's method names over the orbx_kfdb_* calls.
The demo program adds four keyframes in the order 9, 2, 7, 5, queries, erases
7 and adds it again, and runs DetectLoop's pair of calls as one."""
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


def test_adapter_mirrors_the_reference_names(demo):
    """The header compiles (the demo was built from it) and keeps the
    reference's public members (include/KeyFrameDatabase.h:42-66)."""
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    body = text[text.index("class KeyFrameDatabase {"):]
    assert re.search(r"void add\(int mnId, const BowVector& bow\)", body)
    assert re.search(r"void erase\(int mnId\)", body) and re.search(r"void clear\(\)", body)
    assert re.search(r"std::vector<int> DetectLoopCandidates\(const BowVector& pKF, float minScore,", body)
    assert re.search(r"std::vector<int> DetectRelocalisationCandidates\(const BowVector& F\)", body)
    for fn in ("orbx_kfdb_create(", "orbx_kfdb_destroy(", "orbx_kfdb_add(", "orbx_kfdb_add_slot(", "orbx_kfdb_erase(",
               "orbx_kfdb_clear(", "orbx_kfdb_set_neighbours(", "orbx_kfdb_query(", "orbx_kfdb_score("):
        assert fn in body, fn
    demo_text = (ADAPTERS / "adapter_demo.cpp").read_text()
    assert "kfdb.DetectRelocalisationCandidates(" in demo_text and "kfdb.DetectLoopCandidates(" in demo_text


@pytest.mark.gpu
def test_demo_database_answers(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["kfdb_reloc"] == 7529            # smallest common word, then add order
    assert r["kfdb_reloc_readded"] == 5729    # 7 went to the back of word 10's list
    assert r["kfdb_loop"] == 729 and r["kfdb_min_score"] == 0.5   # 5 is connected; minScore from 2 and 9
    assert r["kfdb_loop_above"] == 0          # every score is 0.5 < 0.75
    assert r["kfdb_score"] == [0.5, 0.5] and r["kfdb_size_after_clear"] == 0
    assert "pnp_same" in r and "n1" in r      # the earlier keys stay
