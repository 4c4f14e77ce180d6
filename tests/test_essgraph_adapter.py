"""The adapter's Optimizer::OptimizeEssentialGraph and EssentialGraph
(orb_slam_amd/adapters/orbx_adapters.hpp).  The demo program closes a small
loop with pure scale drift through the adapter, which builds the edge list by
the reference's rules, and through the plain C call on the same edges."""
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


def test_adapter_keeps_the_reference_entry(demo):
    text = (ADAPTERS / "orbx_adapters.hpp").read_text()
    cls = text[text.index("class Optimizer {"):]
    cls = cls[:cls.index("\n};")]
    assert re.search(r"static void OptimizeEssentialGraph\(orbx_ctx\* ctx, EssentialGraph& G\);", cls)
    body = text[text.index("struct EssentialGraph {"):]
    for piece in ("BuildEdges() const", "sInsertedEdges", "c.weight < minFeat", "lc.id != curKF || c.id != loopKF",
                  "orbx_optimize_essential_graph(ctx, &q)"):
        assert piece in body, piece
    assert "in the caller's order" in text
    demo_text = (ADAPTERS / "adapter_demo.cpp").read_text()
    assert "Optimizer::OptimizeEssentialGraph(" in demo_text and "orbx_optimize_essential_graph(" in demo_text


@pytest.mark.gpu
def test_adapter_equals_the_c_call_and_the_loop_closes(demo):
    p = subprocess.run([str(demo)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print({k: v for k, v in r.items() if k.startswith("essgraph")})
    assert r["essgraph_same"] == 1
    # two loop connections pass minFeat (one by the (cur, loop) exemption), seven
    # spanning-tree edges, six covisibility edges
    assert r["essgraph_edges"] == 15 and 1 <= r["essgraph_iterations"] <= 20
    # The chain's measurements all have scale 1, so no state satisfies them and the loop at once: least squares
    # spreads the discrepancy D over the edges of the cycle.  The shortest cycle through the loop connections has
    # m = 5 edges (four covisibility hops and the loop edge).  Before, D sits on the two edges that join the current
    # keyframe to its uncorrected neighbours (chi2 about 2 D^2); after, on about m edges with D / m each (chi2 about
    # D^2 / m): a fall by 2 m, asserted with a factor of two to spare.  The loop is closed when the current keyframe
    # ends nearer the pose the loop gives it than the drifted one, in position and in scale.
    first, last = r["essgraph_chi2"]
    assert first > 0.1 and last < first / 5
    assert 0.5 < r["essgraph_centre_gap"] < 0.8 and r["essgraph_centre_err"] < 0.5 * r["essgraph_centre_gap"]
    s_opt, s_corrected = r["essgraph_scale"]
    assert abs(s_corrected - 1.21) < 1e-6 and abs(s_opt - s_corrected) < 0.5 * abs(1.0 - s_corrected)
