"""Records tests/golden/culling_sequence.npz: the operation sequence of
culling_cases.golden_ops() and the results the restatement (tests/
culling_numpy.py) gives for it.

usage: python tools/gen_culling_golden.py"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import culling_cases as kc  # noqa: E402

ops = kc.golden_ops()
assert all(kc.scene_properties(ops).values())
out = ROOT / "tests" / "golden" / "culling_sequence.npz"
kc.write_golden(out)
print(out, out.stat().st_size, "bytes,", len(ops), "operations")
