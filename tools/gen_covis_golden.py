"""Records tests/golden/covis_sequence.npz: the operation sequence of
covis_cases.golden_ops() and the results the restatement (tests/
covis_numpy.py) gives for it.

usage: python tools/gen_covis_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import covis_cases as cc  # noqa: E402

ops = cc.golden_ops()
results, _ = cc.run_restatement(ops)
assert all(cc.scene_properties(ops).values())
out = ROOT / "tests" / "golden" / "covis_sequence.npz"
np.savez_compressed(out, **cc.encode(ops, results))
print(out, out.stat().st_size, "bytes,", len(ops), "operations,", len(results), "results")
