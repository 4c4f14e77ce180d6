"""Writes tests/golden/kfdb_queries.npz: one operation sequence on a keyframe
database (adds in shuffled id order, neighbour rows, an erase and a second
add, relocalisation and loop queries) and what this project's restatement
(tests/kfdb_numpy.py) returns for every query.  The reference is not run."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import kfdb_cases as kc  # noqa: E402

if __name__ == "__main__":
    ops, capacity = kc.random_ops(seed=8, members=20, lengths=[20, 25, 30, 0, 1, 28], universe=40, n_queries=8)
    results = kc.run_restatement(ops, capacity)
    out = ROOT / "tests" / "golden" / "kfdb_queries.npz"
    np.savez_compressed(out, **kc.encode(ops, results, capacity))
    print(out, out.stat().st_size, "bytes;", [r["cand"].tolist() for r in results])
