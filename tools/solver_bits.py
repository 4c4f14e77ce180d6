"""Writes every output and tap of the geometry solvers (orbx_init.hip,
orbx_reconstruct.hip, orbx_newpoints.hip, orbx_sim3.hip, orbx_pnp.hip) on the
scenes of their GPU tests to an .npz, so two library builds can be compared
bit for bit: ORBX_LIBRARY=<lib> python3 tools/solver_bits.py out.npz
Compare the arrays' raw bytes (`a.tobytes() == b.tobytes()`), so that NaNs
compare.  A tool, not a test: the device's Jacobi bits are what DESIGN.md
section 4 leaves unspecified, so they are no fixture."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import init_numpy as inp  # noqa: E402
import newpoints_numpy as npn  # noqa: E402
import orb_slam_amd as ox  # noqa: E402
import pnp_numpy as pn  # noqa: E402
import reconstruct_numpy as rn  # noqa: E402
import sim3_numpy as s3  # noqa: E402

out = {}


def keep(prefix, value):
    """Every array, scalar and list of arrays of a result dict, by name."""
    if value is None:
        return
    if isinstance(value, dict):
        for k, v in value.items():
            keep(f"{prefix}_{k}", v)
    elif isinstance(value, (list, tuple)) and any(isinstance(v, (np.ndarray, dict)) for v in value):
        for k, v in enumerate(value):
            keep(f"{prefix}_{k}", v)
    else:
        out[prefix] = np.asarray(value)
        assert out[prefix].dtype != object, prefix


ctx = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=2)

# orbx_init_models: the inputs of init_numpy.case, without its restatement
for i, (N, M, planar, seed, dseed) in enumerate(inp.CASES):
    k1, k2, m = inp.scene(seed, N, planar=planar)
    keep(f"init{i}", ctx.init_models(k1, k2, m, inp.make_draws(dseed, M), 1.0, M, taps=True))

# orbx_init_reconstruct: the cases, and the constructed match in both fp-contract modes
for name in sorted(rn.CASES):
    a = rn.case_inputs(name)
    keep(f"rec_{name}", ctx.init_reconstruct(*a[:7], taps=True, **a[8]))
contract_args = rn.contract_case()
big = npn.scene(31, 300, 3)
fixture = np.load(ROOT / "tests" / "golden" / "new_points.npz")
edited = npn.unpack_contract(fixture)
chain = npn.unpack(fixture, "c_", npn.CHAIN_CASE["n"])
V1, V2s, views_keep = npn.views(chain)
for c in (1, 0):
    ctx.set_fp_contract(c)
    keep(f"rec_contract{c}", ctx.init_reconstruct(*contract_args, taps=True))
    for name in ("H-65", "H-64", "H-256", "H-ambiguous-65"):
        a = rn.case_inputs(name)
        keep(f"rec_{name}_contract{c}", ctx.init_reconstruct(*a[:7], taps=True, **a[8]))
    # orbx_triangulate_matches / orbx_create_new_map_points
    keep(f"tri_big_contract{c}", ctx.triangulate_matches(big["keys1"], big["g1"], big["keys2"], big["g2"], big["truth"],
                                                        v4=True))
    keep(f"tri_edited_contract{c}", ctx.triangulate_matches(edited[0], edited[1], [edited[2]], [edited[3]], [edited[4]],
                                                           v4=True))
    for chained in (False, True):
        keep(f"newpoints_chain{int(chained)}_contract{c}",
             ctx.create_new_map_points(V1, chain["g1"], V2s, chain["g2"], np.concatenate(chain["F12"]), chain=chained,
                                       v4=True))

# orbx_sim3_ransac: the inputs of sim3_numpy.case, without its restatement
for i, (N, M, mi, use_idx1, seed, dseed) in enumerate(s3.CASES):
    kf1, kf2, m, idx1 = s3.scene(seed, N, use_idx1=use_idx1)
    d = s3.make_draws(dseed, M, N if N < 8 else None)
    for c in ((0, 1) if (N, M) == (65, 65) else (0,)):
        ctx.set_fp_contract(c)
        keep(f"sim3_{i}_contract{c}", ctx.sim3_ransac(kf1, kf2, m, d, taps=True, idx1=idx1, min_inliers=mi))
ctx.set_fp_contract(0)

# orbx_pnp_ransac
for i, (N, T) in enumerate(pn.CASES):
    sc, d, params = pn.case(i)
    for c in ((0, 1) if (N, T) == (65, 35) else (0,)):
        ctx.set_fp_contract(c)
        keep(f"pnp_{i}_contract{c}", ctx.pnp_ransac(pn.frame_of(sc), d, taps=True, **params))
ctx.set_fp_contract(0)
ctx.close()

np.savez(sys.argv[1], **out)
print("saved", sys.argv[1], len(out), "arrays from", ox.LIB_PATH)
