"""Local BA on the device over the constructed graphs of tests/lba_graphs.py:
the graph-structure paths of orbx_lba.hip that synth_ba's problems do not
enter ("Constructed graphs for local BA", has the table).

Against the oracle at tests/test_lba_gpu.py's bar (compare: poses 1e-5, points
1e-4, identical edge status, bad flags, iterations, trials, outlier counts);
between launch forms -- workgroup counts, batch and single, resident, polled
-- bit for bit (tests/test_lba_split_gpu.py's same_bits).  The oracle's
results are computed once per graph (lba_graphs.oracle) and shared.
"""
import ctypes

import numpy as np
import pytest

import lba_graphs as lg
import orb_slam_amd as ox
from orb_slam_amd import synth_ba as sb
from test_lba_gpu import compare
from test_lba_split_gpu import same_bits

pytestmark = pytest.mark.gpu

# the reduced system in LDS beside the staged Schur (lba_plan_stage's
# lds_split_bytes <= 160 KB - 2 KB): at most 18 free poses with 129 poses in
# all, 20 with 23 -- every graph but poses128 / poses129
SPLIT = [n for n in lg.GRAPHS if not n.startswith("poses")]
BATCH = ["thr6", "thr2", "no_edges", "rec_double", "unused", "away_free", "point_leaves", "thin"]


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=100, max_w=64, max_h=64, slots=1)
    yield c
    ox.lib().orbx_lba_set_workgroups(c.handle, 0)
    c.close()


def solve(ctx, name, wg=0, abort=None):
    c = lg.named(name)
    assert ox.lib().orbx_lba_set_workgroups(ctx.handle, wg) == 0
    p, arrs = sb.to_ctypes(c.prob)
    es = np.zeros(p.n_edges, np.uint8)
    pb = np.zeros(p.n_points, np.uint8)
    st = sb.BAStats()
    ab = None if abort is None else ctypes.byref(ctypes.c_uint8(abort))
    r = ox.lib().orbx_lba_solve(ctx.handle, ctypes.byref(p), c.iters[0], c.iters[1], ab, es.ctypes.data,
                                pb.ctypes.data, ctypes.byref(st))
    assert r == 0, r
    return arrs, es, pb, st


def workgroups(ctx):
    return ox.lib().orbx_lba_last_workgroups(ctx.handle)


def untouched(prob, arrs, poses, points):
    for k in poses:
        assert arrs["pose_q"][k].tobytes() == prob["pose_q"][k].tobytes()
        assert arrs["pose_t"][k].tobytes() == prob["pose_t"][k].tobytes()
    for p in points:
        assert arrs["points"][p].tobytes() == prob["points"][p].tobytes()


@pytest.mark.parametrize("name", list(lg.GRAPHS))
def test_graph_matches_oracle(ctx, name):
    """orbx_lba_solve at the automatic workgroup setting."""
    c = lg.named(name)
    gpu = solve(ctx, name)
    compare(lg.oracle(name), gpu)
    arrs, es, pb, st = gpu
    if name.startswith("unused"):
        untouched(c.prob, arrs, c.idle_poses, c.idle_points)
        assert not pb[list(c.idle_points)].any()
    if name == "no_edges":
        untouched(c.prob, arrs, range(2), range(10))
        assert list(st.iterations) == [0, 0]
    if name == "all_behind":
        assert st.iterations[1] == 0 and list(st.n_outliers) == [20, 0]


@pytest.mark.parametrize("name", SPLIT)
def test_graph_split_equals_one_workgroup(ctx, name):
    """k_lba_split at workgroup settings 0 (automatic), 3 and 64 against
    k_lba_iteration (setting 1), bit for bit.  Point l belongs to workgroup
    l mod G; the staged Schur takes chunks of up to kSP = 64 points whose free
    edges fit kSE = 128 slots; the edge-parallel linearisation / back-
    substitution serve a workgroup of up to 64 points and kLinEdges = 307 /
    kBsEdges = 960 edges.

    sparse_free (200 points: 150 with one free edge, every fourth with
      none), setting 3: 67 | 67 | 66 points per workgroup, so a chunk ends
      on the 64-point limit (about 48 slots used) with about 16 points of
      no free edge inside it, and the per-point fallbacks run (over 64
      points); automatic setting ceil(200 / 32) = 7: 29 points a workgroup.
    dense_free (130 points x 23 edges, 20 of them free): 128 / 20 = 6 points
      per chunk, the seventh not fitting (120 slots; 6 x 210 = 1260 pairs);
      automatic setting min(64, ceil(130 / 32)) = 5: 26 points x 23 = 598
      edges, over kLinEdges and under kBsEdges; setting 3: 44 | 43 | 43
      points x 23 = 1012 | 989 | 989 edges, over both.
    wide128 / wide129: the most edges on one point is 128 | 129 against the
      host's rule max_obs0 > kSE -> one workgroup.
    """
    one = solve(ctx, name, 1)
    assert workgroups(ctx) == 1
    n_points = len(lg.named(name).prob["points"])
    for wg in (0, 3, 64):
        same_bits(solve(ctx, name, wg), one)
        g = workgroups(ctx)
        if name == "wide129":
            assert g == 1
        elif wg > 1:
            assert g > 1        # wide128 at 64 among them
        elif n_points >= 128:
            assert g == min(64, (n_points + 31) // 32)
    compare(lg.oracle(name), one)


@pytest.mark.parametrize("name", ["poses128", "poses129", "points8192", "points8193"])
def test_build_tables_either_side(ctx, name):
    """k_lba_build with 128 | 129 pose blocks (kBuildPoses: the chunked
    stable scatter in LDS | atomic counts and a wave per pose) and 8192 | 8193
    active points (kBuildPoints: counts and cursors in LDS | in global
    memory): the oracle's result, and the same bits twice (the atomics decide
    places that the sort by edge index then fixes)."""
    a = solve(ctx, name)
    b = solve(ctx, name)
    same_bits(a, b)
    compare(lg.oracle(name), a)
    assert sum(a[3].iterations) > 0


def marshal(names):
    n = len(names)
    cps = [sb.to_ctypes(lg.named(k).prob) for k in names]
    arr = (sb.BAProblem * n)(*[c[0] for c in cps])
    es = [np.zeros(c[0].n_edges, np.uint8) for c in cps]
    pb = [np.zeros(c[0].n_points, np.uint8) for c in cps]
    esp = (ctypes.c_void_p * n)(*[e.ctypes.data for e in es])
    pbp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in pb])
    return cps, arr, es, pb, esp, pbp, (sb.BAStats * n)()


@pytest.fixture(scope="module")
def singles(ctx):
    return {k: solve(ctx, k, 1) for k in BATCH}


@pytest.mark.parametrize("order", ["listed", "reversed"])
@pytest.mark.parametrize("resident", [False, True], ids=["batch", "resident"])
def test_batch_equals_single_solves(ctx, singles, order, resident):
    """Problems with different thresholds (thr2 beside thr6: each must be
    gated by its own chi2_threshold, as it is solved with its own
    huber_delta), an empty graph among them, and float-exact problems staged
    beside one that is not (rec_double: the batch takes 32-byte records, the
    single solves of the others 16-byte ones): every problem of the batch
    equals its own one-workgroup solve bit for bit."""
    names = BATCH if order == "listed" else BATCH[::-1]
    assert all(tuple(lg.named(k).iters) == (5, 10) for k in names)
    cps, arr, es, pb, esp, pbp, st = marshal(names)
    L = ox.lib()
    if resident:
        assert L.orbx_lba_stage(ctx.handle, len(names), arr) == 0
        assert L.orbx_lba_run(ctx.handle, 5, 10, None) == 0
        assert L.orbx_lba_fetch(ctx.handle, arr, esp, pbp, st) == 0
    else:
        assert L.orbx_lba_solve_batch(ctx.handle, len(names), arr, 5, 10, None, esp, pbp, st) == 0
    for i, k in enumerate(names):
        try:
            same_bits((cps[i][1], es[i], pb[i], st[i]), singles[k])
        except AssertionError as exc:
            raise AssertionError(f"problem {i} ({k})") from exc
    # what the thresholds decide differently is there to be got wrong
    a, b = singles["thr2"][1], singles["thr6"][1]
    assert np.count_nonzero(a != b) >= 10


@pytest.mark.parametrize("name", ["away_free", "point_leaves"])
def test_polled_run_equals_unpolled(ctx, name):
    """With an abort flag (never raised) every iteration is its own launch
    and the host reads the state between them: the same bits, through the
    rebuild that drops a pose block / a point."""
    base = solve(ctx, name, 1)
    same_bits(solve(ctx, name, 1, abort=0), base)
    same_bits(solve(ctx, name, 0, abort=0), base)
    same_bits(solve(ctx, name, 3, abort=0), base)
