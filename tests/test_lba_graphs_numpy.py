"""The constructed local-BA graphs (tests/lba_graphs.py) on the CPU: each
graph is what its name says (the facts asserted on the oracle's result), and
the two CPU solvers -- the oracle (oracle/ref_lba.cpp, Schur complement) and
the dense numpy restatement (tests/test_lba_numpy.py) -- agree on every graph
small enough for the dense one, at that file's bar: 1e-8 on poses and points,
identical edge status, bad flags, iterations and trials.

That agreement admits a graph to tests/test_lba_graphs_gpu.py: it is 1000 x
under the device bar, so the structure is conditioned well enough that a
device miss is the device's.
"""
import numpy as np
import pytest

import lba_graphs as lg
from test_lba_numpy import Graph, local_ba


def status_of(name, point):
    c = lg.named(name)
    return lg.oracle(name)[1][lg.edges_of(c.prob, point)].tolist()


def untouched(prob, arrs, poses, points):
    for k in poses:
        assert arrs["pose_q"][k].tobytes() == prob["pose_q"][k].tobytes()
        assert arrs["pose_t"][k].tobytes() == prob["pose_t"][k].tobytes()
    for p in points:
        assert arrs["points"][p].tobytes() == prob["points"][p].tobytes()


@pytest.mark.parametrize("name", lg.SMALL)
def test_numpy_matches_oracle(name):
    c = lg.named(name)
    g, status, bad, stats = local_ba(c.prob, *c.iters)
    ra, res, rpb, rst = lg.oracle(name)
    assert np.abs(g.q - ra["pose_q"]).max() <= 1e-8
    assert np.abs(g.t - ra["pose_t"]).max() <= 1e-8
    assert np.abs(g.X - ra["points"]).max() <= 1e-8
    assert np.array_equal(status, res), (np.count_nonzero(status), np.count_nonzero(res))
    assert np.array_equal(bad, rpb)
    assert [s[0] for s in stats] == list(rst.iterations)
    assert [s[1] for s in stats] == list(rst.levenberg_trials)
    assert list(rst.n_outliers) == [int(np.count_nonzero(status == 1)), int(np.count_nonzero(status == 2))]


@pytest.mark.parametrize("name", ["unused", "unused_ids"])
def test_unused_entries_come_back_untouched(name):
    c = lg.named(name)
    arrs, es, pb, st = lg.oracle(name)
    n_free, n_active, _, _ = lg.counts(c.prob)
    assert n_free == 3 and int(np.count_nonzero(c.prob["pose_fixed"] == 0)) == 4   # fewer blocks than free poses
    assert n_active == 37
    untouched(c.prob, arrs, c.idle_poses, c.idle_points)
    assert not pb[list(c.idle_points)].any()
    assert st.iterations[0] > 0 and st.iterations[1] > 0
    ids = c.prob["pose_id"]
    assert (np.diff(ids) > 0).all() == (name == "unused")


def test_thin_points():
    c = lg.named("thin")
    arrs, es, pb, st = lg.oracle("thin")
    assert [len(lg.edges_of(c.prob, p)) for p in c.thin_points] == [1, 1, 2, 2]
    assert status_of("thin", c.gross_point) == [1, 0] and pb[c.gross_point] == 1
    assert not pb[list(c.thin_points)].any()


def final_chi2(name, edges):
    """chi2 of some edges at the oracle's final state, by the numpy restatement."""
    c = lg.named(name)
    arrs = lg.oracle(name)[0]
    g = Graph(dict(c.prob, pose_q=arrs["pose_q"], pose_t=arrs["pose_t"], points=arrs["points"]))
    out = []
    for e in edges:
        g.err[e] = g.error(e)
        out.append((g.chi2(e), g.pc(e)[2]))
    return out


def test_away_fixed_edges_fail_on_depth_alone():
    c = lg.named("away_fixed")
    arrs, es, pb, st = lg.oracle("away_fixed")
    assert es[c.away_edges].tolist() == [1, 1, 1]
    for e in c.away_edges:   # in the middle of its point's edges
        own = lg.edges_of(c.prob, c.prob["edge_point"][e]).tolist()
        assert 0 < own.index(e) < len(own) - 1
    for chi2, z in final_chi2("away_fixed", c.away_edges):
        assert chi2 < 1 and z < 0


def test_away_free_pose_is_absent_from_pass_2():
    c = lg.named("away_free")
    arrs, es, pb, st = lg.oracle("away_free")
    assert len(c.away_edges) == 8 and es[c.away_edges].tolist() == [1] * 8
    assert np.array_equal(np.nonzero(c.prob["edge_pose"] == c.away_pose)[0], np.sort(c.away_edges))
    free = np.nonzero(c.prob["pose_fixed"] == 0)[0].tolist()
    assert free.index(c.away_pose) == len(free) // 2   # the middle pose block
    assert st.iterations[1] > 0
    for chi2, z in final_chi2("away_free", c.away_edges):
        assert z < 0


def test_point_leaves_without_going_bad():
    c = lg.named("point_leaves")
    arrs, es, pb, st = lg.oracle("point_leaves")
    assert status_of("point_leaves", c.leaves) == [1, 1, 1, 1, 1] and pb[c.leaves] == 0
    assert status_of("point_leaves", c.goes_bad) == [1, 1, 1, 0, 0] and pb[c.goes_bad] == 1
    assert st.iterations[1] > 0


def test_all_behind_empties_the_graph():
    c = lg.named("all_behind")
    arrs, es, pb, st = lg.oracle("all_behind")
    assert list(st.n_outliers) == [20, 0]
    assert st.iterations[0] > 0 and st.iterations[1] == 0
    assert not pb.any()
    for chi2, z in final_chi2("all_behind", range(20)):
        assert chi2 < 1 and z < 0   # rejected on depth alone


def test_no_edges_changes_nothing():
    c = lg.named("no_edges")
    arrs, es, pb, st = lg.oracle("no_edges")
    assert list(st.iterations) == [0, 0] and list(st.n_outliers) == [0, 0]
    untouched(c.prob, arrs, range(2), range(10))
    assert not pb.any()


def test_thresholds_decide_differently():
    a, b = lg.named("thr2").prob, lg.named("thr6").prob
    for k in ("edge_obs", "pose_q", "points", "edge_pose", "edge_inv_sigma2"):
        assert np.array_equal(a[k], b[k])
    assert (a["chi2_threshold"], b["chi2_threshold"]) == (2.0, 5.991)
    assert a["huber_delta"] == float(np.float32(np.sqrt(2.0)))
    differ = int(np.count_nonzero(lg.oracle("thr2")[1] != lg.oracle("thr6")[1]))
    assert differ >= 10, differ
    # rec_double: thr6 but for one observation that is no float
    d = lg.named("rec_double").prob
    off = np.nonzero(d["edge_obs"] != b["edge_obs"])
    assert len(off[0]) == 1
    v = d["edge_obs"][off][0]
    assert float(np.float32(v)) != v and abs(v - b["edge_obs"][off][0]) == 2.0 ** -40


@pytest.mark.parametrize("name,free,active,most,most_free", [
    ("poses128", 128, 60, 11, None), ("poses129", 129, 60, 11, None),
    ("points8192", 3, 8192, 3, None), ("points8193", 3, 8193, 3, None),
    ("wide128", 18, 130, 128, 18), ("wide129", 18, 130, 129, 18),
    ("sparse_free", 3, 200, 3, 1), ("dense_free", 20, 130, 23, 20)])
def test_sizes_straddle_the_kernel_constants(name, free, active, most, most_free):
    """The counts the kernels branch on (orbx_lba.hip: kBuildPoses = 128,
    kBuildPoints = 8192, kSE = 128, kSP = 64)."""
    prob = lg.named(name).prob
    n_free, n_active, n_most, n_most_free = lg.counts(prob)
    assert (n_free, n_active, n_most) == (free, active, most)
    if most_free is not None:
        assert n_most_free == most_free
    ek, ep = prob["edge_pose"], prob["edge_point"]
    if name.startswith("poses"):
        per_pose = np.bincount(ek, minlength=len(prob["pose_fixed"]))
        assert per_pose[prob["pose_fixed"] == 0].min() >= 2
        assert np.bincount(ep).min() == 2
    if name == "sparse_free":
        fr = np.bincount(ep[prob["pose_fixed"][ek] == 0], minlength=200)
        assert np.count_nonzero(fr == 1) == 150 and np.count_nonzero(fr == 0) == 50
        assert (np.bincount(ep) == 3).all()
