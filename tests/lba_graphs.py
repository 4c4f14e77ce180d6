"""Constructed local-BA graphs: problems whose *structure* is chosen edge by
edge, for the paths of orbx_lba.hip that synth_ba.make_problem's graphs never
enter (test data only; no device calls).

make_problem gives every point 3-10 edges, every listed pose and point an
edge, every camera a positive depth and every problem one threshold.  Here
the caller lists, per point, the poses that see it: graph(poses, fixed,
points, obs, ...) turns that list into a problem in synth_ba's layout
(sb.to_ctypes takes it), with make_problem's observation model -- the true
projection plus N(0, 1.2^octave) px, octave uniform in 0..7, rounded to
float32, information sb.inv_sigma2_table()[octave] -- and its initial
perturbation (free poses 0.01 rad / 0.02 m, points 0.02 m, all rounded to
float32).  Options:

  gross          (point, pose) edges moved by 20-60 px in u and v;
  exact          (point, pose) edges with the noise-free projection at octave 0;
  point_nobs     MapPoint::Observations() per point (default: its edge count);
  chi2_threshold the problem's own gate, huber_delta = float32(sqrt(thr));
  not_float      2^-40 px added to one observation: not a float any more, so
                 the whole staged batch takes the 32-byte edge records;
  id_order       pose_id / point_id permuted (the Hessian block order follows
                 the ids, not the indices).

arc(n) are make_problem's cameras (a 2 m arc at 4 m looking at the cloud's
centre); away(pose) is the same camera centre turned by pi about the
camera's y axis, so every cloud point lies *behind* it.  An `exact`
observation of such a point is the mirrored projection fx x / z + cx with
z < 0: the edge's chi2 is ~0 at the solution and only the depth gate
(src/Optimizer.cc:459, :505) can reject it.

GRAPHS names the structures; named(name) builds one (cached) and returns a
Case: the problem, the iteration counts its tests use, and the facts that
make it what its name says (tests/test_lba_graphs_numpy.py asserts them on
the oracle's result).  DESIGN.md, "Constructed graphs for local BA", lists
the path each one reaches.
"""
import functools
from types import SimpleNamespace

import numpy as np

from orb_slam_amd import synth_ba as sb

CENTER = np.array([0.0, 0.0, 4.0])
CAM = (500.0, 500.0, 320.0, 240.0)
THR = 5.991
MIRROR = np.diag([-1.0, 1.0, -1.0])   # a turn by pi about the camera's y axis


def arc(n):
    """make_problem's n cameras as (Rcw, tcw)."""
    out = []
    for k in range(n):
        ang = -0.25 + 0.5 * k / max(1, n - 1)
        c = CENTER + 4.0 * np.array([np.sin(ang), 0.05 * np.cos(3 * ang), -np.cos(ang)])
        fwd = CENTER - c
        fwd /= np.linalg.norm(fwd)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rcw = np.stack([right, down, fwd], 1).T
        out.append((Rcw, -Rcw @ c))
    return out


def away(pose):
    R, t = pose
    return MIRROR @ R, MIRROR @ t


def cloud(n, rng):
    """Points every arc camera has in front of it (depth 2.5 .. 5.5 m) and
    inside a 640 x 480 image."""
    return CENTER + rng.uniform([-1.2, -0.9, -1.2], [1.2, 0.9, 1.2], size=(n, 3))


def graph(poses, fixed, points, obs, seed=0, gross=(), exact=(), point_nobs=None, chi2_threshold=THR,
          not_float=False, id_order=False):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAM
    n_poses, n_points = len(poses), len(points)
    points = np.asarray(points, np.float64).reshape(n_points, 3)
    fixed = np.asarray(fixed, np.uint8)
    gross, exact = set(gross), set(exact)
    isig = sb.inv_sigma2_table()
    e_point, e_pose, e_obs, e_isig = [], [], [], []
    for p in range(n_points):
        assert len(set(obs[p])) == len(obs[p]), p
        for k in obs[p]:
            R, t = poses[k]
            pc = R @ points[p] + t
            u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
            octave = int(rng.integers(0, 8))
            sd = 1.2 ** octave
            nu, nv = rng.normal(0, sd), rng.normal(0, sd)
            su, sv = rng.choice([-1, 1]), rng.choice([-1, 1])
            gu, gv = rng.uniform(20, 60), rng.uniform(20, 60)
            if (p, k) in exact:
                octave, nu, nv = 0, 0.0, 0.0
            if (p, k) in gross:
                nu, nv = nu + su * gu, nv + sv * gv
            e_point.append(p)
            e_pose.append(k)
            e_obs.append((np.float32(u + nu), np.float32(v + nv)))   # cv::KeyPoint coords are float
            e_isig.append(isig[octave])
    q = np.zeros((n_poses, 4))
    t = np.zeros((n_poses, 3))
    for k, (R, tt) in enumerate(poses):
        if not fixed[k]:
            R = sb._exp_so3(rng.normal(0, 0.01, 3)) @ R
            tt = tt + rng.normal(0, 0.02, 3)
        q[k] = sb._normalize_q(sb._rot_to_quat(R.astype(np.float32).astype(np.float64)))
        t[k] = tt.astype(np.float32).astype(np.float64)
    pts0 = (points + rng.normal(0, 0.02, points.shape)).astype(np.float32).astype(np.float64)
    e_obs = np.array(e_obs, np.float64).reshape(len(e_point), 2)
    if not_float:
        e_obs[len(e_obs) // 2, 0] += 2.0 ** -40
        assert float(np.float32(e_obs[len(e_obs) // 2, 0])) != e_obs[len(e_obs) // 2, 0]
    pose_id = np.arange(n_poses, dtype=np.int64)
    point_id = np.arange(n_points, dtype=np.int64) + n_poses
    if id_order:
        pose_id, point_id = rng.permutation(pose_id), rng.permutation(point_id)
    nobs = np.array([len(o) for o in obs], np.int32).reshape(n_points)
    if isinstance(point_nobs, dict):        # {point: count} over the default
        for p, v in point_nobs.items():
            nobs[p] = v
    elif point_nobs is not None:            # one count for all, or one per point
        nobs[:] = point_nobs
    prob = {
        "pose_q": q, "pose_t": t, "pose_fixed": fixed, "pose_id": pose_id,
        "pose_cam": np.tile(CAM, (n_poses, 1)).astype(np.float64),
        "points": pts0, "point_id": point_id, "point_nobs": nobs,
        "edge_point": np.array(e_point, np.int32), "edge_pose": np.array(e_pose, np.int32),
        "edge_obs": e_obs, "edge_inv_sigma2": np.array(e_isig, np.float64),
        "huber_delta": float(np.float32(np.sqrt(chi2_threshold))), "chi2_threshold": float(chi2_threshold),
        "points_true": points, "poses_true": list(poses),
    }
    for k in ["pose_q", "pose_t", "pose_cam", "points", "edge_obs", "edge_inv_sigma2"]:
        prob[k] = np.ascontiguousarray(prob[k], np.float64)
    return prob


def edges_of(prob, point):
    """The edge indices of a point, in edge order."""
    return np.nonzero(prob["edge_point"] == point)[0]


def edge(prob, point, pose):
    e = np.nonzero((prob["edge_point"] == point) & (prob["edge_pose"] == pose))[0]
    assert len(e) == 1
    return int(e[0])


def random_obs(n_points, n_poses, lo, hi, rng):
    """Per point lo..hi distinct poses, in increasing pose order."""
    return [sorted(int(k) for k in rng.choice(n_poses, int(rng.integers(lo, hi + 1)), replace=False))
            for _ in range(n_points)]


def case(prob, iters=(5, 10), **facts):
    return SimpleNamespace(prob=prob, iters=iters, **facts)


# ---------------------------------------------------------------------------
# the named graphs
# ---------------------------------------------------------------------------
def _fixed(n, which):
    f = np.zeros(n, np.uint8)
    f[list(which)] = 1
    return f


def _unused(id_order=False):
    """Pose 3 (free) and pose 5 (fixed), points 0, 17 and 39 without an edge:
    inactive entries in the middle and at both ends of lba_rank's scans, fewer
    pose blocks (3) than free poses (4)."""
    rng = np.random.default_rng(101)
    obs = [sorted(int(k) for k in rng.choice([0, 1, 2, 4], int(rng.integers(3, 5)), replace=False)) for _ in range(40)]
    idle_points = (0, 17, 39)
    for p in idle_points:
        obs[p] = []
    prob = graph(arc(6), _fixed(6, (0, 5)), cloud(40, rng), obs, seed=1, id_order=id_order)
    return case(prob, idle_poses=(3, 5), idle_points=idle_points)


def _thin():
    """Points with one or two edges among ordinary ones (point_nobs = 9, as
    if the other observations were outside the local window)."""
    rng = np.random.default_rng(102)
    obs = random_obs(40, 6, 3, 6, rng)
    obs[3] = [2]          # one edge, to a free pose
    obs[8] = [0]          # one edge, to a fixed pose
    obs[13] = [0, 5]      # two edges, both fixed
    obs[21] = [1, 4]      # two edges, both free
    obs[30] = [2, 3]      # two edges and two observations in all: the first is gross
    prob = graph(arc(6), _fixed(6, (0, 5)), cloud(40, rng), obs, seed=2, gross=[(30, 2)],
                 point_nobs={**{p: 9 for p in range(40)}, 30: 2})
    return case(prob, thin_points=(3, 8, 13, 21), gross_point=30)


def _away(free):
    """A seventh camera that every point is behind.  Fixed: three exact
    edges, each in the middle of its (exact) point's edges.  Free: index and id 3 of
    7 (the middle pose block of pass 1), eight exact edges; all of them leave
    in pass 1, so pass 2 has one pose block less and the blocks after it
    move down."""
    rng = np.random.default_rng(103)
    base = arc(6)
    if free:
        poses = base[:3] + [away(base[3])] + base[3:]
        fixed, cam, ordinary = _fixed(7, (0, 6)), 3, [0, 1, 2, 4, 5, 6]
        seen = (2, 7, 11, 16, 23, 28, 31, 36)
    else:
        poses = base + [away(base[2])]
        fixed, cam, ordinary = _fixed(7, (0, 5, 6)), 6, [0, 1, 2, 3, 4, 5]
        seen = (4, 19, 33)
    obs = []
    for p in range(40):
        o = sorted(int(k) for k in rng.choice(ordinary, int(rng.integers(4, 7)), replace=False))
        if p in seen:
            o.insert(len(o) // 2, cam)
        obs.append(o)
    # fixed: the three points' other edges are exact too, so the points end
    # where the away camera's observation has them (its chi2 stays ~0 after
    # pass 2 has dropped it: nothing but the depth rejects the edge)
    exact = [(p, cam) for p in seen] if free else [(p, k) for p in seen for k in obs[p]]
    prob = graph(poses, fixed, cloud(40, rng), obs, seed=14, exact=exact, point_nobs=9)
    return case(prob, away_pose=cam, away_edges=[edge(prob, p, cam) for p in seen])


def _point_leaves():
    """Every edge of points 5 and 9 is gross.  Point 5 (12 observations)
    loses all five edges and stays a good point: it leaves the pass-2 graph
    without being bad.  Point 9 (5 observations) goes bad at its third
    outlier: its last two edges are skipped, keep status 0 and stay in the
    pass-2 graph."""
    rng = np.random.default_rng(104)
    obs = [sorted(int(k) for k in rng.choice(6, 5, replace=False)) for _ in range(40)]
    gross = [(p, k) for p in (5, 9) for k in obs[p]]
    prob = graph(arc(6), _fixed(6, (0, 5)), cloud(40, rng), obs, seed=4, gross=gross, point_nobs={5: 12})
    return case(prob, leaves=5, goes_bad=9)


def _all_behind():
    """Two away cameras (fixed, free), ten points, twenty exact edges: the
    first pass rejects every edge on depth alone, the second optimize() has
    an empty graph."""
    rng = np.random.default_rng(105)
    base = arc(2)
    prob = graph([away(base[0]), away(base[1])], _fixed(2, (0,)), cloud(10, rng), [[0, 1]] * 10, seed=5,
                 exact=[(p, k) for p in range(10) for k in (0, 1)], point_nobs=9)
    return case(prob)


def _no_edges():
    rng = np.random.default_rng(106)
    prob = graph(arc(2), _fixed(2, (0,)), cloud(10, rng), [[]] * 10, seed=6)
    return case(prob)


def _thr(thr, not_float=False):
    """One 5-pose, 40-point graph under two gates (and two Huber widths)."""
    rng = np.random.default_rng(107)
    obs = random_obs(40, 5, 3, 5, rng)
    gross = [(p, obs[p][1]) for p in (6, 22)]
    prob = graph(arc(5), _fixed(5, (0, 4)), cloud(40, rng), obs, seed=7, gross=gross, chi2_threshold=thr,
                 not_float=not_float)
    return case(prob)


def _poses(n_free):
    """n_free free poses between two fixed ones, 128 | 129: k_lba_build's
    LDS pose tables (kBuildPoses = 128) | its wave-per-pose lists and atomic
    counts.  60 points; free pose j sees points j mod 59 and (j + 31) mod 59
    (4-6 free edges per point), point 59 two poses only, point 0 eleven, and
    every third point both fixed poses."""
    rng = np.random.default_rng(108)
    n = n_free + 2
    obs = [[] for _ in range(60)]
    for j in range(n_free):
        obs[j % 59].append(1 + j)
        obs[(j + 31) % 59].append(1 + j)
    for p in range(0, 59, 3):
        obs[p] += [0, n - 1]
    obs[59] = [0, 7]
    while len(obs[0]) < 11:
        k = int(rng.integers(1, n - 1))
        if k not in obs[0]:
            obs[0].append(k)
    obs = [sorted(o) for o in obs]
    prob = graph(arc(n), _fixed(n, (0, n - 1)), cloud(60, rng), obs, seed=8)
    return case(prob, iters=(2, 2))


def _points(n_points):
    """8192 | 8193 active points: k_lba_build's per-point counts and cursors
    in LDS (kBuildPoints = 8192) | in global memory."""
    rng = np.random.default_rng(109)
    obs = [sorted(int(k) for k in rng.choice(5, 3, replace=False)) for _ in range(n_points)]
    prob = graph(arc(5), _fixed(5, (0, 4)), cloud(n_points, rng), obs, seed=9)
    return case(prob, iters=(2, 2))


def _wide(n_poses):
    """Four points seen by every one of 128 | 129 poses (18 free, the rest
    fixed): the most edges on one point is kSE = 128 | one more, the host's
    rule for splitting a problem over workgroups."""
    rng = np.random.default_rng(110)
    free = set(range(3, 3 + 6 * 18, 6))
    obs = random_obs(130, n_poses, 3, 6, rng)
    for p in (0, 43, 88, 129):
        obs[p] = list(range(n_poses))
    for i, k in enumerate(sorted(free)):   # every free pose well observed
        for p in range(1 + i, 129, 9):
            if k not in obs[p]:
                obs[p] = sorted(obs[p] + [k])
    prob = graph(arc(n_poses), _fixed(n_poses, set(range(n_poses)) - free), cloud(130, rng), obs, seed=10)
    return case(prob)


def _sparse_free():
    """3 free and 6 fixed poses; 150 points with one free and two fixed
    edges, 50 (every fourth) with fixed edges only."""
    rng = np.random.default_rng(111)
    free, fixed = (2, 4, 6), (0, 1, 3, 5, 7, 8)
    obs = []
    for p in range(200):
        o = [int(k) for k in rng.choice(fixed, 2 if p % 4 else 3, replace=False)]
        if p % 4:
            o.append(free[(p // 4) % 3])
        obs.append(sorted(o))
    prob = graph(arc(9), _fixed(9, fixed), cloud(200, rng), obs, seed=11)
    return case(prob)


def _dense_free():
    """20 free and 3 fixed poses, 130 points each seen by all 23."""
    rng = np.random.default_rng(112)
    prob = graph(arc(23), _fixed(23, (0, 11, 22)), cloud(130, rng), [list(range(23))] * 130, seed=12)
    return case(prob)


GRAPHS = {
    "unused": _unused,
    "unused_ids": lambda: _unused(id_order=True),
    "thin": _thin,
    "away_fixed": lambda: _away(False),
    "away_free": lambda: _away(True),
    "point_leaves": _point_leaves,
    "all_behind": _all_behind,
    "no_edges": _no_edges,
    "thr2": lambda: _thr(2.0),
    "thr6": lambda: _thr(THR),
    "rec_double": lambda: _thr(THR, not_float=True),
    "poses128": lambda: _poses(128),
    "poses129": lambda: _poses(129),
    "points8192": lambda: _points(8192),
    "points8193": lambda: _points(8193),
    "wide128": lambda: _wide(128),
    "wide129": lambda: _wide(129),
    "sparse_free": _sparse_free,
    "dense_free": _dense_free,
}
# small enough for the dense numpy restatement (at most about 400 edges)
SMALL = ["unused", "unused_ids", "thin", "away_fixed", "away_free", "point_leaves", "all_behind", "no_edges", "thr2",
         "thr6", "rec_double", "poses128", "poses129"]


@functools.lru_cache(maxsize=None)
def named(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, iters=None):
    """The oracle's result for a named graph (cached, shared by the tests;
    read-only): (arrays, edge status, bad points, statistics)."""
    from test_lba_numpy import run_ref
    c = named(name)
    arrs, es, pb, st = run_ref(c.prob, *(iters or c.iters))
    for a in list(arrs.values()) + [es, pb]:
        a.setflags(write=False)
    return arrs, es, pb, st


def counts(prob):
    """(free poses with an edge, points with an edge, most edges on one point,
    most free edges on one point)."""
    ep, ek = prob["edge_point"], prob["edge_pose"]
    free = prob["pose_fixed"][ek] == 0
    per_point = np.bincount(ep, minlength=len(prob["points"]))
    per_point_free = np.bincount(ep[free], minlength=len(prob["points"]))
    return (len(set(ek[free].tolist())), int(np.count_nonzero(per_point)), int(per_point.max(initial=0)),
            int(per_point_free.max(initial=0)))
