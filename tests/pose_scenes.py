"""Constructed scenes for the keyframe projection searches under general
camera poses, and a float64 restatement of each search (test data and
checker only).

The searches: Fuse in both overloads (src/ORBmatcher.cc:1016-1265),
SearchByProjection(KF, Scw) (:286-407), SearchByProjection(Frame, KF)
(:1622-1746) and SearchBySim3 (:1267-1505); and Frame::isInFrustum
(src/Frame.cc:136-197) ahead of the local-map search, on the same scenes.

Poses.  Built in float64 by Rodrigues' formula and rounded to float32
row-major, as the ABI takes them.  A rotation about a coordinate axis has
four zero entries, so every named pose is its main rotation (0.4 or 1.2 rad
about x, y or z; 0.9 rad about (1,2,3)/sqrt(14); 2.8 rad about y, which looks
back) followed by the fixed tilt TILT (0.2 rad about the next axis, then 0.1
about the third): all nine entries of R are non-zero and no off-diagonal
entry equals its transpose.  Translations have three unequal non-zero
components.  The Scw entry points take s [R | t] with s = 0.6 or 1.7.

Searched keyframes are lists of keypoints at integer pixels with constructed
descriptors (area_scenes' bits(n) and far()): a candidate's distance to the
all-zero query descriptor is its bit count.  Groups stand on a 40 px lattice;
the largest radius is TH * 1.2^7 < 22 px and candidates lie within 4 px of
their group's centre (6 px for the tie rows), so a group's search box holds its own candidates only.

Map points are built backwards: target pixel, camera-frame depth and target
level first, then Xw = R^T (Xc - t) in float64 rounded to float32, and the
normal / min_dist / max_dist from PO = Xw - Ow so that the point passes or
fails each gate by a chosen margin.

reference() restates a search in float64: projection, the gates in the
reference's order and with its comparison operators, lower_bound for the
predicted level, GetFeaturesInArea order (cell x, cell y, index), the first
strict minimum, the accept threshold, the sequential `taken` state, the
rotation histogram, and SearchBySim3's mutual agreement.  Per point it
reports the gate that rejected it or the winner, and whether the point is
*decided*: every comparison of the float64 run clears MARGIN_PX = 0.01 px
(image bounds, search box, cell range) or MARGIN_REL = 1e-4 (z, dist3D
against min/max distance, ratio against every scale factor, the viewing
cosine against 0.5), and |z| >= MIN_Z so that 1/z is well conditioned.  The
margins are at least 100 x what a dozen float32 roundings (eps 6e-8) can move
those quantities; they are conditions on the inputs, not tolerances on the
results.  In the sequential searches an undecided point taints the keypoints
it could have taken, and a later point that could take a tainted keypoint is
undecided too.

The gate "empty" is GetFeaturesInArea returning nothing (no keypoint of the
level window in the box).  Its early returns on an empty *cell range* cannot
be reached from an in-image centre with a positive radius: u >= min_x gives
ceil((u - min_x + r) winv) >= 0 and u <= max_x gives floor((u - min_x - r)
winv) < 64.

Exact edges (u == max_x, dist3D == min_dist, ratio == a scale factor, a
keypoint on the box edge ...) stand in exact_scene(): identity pose, camera
(256, 256, 320, 240), coordinates that are dyadic rationals, so every
quantity of the float32 run is exact and equals the float64 one.  Its points
are decided by that exactness (the margins do not apply; the scene's
`exact` flag says so).
"""
import ctypes

import numpy as np

import orb_slam_amd as ox
from area_scenes import H, W, bits, far, scale_factors
from oracle_lib import KEYPOINT, load, ptr
from proj_data import MapPointView
from test_match_numpy import COLS, HISTO, POP, ROWS, three_maxima
from test_proj_numpy import rot_bin

F32 = np.float32
CAM = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
CAM_EXACT = np.array([256.0, 256.0, 320.0, 240.0], np.float32)
BOUNDS_IMAGE = (0.0, float(W), 0.0, float(H))
BOUNDS_UNDIST = (-13.5, 655.25, -9.75, 490.5)     # Frame::ComputeImageBounds of a distorted camera
TH = 6.0
TH_LOW, TH_HIGH = 50, 100
INT_MAX = 0x7fffffff
SET_BY_CALLER = 10 ** 6
MARGIN_PX, MARGIN_REL, MIN_Z = 0.01, 1e-4, 0.05
SF = scale_factors()
NLEV = len(SF)
ENTRIES = ("fuse0", "fuse1", "kfsim3", "framekf")

# gates of each entry point, in the reference's order
GATES = {
    "fuse0": ("z", "umin", "umax", "vmin", "vmax", "dmin", "dmax", "cos", "empty"),
    "fuse1": ("z", "umin", "umax", "vmin", "vmax", "dmin", "dmax", "cos", "empty"),
    "kfsim3": ("skip", "z", "umin", "umax", "vmin", "vmax", "dmin", "dmax", "cos", "empty", "taken", "thresh"),
    "framekf": ("skip", "umin", "umax", "vmin", "vmax", "empty", "taken", "thresh"),
    "sim3": ("skip", "z", "umin", "umax", "vmin", "vmax", "dmin", "dmax", "empty", "thresh"),
    "frustum": ("skip", "z", "umin", "umax", "vmin", "vmax", "dmin", "dmax", "cos"),
}


# ---------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


AXES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}
NEXT = {"x": "y", "y": "z", "z": "x", "g": "x"}


def tilted(axis, angle):
    """Main rotation, then TILT: 0.2 rad about the next axis, 0.1 about the third."""
    name = axis if isinstance(axis, str) else "g"
    main = rodrigues(AXES[axis] if isinstance(axis, str) else axis, angle)
    nxt = NEXT[name]
    return rodrigues(AXES[NEXT[nxt]], 0.1) @ rodrigues(AXES[nxt], 0.2) @ main


POSES = {
    "x0.4": (tilted("x", 0.4), (0.31, -0.17, 0.45)),
    "x1.2": (tilted("x", 1.2), (-0.52, 0.23, 0.11)),
    "y0.4": (tilted("y", 0.4), (0.12, 0.37, -0.29)),
    "y1.2": (tilted("y", 1.2), (-0.21, -0.43, 0.64)),
    "z0.4": (tilted("z", 0.4), (0.47, 0.15, -0.33)),
    "z1.2": (tilted("z", 1.2), (-0.14, 0.58, 0.26)),
    "axis0.9": (tilted(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), 0.9), (0.25, -0.61, 0.38)),
    "back2.8": (tilted("y", 2.8), (-0.35, 0.19, 0.72)),
}
SIM3_SCALES = (0.6, 1.7)


def pose32(R, t, s=1.0):
    """4x4 row-major float32 of s [R | t]."""
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R, np.float64)
    T[:3, 3] = s * np.asarray(t, np.float64)
    return np.ascontiguousarray(T.astype(np.float32))


def pose_parts64(T, sim3):
    """Rcw, tcw, Ow in float64 from the float32 matrix the call receives."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    s = np.sqrt(T[0, :3] @ T[0, :3]) if sim3 else 1.0
    R, t = T[:3, :3] / s, T[:3, 3] / s
    return R, t, -R.T @ t


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
class Keyframe:
    """Keypoints, descriptors, bounds; the float64 grid cell of each keypoint."""

    def __init__(self, keys, desc, bounds=BOUNDS_IMAGE):
        self.keys, self.desc, self.bounds = keys, np.ascontiguousarray(desc), tuple(float(b) for b in bounds)
        self.n = len(keys)
        mnx, mxx, mny, mxy = self.bounds
        self.winv, self.hinv = COLS / (mxx - mnx), ROWS / (mxy - mny)
        gx = (keys["x"].astype(np.float64) - mnx) * self.winv
        gy = (keys["y"].astype(np.float64) - mny) * self.hinv
        # no keypoint within 1e-3 of a cell's rounding boundary
        assert (np.abs(gx - np.floor(gx) - 0.5) > 1e-3).all() and (np.abs(gy - np.floor(gy) - 0.5) > 1e-3).all()
        cx, cy = np.floor(gx + 0.5).astype(np.int64), np.floor(gy + 0.5).astype(np.int64)
        ok = (cx >= 0) & (cx < COLS) & (cy >= 0) & (cy < ROWS)
        self.cx, self.cy = cx, cy
        self.cell = np.where(ok, cx * ROWS + cy, -1)
        self.x, self.y = keys["x"].astype(np.float64), keys["y"].astype(np.float64)
        self.oct = keys["octave"].astype(np.int64)

    def view(self):
        v = ox.frame_view(self.keys, self.desc, W, H)
        v.min_x, v.max_x, v.min_y, v.max_y = self.bounds
        return v


class Scene:
    """One searched keyframe, the map points and one pose: the inputs of all
    four single-keyframe entry points."""

    def __init__(self, name, K, mp, T, R, t, cam, skip, taken, angles, rows, exact=False):
        self.name, self.K, self.mp, self.T, self.R, self.t, self.cam = name, K, mp, T, R, t, cam
        self.skip, self.taken, self.rows, self.exact = skip, taken, rows, exact
        self.nq = len(mp["pos"])
        self.qkeys = np.zeros(self.nq, KEYPOINT)       # the Frame/KF search's keyframe: only the angles are read
        self.qkeys["angle"] = angles
        self.qkeys["size"] = 31.0

    def pose(self, entry, s=1.7):
        """The matrix the entry point takes: Tcw, or Scw = s [R | t]."""
        return pose32(self.R, self.t, s) if entry in ("fuse1", "kfsim3") else self.T

    def mpview(self, nq=None):
        return mp_view(self.mp, self.nq if nq is None else nq)


class Builder:
    def __init__(self, R, t, cam, bounds, seed, cam_dist=False):
        """World to camera: Xc = R Xw + t (R a rotation, or for SearchBySim3
        the similarity both transforms make up; cam_dist: dist3D is the
        camera point's norm, as there)."""
        self.R, self.t = np.asarray(R, np.float64), np.asarray(t, np.float64)
        self.cam, self.bounds, self.cam_dist = cam, bounds, cam_dist
        self.rng = np.random.default_rng(seed)
        self.p, self.c = [], []
        self.rows = {}       # gate -> (rejected point, passing neighbour)
        self.expect = {}     # point -> candidate id (or -1), per entry family, by construction
        self.pin = {}        # candidate id -> final index
        self.above = []      # (a, b): candidate a gets a larger index than b
        spots = [(40 + 40 * ix, 40 + 40 * iy) for iy in range(11) for ix in range(15)]
        self.spots = iter(spots)

    def spot(self):
        return next(self.spots)

    def point(self, px, py, z=4.0, oct=2, ratio=None, dmax=1.5, cos=1.0, desc=None, skip=0, angle=0.0):
        """Target pixel (px, py) at camera depth z; ratio = dist3D / min_dist
        (default: between scale[oct - 1] and scale[oct], so the predicted
        level is oct); max_dist = dmax * dist3D; `cos` between PO and the
        normal."""
        if ratio is None:
            ratio = float(SF[oct]) * 0.93
        self.p.append(dict(px=px, py=py, z=z, ratio=ratio, dmax=dmax, cos=cos,
                           desc=np.zeros(32, np.uint8) if desc is None else desc, skip=skip, angle=angle))
        return len(self.p) - 1

    def cand(self, x, y, oct, desc, taken=0, angle=0.0):
        mnx, mxx, mny, mxy = self.bounds
        while abs(((x - mnx) * COLS / (mxx - mnx)) % 1 - 0.5) < 0.02:     # off the cells' rounding boundaries
            x += 1
        while abs(((y - mny) * ROWS / (mxy - mny)) % 1 - 0.5) < 0.02:
            y += 1
        self.c.append(dict(x=x, y=y, oct=oct, desc=desc, taken=taken, angle=angle))
        return len(self.c) - 1

    def row(self, gate, rejected, passing):
        self.rows[gate] = (rejected, passing)

    def finish(self, name, n_total=None, exact=False):
        rng, fx, fy, cx, cy = self.rng, *[float(c) for c in self.cam]
        if n_total is not None:          # never-accepted keypoints up to n_total, anywhere on the grid
            while len(self.c) < n_total:
                x, y = int(rng.integers(0, 63)) * 10 + int(rng.integers(-4, 5)), int(rng.integers(0, 47)) * 10 + int(rng.integers(-4, 5))
                self.cand(max(x, 0), max(y, 0), int(rng.integers(0, NLEV)), far(rng))
        n = len(self.c)
        cpos = np.full(n, -1, np.int64)
        pinned = set(self.pin.values())
        free = [i for i in rng.permutation(n) if i not in pinned]
        for cid, at in self.pin.items():
            cpos[cid] = at
        rest = [cid for cid in range(n) if cid not in self.pin]
        cpos[rest] = free
        for a, b in self.above:
            if cpos[a] < cpos[b]:
                cpos[a], cpos[b] = cpos[b], cpos[a]
        corder = np.empty(n, np.int64)
        corder[cpos] = np.arange(n)
        keys = np.zeros(n, KEYPOINT)
        for f, key in (("x", "x"), ("y", "y"), ("octave", "oct"), ("angle", "angle")):
            keys[f] = [self.c[i][key] for i in corder]
        keys["size"] = 31.0
        desc = np.array([self.c[i]["desc"] for i in corder], np.uint8).reshape(n, 32)
        taken = np.array([self.c[i]["taken"] for i in corder], np.uint8)
        # the map points, backwards
        P = self.p
        z = np.array([q["z"] for q in P], np.float64)
        Xc = np.stack([(np.array([q["px"] for q in P], np.float64) - cx) / fx * z,
                       (np.array([q["py"] for q in P], np.float64) - cy) / fy * z, z], 1)
        Rinv = np.linalg.inv(self.R)                               # R^T for a rotation
        Xw = ((Xc - self.t) @ Rinv.T).astype(np.float32)           # rows of R^-1 (Xc - t)
        Ow = -Rinv @ self.t
        PO = Xw.astype(np.float64) - Ow
        dist = np.linalg.norm(Xw.astype(np.float64) @ self.R.T + self.t if self.cam_dist else PO, axis=1)
        nrm = np.empty_like(PO)
        for i, q in enumerate(P):
            e = PO[i] / dist[i]
            o = np.cross(e, [0.3, -0.5, 0.8])
            o /= np.linalg.norm(o)
            nrm[i] = q["cos"] * e + np.sqrt(1 - q["cos"] ** 2) * o
        mp = {"pos": np.ascontiguousarray(Xw), "normal": np.ascontiguousarray(nrm.astype(np.float32)),
              "min_dist": (dist / np.array([q["ratio"] for q in P])).astype(np.float32),
              "max_dist": (dist * np.array([q["dmax"] for q in P])).astype(np.float32),
              "desc": np.ascontiguousarray(np.array([q["desc"] for q in P], np.uint8).reshape(len(P), 32))}
        s = Scene(name, Keyframe(keys, desc, self.bounds), mp, pose32(self.R, self.t), self.R, self.t, self.cam,
                  np.array([q["skip"] for q in P], np.uint8), taken, [q["angle"] for q in P], dict(self.rows), exact)
        s.cpos = cpos
        s.expect = {k: {p: (int(cpos[c]) if c >= 0 else -1) for p, c in v.items()} for k, v in self.expect.items()}
        return s


ONE = np.array([0b11111] + [0] * 31, np.uint8)      # two descriptors five bits from zero
TWO = np.array([0, 0b11111] + [0] * 30, np.uint8)


def inside(bounds, px, py):
    """The integer pixel nearest (px, py) that is at least 1 px inside the
    bounds and inside the grid's last cell."""
    mnx, mxx, mny, mxy = bounds
    x = int(min(max(round(px), np.ceil(mnx) + 1), np.floor(mnx + 63.4 * (mxx - mnx) / COLS)))
    y = int(min(max(round(py), np.ceil(mny) + 1), np.floor(mny + 47.4 * (mxy - mny) / ROWS)))
    return x, y


def add_gate_rows(b):
    """A rejected point and a passing neighbour for every gate, each with an
    acceptable candidate (3 bits) of its level at its own spot."""
    mnx, mxx, mny, mxy = b.bounds

    def own(px, py, oct=2, d=3, **kw):
        return b.cand(*inside(b.bounds, px, py), oct, bits(d), **kw)

    def pair(gate, rej, acc):
        pts = []
        for kw in (rej, acc):
            kw = dict(kw)
            px, py = kw.pop("at", None) or b.spot()
            own(px, py, kw.get("oct", 2))
            pts.append(b.point(px, py, **kw))
        b.row(gate, *pts)
        return pts

    pair("z", dict(z=-4.0), dict(z=4.0))
    x0, y0 = 320, 200
    pair("umin", dict(at=(mnx - 0.5, y0)), dict(at=(mnx + 0.5, y0)))
    pair("umax", dict(at=(mxx + 0.5, y0 + 80)), dict(at=(mxx - 0.5, y0 + 80)))
    pair("vmin", dict(at=(x0, mny - 0.5)), dict(at=(x0, mny + 0.5)))
    pair("vmax", dict(at=(x0 + 80, mxy + 0.5)), dict(at=(x0 + 80, mxy - 0.5)))
    pair("dmin", dict(ratio=0.99), dict(ratio=1.01, oct=1))
    pair("dmax", dict(dmax=0.99), dict(dmax=1.01))
    pair("cos", dict(cos=0.45), dict(cos=0.55))
    # nothing of the level window in the box / something
    e = b.spot()
    b.cand(e[0], e[1], 5, bits(1))                 # wrong level for every search at pred 2
    b.cand(e[0] + 14, e[1], 2, bits(1))            # right level, outside the box (r = 8.64)
    g = b.spot()
    own(*g)
    b.row("empty", b.point(*e), b.point(*g))
    # masks: a skipped point beside one that is searched
    g1, g2 = b.spot(), b.spot()
    own(*g1), own(*g2)
    b.row("skip", b.point(*g1, skip=1), b.point(*g2))
    # the nearest candidate already taken / assigned: the next one wins
    g = b.spot()
    b.cand(g[0] - 2, g[1] + 1, 2, bits(2), taken=1)
    second = b.cand(g[0] + 2, g[1] - 1, 2, bits(9))
    p_taken = b.point(*g)
    g = b.spot()
    b.cand(g[0], g[1], 2, bits(2), taken=1)        # its only candidate taken
    b.row("taken", b.point(*g), p_taken)
    b.expect.setdefault("seq", {})[p_taken] = second
    # accept thresholds: 40 | 41, 50 | 51, 100 | 101
    th = {}
    for d in (40, 41, 50, 51, 100, 101):
        g = b.spot()
        c = b.cand(g[0] + 1, g[1] - 2, 2, bits(d))
        th[d] = (b.point(*g), c)
    b.thresh = th
    b.row("thresh", th[101][0], th[40][0])
    # level windows: candidates at pred - 2 .. pred + 2 around pred = 3
    g = b.spot()
    b.cand(g[0] - 1, g[1], 1, bits(1))
    lo = b.cand(g[0] + 1, g[1], 2, bits(5))
    p_lo = b.point(*g, oct=3)
    g = b.spot()
    at = b.cand(g[0] - 1, g[1] + 1, 3, bits(7))
    up = b.cand(g[0] + 1, g[1], 4, bits(3))
    b.cand(g[0], g[1] - 1, 5, bits(2))
    p_hi = b.point(*g, oct=3)
    b.levels = (p_lo, p_hi)
    b.expect.setdefault("fuse", {}).update({p_lo: lo, p_hi: at})
    b.expect.setdefault("framekf", {}).update({p_lo: lo, p_hi: up})
    # predicted level 0 (ratio below 1: only the Frame/KF search has no min_dist gate) and the clamp at nlevels - 1
    g = b.spot()
    c0 = b.cand(g[0], g[1], 0, bits(4))
    b.cand(g[0] + 1, g[1] + 1, 2, bits(1))
    p0 = b.point(*g, ratio=0.9)
    g = b.spot()
    c7 = b.cand(g[0], g[1], NLEV - 1, bits(4))
    b.cand(g[0] + 2, g[1] + 1, NLEV - 3, bits(1))
    p7 = b.point(*g, ratio=float(SF[-1]) * 1.3, dmax=1.5)
    b.pred_edges = (p0, p7)
    b.expect["framekf"].update({p0: c0, p7: c7})
    b.expect["fuse"].update({p7: c7})
    # ties: equal best distances in cells that differ in ix, in iy, and in one cell; the earlier
    # cell's (the lower index's) candidate wins, whichever of the two has the larger index
    tie = []
    for kind, (dx1, dy1), (dx2, dy2) in (("ix", (-6, 1), (6, 1)), ("iy", (1, -6), (1, 6)), ("cell", (1, 1), (2, 2))):
        for hi_first in ((True, False) if kind != "cell" else (False,)):
            g = b.spot()
            first = b.cand(g[0] + dx1, g[1] + dy1, 2, ONE)
            second = b.cand(g[0] + dx2, g[1] + dy2, 2, TWO)
            b.above.append((first, second) if hi_first else (second, first))
            tie.append((kind, b.point(*g), first, second))
    b.ties = tie
    for _, p, c, _ in tie:
        b.expect["fuse"][p] = c
    # a chain: three points that want one keypoint
    g = b.spot()
    cs = [b.cand(g[0] + k - 1, g[1], 2, bits(k + 1)) for k in range(3)]
    ps = [b.point(*g) for _ in range(3)]
    b.chain = ps
    for k in range(3):
        b.expect["fuse"][ps[k]] = cs[0]
        b.expect["seq"][ps[k]] = cs[k]


def add_rotation(b):
    """Matches in rotation bins 0, 3 and 6 (the population fills the same
    three) and one in bin 9: the three-maxima rule removes that one."""
    pts = []
    for a in [0.0, 0.0, 90.0, 90.0, 180.0, 180.0, 270.0]:
        g = b.spot()
        b.cand(g[0], g[1], 2, bits(2))
        pts.append(b.point(*g, angle=a))
    b.rotation = pts


def add_population(b, n):
    """Unrelated points: random pixels in and around the image, depths on both
    sides of the camera, random ranges and normals; a candidate near most."""
    rng = b.rng
    mnx, mxx, mny, mxy = b.bounds
    for _ in range(n):
        px, py = rng.uniform(mnx - 30, mxx + 30), rng.uniform(mny - 30, mxy + 30)
        o = int(rng.integers(1, NLEV))
        z = float(rng.uniform(1.0, 8.0)) * (-1 if rng.random() < 0.15 else 1)
        if rng.random() < 0.8 and mnx + 6 < px < min(mxx, 634) - 6 and mny + 6 < py < min(mxy, 474) - 6 and px > 6 and py > 6:
            x, y = int(round(px)) + int(rng.integers(-3, 4)), int(round(py)) + int(rng.integers(-3, 4))
            b.cand(x, y, o - int(rng.integers(0, 2)), bits(int(rng.integers(1, 120))), taken=int(rng.random() < 0.1))
        b.point(px, py, z=z, oct=o, ratio=float(SF[o]) * rng.uniform(0.85, 0.99) if rng.random() < 0.8 else rng.uniform(0.7, 5.0),
                dmax=rng.choice([1.5, 1.5, 1.5, 0.9]), cos=rng.uniform(0.2, 1.0), skip=int(rng.random() < 0.1),
                angle=float(rng.choice([0.0, 3.0, 90.0, 92.0, 180.0, 178.0])))


def gate_scene(pose, bounds=BOUNDS_IMAGE, seed=0, population=215):
    R, t = POSES[pose]
    b = Builder(R, t, CAM, bounds, seed)
    add_gate_rows(b)
    add_rotation(b)
    add_population(b, population)
    s = b.finish(f"{pose}-{'image' if bounds == BOUNDS_IMAGE else 'undist'}")
    s.thresh = {d: (p, int(s.cpos[c])) for d, (p, c) in b.thresh.items()}
    s.levels, s.pred_edges, s.chain, s.rotation = b.levels, b.pred_edges, b.chain, b.rotation
    s.ties = [(kind, p, int(s.cpos[c]), int(s.cpos[c2])) for kind, p, c, c2 in b.ties]
    return s


SIZE_WINNERS = (0, 63, 64, 4032, 4095)


def size_scene(pose="axis0.9", n=4096, seed=11):
    """A searched keyframe of n keypoints: decided winners at indices 0, 63,
    64, 4032 and n - 1; index n - 1 stands in cell 0 and index 0 in the
    highest-numbered occupied cell (63, 47); a chain of three for the
    sequential searches; the rest never-accepted keypoints all over the grid."""
    R, t = POSES[pose]
    b = Builder(R, t, CAM, BOUNDS_IMAGE, seed)
    where = [(630, 470), (200, 120), (240, 120), (280, 120), (3, 3)]
    at = [0, 63, 64, n - 64, n - 1]
    b.expect["fuse"], b.expect["seq"] = {}, {}
    b.winners = []
    for (x, y), idx in zip(where, at):
        c = b.cand(x, y, 2, bits(3))
        b.pin[c] = idx
        p = b.point(x + 0.5, y - 0.5)
        b.expect["fuse"][p] = b.expect["seq"][p] = c
        b.winners.append(p)
    g = (400, 300)
    cs = [b.cand(g[0] + k - 1, g[1], 2, bits(k + 1)) for k in range(3)]
    for k in range(3):
        p = b.point(*g)
        b.expect["fuse"][p], b.expect["seq"][p] = cs[0], cs[k]
    for k in range(12):       # some ordinary groups beside them
        g = (60 + 40 * k, 200)
        b.cand(g[0] + 1, g[1] - 1, 2, bits(5 + k))
        b.point(*g, angle=0.0)
    s = b.finish(f"size{n}", n_total=n)
    s.winners = b.winners
    return s


def exact_scene():
    """Identity pose, camera (256, 256, 320, 240), dyadic coordinates: every
    float32 quantity of the searches is exact.  Rows, as (name, point):
    u == max_x and v == max_y (Fuse and KF/Scw reject, Frame/KF accepts),
    u == min_x, dist3D == min_dist, dist3D == max_dist, ratio == scale[1],
    a keypoint exactly on the box edge."""
    b = Builder(np.eye(3), np.zeros(3), CAM_EXACT, BOUNDS_IMAGE, 5)
    b.expect["fuse"], b.expect["framekf"] = {}, {}
    rows = {}
    # pixel = 256 * X / 2 + 320: depth 2, X a multiple of 1/128
    c = b.cand(634, 200, 1, bits(3))
    rows["u==max_x"] = b.point(640, 200, z=2.0, ratio=1.125, oct=1)
    b.expect["fuse"][rows["u==max_x"]], b.expect["framekf"][rows["u==max_x"]] = -1, c
    c = b.cand(200, 474, 1, bits(3))
    rows["v==max_y"] = b.point(200, 480, z=2.0, ratio=1.125, oct=1)
    b.expect["fuse"][rows["v==max_y"]], b.expect["framekf"][rows["v==max_y"]] = -1, c
    c = b.cand(4, 120, 1, bits(3))
    rows["u==min_x"] = b.point(0, 120, z=2.0, ratio=1.125, oct=1)
    b.expect["fuse"][rows["u==min_x"]] = b.expect["framekf"][rows["u==min_x"]] = c
    # PO = (1.5, 0, 2): dist3D = 2.5 exactly, u = 512
    c = b.cand(512, 240, 0, bits(3))
    e = b.cand(518, 244, 0, bits(1))       # |518 - 512| == r == 6: inside
    b.cand(519, 240, 0, bits(0))           # 7 > r: outside
    rows["dist==min_dist"] = b.point(512, 240, z=2.0, ratio=1.0, dmax=2.0)
    rows["box_edge"] = rows["dist==min_dist"]
    b.expect["fuse"][rows["dist==min_dist"]] = b.expect["framekf"][rows["dist==min_dist"]] = e
    # PO = (-1.5, 0, 2): dist3D == max_dist
    c = b.cand(128, 240, 1, bits(3))
    rows["dist==max_dist"] = b.point(128, 240, z=2.0, ratio=1.125, dmax=1.0)
    b.expect["fuse"][rows["dist==max_dist"]] = b.expect["framekf"][rows["dist==max_dist"]] = c
    # PO = (0, 0, scale[1]), min_dist 1: ratio == scale[1], lower_bound gives level 1 (window 0 .. 1), not 2
    # (Frame/KF: window 0 .. 2, not 1 .. 3)
    c = b.cand(320, 242, 0, bits(2))
    c2 = b.cand(322, 240, 2, bits(1))
    b.cand(318, 241, 3, bits(0))
    rows["ratio==scale"] = b.point(320, 240, z=float(SF[1]), ratio=float(SF[1]), dmax=2.0)
    b.expect["fuse"][rows["ratio==scale"]], b.expect["framekf"][rows["ratio==scale"]] = c, c2
    s = b.finish("exact", exact=True)
    s.exact_rows = rows
    return s


# ---------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------
class Result:
    def __init__(self, n):
        self.gate = ["?"] * n
        self.idx = np.full(n, -1, np.int64)
        self.dist = np.full(n, INT_MAX, np.int64)
        self.decided = np.ones(n, bool)
        self.removed = np.zeros(n, bool)       # Frame/KF: match removed by the rotation filter
        self.ori_stable = True                 # ... and the undecided points cannot change which bins it keeps


def _rel(a, b):
    return abs(a - b) >= MARGIN_REL * abs(b)


def project64(K, cam, R, t, Ow, Xw, normal, dmin, dmax, mode):
    """One point through the gates of `mode` ("fuse", "sim3", "framekf",
    "frustum": Frame::isInFrustum, src/Frame.cc:136-197, bounds inclusive).
    Returns (gate or None, u, v, pred, radius, decided).  For "sim3" R, t map
    the world point to the searched camera and dist3D is the camera point's
    norm; Ow is unused."""
    mnx, mxx, mny, mxy = K.bounds
    fx, fy, cx, cy = [float(c) for c in cam]
    Xc = R @ Xw + t
    ok = abs(Xc[2]) >= MIN_Z
    if mode != "framekf":
        ok &= abs(Xc[2]) >= MARGIN_REL * np.linalg.norm(Xc)
        if Xc[2] < 0:
            return "z", 0, 0, 0, 0, ok
    if Xc[2] == 0:
        return "z", 0, 0, 0, 0, False
    u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
    strict = mode in ("fuse", "sim3")
    for val, lo, hi, names in ((u, mnx, mxx, ("umin", "umax")), (v, mny, mxy, ("vmin", "vmax"))):
        ok &= abs(val - lo) >= MARGIN_PX and abs(val - hi) >= MARGIN_PX
        if val < lo:
            return names[0], u, v, 0, 0, ok
        if (val >= hi) if strict else (val > hi):
            return names[1], u, v, 0, 0, ok
    dist = np.linalg.norm(Xc) if mode == "sim3" else np.linalg.norm(Xw - Ow)
    if mode != "framekf":
        ok &= _rel(dist, dmin) and _rel(dist, dmax)
        if dist < dmin:
            return "dmin", u, v, 0, 0, ok
        if dist > dmax:
            return "dmax", u, v, 0, 0, ok
    if mode in ("fuse", "frustum"):
        c = (Xw - Ow) @ normal / dist
        ok &= abs(c - 0.5) >= MARGIN_REL
        if c < 0.5:
            return "cos", u, v, 0, 0, ok
    ratio = dist / dmin
    ok &= all(_rel(ratio, float(s)) for s in SF)
    pred = min(int(np.searchsorted(SF.astype(np.float64), ratio, side="left")), NLEV - 1)   # lower_bound
    return None, u, v, pred, float(F32(TH)) * float(SF[pred]), ok


def area64(K, u, v, r, lo, hi):
    """GetFeaturesInArea: indices in its order, and whether every test clears
    the pixel margin."""
    mnx, _, mny, _ = K.bounds
    ax0, ax1 = (u - mnx - r) * K.winv, (u - mnx + r) * K.winv
    ay0, ay1 = (v - mny - r) * K.hinv, (v - mny + r) * K.hinv
    x0, x1 = max(0, int(np.floor(ax0))), min(COLS - 1, int(np.ceil(ax1)))
    y0, y1 = max(0, int(np.floor(ay0))), min(ROWS - 1, int(np.ceil(ay1)))
    ok = abs(ax0 - COLS) >= MARGIN_PX * K.winv and abs(ax1) >= MARGIN_PX * K.winv
    ok &= abs(ay0 - ROWS) >= MARGIN_PX * K.hinv and abs(ay1) >= MARGIN_PX * K.hinv
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return np.zeros(0, np.int64), ok
    lvl = (K.oct >= lo) & (K.oct <= hi) & (K.cell >= 0)
    dx, dy = np.abs(K.x - u), np.abs(K.y - v)
    # a keypoint of a cell outside the range lies outside the box too (its cell is its rounded
    # position), so the box test alone decides; the cell range is checked for the record
    box = lvl & ~(dx > r) & ~(dy > r)
    near = lvl & (dx <= r + 1) & (dy <= r + 1)
    ok &= bool(((np.abs(dx[near] - r) >= MARGIN_PX) & (np.abs(dy[near] - r) >= MARGIN_PX)).all())
    idx = np.nonzero(box & (K.cx >= x0) & (K.cx <= x1) & (K.cy >= y0) & (K.cy <= y1))[0]
    assert len(idx) == int(box.sum())
    return idx[np.lexsort((idx, K.cell[idx]))], ok


def hamming(d, D):
    return POP[np.bitwise_xor(d[None, :], D)].sum(axis=1).astype(np.int64)


def reference(s, entry, scale=1.7, orb_dist=100, check_ori=0, nq=None):
    """Float64 restatement of one entry point over scene s: (Result, out, n)
    with `out` the call's output (best_idx / matched / matches_f) as far as
    the float64 run decides it."""
    K, mp = s.K, s.mp
    nq = s.nq if nq is None else nq
    sim3 = entry in ("fuse1", "kfsim3")
    R, t, Ow = pose_parts64(s.pose(entry, scale), sim3)
    mode = "framekf" if entry == "framekf" else "fuse"
    seq = entry in ("kfsim3", "framekf")
    lo_off, hi_off = (-1, 1) if entry == "framekf" else (-1, 0)
    accept = {"fuse0": INT_MAX, "fuse1": INT_MAX, "kfsim3": TH_LOW, "framekf": orb_dist}[entry]
    res = Result(nq)
    taken = s.taken.astype(bool).copy()
    tainted = np.zeros(K.n, bool)
    out = np.full(K.n, -1, np.int64)
    if entry == "kfsim3":
        out[taken] = SET_BY_CALLER
    pos, nrm = mp["pos"].astype(np.float64), mp["normal"].astype(np.float64)
    dmin, dmax = mp["min_dist"].astype(np.float64), mp["max_dist"].astype(np.float64)
    rmax = float(F32(TH)) * float(SF[-1]) + 1
    hist = [[] for _ in range(HISTO)]
    for m in range(nq):
        if seq and s.skip[m]:
            res.gate[m] = "skip"
            continue
        gate, u, v, pred, r, ok = project64(K, s.cam, R, t, Ow, pos[m], nrm[m], dmin[m], dmax[m], mode)
        idx = np.zeros(0, np.int64)
        if gate is None:
            idx, ok_area = area64(K, u, v, r, pred + lo_off, pred + hi_off)
            ok &= ok_area
            if len(idx) == 0:
                gate = "empty"
        if gate is None:
            if seq:
                ok &= not tainted[idx].any()
                idx = idx[~taken[idx]]
            if len(idx) == 0:
                gate = "taken"
            else:
                d = hamming(mp["desc"][m], K.desc[idx])
                k = int(np.argmin(d))          # first strict minimum in GetFeaturesInArea order
                res.idx[m], res.dist[m] = idx[k], d[k]
                gate = "win" if d[k] <= accept else "thresh"
                if gate == "win" and seq:
                    taken[idx[k]] = True
                    out[idx[k]] = m
                    if entry == "framekf" and check_ori:
                        hist[rot_bin(s.qkeys["angle"][m], K.keys["angle"][idx[k]])].append(m)
        res.gate[m], res.decided[m] = gate, bool(ok) or s.exact
        if seq and not res.decided[m]:
            if np.isfinite(u) and np.isfinite(v) and gate != "z":
                tainted |= (np.abs(K.x - u) <= rmax) & (np.abs(K.y - v) <= rmax)
            else:
                tainted[:] = True
    if entry == "framekf" and check_ori:
        keep = three_maxima(hist)
        # U undecided points can move a bin's count by U: the kept set stands when the third and
        # fourth counts are further apart and the 10 % rule holds with that slack
        U = int((~res.decided).sum())
        c = sorted((len(h) for h in hist), reverse=True)
        res.ori_stable = U == 0 or (c[2] - c[3] > 2 * U and c[2] - U >= 0.1 * (c[0] + U))
        for bno in range(HISTO):
            if bno not in keep:
                for m in hist[bno]:
                    res.removed[m] = True
                    out[res.idx[m]] = -1
    if not seq:
        return res, res.idx.copy(), None
    n = int(((out >= 0) & (out != SET_BY_CALLER)).sum())
    return res, out, n


def check_decided(s, entry, res, got, got_dist=None):
    """The decided points of `res` against a call's output `got` (best_idx for
    Fuse, matched / matches_f for the sequential searches).  Returns the
    undecided share."""
    nq = len(res.gate)
    check_removed = res.ori_stable
    for m in range(nq):
        if not res.decided[m]:
            continue
        if entry in ("fuse0", "fuse1"):
            want = (int(res.idx[m]), int(res.dist[m]))
            assert (int(got[m]), int(got_dist[m])) == want, (s.name, entry, m, res.gate[m], want)
        else:
            at = np.nonzero(got == m)[0]
            if res.gate[m] != "win" or (res.removed[m] and check_removed):
                assert len(at) == 0, (s.name, entry, m, res.gate[m], list(at))
            elif check_removed:
                assert list(at) == [int(res.idx[m])], (s.name, entry, m, res.gate[m], list(at), int(res.idx[m]))
    return 1.0 - float(res.decided.mean())


# ---------------------------------------------------------------------------
# the calls: the oracle's restatement, or with a context handle the library
# ---------------------------------------------------------------------------
def _oracle():
    L = load()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.orbx_ref_fuse_candidates.argtypes = [vp] * 8 + [vp, i, f, vp, vp]
    L.orbx_ref_search_by_projection_kf_sim3.argtypes = [vp, vp, i] + [vp] * 7 + [i, vp, vp]
    L.orbx_ref_search_by_projection_frame_kf.argtypes = [vp] * 9 + [f, i, i, vp, vp]
    L.orbx_ref_search_by_sim3.argtypes = [vp] * 15 + [f, vp, vp, f, vp, vp, vp]
    return L


def mp_view(mp, nq):
    v = MapPointView()
    v.n = nq
    for key, a in mp.items():
        setattr(v, key, a.ctypes.data)
    return v


def fuse_call(kv, cam, mp, nq, T, sim3, handle=None):
    """Fuse's candidates of the first nq points of mp in the keyframe view kv:
    (rc, best_idx, best_dist)."""
    bi, bd = np.full(max(nq, 1), -9, np.int32), np.full(max(nq, 1), -9, np.int32)
    if handle is None:
        rc = _oracle().orbx_ref_fuse_candidates(ctypes.byref(kv), ptr(cam), nq, ptr(mp["pos"]), ptr(mp["normal"]),
                                                ptr(mp["min_dist"]), ptr(mp["max_dist"]), ptr(mp["desc"]), ptr(T),
                                                sim3, TH, ptr(bi), ptr(bd))
    else:
        mv = mp_view(mp, nq)
        rc = ox.lib().orbx_fuse_candidates(handle, ctypes.byref(kv), ptr(cam), ctypes.byref(mv), ptr(T), sim3, TH,
                                           ptr(bi), ptr(bd))
    return rc, bi[:nq], bd[:nq]


def run(s, entry, handle=None, scale=1.7, orb_dist=100, check_ori=0, nq=None, view=None):
    """One entry point over scene s.  Fuse: (rc, best_idx, best_dist); the
    sequential searches: (rc, out, n)."""
    nq = s.nq if nq is None else nq
    kv = s.K.view() if view is None else view
    a, T = s.mp, s.pose(entry, scale)
    n = ctypes.c_int(-9)
    if entry in ("fuse0", "fuse1"):
        return fuse_call(kv, s.cam, s.mp, nq, T, int(entry == "fuse1"), handle)
    if entry == "kfsim3":
        out = np.where(s.taken != 0, SET_BY_CALLER, -1).astype(np.int32)
        if handle is None:
            rc = _oracle().orbx_ref_search_by_projection_kf_sim3(
                ctypes.byref(kv), ptr(s.cam), nq, ptr(a["pos"]), ptr(a["normal"]), ptr(a["min_dist"]),
                ptr(a["max_dist"]), ptr(a["desc"]), ptr(s.skip), ptr(T), int(TH), ptr(out), ctypes.byref(n))
        else:
            mv = s.mpview(nq)
            rc = ox.lib().orbx_search_by_projection_kf_sim3(handle, ctypes.byref(kv), ptr(s.cam), ctypes.byref(mv),
                                                            ptr(s.skip), ptr(T), int(TH), ptr(out), ctypes.byref(n))
        return rc, out, n.value
    assert entry == "framekf" and nq == s.nq
    out = np.full(max(s.K.n, 1), -9, np.int32)
    qv = ox.frame_view(s.qkeys, a["desc"], W, H)
    valid = (s.skip == 0).astype(np.uint8)
    if handle is None:
        rc = _oracle().orbx_ref_search_by_projection_frame_kf(
            ctypes.byref(kv), ctypes.byref(qv), ptr(s.cam), ptr(a["pos"]), ptr(a["min_dist"]), ptr(a["desc"]),
            ptr(valid), ptr(s.taken), ptr(T), TH, orb_dist, check_ori, ptr(out), ctypes.byref(n))
    else:
        mv = s.mpview()
        rc = ox.lib().orbx_search_by_projection_frame_kf(handle, ctypes.byref(kv), ctypes.byref(qv), ptr(s.cam),
                                                         ctypes.byref(mv), ptr(valid), ptr(s.taken), ptr(T), TH,
                                                         orb_dist, check_ori, ptr(out), ctypes.byref(n))
    return rc, out[:s.K.n], n.value


# ---------------------------------------------------------------------------
# Frame::isInFrustum ahead of the local-map search (orbx_search_local_map)
# ---------------------------------------------------------------------------
def reference_frustum(s):
    """Per point: the gate that rejects it (or "win": in view), u, v and the
    predicted level in float64, and whether the point is decided."""
    R, t, Ow = pose_parts64(s.T, 0)
    res = Result(s.nq)
    res.u, res.v, res.pred = np.zeros(s.nq), np.zeros(s.nq), np.zeros(s.nq, np.int64)
    mp = s.mp
    for m in range(s.nq):
        if s.skip[m]:
            res.gate[m] = "skip"
            continue
        gate, u, v, pred, _, ok = project64(s.K, s.cam, R, t, Ow, mp["pos"][m].astype(np.float64),
                                            mp["normal"][m].astype(np.float64), float(mp["min_dist"][m]),
                                            float(mp["max_dist"][m]), "frustum")
        res.gate[m], res.decided[m] = gate or "win", bool(ok) or s.exact
        res.u[m], res.v[m], res.pred[m] = u, v, pred
    return res


def run_frustum(s, handle=None):
    """orbx_search_local_map over scene s (th 1, nnratio 0.8): (rc, in_view,
    proj, pred, cos, matches, n_in_view, n_matches) from the oracle, or with
    a handle from the library."""
    from local_map_data import LocalMapQuery
    T, nq = s.T, max(s.nq, 1)
    kv = s.K.view()
    Ow = (-(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))).astype(np.float32)
    keep = dict(Rcw=np.ascontiguousarray(T[:3, :3]).reshape(-1), tcw=np.ascontiguousarray(T[:3, 3]), Ow=Ow, cam=s.cam,
                mp_pos=s.mp["pos"], mp_normal=s.mp["normal"],
                mp_dist=np.ascontiguousarray(np.stack([s.mp["min_dist"], s.mp["max_dist"]], 1)), mp_skip=s.skip,
                mp_desc=s.mp["desc"], f_assigned=s.taken, in_view=np.full(nq, 9, np.uint8),
                proj_xy=np.zeros((nq, 2), np.float32), pred_level=np.zeros(nq, np.int32),
                view_cos=np.zeros(nq, np.float32), matches_f=np.full(max(s.K.n, 1), -9, np.int32))
    q = LocalMapQuery()
    q.frame = ctypes.addressof(kv)
    for field, arr in keep.items():
        setattr(q, field, arr.ctypes.data)
    q.n_mp, q.view_cos_limit, q.th, q.nnratio = s.nq, 0.5, 1.0, 0.8
    if handle is None:
        L = load()
        L.orbx_ref_search_local_map.argtypes = [ctypes.c_void_p]
        rc = L.orbx_ref_search_local_map(ctypes.byref(q))
    else:
        rc = ox.lib().orbx_search_local_map(handle, ctypes.byref(q))
    return (rc, keep["in_view"], keep["proj_xy"], keep["pred_level"], keep["view_cos"], keep["matches_f"], q.n_in_view,
            q.n_matches)


# a dozen float32 roundings of pixel-sized values: 12 x 700 x 6e-8 = 5e-4 px
PROJ_BOUND = 1e-3


def check_frustum(s, res, got):
    """The decided points of reference_frustum against a call's outputs;
    returns the undecided share."""
    _, in_view, proj, pred, _, _, n_in, _ = got
    for m in range(s.nq):
        if not res.decided[m]:
            continue
        assert bool(in_view[m]) == (res.gate[m] == "win"), (s.name, m, res.gate[m])
        if res.gate[m] == "win":
            assert pred[m] == res.pred[m], (s.name, m, int(pred[m]), int(res.pred[m]))
            assert abs(proj[m][0] - res.u[m]) < PROJ_BOUND and abs(proj[m][1] - res.v[m]) < PROJ_BOUND, (s.name, m)
    if res.decided.all():
        assert n_in == sum(g == "win" for g in res.gate)
    return 1.0 - float(res.decided.mean())


# ---------------------------------------------------------------------------
# SearchBySim3
# ---------------------------------------------------------------------------
class Sim3Scene:
    pass


SIM3_R12 = {"a": tilted("z", 0.7), "b": tilted(np.array([3.0, -1.0, 2.0]) / np.sqrt(14.0), 1.1)}
SIM3_CASES = [(r, s12) for r in SIM3_R12 for s12 in (0.5, 1.0, 2.0)]


def sim3_scene(r12="a", s12=2.0, seed=21, bounds=BOUNDS_IMAGE, population=45):
    """Pairs (KF1 keypoint i at pixel A, KF2 keypoint j at pixel B): i's map
    point projects to B in KF2 and j's to A in KF1, so they agree; rows break
    one direction at one gate.  In both directions also: candidates at
    pred - 2 .. pred + 2 around a point of predicted level 3, a point whose
    level is clamped at nlevels - 1, and equal best distances between cells
    that differ in ix, in iy and inside one cell (the pair's own keypoint is
    the one the reference takes, so the pair still agrees).  General R12,
    t12, T1w and T2w (T2w is not the pose the other three imply; the search
    does not ask for that)."""
    rng = np.random.default_rng(seed)
    R12 = SIM3_R12[r12].astype(np.float32)
    t12 = np.array([0.23, -0.41, 0.37], np.float32)
    T1w = pose32(*POSES["y0.4"])
    T2w = pose32(*POSES["axis0.9"])
    s12 = F32(s12)
    f = np.float64
    sR12 = f(s12) * R12.astype(f)
    sR21 = (1.0 / f(s12)) * R12.astype(f).T
    t21 = -sR21 @ t12.astype(f)
    R1w, t1w, R2w, t2w = T1w[:3, :3].astype(f), T1w[:3, 3].astype(f), T2w[:3, :3].astype(f), T2w[:3, 3].astype(f)
    A12, a12 = sR21 @ R1w, sR21 @ t1w + t21           # world -> camera 2 for KF1's points
    A21, a21 = sR12 @ R2w, sR12 @ t2w + t12.astype(f)  # world -> camera 1 for KF2's points
    b12 = Builder(A12, a12, CAM, bounds, seed, cam_dist=True)     # points of KF1, keypoints of KF2
    b21 = Builder(A21, a21, CAM, bounds, seed + 1, cam_dist=True)
    spots = iter([(40 + 40 * ix, 40 + 40 * iy) for iy in range(11) for ix in range(15)])
    mnx, mxx, mny, mxy = bounds
    specs, rows = [], {}

    def pair(p1=None, p2=None, d12=3, d21=4, A=None, B=None, o1=None, o2=None, desc12=None, desc21=None):
        """o1 / o2: octave of the KF1 / KF2 keypoint (default: the level of
        the point that looks for it); desc21 / desc12: its descriptor
        (default bits(d21) / bits(d12))."""
        p1, p2 = dict(p1 or {}), dict(p2 or {})
        g = next(spots)
        A, B = A or (g[0], g[1]), B or (W - g[0], H - g[1])
        specs.append(dict(A=A, B=B, at1=p1.pop("at", B), at2=p2.pop("at", A), p1=p1, p2=p2,
                          o1=p2.get("oct", 2) if o1 is None else o1, o2=p1.get("oct", 2) if o2 is None else o2,
                          desc21=bits(d21) if desc21 is None else desc21, desc12=bits(d12) if desc12 is None else desc12))
        return len(specs) - 1

    def extra(d, at, octave, desc):
        """One more keypoint at `at` in the keyframe that direction d
        searches; its map points are not valid."""
        kw = dict(B=at, o2=octave, desc12=desc) if d == 1 else dict(A=at, o1=octave, desc21=desc)
        return pair(p1=dict(skip=1), p2=dict(skip=1), **kw)

    levels, ties, perm_above = {}, [], []

    edge = {"umin": ((mnx - 0.5, 200), (mnx + 0.5, 200)), "umax": ((mxx + 0.5, 280), (mxx - 0.5, 280)),
            "vmin": ((320, mny - 0.5), (320, mny + 0.5)), "vmax": ((400, mxy + 0.5), (400, mxy - 0.5))}
    for d in (1, 2):
        key = "p1" if d == 1 else "p2"
        where = "B" if d == 1 else "A"

        def two(gate, rej, acc):
            out = []
            for kw in (rej, acc):
                extra = {}
                if "at" in kw:
                    extra[where] = inside(bounds, *kw["at"])
                out.append(pair(**{key: kw}, **extra))
            rows[gate, d] = tuple(out)

        two("z", dict(z=-4.0), dict(z=4.0))
        for gate, (rej, acc) in edge.items():
            two(gate, dict(at=rej), dict(at=acc))
        two("dmin", dict(ratio=0.99), dict(ratio=1.01, oct=1))
        two("dmax", dict(dmax=0.99), dict(dmax=1.01))
        two("skip", dict(skip=1), dict())
        rows["thresh", d] = (pair(**{"d12" if d == 1 else "d21": 101}), pair(**{"d12" if d == 1 else "d21": 100}))
        # nothing in the box: the point aims 14 px beside its keypoint (r = 8.64)
        g = next(spots)
        off = (g[0] + 14, g[1]) if d == 2 else (W - g[0] + 14, H - g[1])
        rows["empty", d] = (pair(**{key: dict(at=off)}, A=(g[0], g[1]), B=(W - g[0], H - g[1])), pair())
        # level window pred - 1 .. pred around pred = 3, and the clamp at nlevels - 1: nearer
        # keypoints of the levels outside the window stand beside the pair's own
        okey, dkey = ("o2", "d12") if d == 1 else ("o1", "d21")
        for name, kw, own_oct, own_d, others in (
                ("lo", dict(oct=3), 2, 5, [((-1, 0), 1, 1)]),
                ("hi", dict(oct=3), 3, 7, [((1, 0), 4, 3), ((0, -1), 5, 2)]),
                ("clamp", dict(ratio=float(SF[-1]) * 1.3), NLEV - 1, 4, [((2, 1), NLEV - 3, 1)])):
            main = pair(**{key: kw, okey: own_oct, dkey: own_d})
            c = specs[main][where]
            levels[name, d] = (main, [extra(d, (c[0] + off[0], c[1] + off[1]), o, bits(nb)) for off, o, nb in others])
        # ties: the pair's own keypoint (ONE) in the earlier cell or at the lower index, its rival (TWO)
        for kind, off1, off2 in (("ix", (-6, 1), (6, 1)), ("iy", (1, -6), (1, 6)), ("cell", (1, 1), (2, 2))):
            for hi_first in ((True, False) if kind != "cell" else (False,)):
                riv = extra(d, (0, 0), 2, TWO) if hi_first else None      # made first: the lower KF1 index
                main = pair(**{"desc12" if d == 1 else "desc21": ONE})
                c = specs[main][where]                                    # the point aims at c
                specs[main][where] = (c[0] + off1[0], c[1] + off1[1])
                if riv is None:
                    riv = extra(d, (0, 0), 2, TWO)
                specs[riv][where] = (c[0] + off2[0], c[1] + off2[1])
                if d == 1:                                                # KF2 indices are perm's
                    perm_above.append((main, riv) if hi_first else (riv, main))
                ties.append((d, kind, hi_first, main, riv))
    # vpMatches12 priors: -1 (matched to a point KF2 does not see), and the KF2 keypoint of another pair
    pr_none, pr_other, pr_victim = pair(), pair(), pair()
    # no agreement: j's point is nearer to a second KF1 keypoint beside A (one bit against four)
    g = next(spots)
    lone = pair(A=(g[0], g[1]), B=(W - g[0], H - g[1]))
    rival = pair(p1=dict(skip=1), p2=dict(skip=1), d21=1, A=(g[0] + 2, g[1] + 1))
    n_rows = len(specs)
    for _ in range(population):
        o = int(rng.integers(1, NLEV))
        kw = lambda: dict(z=float(rng.uniform(1.0, 8.0)) * (-1 if rng.random() < 0.1 else 1), oct=o,
                          dmax=rng.choice([1.5, 1.5, 0.9]), skip=int(rng.random() < 0.1))
        pair(kw(), kw(), d12=int(rng.integers(1, 120)), d21=int(rng.integers(1, 120)))
    n = len(specs)
    perm = rng.permutation(n)             # pair -> KF2 index
    for a, b in perm_above:
        if perm[a] < perm[b]:
            perm[a], perm[b] = perm[b], perm[a]
    inv = np.argsort(perm)
    for p, sp in enumerate(specs):        # KF1 order
        b12.point(*sp["at1"], **sp["p1"])
        c = b21.cand(sp["A"][0], sp["A"][1], sp["o1"], sp["desc21"])
        b21.pin[c] = c
    for j in range(n):                    # KF2 order
        sp = specs[inv[j]]
        b21.point(*sp["at2"], **sp["p2"])
        c = b12.cand(sp["B"][0], sp["B"][1], sp["o2"], sp["desc12"])
        b12.pin[c] = c
    s = Sim3Scene()
    s.name = f"sim3-{r12}-{float(s12)}-{'image' if bounds == BOUNDS_IMAGE else 'undist'}"
    s.d12, s.d21 = b12.finish("12"), b21.finish("21")     # d12: mp1 searched in KF2
    s.K1, s.K2, s.mp1, s.mp2 = s.d21.K, s.d12.K, s.d12.mp, s.d21.mp
    s.valid1, s.valid2 = (s.d12.skip == 0).astype(np.uint8), (s.d21.skip == 0).astype(np.uint8)
    s.T1w, s.T2w, s.s12, s.R12, s.t12 = T1w, T2w, s12, np.ascontiguousarray(R12), t12
    s.maps = ((A12, a12), (A21, a21))
    s.perm, s.n, s.n_rows = perm, n, n_rows
    s.prior12 = np.full(n, -2, np.int32)
    s.prior12[pr_none] = -1
    s.prior12[pr_other] = perm[pr_victim]
    s.rows, s.priors, s.lone = rows, (pr_none, pr_other, pr_victim), (lone, rival)
    s.levels, s.ties = levels, ties
    return s


def sim3_maps64(s):
    """The two world-to-camera maps in float64 from the float32 inputs, as
    the reference composes them (src/ORBmatcher.cc:1284-1286)."""
    f = np.float64
    R12, t12, s12 = s.R12.astype(f), s.t12.astype(f), f(s.s12)
    sR12, sR21 = s12 * R12, (1.0 / s12) * R12.T
    t21 = -sR21 @ t12
    T1, T2 = s.T1w.astype(f), s.T2w.astype(f)
    return ((sR21 @ T1[:3, :3], sR21 @ T1[:3, 3] + t21), (sR12 @ T2[:3, :3], sR12 @ T2[:3, 3] + t12))


def reference_sim3(s):
    """(new12, decided, res1, res2): the float64 restatement of SearchBySim3."""
    N1, N2 = s.K1.n, s.K2.n
    already1 = s.prior12 != -2
    already2 = np.zeros(N2, bool)
    already2[s.prior12[(s.prior12 >= 0) & (s.prior12 < N2)]] = True
    maps = sim3_maps64(s)
    out = []
    for K, mp, valid, already, (A, a) in ((s.K2, s.mp1, s.valid1, already1, maps[0]),
                                         (s.K1, s.mp2, s.valid2, already2, maps[1])):
        n = len(valid)
        res = Result(n)
        pos, dmin, dmax = mp["pos"].astype(np.float64), mp["min_dist"].astype(np.float64), mp["max_dist"].astype(np.float64)
        for m in range(n):
            if not valid[m] or already[m]:
                res.gate[m] = "skip"
                continue
            gate, u, v, pred, r, ok = project64(K, CAM, A, a, None, pos[m], None, dmin[m], dmax[m], "sim3")
            if gate is None:
                idx, ok_area = area64(K, u, v, r, pred - 1, pred)
                ok &= ok_area
                if len(idx) == 0:
                    gate = "empty"
                else:
                    d = hamming(mp["desc"][m], K.desc[idx])
                    k = int(np.argmin(d))
                    res.idx[m], res.dist[m] = idx[k], d[k]
                    gate = "win" if d[k] <= TH_HIGH else "thresh"
            res.gate[m], res.decided[m] = gate, bool(ok)
        out.append(res)
    r1, r2 = out
    new12 = np.full(N1, -1, np.int64)
    decided = r1.decided.copy()
    for i in range(N1):
        if r1.gate[i] == "win":
            j = int(r1.idx[i])
            decided[i] &= r2.decided[j]
            if r2.gate[j] == "win" and r2.idx[j] == i:
                new12[i] = j
    return new12, decided, r1, r2


def run_sim3(s, handle=None):
    """(rc, new12, n_found) from the oracle, or with a handle the library."""
    new = np.full(max(s.K1.n, 1), -9, np.int32)
    n = ctypes.c_int(-9)
    k1, k2 = s.K1.view(), s.K2.view()
    a, b = s.mp1, s.mp2
    tail = (ptr(s.T1w), ptr(s.T2w), float(s.s12), ptr(s.R12), ptr(s.t12), TH, ptr(s.prior12), ptr(new),
            ctypes.byref(n))
    if handle is None:
        rc = _oracle().orbx_ref_search_by_sim3(ctypes.byref(k1), ctypes.byref(k2), ptr(CAM), ptr(a["pos"]),
                                               ptr(a["min_dist"]), ptr(a["max_dist"]), ptr(a["desc"]), ptr(s.valid1),
                                               ptr(b["pos"]), ptr(b["min_dist"]), ptr(b["max_dist"]), ptr(b["desc"]),
                                               ptr(s.valid2), *tail)
    else:
        m1, m2 = s.d12.mpview(), s.d21.mpview()
        rc = ox.lib().orbx_search_by_sim3(handle, ctypes.byref(k1), ctypes.byref(k2), ptr(CAM), ctypes.byref(m1),
                                          ptr(s.valid1), ctypes.byref(m2), ptr(s.valid2), *tail)
    return rc, new[:s.K1.n], n.value


# the scenes both test files walk, built once
GATE_SCENES = [(p, "image") for p in POSES] + [("y0.4", "undist"), ("back2.8", "undist")]
_built = {}


def scene(pose, bounds):
    if (pose, bounds) not in _built:
        _built[pose, bounds] = gate_scene(pose, BOUNDS_IMAGE if bounds == "image" else BOUNDS_UNDIST,
                                          seed=list(POSES).index(pose) + (100 if bounds == "undist" else 0))
    return _built[pose, bounds]


def built(name, fn):
    if name not in _built:
        _built[name] = fn()
    return _built[name]
