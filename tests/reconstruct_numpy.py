"""numpy restatement of the end of Initializer::Initialize
(src/Initializer.cc:468-745, :796-927): ReconstructF / ReconstructH, CheckRT,
Triangulate and DecomposeE, as orbx_init_reconstruct defines them.

Every float operation is a numpy float32 operation (vectorised over the
matches, which are independent of each other), every place where OpenCV 2.4
accumulates in double is a float64 sum in order.  The
two decompositions -- the 3x3 SVD of E21 / A and the 4x4 null vector of
Triangulate -- come from np.linalg.svd in float64, rounded once, or from the
caller (`svd=`, `v4=`), which makes everything after them independent of the
linear-algebra library: the fixture and the GPU tests feed recorded / device
decompositions and compare bytes.
"""
from pathlib import Path

import numpy as np

import init_numpy as inp

f32, f64 = np.float32, np.float64
RANK_CUT = 1e-6          # sigma3 <= RANK_CUT * sigma1: U's third column is the cross product of the first two
CUT = 1e-4               # relative singular gap below which two accurate solves may differ (layer 2)


# ---------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------
def fmaf(a, b, c):
    """fma(a, b, c) in float32, exactly, elementwise: the product of two
    floats is exact in float64, the sum is rounded to odd there (TwoSum gives
    the error term), and 53 >= 24 + 2 bits make the final rounding the single
    one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p = a.astype(f64) * b.astype(f64)
        c = c.astype(f64)
        s = np.array(p + c, f64)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def cam_matrix(cam):
    fx, fy, cx, cy = np.asarray(cam, f32)
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], f32)


def mul3(a, b):
    """3x3 float products: float64 accumulation over k in order, rounded once."""
    return inp.mul3(a, b).reshape(9)


def det3(m):
    """cv::determinant of a 3x3 float matrix, defined: float64 cofactor
    expansion along the first row, (m0 c0 + m1 c3) + m2 c6; a double."""
    m = np.asarray(m, f32).astype(f64).reshape(9)
    c0 = m[4] * m[8] - m[5] * m[7]
    c3 = m[5] * m[6] - m[3] * m[8]
    c6 = m[3] * m[7] - m[4] * m[6]
    return (m[0] * c0 + m[1] * c3) + m[2] * c6


def matvec(m, v):
    """3x3 times 3: float64 sums in order, rounded once."""
    m = np.asarray(m, f32).astype(f64).reshape(3, 3)
    v = np.asarray(v, f32).astype(f64)
    out = m[:, 0] * v[0]
    out = out + m[:, 1] * v[1]
    out = out + m[:, 2] * v[2]
    return out.astype(f32)


def _norm3(v):
    v = np.asarray(v, f32).astype(f64)
    s = v[..., 0] * v[..., 0]
    s = s + v[..., 1] * v[..., 1]
    s = s + v[..., 2] * v[..., 2]
    return np.sqrt(s)


def unit(t):
    """t / cv::norm(t): a scaled convert with the float scale 1 / norm."""
    with np.errstate(all="ignore"):
        return (np.asarray(t, f32) * f32(f64(1.0) / _norm3(t))).astype(f32)


def svd3(m):
    """The defined 3x3 decomposition (U, w, Vt as 21 floats) of a float
    matrix: float64 from the float entries, singular values descending,
    rounded once; where sigma3 <= RANK_CUT sigma1 U's third column is the
    cross product of the first two.  Signs (and the rotation inside a pair of
    equal singular values) are unspecified."""
    u, w, vt = np.linalg.svd(np.asarray(m, f32).astype(f64).reshape(3, 3))
    if w[2] <= RANK_CUT * w[0]:
        u[:, 2] = np.cross(u[:, 0], u[:, 1])
    return np.concatenate([u.reshape(9), w, vt.reshape(9)]).astype(f32)


def svd_input(model, M21, cam):
    """E21 = K.t()*F21*K (:477) or A = invK*H21*K (:583), left product first."""
    K = cam_matrix(cam)
    M21 = np.asarray(M21, f32).reshape(9)
    if model == 1:
        return mul3(mul3(K.reshape(3, 3).T.reshape(9), M21), K)
    return mul3(mul3(inp.inv3(K).reshape(9), M21), K)


# ---------------------------------------------------------------------------
# hypotheses
# ---------------------------------------------------------------------------
def decompose_e(svd):
    """DecomposeE (:907-927) and the order of ReconstructF (:492-495):
    (R1, t), (R2, t), (R1, -t), (R2, -t)."""
    U, Vt = svd[:9], svd[12:]
    t = unit(U[2::3])
    W = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1], f32)
    Rs = []
    for w in (W, W.reshape(3, 3).T.reshape(9)):
        R = mul3(mul3(U, w), Vt)
        if det3(R) < 0:
            R = -R
        Rs.append(R)
    return [(Rs[0], t), (Rs[1], t), (Rs[0], -t), (Rs[1], -t)]


def _scaled_mul3(s, a, b):
    """(s*a)*b of the MatExpr s*U*Rp*Vt: alpha * sum in float64, rounded once."""
    a = np.asarray(a, f32).astype(f64).reshape(3, 3)
    b = np.asarray(b, f32).astype(f64).reshape(3, 3)
    out = np.zeros((3, 3), f64)
    for i in range(3):
        for j in range(3):
            acc = a[i, 0] * b[0, j]
            acc = acc + a[i, 1] * b[1, j]
            acc = acc + a[i, 2] * b[2, j]
            out[i, j] = f64(s) * acc
    return out.astype(f32).reshape(9)


def faugeras(svd, contract=0):
    """The eight hypotheses of ReconstructH (:589-684), or [] on the early
    return of :595-598."""
    with np.errstate(all="ignore"):
        U, w, Vt = svd[:9], svd[9:12], svd[12:]
        s = f32(det3(U) * det3(Vt))
        d1, d2, d3 = w
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return []
        if contract:
            d12, d23, d13 = fmaf(d1, d1, -(d2 * d2)), fmaf(d2, d2, -(d3 * d3)), fmaf(d1, d1, -(d3 * d3))
            c_num, p_num = fmaf(d2, d2, d1 * d3), fmaf(d1, d3, -(d2 * d2))
        else:
            d12, d23, d13 = d1 * d1 - d2 * d2, d2 * d2 - d3 * d3, d1 * d1 - d3 * d3
            c_num, p_num = d2 * d2 + d1 * d3, d1 * d3 - d2 * d2
        aux1, aux3 = np.sqrt(f32(d12 / d13)), np.sqrt(f32(d23 / d13))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        root = np.sqrt(f32(d12 * d23))
        aux_st = f32(root / f32(f32(d1 + d3) * d2))
        ct = f32(c_num / f32(f32(d1 + d3) * d2))
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = f32(root / f32(f32(d1 - d3) * d2))
        cp = f32(p_num / f32(f32(d1 - d3) * d2))
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for i in range(4):
            Rp = np.array([ct, 0, -st[i], 0, 1, 0, st[i], 0, ct], f32)
            R = mul3(_scaled_mul3(s, U, Rp), Vt)
            sc = f32(d1 - d3)
            tp = np.array([x1[i] * sc, f32(0), f32(-x3[i]) * sc], f32)
            out.append((R, unit(matvec(U, tp))))
        for i in range(4):
            Rp = np.array([cp, 0, sp[i], 0, -1, 0, sp[i], 0, -cp], f32)
            R = mul3(_scaled_mul3(s, U, Rp), Vt)
            sc = f32(d1 + d3)
            tp = np.array([x1[i] * sc, f32(0), x3[i] * sc], f32)
            out.append((R, unit(matvec(U, tp))))
        return out


# ---------------------------------------------------------------------------
# CheckRT
# ---------------------------------------------------------------------------
def projection(cam, R, t):
    """P2 = K*[R|t] (:819-822) and O2 = -R.t()*t (:824)."""
    K = cam_matrix(cam).astype(f64).reshape(3, 3)
    Rt = np.concatenate([np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3, 1)], 1).astype(f64)
    P2 = np.zeros((3, 4), f64)
    for i in range(3):
        acc = K[i, 0] * Rt[0]
        acc = acc + K[i, 1] * Rt[1]
        acc = acc + K[i, 2] * Rt[2]
        P2[i] = acc
    R64, t64 = Rt[:, :3], Rt[:, 3]
    acc = R64[0] * t64[0]
    acc = acc + R64[1] * t64[1]
    acc = acc + R64[2] * t64[2]
    return P2.astype(f32), (-acc).astype(f32)


def build_A(cam, P2, xy):
    """Triangulate's A (:736-739) of every match: (N, 4, 4); a rounded
    multiply, then a rounded subtract."""
    fx, fy, cx, cy = np.asarray(cam, f32)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    u1, v1, u2, v2 = (xy[:, k:k + 1] for k in range(4))
    with np.errstate(all="ignore"):
        return np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]], 1).astype(f32)


def null_vectors(A):
    """(v4 (N, 4) float32, gap (N,)): the right singular vector of the
    smallest singular value in float64, rounded once, and (s3 - s4) / s1."""
    v4, gap = np.zeros((len(A), 4), f32), np.zeros(len(A))
    for k, a in enumerate(A.astype(f64)):
        if not np.isfinite(a).all():
            v4[k] = (1, 0, 0, 0)
            continue
        _, s, vt = np.linalg.svd(a)
        v4[k] = vt[3].astype(f32)
        gap[k] = (s[2] - s[3]) / s[0] if s[0] > 0 else 0.0
    return v4, gap


def check_rt(R, t, xy, inliers, cam, th2, v4=None, contract=0):
    """CheckRT (:796-905) over the compacted matches xy (N, 4) by match
    index: a dict of n_good, parallax, cos (N, NaN where the match did not
    reach :886), points (N, 3) and good (N) by match index (zero elsewhere),
    v4 (N, 4, zero at non-inliers) and gap."""
    N = len(xy)
    inl = np.asarray(inliers[:N]).astype(bool)
    fx, fy, cx, cy = np.asarray(cam, f32)
    P2, O2 = projection(cam, R, t)
    out = dict(cos=np.full(N, np.nan, f32), points=np.zeros((N, 3), f32), good=np.zeros(N, np.uint8),
               v4=np.zeros((N, 4), f32), gap=np.full(N, np.nan), n_good=0, parallax=f32(0))
    idx = np.flatnonzero(inl)
    if not len(idx):
        return out
    p = xy[idx]
    with np.errstate(all="ignore"):
        if v4 is None:
            v, gap = null_vectors(build_A(cam, P2, p))
            out["gap"][idx] = gap
        else:
            v = np.asarray(v4, f32)[idx]
        out["v4"][idx] = v
        inv = (f64(1.0) / v[:, 3].astype(f64)).astype(f32)
        x = (v[:, :3] * inv[:, None]).astype(f32)
        alive = np.isfinite(x).all(1)
        dist1 = _norm3(x).astype(f32)
        n2 = (x - O2).astype(f32)
        dist2 = _norm3(n2).astype(f32)
        x64, n64 = x.astype(f64), n2.astype(f64)
        dot = x64[:, 0] * n64[:, 0]
        dot = dot + x64[:, 1] * n64[:, 1]
        dot = dot + x64[:, 2] * n64[:, 2]
        cosv = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        low = cosv.astype(f64) < 0.99998
        alive &= ~((x[:, 2] <= 0) & low)
        R64, t64 = np.asarray(R, f32).astype(f64).reshape(3, 3), np.asarray(t, f32).astype(f64)
        x2 = np.zeros_like(x)
        for r in range(3):
            acc = R64[r, 0] * x64[:, 0]
            acc = acc + R64[r, 1] * x64[:, 1]
            acc = acc + R64[r, 2] * x64[:, 2]
            x2[:, r] = (acc + t64[r]).astype(f32)
        alive &= ~((x2[:, 2] <= 0) & low)
        for pt, uv in ((x, p[:, 0:2]), (x2, p[:, 2:4])):
            invz = (f64(1.0) / pt[:, 2].astype(f64)).astype(f32)
            if contract:
                imx, imy = fmaf(fx * pt[:, 0], invz, cx), fmaf(fy * pt[:, 1], invz, cy)
            else:
                imx, imy = fx * pt[:, 0] * invz + cx, fy * pt[:, 1] * invz + cy
            ex, ey = imx - uv[:, 0], imy - uv[:, 1]
            e2 = fmaf(ex, ex, ey * ey) if contract else ex * ex + ey * ey
            alive &= ~(e2 > f32(th2))
    out["cos"][idx[alive]] = cosv[alive]
    out["points"][idx[alive]] = x[alive]
    out["good"][idx[alive & low]] = 1
    out["n_good"] = int(alive.sum())
    if out["n_good"] > 0:
        c = np.sort(cosv[alive])[min(50, out["n_good"] - 1)]
        out["parallax"] = parallax_of(c)
    return out


def parallax_of(c):
    """acos(vCosParallax[idx])*180/CV_PI (:899): std::acos(float) (section 4),
    the float product by 180, the double division by CV_PI, rounded."""
    with np.errstate(all="ignore"):
        a = f32(np.arccos(f64(c)))
        return f32(f64(a * f32(180)) / f64(3.1415926535897932384626433832795))


# ---------------------------------------------------------------------------
# ReconstructF / ReconstructH
# ---------------------------------------------------------------------------
def compact_xy(keys1, keys2, matches12):
    pairs = inp.compact(matches12)
    xy = np.stack([keys1["x"][pairs[:, 0]], keys1["y"][pairs[:, 0]],
                   keys2["x"][pairs[:, 1]], keys2["y"][pairs[:, 1]]], 1).astype(f32).reshape(-1, 4)
    return pairs, xy


def select_f(n_good, parallax, N, min_parallax, min_tri):
    """:497-567: (ok, best)."""
    mx = max(n_good)
    n_min = max(int(0.9 * N), min_tri)
    similar = sum(1 for g in n_good if g > 0.7 * mx)
    if mx < n_min or similar > 1:
        return 0, -1
    k = n_good.index(mx)
    if parallax[k] > f32(min_parallax):
        return 1, k
    return 0, -1


def select_h(n_good, parallax, N, min_parallax, min_tri):
    """:687-729."""
    best = second = 0
    idx, par = -1, f32(-1)
    for i, g in enumerate(n_good):
        if g > best:
            second, best, idx, par = best, g, i, parallax[i]
        elif g > second:
            second = g
    if second < 0.75 * best and par >= f32(min_parallax) and best > min_tri and best > 0.9 * N:
        return 1, idx
    return 0, -1


def reconstruct(keys1, keys2, matches12, inliers, model, M21, cam, sigma=1.0, min_parallax=1.0, min_triangulated=50,
                svd=None, v4=None, contract=0):
    """orbx_init_reconstruct: a dict with the query's outputs and taps.
    svd: the 21 floats to use (None: svd3); v4: (n_hyp, N, 4) null vectors to
    use (None: null_vectors, and `gap` holds each solve's conditioning)."""
    n1 = len(keys1)
    pairs, xy = compact_xy(keys1, keys2, matches12)
    N = len(pairs)
    inl = np.asarray(inliers, np.uint8)[:N]
    cam = np.asarray(cam, f32)
    out = dict(ok=0, n_inliers=int(np.count_nonzero(inl)), n_hyp=0, best=-1, R21=None, t21=None,
               n_good=np.zeros(8, np.int32), parallax=np.zeros(8, f32), p3d=np.zeros((n1, 3), f32),
               triangulated=np.zeros(n1, np.uint8), svd=np.zeros(21, f32), R_all=np.zeros((8, 9), f32),
               t_all=np.zeros((8, 3), f32), N=N, pairs=pairs)
    if N == 0:
        out.update(v4=np.zeros((0, 0, 4), f32), cos_parallax=np.zeros((0, 0), f32), gap=np.zeros((0, 0)))
        return out
    S = svd3(svd_input(model, M21, cam)) if svd is None else np.asarray(svd, f32).reshape(21)
    out["svd"] = S
    hyps = decompose_e(S) if model == 1 else faugeras(S, contract)
    nh = len(hyps)
    out["n_hyp"] = nh
    sig2 = f32(sigma) * f32(sigma)
    th2 = f32(4.0 * f64(sig2))
    res = []
    for h, (R, t) in enumerate(hyps):
        out["R_all"][h], out["t_all"][h] = R, t
        r = check_rt(R, t, xy, inl, cam, th2, None if v4 is None else v4[h], contract)
        out["n_good"][h], out["parallax"][h] = r["n_good"], r["parallax"]
        res.append(r)
    out["v4"] = np.stack([r["v4"] for r in res]) if nh else np.zeros((0, N, 4), f32)
    out["cos_parallax"] = np.stack([r["cos"] for r in res]) if nh else np.zeros((0, N), f32)
    out["gap"] = np.stack([r["gap"] for r in res]) if nh else np.zeros((0, N))
    if nh == 0:
        return out
    sel = select_f if model == 1 else select_h
    ok, best = sel([int(g) for g in out["n_good"][:nh]], list(out["parallax"][:nh]), out["n_inliers"], min_parallax,
                   min_triangulated)
    out["ok"], out["best"] = ok, best
    if ok:
        out["R21"], out["t21"] = out["R_all"][best].copy(), out["t_all"][best].copy()
        keep = ~np.isnan(res[best]["cos"])
        out["p3d"][pairs[keep, 0]] = res[best]["points"][keep]
        out["triangulated"][pairs[:, 0]] = res[best]["good"]
    return out


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
CAM = np.array([500.0, 500.0, 320.0, 240.0], f32)
MOTION = dict(angle=0.08, t=(-0.6, 0.05, 0.1))
PLANE_AMBIGUOUS = dict(normal=(0.2, -0.1, 1.0), d=6.0)     # init_numpy.scene's plane: fails the second-best rule
PLANE_CLEAR = dict(normal=(0.8, -0.3, 1.0), d=6.0)         # a slanted plane with a clear winner


def rotation(angle):
    return np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])


def scene(seed, N, plane=None, angle=MOTION["angle"], t=MOTION["t"], noise=0.5, outliers=0.0, extra1=7, extra2=12,
          depth=(3.0, 12.0), w=640, h=480):
    """Two views (camera CAM) of N points -- a cloud at `depth`, or the plane
    normal . X = d -- under the motion X2 = R_y(angle) X1 + t: (keys1, keys2,
    matches12, truth) with the matched keypoints at shuffled positions among
    extra1 / extra2 unmatched ones and pixel noise on frame 2.  truth: R, t
    and the points X (camera 1) by keys1 index."""
    rng = np.random.RandomState(seed)
    f, cx, cy = 500.0, w / 2.0, h / 2.0
    x1 = np.stack([rng.uniform(20, w - 20, N), rng.uniform(20, h - 20, N)], 1)
    ray = np.stack([(x1[:, 0] - cx) / f, (x1[:, 1] - cy) / f, np.ones(N)], 1)
    if plane is not None:
        z = plane["d"] / (ray @ np.asarray(plane["normal"], f64))
    else:
        z = rng.uniform(depth[0], depth[1], N)
    X = ray * z[:, None]
    R, t = rotation(angle), np.asarray(t, f64)
    Xc = X @ R.T + t
    x2 = np.stack([f * Xc[:, 0] / Xc[:, 2] + cx, f * Xc[:, 1] / Xc[:, 2] + cy], 1)
    if noise > 0:
        x2 = x2 + rng.normal(0, noise, x2.shape)
    n_out = int(round(outliers * N))
    if n_out:
        bad = rng.choice(N, n_out, replace=False)
        x2[bad] = np.stack([rng.uniform(0, w, n_out), rng.uniform(0, h, n_out)], 1)
    n1, n2 = N + extra1, N + extra2
    pos1, pos2 = rng.permutation(n1)[:N], rng.permutation(n2)[:N]
    k1 = np.stack([rng.uniform(0, w, n1), rng.uniform(0, h, n1)], 1)
    k2 = np.stack([rng.uniform(0, w, n2), rng.uniform(0, h, n2)], 1)
    k1[pos1], k2[pos2] = x1, x2
    m = np.full(n1, -1, np.int32)
    m[pos1] = pos2
    Xfull = np.zeros((n1, 3))
    Xfull[pos1] = X
    return inp.make_keys(k1.astype(f32)), inp.make_keys(k2.astype(f32)), m, dict(R=R, t=t, X=Xfull)


def true_model(model, truth, plane=None):
    """F21 or H21 of the scene's motion in float64, rounded once (an input)."""
    K = cam_matrix(CAM).astype(f64).reshape(3, 3)
    Ki = np.linalg.inv(K)
    R, t = truth["R"], truth["t"]
    if model == 1:
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        M = Ki.T @ tx @ R @ Ki
    else:
        n = np.asarray(plane["normal"], f64)
        M = K @ (R + np.outer(t, n) / plane["d"]) @ Ki
    return (M / np.abs(M).max()).astype(f32).reshape(9)


# Every case of the tests, by name: (model, scene arguments, expected ok).  The models are the motion's true ones
# and every match is an inlier unless `inliers` keeps the first k.  The seeds are pinned with the restatement.
CASES = {
    "F-300": dict(model=1, seed=111, N=300, ok=1),
    "F-257": dict(model=1, seed=112, N=257, ok=1),
    "F-256": dict(model=1, seed=113, N=256, ok=1),
    "F-65": dict(model=1, seed=112, N=65, ok=1),
    "F-64": dict(model=1, seed=114, N=64, ok=1),
    "F-rotation": dict(model=1, seed=115, N=300, t=(0.0, 0.0, 0.0), ok=0, M21_t=(-0.6, 0.05, 0.1)),
    "F-parallax": dict(model=1, seed=119, N=300, t=(-0.06, 0.005, 0.01), ok=0),
    "F-few": dict(model=1, seed=116, N=40, ok=0),
    "F-noisy": dict(model=1, seed=117, N=65, noise=2.5, ok=0),
    "H-300": dict(model=0, seed=111, N=300, plane=PLANE_CLEAR, ok=1),
    "H-257": dict(model=0, seed=112, N=257, plane=PLANE_CLEAR, ok=1),
    "H-256": dict(model=0, seed=113, N=256, plane=PLANE_CLEAR, ok=1),
    "H-65": dict(model=0, seed=111, N=65, plane=PLANE_CLEAR, ok=1),
    "H-64": dict(model=0, seed=114, N=64, plane=PLANE_CLEAR, ok=1),
    "H-ambiguous": dict(model=0, seed=111, N=300, plane=PLANE_AMBIGUOUS, ok=0),
    "H-ambiguous-65": dict(model=0, seed=112, N=65, plane=PLANE_AMBIGUOUS, ok=0),
    "H-parallax": dict(model=0, seed=111, N=300, plane=PLANE_CLEAR, min_parallax=8.0, ok=0),
    "H-few": dict(model=0, seed=116, N=40, plane=PLANE_CLEAR, ok=0),
    "H-rotation": dict(model=0, seed=115, N=300, plane=PLANE_CLEAR, t=(0.0, 0.0, 0.0), ok=0),
}
_cache = {}


def case_inputs(name):
    """(keys1, keys2, matches12, inliers, model, M21, cam, truth, keyword
    arguments) of a case."""
    c = dict(CASES[name])
    model, want = c.pop("model"), c.pop("ok")
    m21_t = c.pop("M21_t", None)
    kw = {k: c.pop(k) for k in ("min_parallax", "min_triangulated") if k in c}
    k1, k2, m, truth = scene(c.pop("seed"), c.pop("N"), **c)
    tm = dict(truth, t=np.asarray(m21_t, f64)) if m21_t is not None else truth
    M21 = true_model(model, tm, c.get("plane"))
    return k1, k2, m, np.ones(int((m >= 0).sum()), np.uint8), model, M21, CAM, truth, kw


def case(name, contract=0):
    """(inputs, restatement result), computed once."""
    key = (name, contract)
    if key not in _cache:
        a = case_inputs(name)
        _cache[key] = (a, reconstruct(*a[:7], contract=contract, **a[8]))
    return _cache[key]


def inliers_for_n_good(name, want):
    """Inlier flags of a case cut to the first matches that make the winning
    hypothesis count `want` good points (the min(50, size - 1) clamp)."""
    a, r = case(name)
    best = int(np.argmax(r["n_good"]))
    reached = np.cumsum(~np.isnan(r["cos_parallax"][best]))
    keep = int(np.searchsorted(reached, want)) + 1
    inl = np.zeros(r["N"], np.uint8)
    inl[:keep] = 1
    return inl


# ---------------------------------------------------------------------------
# the match on which the fp-contract modes differ
# ---------------------------------------------------------------------------
# scene(118, 65) with the true F: frame 2's keypoint of match CONTRACT_EDIT[0] moved along y, by bisection between
# an accepted point and a reprojection reject, to where mode 0 and mode 1 decide differently (find_contract_edit
# gives the pair; it is pinned here and the fixture carries the edited keypoints).
CONTRACT_SEED, CONTRACT_N = 118, 65
CONTRACT_EDIT = (1, 378.50103759765625)


def contract_base():
    k1, k2, m, truth = scene(CONTRACT_SEED, CONTRACT_N)
    M21 = true_model(1, truth)
    S = svd3(svd_input(1, M21, CAM))
    r = reconstruct(k1, k2, m, np.ones(CONTRACT_N, np.uint8), 1, M21, CAM, svd=S)
    return k1, k2, m, M21, S, r


def find_contract_edit(R=None, t=None, tries=40):
    """(match index, y): for one match after the other, bisect frame 2's y
    under mode 0 to the adjacent floats (accepted, rejected) of the
    reprojection gate under the motion (R, t) -- the restatement's winning
    hypothesis of the base scene, or the caller's, such as a device's own --
    and look whether mode 1 decides otherwise on either."""
    k1, k2, m, M21, S, r = contract_base()
    if R is None:
        R, t = r["R_all"][r["best"]], r["t_all"][r["best"]]
    pairs, xy = r["pairs"], compact_xy(k1, k2, m)[1]
    th2 = f32(4.0)

    def accepted(i, y, c):
        p = xy[i:i + 1].copy()
        p[0, 3] = y
        return check_rt(R, t, p, np.ones(1, np.uint8), CAM, th2, contract=c)["n_good"] == 1

    for i in range(min(tries, len(xy))):
        lo, hi = f32(xy[i, 3]), f32(xy[i, 3] + 8)
        if not accepted(i, lo, 0) or accepted(i, hi, 0):
            continue
        while np.nextafter(lo, hi) < hi:
            mid = f32((f64(lo) + f64(hi)) / 2)
            if accepted(i, mid, 0):
                lo = mid
            else:
                hi = mid
        for y in (lo, hi):
            if accepted(i, y, 0) != accepted(i, y, 1):
                return i, float(y)
    return None


def contract_case(edit=None):
    """(keys1, keys2, matches12, inliers, model, M21, cam) of the constructed
    match: the edited keypoint, its inlier flag alone set.  edit: (match
    index, y), by default the pinned CONTRACT_EDIT."""
    k1, k2, m, M21, S, r = contract_base()
    i, y = CONTRACT_EDIT if edit is None else edit
    k2 = k2.copy()
    k2["y"][r["pairs"][i, 1]] = f32(y)
    one = np.zeros(CONTRACT_N, np.uint8)
    one[i] = 1
    return k1, k2, m, one, 1, M21, CAM


# ---------------------------------------------------------------------------
# the committed fixture
# ---------------------------------------------------------------------------
GOLDEN_CASES = (("cloud", 1, 21, 120, None), ("plane", 0, 22, 120, PLANE_CLEAR))
_OUT = ("ok", "n_inliers", "n_hyp", "best", "n_good", "parallax", "p3d", "triangulated", "svd", "R_all", "t_all", "v4",
        "cos_parallax")


def golden_arrays():
    out = {}
    for tag, model, seed, N, plane in GOLDEN_CASES:
        k1, k2, m, truth = scene(seed, N, plane=plane)
        M21 = true_model(model, truth, plane)
        inl = np.ones(N, np.uint8)
        inl[::9] = 0
        out.update({f"{tag}_keys1": k1, f"{tag}_keys2": k2, f"{tag}_matches12": m, f"{tag}_inliers": inl,
                    f"{tag}_M21": M21, f"{tag}_model": np.int32(model)})
        for c in (0, 1):
            r = reconstruct(k1, k2, m, inl, model, M21, CAM, contract=c)
            for name in _OUT:
                out[f"{tag}_{name}{c}"] = np.asarray(r[name])
            out[f"{tag}_R21{c}"] = r["R21"] if r["ok"] else np.zeros(9, f32)
            out[f"{tag}_t21{c}"] = r["t21"] if r["ok"] else np.zeros(3, f32)
    if CONTRACT_EDIT is not None:
        a = contract_case()
        S = svd3(svd_input(1, a[5], CAM))
        out.update(f_keys1=a[0], f_keys2=a[1], f_matches12=a[2], f_inliers=a[3], f_M21=a[5], f_svd=S)
        for c in (0, 1):
            r = reconstruct(*a, svd=S, contract=c)
            out[f"f_n_good{c}"], out[f"f_cos_parallax{c}"], out[f"f_v4{c}"] = r["n_good"], r["cos_parallax"], r["v4"]
    out["cam"] = CAM
    return out


def write_golden(path):
    np.savez_compressed(path, **golden_arrays())


if __name__ == "__main__":
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    write_golden(Path(__file__).resolve().parent / "golden" / "init_reconstruct.npz")
