"""Second restatement of Sim3Solver (src/Sim3Solver.cc) in numpy: the
comparator of the device's orbx_sim3_ransac.

The bit-exact parts are float32 arithmetic operation by operation (numpy
ufuncs round every operation once), vectorised across the RANSAC iterations
and the correspondences only.  The places that go through OpenCV follow the
definitions of DESIGN.md section 4: float64 accumulation over k in order,
rounded once; scaled converts with a float scale; cv::Rodrigues in float64.
The quaternion is the unit eigenvector of N for its largest eigenvalue from
np.linalg.eigh in float64, rounded once, with q0 >= 0.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
RAND_MAX = 2**31 - 1


# --- the constructor (:37-112) -----------------------------------------------
def random_int(r, size):
    """DUtils::Random::RandomInt(0, size - 1) of the rand() value r
    (Thirdparty/DBoW2/DUtils/Random.cpp:47-50)."""
    return int((float(r) / (float(RAND_MAX) + 1.0)) * float(size))


def max_error(sigma2):
    """mvnMaxError (:87-88): 9.210 * sigma2 in double, truncated into a
    std::vector<size_t> (include/Sim3Solver.h:79-80)."""
    return int(9.210 * float(F32(sigma2)))


def dot3(rows, x):
    """rows (..., 3) . x (..., 3): float64 accumulation over k = 0..2 in
    order (a float64 array; the caller rounds)."""
    rows, x = np.asarray(rows, F32).astype(F64), np.asarray(x, F32).astype(F64)
    acc = rows[..., 0] * x[..., 0]
    acc = acc + rows[..., 1] * x[..., 1]
    acc = acc + rows[..., 2] * x[..., 2]
    return acc


def transform(T, X):
    """Rcw*X+tcw (:95, :98, :391) of points X (n, 3) under the 4x4 T (or a
    stack (M, 16) against one point): the float gemm with its addend."""
    T = np.asarray(T, F32).reshape(-1, 4, 4)
    X = np.asarray(X, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        out = [(dot3(T[:, r, :3], X) + T[:, r, 3].astype(F64)).astype(F32) for r in range(3)]
    return np.stack(out, -1)


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def cam_to_image(cam, Xc, contract=False):
    """FromCameraToImage / Project's tail (:392-396, :412-416): float invz =
    1/z, x*invz, fx*x+cx (fused under contract)."""
    fx, fy, cx, cy = (F32(c) for c in np.asarray(cam, F32).reshape(4))
    Xc = np.asarray(Xc, F32)
    with np.errstate(all="ignore"):
        invz = F32(1) / Xc[..., 2]
        x, y = Xc[..., 0] * invz, Xc[..., 1] * invz
        if contract:
            ones = np.ones_like(x)
            return np.stack([_fma(fx * ones, x, cx * ones), _fma(fy * ones, y, cy * ones)], -1)
        return np.stack([fx * x + cx, fy * y + cy], -1).astype(F32)


def construct(kf1, kf2, matches12, idx1=None, contract=False):
    """The correspondences in i1 order and what the constructor computes for
    each: N, indices1, x3dc1 / 2, p1im1 / p2im2, max_err1 / 2."""
    m = np.asarray(matches12, np.int32)
    n1, n2 = len(kf1["keys"]), len(kf2["keys"])
    k1 = np.arange(n1, dtype=np.int32) if idx1 is None else np.asarray(idx1, np.int32)
    keep = [(i1, int(k1[i1]), int(m[i1])) for i1 in range(n1)
            if m[i1] >= 0 and m[i1] < n2 and 0 <= k1[i1] < n1 and kf1["valid"][k1[i1]] and kf2["valid"][m[i1]]]
    i1 = np.array([k[0] for k in keep], np.int32)
    a = np.array([k[1] for k in keep], np.int64)
    b = np.array([k[2] for k in keep], np.int64)
    x1 = transform(kf1["Tcw"], np.asarray(kf1["pos"], F32).reshape(-1, 3)[a]).reshape(-1, 3)
    x2 = transform(kf2["Tcw"], np.asarray(kf2["pos"], F32).reshape(-1, 3)[b]).reshape(-1, 3)
    l1 = np.array([max_error(kf1["sigma2"][o]) for o in kf1["keys"]["octave"][a]], np.int32)
    l2 = np.array([max_error(kf2["sigma2"][o]) for o in kf2["keys"]["octave"][b]], np.int32)
    return dict(N=len(keep), indices1=i1, x3dc1=x1, x3dc2=x2,
                p1im1=cam_to_image(kf1["cam"], x1, contract).reshape(-1, 2),
                p2im2=cam_to_image(kf2["cam"], x2, contract).reshape(-1, 2), max_err1=l1, max_err2=l2)


def ransac_max_its(N, min_inliers=20, probability=0.99, max_iterations=300):
    """SetRansacParameters (:114-138): the float epsilon, double log / pow /
    ceil.  N < min_inliers (the reference converts a NaN) is reported as 0."""
    if N < min_inliers:
        return 0
    if min_inliers == N:
        n = 1
    else:
        eps = F32(min_inliers) / F32(N)
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(1 - F64(probability)) / np.log(1 - np.power(F64(eps), 3)))
        n = 2**31 - 1 if not v < 2147483647.0 else (1 if v < 1 else int(v))
    return max(1, min(n, max_iterations))


# --- the minimal sets (:163-177) ---------------------------------------------
def make_sets(N, draws):
    """Three picks per iteration.  vAvailableIndices[idx] = back(); pop_back()
    writes at the drawn *value* idx, not at the drawn position: the picked
    position keeps its value (a correspondence can repeat), and the write can
    land at or past the new size, where nothing reads it again."""
    draws = np.asarray(draws).reshape(-1, 3)
    sets = np.zeros((len(draws), 3), np.int32)
    if N < 3:
        return sets
    for it in range(len(draws)):
        buf, size = list(range(N)), N      # the vector's storage and its size
        for j in range(3):
            randi = random_int(draws[it, j], size)
            idx = buf[randi]
            sets[it, j] = idx
            buf[idx] = buf[size - 1]
            size -= 1
    return sets


# --- computeT (:226-332) -------------------------------------------------------
THIRD = F32(1.0 / 3.0)


def relative(P):
    """centroid (:215-224) of (M, 3, 3) sets (row, point): cv::reduce sums a
    row in float, C/P.cols scales by float(1.0/3): (O (M, 3), Pr (M, 3, 3))."""
    P = np.asarray(P, F32)
    with np.errstate(all="ignore"):
        s = P[..., 0] + P[..., 1]
        s = s + P[..., 2]
        O = s * THIRD
        return O, P - O[..., None]


def n_matrix(Pr1, Pr2):
    """M = Pr2*Pr1.t() (:243) and N (:251-265): sums and differences of float
    entries are float arithmetic.  (M, 4, 4) float32."""
    M = np.zeros(Pr1.shape[:-2] + (3, 3), F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                M[..., i, j] = dot3(Pr2[..., i, :], Pr1[..., j, :]).astype(F32)
        m = lambda i, j: M[..., i, j]
        N11 = m(0, 0) + m(1, 1) + m(2, 2)
        N12 = m(1, 2) - m(2, 1)
        N13 = m(2, 0) - m(0, 2)
        N14 = m(0, 1) - m(1, 0)
        N22 = m(0, 0) - m(1, 1) - m(2, 2)
        N23 = m(0, 1) + m(1, 0)
        N24 = m(2, 0) + m(0, 2)
        N33 = -m(0, 0) + m(1, 1) - m(2, 2)
        N34 = m(1, 2) + m(2, 1)
        N44 = -m(0, 0) - m(1, 1) + m(2, 2)
    rows = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return np.stack([np.stack(r, -1) for r in rows], -2).astype(F32)


def fix_sign(q):
    """q0 >= 0 (a zero q0: the first non-zero of the rest positive)."""
    q = np.array(q, F64).reshape(-1, 4)
    for v in q:
        nz = [x for x in v if x != 0.0]
        if nz and nz[0] < 0:
            v *= -1.0
    return q


def quaternion(N):
    """(q (M, 4) float32, gap (M,)): the unit eigenvector of N for its largest
    eigenvalue and gap = (l1 - l2) / max |l|.  NaN systems give NaNs."""
    N = np.asarray(N, F32).astype(F64).reshape(-1, 4, 4)
    q = np.full((len(N), 4), np.nan, F64)
    gap = np.zeros(len(N))
    for k, a in enumerate(N):
        if not np.isfinite(a).all():
            continue
        w, v = np.linalg.eigh(a)
        q[k] = v[:, 3]
        big = np.abs(w).max()
        gap[k] = (w[3] - w[2]) / big if big > 0 else 0.0
    return fix_sign(q).astype(F32), gap


def rotation(q):
    """ang (:278), vec = 2*ang*vec/norm(vec) (:280) as a scaled convert with
    the float scale float((2*ang)*(1/norm)), and cv::Rodrigues (:284) in
    float64 from the float vector: (M, 9) float32."""
    q = np.asarray(q, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        d = q.astype(F64)
        nrm = d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        nrm = np.sqrt(nrm + d[:, 3] * d[:, 3])
        ang = np.arctan2(nrm, d[:, 0])
        av = ((2.0 * ang) * (1.0 / nrm)).astype(F32)
        vec = q[:, 1:] * av[:, None]
        r = vec.astype(F64)
        rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
        theta = np.sqrt((rx * rx + ry * ry) + rz * rz)
        c, s = np.cos(theta), np.sin(theta)
        c1, itheta = 1.0 - c, 1.0 / theta
        rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
        z = np.zeros_like(rx)
        eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
        rcr = [z, -rz, ry, rz, z, -rx, -ry, rx, z]
        R = np.stack([(c * eye[k] + c1 * rrt[k]) + s * rcr[k] for k in range(9)], -1)
        small = theta < np.finfo(F64).eps
        R[small] = eye
    return R.astype(F32)


def finish(O1, Pr1, O2, Pr2, R):
    """From mR12i on (:288-331): P3, the scale, the translation, T12, T21:
    (scale (M,), T12 (M, 16), T21 (M, 16)) float32."""
    R = np.asarray(R, F32).reshape(-1, 3, 3)
    M = len(R)
    with np.errstate(all="ignore"):
        nom, den = np.zeros(M), np.zeros(M)
        for i in range(3):
            for j in range(3):
                p3 = dot3(R[:, i, :], Pr2[:, :, j]).astype(F32)
                nom = nom + Pr1[:, i, j].astype(F64) * p3.astype(F64)
                den = den + (p3 * p3).astype(F64)
        s = (nom / den).astype(F32)
        T12, T21 = np.zeros((M, 4, 4), F32), np.zeros((M, 4, 4), F32)
        T12[:, 3, 3] = T21[:, 3, 3] = 1
        t = np.stack([(-s.astype(F64) * dot3(R[:, i, :], O2) + O1[:, i].astype(F64)).astype(F32) for i in range(3)], -1)
        sinv = (1.0 / s.astype(F64)).astype(F32)
        T12[:, :3, :3] = R * s[:, None, None]
        T12[:, :3, 3] = t
        sRinv = np.transpose(R, (0, 2, 1)) * sinv[:, None, None]
        T21[:, :3, :3] = sRinv
        T21[:, :3, 3] = np.stack([(-dot3(sRinv[:, i, :], t)).astype(F32) for i in range(3)], -1)
    return s, T12.reshape(M, 16), T21.reshape(M, 16)


def gather(c, sets):
    """P3Dc1i, P3Dc2i (:172-173) of every set: (M, 3, 3) each, (row, point)."""
    sets = np.asarray(sets).reshape(-1, 3)
    return (np.transpose(c["x3dc1"][sets], (0, 2, 1)).astype(F32), np.transpose(c["x3dc2"][sets], (0, 2, 1)).astype(F32))


def compute_t(c, sets, q=None, R=None):
    """computeT of every set; q / R given: the solve / the rotation taken from
    the caller (the device's taps)."""
    P1, P2 = gather(c, sets)
    O1, Pr1 = relative(P1)
    O2, Pr2 = relative(P2)
    out = {}
    if q is None and R is None:
        out["Nmat"] = n_matrix(Pr1, Pr2)
        q, out["gap"] = quaternion(out["Nmat"])
    if R is None:
        R = rotation(q)
    s, T12, T21 = finish(O1, Pr1, O2, Pr2, R)
    out.update(q=q, R=np.asarray(R, F32).reshape(-1, 9), scale=s, T12_all=T12, T21_all=T21)
    return out


# --- CheckInliers (:335-359) ---------------------------------------------------
def check_inliers(c, kf1, kf2, T12_all, T21_all, contract=False):
    """(count (M,), mask (M, N)) of M transformations over the N
    correspondences.  err < limit compares the float with the size_t limit
    converted to float; NaNs fail it."""
    T12 = np.asarray(T12_all, F32).reshape(-1, 1, 4, 4)
    T21 = np.asarray(T21_all, F32).reshape(-1, 1, 4, 4)
    M, N = len(T12), c["N"]
    if N == 0:
        return np.zeros(M, np.int32), np.zeros((M, 0), bool)
    with np.errstate(all="ignore"):
        def tr(T, X):
            X = X[None, :, :]
            return np.stack([(dot3(T[:, :, r, :3], X) + T[:, :, r, 3].astype(F64)).astype(F32) for r in range(3)], -1)
        p2im1 = cam_to_image(kf1["cam"], tr(T12, c["x3dc2"]), contract)
        p1im2 = cam_to_image(kf2["cam"], tr(T21, c["x3dc1"]), contract)
        d1 = c["p1im1"][None] - p2im1
        d2 = p1im2 - c["p2im2"][None]
        e1 = (d1[..., 0].astype(F64) * d1[..., 0].astype(F64) + d1[..., 1].astype(F64) * d1[..., 1].astype(F64)).astype(F32)
        e2 = (d2[..., 0].astype(F64) * d2[..., 0].astype(F64) + d2[..., 1].astype(F64) * d2[..., 1].astype(F64)).astype(F32)
        mask = (e1 < c["max_err1"].astype(F32)[None]) & (e2 < c["max_err2"].astype(F32)[None])
    return mask.sum(1).astype(np.int32), mask


# --- iterate (:140-207) ----------------------------------------------------------
def iterate_select(counts, N, min_inliers, max_its, iter_done=0, best_inliers=0):
    """The loop's bookkeeping over the inlier counts of the call's iterations:
    iters_run, no_more, found, found_iter, n_inliers, best_inliers_out and
    best_iter (the iteration holding the mBest* state, -1: none)."""
    if N < min_inliers:
        return dict(iters_run=0, no_more=1, found=0, found_iter=-1, n_inliers=0, best_inliers_out=best_inliers,
                    best_iter=-1)
    E = max(0, min(len(counts), max_its - iter_done))
    best, best_iter, found = best_inliers, -1, -1
    for it in range(E):
        if counts[it] >= best:
            best, best_iter = int(counts[it]), it
            if counts[it] > min_inliers:
                found = it
                break
    run = found + 1 if found >= 0 else E
    return dict(iters_run=run, no_more=int(found < 0 and iter_done + run >= max_its), found=int(found >= 0),
                found_iter=found, n_inliers=int(counts[found]) if found >= 0 else 0, best_inliers_out=best,
                best_iter=best_iter)


def outputs(c, sel, t, mask, n1):
    """The query's remaining outputs from the selection: T12, inliers by i1,
    R12 / t12 / s12."""
    out = dict(sel)
    f, b = sel["found_iter"], sel["best_iter"]
    inl = np.zeros(n1, np.uint8)
    if f >= 0:
        inl[c["indices1"][mask[f]]] = 1
    out.update(T12=t["T12_all"][f] if f >= 0 else None, inliers=inl, R12=t["R"][b] if b >= 0 else None,
               t12=t["T12_all"][b].reshape(4, 4)[:3, 3] if b >= 0 else None, s12=t["scale"][b] if b >= 0 else None)
    return out


def sim3_ransac(kf1, kf2, matches12, draws, n_iter=None, idx1=None, probability=0.99, min_inliers=20,
                max_iterations=300, iter_done=0, best_inliers=0, contract=False):
    """One Sim3Solver::iterate call: a dict with the outputs and taps of
    orbx_sim3_query, plus gap (the eigen-gap of every solve)."""
    draws = np.asarray(draws).reshape(-1, 3)
    M = len(draws) if n_iter is None else n_iter
    c = construct(kf1, kf2, matches12, idx1, contract)
    N, n1 = c["N"], len(kf1["keys"])
    out = dict(c)
    out["ransac_max_its"] = ransac_max_its(N, min_inliers, probability, max_iterations)
    if N < min_inliers or N < 3:
        out.update(iterate_select([], N, min_inliers, 0, iter_done, best_inliers))
        out.update(T12=None, R12=None, t12=None, s12=None, inliers=np.zeros(n1, np.uint8), sets=np.zeros((M, 3), np.int32),
                   q=np.zeros((M, 4), F32), R=np.zeros((M, 9), F32), scale=np.zeros(M, F32),
                   T12_all=np.zeros((M, 16), F32), T21_all=np.zeros((M, 16), F32), count=np.zeros(M, np.int32),
                   gap=np.ones(M))
        return out
    sets = make_sets(N, draws[:M])
    t = compute_t(c, sets)
    count, mask = check_inliers(c, kf1, kf2, t["T12_all"], t["T21_all"], contract)
    sel = iterate_select(count, N, min_inliers, out["ransac_max_its"], iter_done, best_inliers)
    out.update(sets=sets, count=count, mask=mask, **t)
    out.update(outputs(c, sel, t, mask, n1))
    return out


# --- synthetic scenes ------------------------------------------------------------
NLEVELS = 8
SIGMA2 = (F32(1.2) ** np.arange(NLEVELS, dtype=F32)) ** 2
CAM = np.array([500.0, 505.0, 320.0, 240.0], F32)


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(F32)


def make_keys(n, octaves):
    import orb_slam_amd as ox
    k = np.zeros(n, ox.KEYPOINT)
    k["size"], k["class_id"], k["octave"] = 31.0, -1, octaves
    return k


def scene(seed, N, outliers=0.2, noise=0.003, use_idx1=False, unmatched=5, invalid=3, extra2=6):
    """Two keyframes seeing N common map points, the second map a similarity
    (scale 1.1, a rotation, a shift) of the first with noise, a share of the
    partners replaced by unrelated points, plus keypoints without a match,
    matches onto missing / bad map points on either side and, under
    use_idx1, a permuted GetIndexInKeyFrame with two negative entries.
    Returns (kf1, kf2, matches12, idx1 or None); construct() keeps N."""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 9, N)], 1)
    S_R, S_t, S_s = _rot([0.05, -0.08, 0.03]), np.array([0.4, -0.2, 0.3]), 1.1
    Y = S_s * X @ S_R.T + S_t + rng.normal(0, noise, X.shape)
    n_out = int(round(outliers * N))
    if n_out:
        bad = rng.choice(N, n_out, replace=False)
        Y[bad] = np.stack([rng.uniform(-3, 3, n_out), rng.uniform(-2, 2, n_out), rng.uniform(4, 9, n_out)], 1)
    T1 = _pose(_rot([0.02, 0.01, -0.01]), [0.1, 0.0, 0.2])
    # KF2 looks at its own (transformed) map from about where KF1 looks at the first
    T2 = _pose(_rot([-0.01, 0.03, 0.02]) @ S_R.T, -(_rot([-0.01, 0.03, 0.02]) @ S_R.T) @ S_t / 1.0 + [0.0, 0.1, 0.5])
    extra = unmatched + 2 * invalid + (2 if use_idx1 else 0)
    n1, n2 = N + extra, N + extra + extra2
    slot1, slot2 = rng.permutation(n1), rng.permutation(n2)
    pos1, pos2 = rng.uniform(-1, 1, (n1, 3)) + [0, 0, 6], rng.uniform(-1, 1, (n2, 3)) + [0, 0, 6]
    valid1, valid2 = np.ones(n1, np.uint8), np.ones(n2, np.uint8)
    m = np.full(n1, -1, np.int32)
    pos1[slot1[:N]], pos2[slot2[:N]] = X, Y
    m[slot1[:N]] = slot2[:N]
    o = N
    o += unmatched                                  # keypoints of KF1 without a match
    for k in range(invalid):                        # matched, but KF1's map point is missing
        m[slot1[o + k]] = slot2[N + k]
        valid1[slot1[o + k]] = 0
    o += invalid
    for k in range(invalid):                        # matched onto a bad map point of KF2
        m[slot1[o + k]] = slot2[N + invalid + k]
        valid2[slot2[N + invalid + k]] = 0
    o += invalid
    kf1 = dict(keys=make_keys(n1, rng.randint(0, NLEVELS, n1)), pos=pos1.astype(F32), valid=valid1, Tcw=T1, cam=CAM,
               sigma2=SIGMA2)
    kf2 = dict(keys=make_keys(n2, rng.randint(0, NLEVELS, n2)), pos=pos2.astype(F32), valid=valid2, Tcw=T2,
               cam=CAM + F32(3), sigma2=SIGMA2)
    idx1 = None
    if use_idx1:
        # the map point at i1 reports another keypoint index: the data moves there
        perm = rng.permutation(n1).astype(np.int32)
        for name in ("keys", "pos", "valid"):
            moved = kf1[name].copy()
            moved[perm] = kf1[name]
            kf1[name] = moved
        idx1 = perm.copy()
        for k in range(2):                          # matched, GetIndexInKeyFrame < 0
            i = slot1[o + k]
            m[i] = slot2[N + 2 * invalid + k]
            idx1[i] = -1
    return kf1, kf2, m, idx1


def make_draws(seed, n_iter, N=None, cap=0.05):
    """n_iter x 3 rand() values.  With N given, a triple whose set repeats a
    correspondence is kept only while such sets number at most cap * n_iter:
    the removal repeats one in 1 / (N (N - 1)) of all sets, a sixth of them at
    N = 3, and a repeated correspondence makes N's largest eigenvalue double,
    which no choice of seed would keep inside the eigen-gap cap."""
    rs = np.random.RandomState(seed)
    if N is None or N < 3:
        return rs.randint(0, 2**31, size=(n_iter, 3), dtype=np.int64).astype(np.int32)
    out, allowed = [], int(cap * n_iter)
    while len(out) < n_iter:
        t = rs.randint(0, 2**31, size=3, dtype=np.int64).astype(np.int32)
        if len(set(make_sets(N, t)[0].tolist())) < 3:
            if allowed == 0:
                continue
            allowed -= 1
        out.append(t)
    return np.stack(out)


# --- the cases of tests/test_sim3_gpu.py ----------------------------------------
# (N, n_iter, min_inliers, use_idx1, scene seed, draw seed): N and n_iter cross
# the lane, the wave and the workgroup on both axes; min_inliers is small where
# N is, so that iterate returns.  The seeds are chosen so that the eigen-gap
# cut of the solve comparison excludes at most 5 % of a case's iterations;
# tests/test_sim3_numpy.py checks that with the restatement alone.
CASES = [(N, M, {3: 3, 19: 6}.get(N, 20), (a + b) % 2 == 1, 300 + 10 * a + b, 400 + 10 * a + b)
         for a, N in enumerate((3, 19, 20, 21, 64, 65, 300)) for b, M in enumerate((1, 5, 64, 65, 300))]
CUT = 1e-4
_case_cache = {}


def case(i):
    """(inputs, restatement result) of CASES[i], computed once: inputs are
    (kf1, kf2, matches12, draws, kwargs)."""
    if i not in _case_cache:
        N, M, mi, use_idx1, seed, dseed = CASES[i]
        kf1, kf2, m, idx1 = scene(seed, N, use_idx1=use_idx1)
        d = make_draws(dseed, M, N if N < 8 else None)
        kw = dict(idx1=idx1, min_inliers=mi)
        _case_cache[i] = ((kf1, kf2, m, d, kw), sim3_ransac(kf1, kf2, m, d, **kw))
    return _case_cache[i]


def considered(r):
    """The iterations whose eigenproblem passes the gap cut."""
    return r["gap"] >= CUT


def write_golden(path):
    """tests/golden/sim3_ransac.npz: two scenes (120 correspondences, one with
    idx1; 64 iterations) with the restatement's sets, q, R, counts, T12 / T21
    and the eigen-gap of every solve."""
    out = {}
    for s, (seed, use_idx1) in enumerate([(31, False), (32, True)]):
        kf1, kf2, m, idx1 = scene(seed, 120, use_idx1=use_idx1)
        d = make_draws(40 + s, 64)
        r = sim3_ransac(kf1, kf2, m, d, idx1=idx1)
        rec = dict(matches12=m, draws=d, idx1=idx1 if idx1 is not None else np.zeros(0, np.int32), N=np.int32(r["N"]),
                   sets=r["sets"], q=r["q"], R=r["R"], count=r["count"], T12_all=r["T12_all"], T21_all=r["T21_all"],
                   gap=r["gap"], found_iter=np.int32(r["found_iter"]))
        for side, kf in (("1", kf1), ("2", kf2)):
            for k, v in kf.items():
                rec[f"kf{side}_{k}"] = v
        for k, v in rec.items():
            out[f"s{s}_{k}"] = v
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    write_golden(Path(__file__).resolve().parent / "golden" / "sim3_ransac.npz")
