"""A numpy restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:791-987):
the comparator of the device's orbx_optimize_sim3.

Written from the reference's code path:

* g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3/sim3.h): the exponential with its
  four branches, operator* without renormalisation, inverse() and map();
* VertexSim3Expmap and the two projection edges
  (types_seven_dof_expmap.h:48-171): oplus = Sim3(update) * estimate,
  e12 = obs1 - cam_map1(project(S.map(P2c))),
  e21 = obs2 - cam_map2(project(S.inverse().map(P1c)));
* BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205): central
  differences with delta = 1e-9 on the Sim3 vertex, and constructQuadraticForm
  (:91-113);
* OptimizationAlgorithmLevenberg with ORB-SLAM's stop rule, structured as
  tests/test_pose_numpy.py, over a dense LDLT with diagonal pivoting and
  Eigen's isPositive() (linear_solver_dense.h:65-113), restated here entry by
  entry so that the trajectory does not depend on a LAPACK build.

Everything is float64 operation by operation: numpy ufuncs across the
correspondences (one rounding per operation, the same as a scalar loop), and
every sum over edges a strictly sequential np.add.accumulate in g2o's
active-edge order e12_0, e21_0, e12_1, e21_1, ...  No @ and no BLAS.

quat_rotate, quat_matrix and matrix_quat are those of tests/test_lba_numpy.py.
Its quat_mul groups the cross product apart from the other two terms; Eigen's
scalar quaternion product (and the device's qmul) adds the four products of a
component from left to right, so quat_mul is restated here in that order.

The Jacobian path evaluates Sim3(update) at update = +-1e-9 e_d only: the
|sigma| < eps, theta < eps branch, which needs + - * /, sqrt and exp at 0 and
+-1e-9.  Those two exponentials are held as the correctly rounded constants
(EXP_P / EXP_M), so linearize() is reproducible bit for bit anywhere.
"""
import math

import numpy as np

from sim3_numpy import CAM, F32, F64, NLEVELS, SIGMA2, _pose, _rot, make_keys, transform
from test_lba_numpy import matrix_quat, quat_matrix, quat_rotate

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EXP_P = float.fromhex("0x1.000000044b830p+0")    # exp(+1e-9), correctly rounded
EXP_M = float.fromhex("0x1.fffffff768fa1p-1")    # exp(-1e-9)
INV_SIGMA2 = (F32(1) / SIGMA2).astype(F32)       # mvInvLevelSigma2 (src/ORBextractor.cc)


# --- g2o::Sim3 as (x, y, z, w, tx, ty, tz, s) --------------------------------------
def quat_mul(a, b):
    """Eigen's scalar quaternion product, each component summed left to right."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def sim3_from_float(R, t, s):
    """g2o::Sim3(Converter::toMatrix3d(R), toVector3d(t), s): widened floats,
    Eigen's quaternion of the matrix, no normalisation."""
    R = np.asarray(R, F32).reshape(3, 3).astype(F64)
    t = np.asarray(t, F32).reshape(3).astype(F64)
    return np.concatenate([matrix_quat(R), t, [float(F32(s))]])


def sim3_exp(u, es=None):
    """Sim3(const Vector7d& update) (sim3.h:70-142); es: exp(update[6]) where
    the caller holds it as a constant."""
    o0, o1, o2 = (float(v) for v in u[:3])
    ups = [float(v) for v in u[3:6]]
    sigma = float(u[6])
    theta = math.sqrt(o0 * o0 + o1 * o1 + o2 * o2)
    Om = [[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]]
    Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    s = math.exp(sigma) if es is None else es
    eye = lambda i, j: 1.0 if i == j else 0.0
    eps = 0.00001

    def rodrigues():
        a, b = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
        return [[eye(i, j) + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]

    def small():
        return [[eye(i, j) + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]

    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1. / 2., 1. / 6.
            R = small()
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            R = rodrigues()
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = small()
        else:
            R = rodrigues()
            a, b = s * math.sin(theta), s * math.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    q = matrix_quat(np.array(R))
    W = [[A * Om[i][j] + B * Om2[i][j] + C * eye(i, j) for j in range(3)] for i in range(3)]
    t = [W[i][0] * ups[0] + W[i][1] * ups[1] + W[i][2] * ups[2] for i in range(3)]
    return np.array([q[0], q[1], q[2], q[3], t[0], t[1], t[2], s])


def sim3_mul(a, b):
    """Sim3::operator* (sim3.h:266-272): no renormalisation."""
    r = quat_mul(a[:4], b[:4])
    t = a[7] * quat_rotate(a[:4], b[4:7]) + a[4:7]
    return np.concatenate([r, t, [a[7] * b[7]]])


def sim3_inverse(a):
    """Sim3::inverse (sim3.h:233-236)."""
    rc = np.array([-a[0], -a[1], -a[2], a[3]])
    return np.concatenate([rc, quat_rotate(rc, (-1. / a[7]) * a[4:7]), [1. / a[7]]])


def sim3_map(a, P):
    """Sim3::map of points P (n, 3)."""
    return a[7] * quat_rotate(a[:4], P) + a[4:7]


def oplus(est, dx):
    """VertexSim3Expmap::oplusImpl, _fix_scale false."""
    return sim3_mul(sim3_exp(dx), est)


def perturbed(est):
    """The 15 estimates of one linearisation (the current one, then +delta and
    -delta per dimension) and their inverses."""
    out = [est]
    for d in range(7):
        for sign, es in ((1.0, EXP_P), (-1.0, EXP_M)):
            u = np.zeros(7)
            u[d] = sign * DELTA
            out.append(sim3_mul(sim3_exp(u, es if d == 6 else 1.0), est))
    return out, [sim3_inverse(e) for e in out]


# --- the problem ---------------------------------------------------------------------
def build_problem(kf1, kf2, matches12, th2=10.0, sigma_inverse=False):
    """The correspondences of :844-923 in i order.  kf1 / kf2: dicts of keys,
    pos, valid, Tcw, cam, inv_sigma2 / sigma2.  sigma_inverse: e21's
    information from KF2's inverse table instead (what :912 does not do)."""
    m = np.asarray(matches12, np.int32)
    idx = np.array([i for i in range(len(m)) if m[i] >= 0 and kf1["valid"][i] and kf2["valid"][m[i]]], np.int64)
    i2 = m[idx].astype(np.int64)
    k1, k2 = kf1["keys"][idx], kf2["keys"][i2]
    pos1 = np.asarray(kf1["pos"], F32).reshape(-1, 3)[idx]
    pos2 = np.asarray(kf2["pos"], F32).reshape(-1, 3)[i2]
    x1 = transform(kf1["Tcw"], pos1).reshape(-1, 3) if len(idx) else np.zeros((0, 3), F32)
    x2 = transform(kf2["Tcw"], pos2).reshape(-1, 3) if len(idx) else np.zeros((0, 3), F32)
    w2 = (kf2["inv_sigma2"] if sigma_inverse else kf2["sigma2"])[k2["octave"]]
    return dict(idx=idx.astype(np.int32), x3dc1=x1, x3dc2=x2, P1=x1.astype(F64), P2=x2.astype(F64),
                obs1=np.stack([k1["x"], k1["y"]], 1).astype(F64), obs2=np.stack([k2["x"], k2["y"]], 1).astype(F64),
                w1=np.asarray(kf1["inv_sigma2"], F32)[k1["octave"]].astype(F64), w2=np.asarray(w2, F32).astype(F64),
                cam1=np.asarray(kf1["cam"], F32).astype(F64), cam2=np.asarray(kf2["cam"], F32).astype(F64),
                delta=float(np.sqrt(F32(th2))), th2=float(F32(th2)), active=np.ones(len(idx), bool))


def _project(cam, p):
    with np.errstate(all="ignore"):
        return np.stack([p[:, 0] / p[:, 2] * cam[0] + cam[2], p[:, 1] / p[:, 2] * cam[1] + cam[3]], 1)


def edge_errors(est, inv, pb):
    """computeError of every pair: (n, 2) for e12 and for e21."""
    return (pb["obs1"] - _project(pb["cam1"], sim3_map(est, pb["P2"])),
            pb["obs2"] - _project(pb["cam2"], sim3_map(inv, pb["P1"])))


def chi2_of(e, w):
    return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])


def huber(e2, delta):
    """RobustKernelHuber::robustify: rho[0], rho[1]."""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        inl = e2 <= dsqr
        return np.where(inl, e2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def seq_sum(terms):
    """Strictly sequential sum over axis 0, from +0.0."""
    z = np.zeros((1,) + terms.shape[1:])
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([z, terms]), axis=0)[-1]


def interleave(a12, a21):
    """Per-pair arrays into g2o's edge order e12_0, e21_0, e12_1, ..."""
    out = np.empty((2 * len(a12),) + a12.shape[1:])
    out[0::2], out[1::2] = a12, a21
    return out


LOWER = [(i, j) for i in range(7) for j in range(i + 1)]


def linearize(est, pb):
    """computeActiveErrors + activeRobustChi2 + buildSystem at est over the
    active pairs: chi2, the 28 lower entries of H (row-major packed), b, and
    per pair (all of them, active or not) the errors (n, 4: e12, e21) and the
    Jacobians (n, 28: e12 2x7 row-major, e21 2x7)."""
    ests, invs = perturbed(np.asarray(est, F64))
    errs = [edge_errors(ests[k], invs[k], pb) for k in range(15)]
    n = len(pb["idx"])
    err = np.concatenate([errs[0][0], errs[0][1]], 1) if n else np.zeros((0, 4))
    J = np.zeros((n, 2, 2, 7))
    with np.errstate(all="ignore"):
        for d in range(7):
            for e in range(2):
                J[:, e, :, d] = SCALAR * (errs[1 + 2 * d][e] - errs[2 + 2 * d][e])
        terms = []
        for e, w in ((0, pb["w1"]), (1, pb["w2"])):
            er = errs[0][e]
            rho0, rho1 = huber(chi2_of(er, w), pb["delta"])
            W = rho1 * w
            om0, om1 = -(w * er[:, 0]) * rho1, -(w * er[:, 1]) * rho1
            J0, J1 = J[:, e, 0, :], J[:, e, 1, :]
            cols = [rho0]
            cols += [(J0[:, i] * W) * J0[:, j] + (J1[:, i] * W) * J1[:, j] for i, j in LOWER]
            cols += [J0[:, i] * om0 + J1[:, i] * om1 for i in range(7)]
            terms.append(np.stack(cols, 1)[pb["active"]])
    s = seq_sum(interleave(terms[0], terms[1]))
    return float(s[0]), s[1:29].copy(), s[29:36].copy(), err, J.reshape(n, 28)


def active_chi2(est, pb):
    """computeActiveErrors + activeRobustChi2 at est."""
    e12, e21 = edge_errors(est, sim3_inverse(est), pb)
    a = pb["active"]
    r12, r21 = huber(chi2_of(e12, pb["w1"]), pb["delta"])[0][a], huber(chi2_of(e21, pb["w2"]), pb["delta"])[0][a]
    return float(seq_sum(interleave(r12, r21)))


def stored_chi2(est, pb):
    """chi2() of every pair's two edges with the errors computeActiveErrors
    left at est: (n, 2)."""
    e12, e21 = edge_errors(est, sim3_inverse(est), pb)
    with np.errstate(all="ignore"):
        return np.stack([chi2_of(e12, pb["w1"]), chi2_of(e21, pb["w2"])], 1)


# --- Eigen::LDLT, as LinearSolverDense uses it ---------------------------------------
def ldlt_solve(H, b):
    """Eigen::LDLT<MatrixXd> (lower, diagonal pivoting) of the symmetric H
    (n x n, the lower triangle is read) and the solve of H x = b: (isPositive,
    x).  The algorithm of the device's ldlt_solve<N> (orbx_lm.h)."""
    n = len(b)
    m = [[float(H[i][j]) if j <= i else 0.0 for j in range(n)] for i in range(n)]
    tr, sign = [0] * n, 0
    for k in range(n):
        big, bv = k, abs(m[k][k])
        for i in range(k + 1, n):
            if abs(m[i][i]) > bv:
                bv, big = abs(m[i][i]), i
        tr[k] = big
        if big != k:
            q = big
            for j in range(k):
                m[k][j], m[q][j] = m[q][j], m[k][j]
            for i in range(q + 1, n):
                m[i][k], m[i][q] = m[i][q], m[i][k]
            m[k][k], m[q][q] = m[q][q], m[k][k]
            for i in range(k + 1, q):
                m[i][k], m[q][i] = m[q][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            acc = m[k][0] * temp[0]
            for j in range(1, k):
                acc += m[k][j] * temp[j]
            m[k][k] -= acc
            for i in range(k + 1, n):
                for j in range(k):
                    m[i][k] -= m[i][j] * temp[j]
        akk = m[k][k]
        if k < n - 1 and abs(akk) > 0.0:
            for i in range(k + 1, n):
                m[i][k] /= akk
        if sign == 1:
            sign = 3 if akk < 0 else 1
        elif sign == 2:
            sign = 3 if akk > 0 else 2
        elif sign == 0:
            sign = 1 if akk > 0 else (2 if akk < 0 else 0)
    x = [float(v) for v in b]
    for k in range(n):
        if tr[k] != k:
            x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(n):
        for j in range(i):
            x[i] -= m[i][j] * x[j]
    for i in range(n):
        x[i] = x[i] / m[i][i] if abs(m[i][i]) > 2.2250738585072014e-308 else 0.0
    for i in range(n - 2, -1, -1):
        s = m[i + 1][i] * x[i + 1]
        for j in range(i + 2, n):
            s += m[j][i] * x[j]
        x[i] -= s
    for k in range(n - 1, -1, -1):
        if tr[k] != k:
            x[k], x[tr[k]] = x[tr[k]], x[k]
    return sign in (0, 1), np.array(x)


def unpack(h):
    H = np.zeros((7, 7))
    for k, (i, j) in enumerate(LOWER):
        H[i, j] = H[j, i] = h[k]
    return H


# --- the Levenberg loop ----------------------------------------------------------------
def levenberg(est, pb, its, log):
    """optimize(its) over the active pairs from est: (estimate, the estimate of
    the last computeActiveErrors, iterations, trials, LDLT failures)."""
    errest = est
    lam = ni = 0.0
    nbad = it_done = tr_done = fails = 0
    for it in range(its):
        chi, h, b, err, J = linearize(est, pb)
        rec = dict(est=est.copy(), chi2=chi, H=h, b=b, dx=[])
        if not log:
            rec["err"], rec["J"] = err, J
        ini = chi
        if it == 0:
            lam = 1e-5 * max(0.0, *[abs(h[k]) for k, (i, j) in enumerate(LOWER) if i == j])
            ni, nbad = 2.0, 0
        H = unpack(h)
        k = 0
        while True:
            ok, dx = ldlt_solve(H + lam * np.eye(7), b)
            est0 = est
            if ok:
                est = oplus(est, dx)
            else:
                dx = np.zeros(7)
                fails += 1
            rec["dx"].append(dx)
            tmp = active_chi2(est, pb)
            errest = est
            if not ok:
                tmp = np.finfo(F64).max
            scale = 0.0
            for j in range(7):
                scale += dx[j] * (lam * dx[j] + b[j])
            scale += 1e-3
            with np.errstate(all="ignore"):
                rho = (chi - tmp) / scale
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                chi = tmp
            else:
                lam *= ni
                ni *= 2
                est = est0
            k += 1
            if not (rho < 0 and k < 10):
                break
        rec["lambda"], rec["trials"] = lam, k
        log.append(rec)
        tr_done += k
        it_done += 1
        if k == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - chi) * 1e3 < ini else 0
        if nbad >= 3:
            break
    return est, errest, it_done, tr_done, fails


def optimize_sim3(kf1, kf2, matches12, R12, t12, s12, th2=10.0, sigma_inverse=False):
    """Optimizer::OptimizeSim3: a dict of matches12 (out), n_in (the return
    value), n_corr, n_bad, returned_early, est (q12, t12d, s12d; the input on
    the early exit), the float R12 / t12 / s12, iterations / trials / not_posdef
    per round, log (one record per LM iteration), chi2 (per check, (n, 2), NaN
    where a pair was not tested), check_est and the problem."""
    pb = build_problem(kf1, kf2, matches12, th2, sigma_inverse)
    m = np.array(matches12, np.int32)
    est0 = sim3_from_float(R12, t12, s12)
    n = len(pb["idx"])
    out = dict(matches12=m, n_in=0, n_corr=n, n_bad=0, returned_early=1, est=est0, iterations=[0, 0], trials=[0, 0],
               not_posdef=[0, 0], log=[], chi2=np.full((2, n, 2), np.nan), check_est=np.zeros((2, 8)), problem=pb)

    def finish(est):
        out["est"] = est
        out["R12"] = quat_matrix(est[:4]).astype(F32)
        out["t12"], out["s12"] = est[4:7].astype(F32), F32(est[7])
        return out
    if n == 0:
        return finish(est0)
    est, errest, out["iterations"][0], out["trials"][0], out["not_posdef"][0] = levenberg(est0, pb, 5, out["log"])
    c = stored_chi2(errest, pb)
    out["chi2"][0], out["check_est"][0] = c, errest
    bad = (c[:, 0] > pb["th2"]) | (c[:, 1] > pb["th2"])
    m[pb["idx"][bad]] = -1
    pb["active"] = ~bad
    out["n_bad"] = int(bad.sum())
    if n - out["n_bad"] < 10:
        return finish(est0)
    more = 10 if out["n_bad"] > 0 else 5
    est, errest, out["iterations"][1], out["trials"][1], out["not_posdef"][1] = levenberg(est, pb, more, out["log"])
    c = stored_chi2(errest, pb)
    out["chi2"][1][~bad], out["check_est"][1] = c[~bad], errest
    bad2 = ~bad & ((c[:, 0] > pb["th2"]) | (c[:, 1] > pb["th2"]))
    m[pb["idx"][bad2]] = -1
    out["n_in"] = int((~bad & ~bad2).sum())
    out["returned_early"] = 0
    return finish(est)


# --- scenes ----------------------------------------------------------------------------
TRUE_S12 = dict(w=np.array([0.04, -0.06, 0.03]), t=np.array([0.3, -0.15, 0.25]), s=1.1)
NOT_OBSERVED = -2     # a non-NULL entry whose point KF2 does not observe


def true_sim3():
    R = _rot(TRUE_S12["w"])
    return np.concatenate([matrix_quat(R), TRUE_S12["t"], [TRUE_S12["s"]]])


def _rows_times(P, M):
    """P (n, 3) times M (3 x 3), written out (no BLAS)."""
    return P[:, 0:1] * M[0] + P[:, 1:2] * M[1] + P[:, 2:3] * M[2]


def scene(seed, N, gross=0.0, noise=0.1, start=0.03, null=4, invalid=3, unobserved=2, extra2=7, behind=0,
          octaves=None):
    """Two keyframes with N correspondences whose camera-frame points are
    related by TRUE_S12 (P1c = s R P2c + t): keypoints at the projections plus
    Gaussian pixel noise, octaves over all levels, a share `gross` of the pairs
    with one observation displaced by tens of pixels, `behind` pairs whose KF2
    point lies behind KF1's camera, and skipped entries of each kind -- NULL
    (-1), KF1's own point missing, the matched point bad, the matched point not
    observed by KF2 (NOT_OBSERVED) -- in n1 != n2 keypoints.  Returns (kf1, kf2,
    matches12, (R12, t12, s12)): the float start, `start` off the truth."""
    rng = np.random.RandomState(seed)
    R, t, s = _rot(TRUE_S12["w"]), TRUE_S12["t"], TRUE_S12["s"]
    P1 = np.stack([rng.uniform(-2.5, 2.5, N), rng.uniform(-1.8, 1.8, N), rng.uniform(4, 9, N)], 1)
    P2 = _rows_times(P1 - t, R) / s                          # R^T (P1 - t) / s
    for k in range(behind):
        P2[k] = _rows_times((np.array([[0.3 * k, -0.2, -3.0 - k]]) - t), R)[0] / s
    T1 = _pose(_rot([0.02, 0.01, -0.01]), [0.1, 0.0, 0.2]).astype(F64)
    T2 = _pose(_rot([-0.01, 0.03, 0.02]), [0.0, 0.1, 0.5]).astype(F64)
    extra = null + 2 * invalid + unobserved
    n1, n2 = N + extra, N + invalid * 2 + extra2
    slot1, slot2 = rng.permutation(n1), rng.permutation(n2)
    pos1, pos2 = rng.uniform(-1, 1, (n1, 3)) + [0, 0, 6], rng.uniform(-1, 1, (n2, 3)) + [0, 0, 6]
    pos1[slot1[:N]] = _rows_times(P1 - T1[:3, 3], T1[:3, :3])
    pos2[slot2[:N]] = _rows_times(P2 - T2[:3, 3], T2[:3, :3])
    pos1, pos2 = pos1.astype(F32), pos2.astype(F32)
    cam1, cam2 = CAM, CAM + F32(3)
    k1 = make_keys(n1, rng.randint(0, NLEVELS, n1) if octaves is None else octaves)
    k2 = make_keys(n2, rng.randint(0, NLEVELS, n2) if octaves is None else octaves)
    c1 = transform(T1.astype(F32), pos1).reshape(-1, 3).astype(F64)
    c2 = transform(T2.astype(F32), pos2).reshape(-1, 3).astype(F64)
    # an exact pair projects KF2's point through the truth into KF1 and back
    uv1, uv2 = _project(cam1.astype(F64), c1), _project(cam2.astype(F64), c2)
    tr = true_sim3()
    uv1[slot1[:N]] = _project(cam1.astype(F64), sim3_map(tr, c2[slot2[:N]]))
    uv2[slot2[:N]] = _project(cam2.astype(F64), sim3_map(sim3_inverse(tr), c1[slot1[:N]]))
    uv1 += rng.normal(0, noise, uv1.shape) if noise else 0
    uv2 += rng.normal(0, noise, uv2.shape) if noise else 0
    n_gross = int(round(gross * N))
    for k in rng.choice(N, n_gross, replace=False) if n_gross else []:
        d = rng.uniform(25, 60) * np.array([np.cos(k), np.sin(k)])
        if k % 2:
            uv1[slot1[k]] += d
        else:
            uv2[slot2[k]] += d
    k1["x"], k1["y"] = uv1[:, 0], uv1[:, 1]
    k2["x"], k2["y"] = uv2[:, 0], uv2[:, 1]
    valid1, valid2 = np.ones(n1, np.uint8), np.ones(n2, np.uint8)
    m = np.full(n1, -1, np.int32)
    m[slot1[:N]] = slot2[:N]
    o = N + null
    for k in range(invalid):                        # matched, but KF1's own map point is missing or bad
        m[slot1[o + k]] = slot2[N + k]
        valid1[slot1[o + k]] = 0
    o += invalid
    for k in range(invalid):                        # matched onto a bad map point
        m[slot1[o + k]] = slot2[N + invalid + k]
        valid2[slot2[N + invalid + k]] = 0
    o += invalid
    for k in range(unobserved):                     # GetIndexInKeyFrame(pKF2) < 0
        m[slot1[o + k]] = NOT_OBSERVED - k
    common = dict(sigma2=SIGMA2, inv_sigma2=INV_SIGMA2)
    kf1 = dict(keys=k1, pos=pos1, valid=valid1, Tcw=T1.astype(F32), cam=cam1, **common)
    kf2 = dict(keys=k2, pos=pos2, valid=valid2, Tcw=T2.astype(F32), cam=cam2, **common)
    R0 = _rot(TRUE_S12["w"] + start * np.array([0.5, -0.4, 0.6]))
    init = (R0.astype(F32), (t * (1 + start * np.array([1.0, -0.7, 0.5]))).astype(F32), F32(s * (1 + start)))
    return kf1, kf2, m, init


# --- the cases of tests/test_sim3opt_gpu.py --------------------------------------------
# name: (N, scene arguments).  The seeds are chosen so that every stored chi2 at
# both checks lies outside th2 (1 +- 1e-3) (tests/test_sim3opt_numpy.py asserts
# it): the decisions then do not turn on the last bits of two maths libraries.
TH2 = 10.0
MARGIN = 1e-3
CASES = {
    "n0": (0, dict(seed=500)),
    "n9": (9, dict(seed=501)),
    "n10": (10, dict(seed=502)),
    "n12_gross3": (12, dict(seed=503, gross=0.25)),
    "n40_gross": (40, dict(seed=504, gross=0.25)),
    "n64": (64, dict(seed=505, gross=0.1)),
    "n65": (65, dict(seed=506, gross=0.1)),
    "n130_clean": (130, dict(seed=507, noise=0.02, start=0.002)),
    "n257": (257, dict(seed=508, gross=0.15)),         # one past the lone call's group of 256 pairs
    "n4000": (4000, dict(seed=509, gross=0.2, null=40, invalid=10, unobserved=5, extra2=0)),
    "behind": (48, dict(seed=510, gross=0.1, behind=2)),
}
_case_cache = {}


def case(name):
    """((kf1, kf2, matches12, init), the restatement's result) of a case,
    computed once and shared."""
    if name not in _case_cache:
        N, kw = CASES[name]
        kf1, kf2, m, init = scene(N=N, **kw)
        _case_cache[name] = ((kf1, kf2, m, init), optimize_sim3(kf1, kf2, m, *init, th2=TH2))
    return _case_cache[name]


def margin_ok(r, th2=TH2, margin=MARGIN):
    c = r["chi2"][np.isfinite(r["chi2"])]
    return bool(np.all((c < th2 * (1 - margin)) | (c > th2 * (1 + margin))))


GOLDEN = ("n12_gross3", "n40_gross", "n65")


def golden_record(name):
    (kf1, kf2, m, init), r = case(name)
    rec = dict(matches12=m, R12=init[0], t12=init[1], s12=init[2], out_matches12=r["matches12"],
               n_in=np.int32(r["n_in"]), n_corr=np.int32(r["n_corr"]), n_bad=np.int32(r["n_bad"]),
               returned_early=np.int32(r["returned_early"]), est=r["est"], chi2=r["chi2"],
               iterations=np.array(r["iterations"], np.int32), trials=np.array(r["trials"], np.int32),
               log_est=np.array([x["est"] for x in r["log"]]), log_chi2=np.array([x["chi2"] for x in r["log"]]),
               log_H=np.array([x["H"] for x in r["log"]]), log_b=np.array([x["b"] for x in r["log"]]))
    for side, kf in (("1", kf1), ("2", kf2)):
        for k, v in kf.items():
            rec[f"kf{side}_{k}"] = np.asarray(v)
    return rec


def write_golden(folder):
    """tests/golden/sim3opt_<case>.npz: the inputs and the restatement's outputs."""
    for name in GOLDEN:
        np.savez_compressed(folder / f"sim3opt_{name}.npz", **golden_record(name))


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    write_golden(Path(__file__).resolve().parent / "golden")
