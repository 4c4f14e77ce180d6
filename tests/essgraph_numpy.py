"""A numpy restatement of Optimizer::OptimizeEssentialGraph
(src/Optimizer.cc:540-789): the comparator of the device's
orbx_optimize_essential_graph.

Written from the reference's code path:

* the vertices (:568-601): CorrectedSim3 where the map has one, else
  Sim3(toMatrix3d(R), toVector3d(t), 1.0) (sim3opt_numpy.sim3_from_float), the
  loop keyframe fixed, the free vertices ordered by id, a vertex without an
  edge outside the system;
* the edges (:604-729): EdgeSim3 with information I7; a loop-connection edge
  (kind 0) measures vScw[j] * vScw[i].inverse(), a normal edge (kind 1) takes
  each side from NonCorrectedSim3 where present;
* the error (types_seven_dof_expmap.h:106-114): (C * v0 * v1.inverse()).log(),
  with Sim3::log (sim3.h:148-230) operation by operation: four branches on
  |sigma| < 1e-5 and d > 1 - 1e-5, deltaR, and W.lu().solve(t) as Eigen's
  partial-pivot LU of a 3 x 3 in its unblocked order (pivot search by |.| down
  the column, row swap, the column scaled, the rank-1 update, the permuted
  forward and back substitution).  B * Omega * Omega is taken as
  (B * Omega) * Omega;
* BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205): central
  differences with delta = 1e-9 on both vertices, Sim3(+-delta e_d) * estimate
  with the two exponentials as constants (sim3opt_numpy.EXP_P / EXP_M);
* constructQuadraticForm with Omega = I: H_ii += Ji^T Ji, H_jj += Jj^T Jj,
  H_ij += Ji^T Jj, b_i -= Ji^T e, b_j -= Jj^T e, a fixed side contributing
  nothing; H and b are sequential sums in edge order, every 7-term product sum
  sequential;
* the solver: (H + lambda I) x = b by a dense Cholesky of its own (a pivot
  that is not positive and finite fails the solve: a zero step, the trial
  rejected), lambda from setUserLambdaInit(1e-16), optimize(20) with at most
  10 trials per iteration and ORB-SLAM's stop rule, the update
  Sim3(dx) * estimate;
* the recovery (:737-755) and the point correction (:758-788).

Everything is float64, vectorised across the edges (one rounding per
operation, the same as a scalar loop).  The five library functions the path
uses -- acos, sin, cos, log, exp -- go through MATH, so that a test can move
their results by an ulp (Ulp) and measure what two conforming maths libraries
may differ by; the tolerances of tests/test_essgraph_gpu.py come from that
measurement (TOL).
"""
import numpy as np

from sim3opt_numpy import DELTA, EXP_M, EXP_P, SCALAR, sim3_from_float
from sim3_numpy import F32, F64, _rot
from test_lba_numpy import matrix_quat, quat_matrix

MAX_LM, MAX_TRIALS, LAMBDA_INIT = 20, 10, 1e-16
EPS = 0.00001


class Exact:
    """The platform's functions as they are."""
    acos, sin, cos, log, exp = (staticmethod(f) for f in (np.arccos, np.sin, np.cos, np.log, np.exp))


class Ulp:
    """Each result moved by -1, 0 or +1 ulp at random."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def _wrap(self, f, x):
        with np.errstate(all="ignore"):
            y = np.asarray(f(x), F64)
        k = self.rng.randint(-1, 2, y.shape)
        out = np.where(k < 0, np.nextafter(y, -np.inf), np.where(k > 0, np.nextafter(y, np.inf), y))
        return out if out.ndim else float(out)

    acos = lambda self, x: self._wrap(np.arccos, x)
    sin = lambda self, x: self._wrap(np.sin, x)
    cos = lambda self, x: self._wrap(np.cos, x)
    log = lambda self, x: self._wrap(np.log, x)
    exp = lambda self, x: self._wrap(np.exp, x)


MATH = Exact


def set_math(m):
    global MATH
    MATH = m


# --- g2o::Sim3 over arrays (..., 8): (x, y, z, w, tx, ty, tz, s) ------------------------
def vqmul(a, b):
    ax, ay, az, aw = (a[..., k] for k in range(4))
    bx, by, bz, bw = (b[..., k] for k in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def vqrot(q, v):
    """Eigen's Quaternion * Vector3: uv = 2 (u x v); v + w uv + u x uv."""
    x, y, z, w = (q[..., k] for k in range(4))
    v0, v1, v2 = (v[..., k] for k in range(3))
    u0, u1, u2 = y * v2 - z * v1, z * v0 - x * v2, x * v1 - y * v0
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0, c1, c2 = y * u2 - z * u1, z * u0 - x * u2, x * u1 - y * u0
    return np.stack([v0 + w * u0 + c0, v1 + w * u1 + c1, v2 + w * u2 + c2], -1)


def vmul(a, b):
    r = vqmul(a[..., :4], b[..., :4])
    t = a[..., 7:8] * vqrot(a[..., :4], b[..., 4:7]) + a[..., 4:7]
    return np.concatenate([r, t, a[..., 7:8] * b[..., 7:8]], -1)


def vinv(a):
    rc = a[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    f = -1. / a[..., 7:8]
    return np.concatenate([rc, vqrot(rc, f * a[..., 4:7]), 1. / a[..., 7:8]], -1)


def vmap(a, P):
    return a[..., 7:8] * vqrot(a[..., :4], P) + a[..., 4:7]


def vqmat(q):
    """Eigen's toRotationMatrix: nine arrays R[i][j]."""
    x, y, z, w = (q[..., k] for k in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def lu3_solve(W, t):
    """Eigen's PartialPivLU of 3 x 3 matrices (W[i][j] arrays) in the unblocked
    order, and the solve of W x = t (t[i] arrays)."""
    m = [[np.array(W[i][j], F64) for j in range(3)] for i in range(3)]
    c = [np.array(t[i], F64) for i in range(3)]

    def swap_rows(i, k, cond):
        for j in range(3):
            m[i][j], m[k][j] = np.where(cond, m[k][j], m[i][j]), np.where(cond, m[i][j], m[k][j])
        c[i], c[k] = np.where(cond, c[k], c[i]), np.where(cond, c[i], c[k])
    with np.errstate(all="ignore"):
        a0, a1, a2 = abs(m[0][0]), abs(m[1][0]), abs(m[2][0])
        p1 = a1 > a0
        big = np.where(p1, a1, a0)
        p2 = a2 > big
        big = np.where(p2, a2, big)
        swap_rows(0, 1, p1 & ~p2)
        swap_rows(0, 2, p2)
        nz = big != 0.0
        m[1][0] = np.where(nz, m[1][0] / m[0][0], m[1][0])
        m[2][0] = np.where(nz, m[2][0] / m[0][0], m[2][0])
        for i in (1, 2):
            for j in (1, 2):
                m[i][j] = m[i][j] - m[i][0] * m[0][j]
        p = abs(m[2][1]) > abs(m[1][1])
        big = np.where(p, abs(m[2][1]), abs(m[1][1]))
        swap_rows(1, 2, p)
        m[2][1] = np.where(big != 0.0, m[2][1] / m[1][1], m[2][1])
        m[2][2] = m[2][2] - m[2][1] * m[1][2]
        c1 = c[1] - m[1][0] * c[0]
        c2 = c[2] - (m[2][0] * c[0] + m[2][1] * c1)
        x2 = c2 / m[2][2]
        x1 = (c1 - m[1][2] * x2) / m[1][1]
        x0 = (c[0] - (m[0][1] * x1 + m[0][2] * x2)) / m[0][0]
    return np.stack([x0, x1, x2], -1)


def vlog(a):
    """Sim3::log of (n, 8): (n, 7) and the branch per row (bit 1: |sigma| >= eps,
    bit 0: d <= 1 - eps)."""
    a = np.asarray(a, F64)
    s = a[..., 7]
    with np.errstate(all="ignore"):
        sigma = np.asarray(MATH.log(s), F64)
        R = vqmat(a[..., :4])
        d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
        dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
        small_s, small_r = abs(sigma) < EPS, d > 1 - EPS
        theta = np.asarray(MATH.acos(np.where(small_r, 0.0, d)), F64)
        sn, cs = np.asarray(MATH.sin(theta), F64), np.asarray(MATH.cos(theta), F64)
        theta2, sigma2 = theta * theta, sigma * sigma
        f = np.where(small_r, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        om = [f * dR[k] for k in range(3)]
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        sa, sb = s * sn, s * cs
        c = theta2 + sigma * sigma
        A = np.where(small_s, np.where(small_r, 1. / 2., (1 - cs) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (sa * sigma + (1 - sb) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_r, 1. / 6., (theta - sn) / (theta2 * theta)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma),
                              (C - ((sb - 1) * sigma + sa * theta) / c) * 1. / theta2))
        z = np.zeros_like(s)
        O = [[z, -om[2], om[1]], [om[2], z, -om[0]], [-om[1], om[0], z]]
        W = [[A * O[i][j] + ((B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j] + (B * O[i][2]) * O[2][j])
              + C * (1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
        ups = lu3_solve(W, [a[..., 4], a[..., 5], a[..., 6]])
    branch = (~small_s).astype(np.int32) * 2 + (~small_r).astype(np.int32)
    return np.concatenate([np.stack(om, -1), ups, sigma[..., None]], -1), branch


def vexp(u, es=None):
    """Sim3(const Vector7d& update) (sim3.h:70-142) of (n, 7); es: exp(u[6])."""
    u = np.asarray(u, F64)
    o0, o1, o2 = u[..., 0], u[..., 1], u[..., 2]
    sigma = u[..., 6]
    with np.errstate(all="ignore"):
        theta = np.sqrt(o0 * o0 + o1 * o1 + o2 * o2)
        z = np.zeros_like(o0)
        Om = [[z, -o2, o1], [o2, z, -o0], [-o1, o0, z]]
        Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
        s = np.asarray(MATH.exp(sigma), F64) if es is None else np.broadcast_to(np.asarray(es, F64), sigma.shape)
        small_s, small_r = abs(sigma) < EPS, theta < EPS
        th = np.where(small_r, 1.0, theta)
        sn, cs = np.asarray(MATH.sin(th), F64), np.asarray(MATH.cos(th), F64)
        theta2, sigma2 = th * th, sigma * sigma
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a, b = s * sn, s * cs
        c = theta2 + sigma2
        A = np.where(small_s, np.where(small_r, 1. / 2., (1 - cs) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * th) / (th * c)))
        B = np.where(small_s, np.where(small_r, 1. / 6., (th - sn) / (theta2 * th)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma),
                              (C - ((b - 1) * sigma + a * th) / c) * 1. / theta2))
        ra, rb = np.where(small_r, 1.0, sn / th), np.where(small_r, 1.0, (1 - cs) / (th * th))
        eye = lambda i, j: 1.0 if i == j else 0.0
        # theta < eps: I + Omega + Omega2, with no factor at all
        R = [[np.where(small_r, eye(i, j) + Om[i][j] + Om2[i][j], eye(i, j) + ra * Om[i][j] + rb * Om2[i][j])
              for j in range(3)] for i in range(3)]
        W = [[A * Om[i][j] + B * Om2[i][j] + C * eye(i, j) for j in range(3)] for i in range(3)]
        t = [W[i][0] * u[..., 3] + W[i][1] * u[..., 4] + W[i][2] * u[..., 5] for i in range(3)]
    Rm = np.stack([np.stack(r, -1) for r in R], -2)
    q = np.array([matrix_quat(m) for m in Rm.reshape(-1, 3, 3)]).reshape(u.shape[:-1] + (4,))
    return np.concatenate([q, np.stack(t, -1), s[..., None]], -1)


def _perturbations():
    out = []
    for d in range(7):
        for sign, es in ((1.0, EXP_P), (-1.0, EXP_M)):
            u = np.zeros(7)
            u[d] = sign * DELTA
            out.append(vexp(u, es if d == 6 else 1.0))
    return np.array(out)


PERT = _perturbations()     # the 14 Sim3(+-delta e_d); free of the maths library


# --- the problem -------------------------------------------------------------------------
def plan(ids, fixed, edges):
    """The free vertices in id order and the envelope: free_index (n_kf),
    first (n_free), row_off, n_blocks, max_row_blocks."""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    e = np.asarray(edges, np.int64).reshape(-1, 3)
    used = np.zeros(n, bool)
    used[e[:, 0]] = used[e[:, 1]] = True
    free_index = np.full(n, -1, np.int32)
    k = 0
    for v in np.argsort(ids, kind="stable"):
        if v != fixed and used[v]:
            free_index[v] = k
            k += 1
    first = np.arange(k, dtype=np.int32)
    for i, j, _ in e:
        a, b = free_index[i], free_index[j]
        if a >= 0 and b >= 0:
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    rows = np.arange(k) - first + 1
    return dict(free_index=free_index, first=first, row_off=np.concatenate([[0], np.cumsum(rows)]).astype(np.int64),
                n_free=k, n_blocks=int(rows.sum()), max_row_blocks=int(rows.max()) if k else 0)


def setup(g):
    """vScw (n_kf, 8) and the measurements (n_edges, 8)."""
    n = len(g["ids"])
    vscw = np.array([g["corrected"][k] if k in g["corrected"] else sim3_from_float(g["Tcw"][k, :9], g["Tcw"][k, 9:], 1.0)
                     for k in range(n)], F64)
    side = np.array([g["noncorrected"].get(k, vscw[k]) for k in range(n)], F64)
    e = g["edges"]
    if len(e) == 0:
        return vscw, np.zeros((0, 8))
    normal = (e[:, 2] == 1)[:, None]
    si, sj = np.where(normal, side[e[:, 0]], vscw[e[:, 0]]), np.where(normal, side[e[:, 1]], vscw[e[:, 1]])
    return vscw, vmul(sj, vinv(si))


def edge_errors(meas, est_i, inv_j):
    return vlog(vmul(vmul(meas, est_i), inv_j))


def seq_dot(A, B, axis):
    """sum_k A_k B_k along `axis`, one product added at a time."""
    A, B = np.moveaxis(A, axis, 0), np.moveaxis(B, axis, 0)
    acc = A[0] * B[0]
    for k in range(1, len(A)):
        acc = acc + A[k] * B[k]
    return acc


def linearize(g, meas, est, pl):
    """computeActiveErrors + buildSystem at est: chi2, the dense H (7 n_free
    square) and b, the per-edge errors (m, 7), Jacobians (m, 2, 7, 7: Ji, Jj,
    row = error component) and branches."""
    e = g["edges"]
    I, J = e[:, 0], e[:, 1]
    fi, fj = pl["free_index"][I], pl["free_index"][J]
    P = np.concatenate([est[None], vmul(PERT[:, None, :], est[None])])       # (15, n_kf, 8)
    PI = vinv(P)
    err, branch = edge_errors(meas, P[0][I], PI[0][J])
    m = len(e)
    Jac = np.zeros((m, 2, 7, 7))
    with np.errstate(all="ignore"):
        for d in range(7):
            ep, _ = edge_errors(meas, P[1 + 2 * d][I], PI[0][J])
            em, _ = edge_errors(meas, P[2 + 2 * d][I], PI[0][J])
            Jac[:, 0, :, d] = np.where((fi >= 0)[:, None], SCALAR * (ep - em), 0.0)
            ep, _ = edge_errors(meas, P[0][I], PI[1 + 2 * d][J])
            em, _ = edge_errors(meas, P[0][I], PI[2 + 2 * d][J])
            Jac[:, 1, :, d] = np.where((fj >= 0)[:, None], SCALAR * (ep - em), 0.0)
        Ji, Jj = Jac[:, 0], Jac[:, 1]
        Hii = seq_dot(Ji[:, :, :, None], Ji[:, :, None, :], 1)        # (m, 7, 7): sum_k J[k, a] J[k, b]
        Hjj = seq_dot(Jj[:, :, :, None], Jj[:, :, None, :], 1)
        Hij = seq_dot(Ji[:, :, :, None], Jj[:, :, None, :], 1)
        bi = seq_dot(Ji, -err[:, :, None], 1)
        bj = seq_dot(Jj, -err[:, :, None], 1)
        chi_e = seq_dot(err, err, 1)
        nf = pl["n_free"]
        H, b = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf)
        chi = 0.0
        for k in range(m):
            chi = chi + chi_e[k]
            a, c = 7 * fi[k], 7 * fj[k]
            if a >= 0:
                H[a:a + 7, a:a + 7] += Hii[k]
                b[a:a + 7] += bi[k]
            if c >= 0:
                H[c:c + 7, c:c + 7] += Hjj[k]
                b[c:c + 7] += bj[k]
            if a >= 0 and c >= 0:
                H[a:a + 7, c:c + 7] += Hij[k]
                H[c:c + 7, a:a + 7] += Hij[k].T
    return float(chi), H, b, err, Jac, branch


def active_chi2(g, meas, est):
    e = g["edges"]
    err, _ = edge_errors(meas, est[e[:, 0]], vinv(est)[e[:, 1]])
    with np.errstate(all="ignore"):
        chi_e = seq_dot(err, err, 1)
        chi = 0.0
        for v in chi_e:
            chi = chi + v
    return float(chi)


def cholesky_solve(H, b):
    """(ok, x) of H x = b by a dense Cholesky, column by column; not ok when a
    pivot is not positive and finite."""
    n = len(b)
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            v = H[j, j] - L[j, :j] @ L[j, :j]
            if not (v > 0.0) or not np.isfinite(v):
                return False, np.zeros(n)
            L[j, j] = np.sqrt(v)
            L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        y = np.zeros(n)
        for j in range(n):
            y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
        x = np.zeros(n)
        for j in range(n - 1, -1, -1):
            x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return True, x


def oplus_all(est, dx, pl):
    """Sim3(dx) * estimate for every vertex of the system."""
    out = est.copy()
    fr = pl["free_index"]
    v = np.nonzero(fr >= 0)[0]
    if len(v):
        out[v] = vmul(vexp(dx.reshape(-1, 7)[fr[v]]), est[v])
    return out


def hdiag(H, nf):
    """The packed lower triangles of the diagonal blocks: (n_free, 28)."""
    return np.array([[H[7 * r + i, 7 * r + j] for i in range(7) for j in range(i + 1)] for r in range(nf)]).reshape(nf, 28)


def recover(est):
    """(:737-755) Tcw (n, 12) float and vCorrectedSwc."""
    out = np.zeros((len(est), 12), F32)
    for k, s in enumerate(est):
        out[k, :9] = quat_matrix(s[:4]).reshape(9).astype(F32)
        out[k, 9:] = (s[4:7] * (1. / s[7])).astype(F32)
    return out, vinv(est)


def correct_points(vscw, swc, pos, ref):
    """(:758-788) for the points with ref >= 0; the others keep their bytes."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    out = pos.copy()
    ok = np.nonzero(np.asarray(ref) >= 0)[0]
    if len(ok):
        r = np.asarray(ref)[ok]
        out[ok] = vmap(swc[r], vmap(vscw[r], pos[ok].astype(F64))).astype(F32)
    return out


def optimize(g):
    """The whole call: a dict of est, Tcw, pos, iterations, trials, not_posdef,
    chi2_first, chi2_last, lambda_last, the plan, vscw, meas and log (one
    record per LM iteration: est, chi2, H, b, err, J, branch, dx (the last
    trial's), lam, trials, gain)."""
    pl = plan(g["ids"], g["loop_kf"], g["edges"])
    vscw, meas = setup(g)
    est = vscw.copy()
    out = dict(plan=pl, vscw=vscw, meas=meas, log=[], iterations=0, trials=0, not_posdef=0, chi2_first=0.0,
               chi2_last=0.0, lambda_last=0.0)
    lam = ni = 0.0
    nbad = 0
    chi = 0.0
    for it in range(MAX_LM if pl["n_free"] else 0):
        chi, H, b, err, Jac, branch = linearize(g, meas, est, pl)
        rec = dict(est=est.copy(), chi2=chi, H=H, b=b, err=err, J=Jac, branch=branch)
        ini = chi
        if it == 0:
            lam, ni, nbad = LAMBDA_INIT, 2.0, 0
            out["chi2_first"] = chi
        k = 0
        while True:
            ok, dx = cholesky_solve(H + lam * np.eye(len(b)), b)
            if not ok:
                out["not_posdef"] += 1
            trial = oplus_all(est, dx, pl)
            tmp = active_chi2(g, meas, trial) if ok else np.finfo(F64).max
            scale = 0.0
            for j in range(len(b)):
                scale += dx[j] * (lam * dx[j] + b[j])
            scale += 1e-3
            with np.errstate(all="ignore"):
                rho = (chi - tmp) / scale
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                chi = tmp
                est = trial
            else:
                lam *= ni
                ni *= 2
            k += 1
            if not (rho < 0 and k < MAX_TRIALS):
                break
        rec.update(dx=dx, lam=lam, trials=k, gain=(ini - chi) / ini if ini > 0 else 0.0)
        out["log"].append(rec)
        out["iterations"] += 1
        out["trials"] += k
        if k == MAX_TRIALS or rho == 0:
            break
        nbad = nbad + 1 if (ini - chi) * 1e3 < ini else 0
        if nbad >= 3:
            break
    out["chi2_last"], out["lambda_last"] = chi, lam
    out["est"] = est
    out["Tcw"], swc = recover(est)
    out["pos"] = correct_points(vscw, swc, g["pos"], g["ref_kf"])
    return out


# --- scenes ------------------------------------------------------------------------------
def sim3_of(R, t, s=1.0):
    return np.concatenate([matrix_quat(np.asarray(R, F64)), np.asarray(t, F64), [float(s)]])


def se3_floats(S):
    """The keyframe pose a Sim3 stands for, [R t/s], as 12 floats."""
    return np.concatenate([quat_matrix(S[:4]).reshape(9), S[4:7] / S[7]]).astype(F32)


def graph(ids, Tcw, edges, loop_kf, cur_kf, corrected=None, noncorrected=None, pos=None, ref_kf=None):
    return dict(ids=np.asarray(ids, np.int64), Tcw=np.asarray(Tcw, F32).reshape(-1, 12),
                edges=np.asarray(edges, np.int64).reshape(-1, 3), loop_kf=int(loop_kf), cur_kf=int(cur_kf),
                corrected=dict(corrected or {}), noncorrected=dict(noncorrected or {}),
                pos=np.zeros((0, 3), F32) if pos is None else np.asarray(pos, F32).reshape(-1, 3),
                ref_kf=np.zeros(0, np.int32) if ref_kf is None else np.asarray(ref_kf, np.int32))


def circle(n, seed, loop=3, rot_drift=0.006, scale_drift=0.012, noise=0.002):
    """n keyframes on a circle that meets itself: the true poses, the drifted
    chain a monocular map would hold (every step off by a small Sim3, so scale
    and rotation drift accumulate), and what CorrectLoop has done before the
    call: the current keyframe (the last) and its two predecessors carry the
    loop-corrected Sim3, their old poses in NonCorrectedSim3 and the corrected
    SE3 as their pose.  Returns (Tcw, corrected, noncorrected, true)."""
    rng = np.random.RandomState(seed)
    true = []
    for k in range(n):
        a = 2 * np.pi * k / (n + 0.7)
        Rwc = _rot([0.0, a, 0.0]) @ _rot([0.02 * np.sin(3 * a), 0.0, 0.03 * np.cos(2 * a)])
        c = np.array([4 * np.cos(a), 0.2 * np.sin(2 * a), 4 * np.sin(a)])
        true.append(sim3_of(Rwc.T, -Rwc.T @ c))
    true = np.array(true)
    chain = [true[0]]
    for k in range(1, n):
        step = vmul(true[k], vinv(true[k - 1]))
        eps = vexp(np.concatenate([rng.normal(0, noise, 3) + rot_drift * np.array([0.3, 1.0, -0.2]),
                                   rng.normal(0, noise, 3), [scale_drift + rng.normal(0, noise)]]))
        chain.append(vmul(vmul(eps, step), chain[-1]))
    Tcw = np.array([se3_floats(s) for s in chain])
    old = [sim3_from_float(T[:9], T[9:], 1.0) for T in Tcw]
    cur = n - 1
    corrected, noncorrected = {}, {}
    Scw = vmul(vmul(true[cur], vinv(true[loop])), old[loop])          # g2oScw of ComputeSim3
    for k in (cur, cur - 1, cur - 2):
        corrected[k] = Scw if k == cur else vmul(vmul(old[k], vinv(old[cur])), Scw)
        noncorrected[k] = old[k]
        Tcw[k] = se3_floats(corrected[k])
    return Tcw, corrected, noncorrected, true


def _loop_case(n, ids, order, seed, loop=3):
    """A loop of n keyframes with the given ids, passed in `order`."""
    Tcw, cor, non, _ = circle(n, seed, loop)
    cur = n - 1
    edges = [(cur, loop, 0), (cur, loop + 1, 0), (cur - 1, loop, 0)]          # LoopConnections
    for k in range(1, n):
        edges.append((k, k - 1, 1))                                           # the spanning tree
        if k >= 2 and k % 3 != 1:
            edges.append((k, k - 2, 1))                                       # covisibility
    at = {k: p for p, k in enumerate(order)}                                  # scene index -> array index
    edges = [(at[i], at[j], kind) for i, j, kind in edges]
    return graph([ids[k] for k in order], Tcw[order], edges, at[loop], at[cur],
                 {at[k]: v for k, v in cor.items()}, {at[k]: v for k, v in non.items()})


def _dyadic(n):
    """Poses whose whole arithmetic is exact: R = I, dyadic translations."""
    return np.array([np.concatenate([np.eye(3).reshape(9), [0.5 * k, 0.25 * k, -0.125 * k]]) for k in range(n)], F32)


def _pair():
    T = _dyadic(2)
    non = {1: vmul(vexp(np.array([0.01, -0.02, 0.015, 0.05, -0.03, 0.02, 0.03])), sim3_from_float(T[1, :9], T[1, 9:], 1.0))}
    return graph([0, 1], T, [(1, 0, 1)], 0, 1, noncorrected=non)


def _chain5():
    return graph(range(5), _dyadic(5), [(k, k - 1, 1) for k in range(1, 5)], 0, 4)


def _branches():
    """Vertex 0 fixed, four edges onto it whose first errors take log's four
    branches: the identity, a scale-only, a rotation-only (about 40 degrees)
    and a combined difference."""
    T = _dyadic(5)
    base = [sim3_from_float(t[:9], t[9:], 1.0) for t in T]
    non = {2: np.concatenate([base[2][:7], [1.25]]),
           3: vmul(sim3_of(_rot([0.3, -0.5, 0.35]), [0, 0, 0]), base[3]),
           4: vmul(sim3_of(_rot([-0.2, 0.4, 0.1]), [0.1, 0, -0.1], 0.9), base[4])}
    return graph(range(5), T, [(k, 0, 1) for k in range(1, 5)], 0, 4, noncorrected=non)


def _band40():
    n, loop = 40, 2
    Tcw, cor, non, _ = circle(n, 41, loop, rot_drift=0.002, scale_drift=0.004, noise=0.001)
    cur = n - 1
    edges = [(cur, loop, 0), (cur - 1, loop, 0), (cur, loop + 1, 0)]
    for k in range(1, n):
        edges.append((k, k - 1, 1))
        if k == 25:
            edges.append((25, 8, 1))      # an old loop edge
        if k == 30:
            edges.append((30, 12, 1))
        for d in (2, 3):
            if k >= d:
                edges.append((k, k - d, 1))
    return graph(range(n), Tcw, edges, loop, cur, cor, non)


def _hub130():
    n, loop, hub = 129, 5, 10
    Tcw, cor, non, _ = circle(n, 130, loop, rot_drift=0.0006, scale_drift=0.0012, noise=0.0004)
    cur = n - 1
    edges = [(cur, loop, 0), (cur - 1, loop, 0)]
    for k in range(1, n):
        edges.append((k, k - 1, 1))
        if k >= 2:
            edges.append((k, k - 2, 1))
        if 20 <= k < 90:
            edges.append((k, hub, 1))      # one keyframe of degree above 64
        if 60 <= k < 122:
            edges.append((k, k - 3, 1))
    lone = se3_floats(sim3_of(_rot([0.1, 0.2, -0.1]), [0.3, -0.2, 1.5]))      # a keyframe without an edge
    return graph(list(range(n)) + [500], np.concatenate([Tcw, lone[None]]), edges, loop, cur, cor, non)


def _floating():
    """loop12 and a two-keyframe component joined to nothing fixed; its one
    edge is consistent in exact arithmetic."""
    g = _loop_case(12, list(range(12)), list(range(12)), 12)
    T = _dyadic(3)[1:]
    return graph(list(g["ids"]) + [100, 101], np.concatenate([g["Tcw"], T]), list(map(tuple, g["edges"])) + [(13, 12, 1)],
                 g["loop_kf"], g["cur_kf"], g["corrected"], g["noncorrected"])


def _points(g, n=300, seed=7):
    rng = np.random.RandomState(seed)
    g = dict(g)
    g["pos"] = rng.uniform(-5, 5, (n, 3)).astype(F32)
    ref = rng.randint(0, len(g["ids"]), n).astype(np.int32)
    ref[:6] = [g["cur_kf"], g["cur_kf"] - 1, g["loop_kf"], 0, 1, g["loop_kf"]]
    ref[rng.choice(np.arange(6, n), 25, replace=False)] = -1
    g["ref_kf"] = ref
    return g


GAP_IDS = [0, 2, 3, 7, 8, 11, 12, 13, 20, 21, 25, 31, 40]
CASES = {
    "pair": _pair,
    "chain5_consistent": _chain5,
    "loop12": lambda: _loop_case(12, list(range(12)), list(range(12)), 12),
    "loop13_gap": lambda: _loop_case(13, GAP_IDS, [5, 0, 12, 3, 9, 1, 7, 11, 2, 4, 10, 6, 8], 13),
    "branches": _branches,
    "band40_fill": _band40,
    "hub130": _hub130,
    "floating": _floating,
    "points": lambda: _points(_loop_case(12, list(range(12)), list(range(12)), 12)),
}
_case_cache = {}


def case(name):
    """(the graph, the restatement's result) of a case, computed once and shared."""
    if name not in _case_cache:
        g = CASES[name]()
        _case_cache[name] = (g, optimize(g))
    return _case_cache[name]


# --- what two conforming maths libraries may differ by -----------------------------------
QUANTITIES = ("err", "J", "chi2", "b", "Hdiag", "dx", "est", "chi2_last")
# The worst relative difference |a - b| / max(1, |a|) seen over every case (but
# `floating`, whose outcome is not defined) between the run as is and five runs
# with acos / sin / cos / log / exp moved by -1, 0 or +1 ulp at random
# (measure()), the first iteration for the per-iteration quantities.  The bar
# of each comparison is this value x 8: the device may also differ in the
# factorisation's summation order, which the perturbation does not exercise.
MEASURED = dict(err=1.2e-15, J=1.2e-6, chi2=4.3e-16, b=3.5e-7, Hdiag=4.6e-6, dx=7.3e-7, est=5.7e-7, chi2_last=4.3e-9)
FACTOR = 8.0
TOL = {k: FACTOR * v for k, v in MEASURED.items()}


def rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a))))


def align(est, ref):
    """est with each quaternion's sign that of ref's."""
    sgn = np.where(np.sum(est[..., :4] * ref[..., :4], -1, keepdims=True) < 0, -1.0, 1.0)
    return np.concatenate([est[..., :4] * sgn, est[..., 4:]], -1)


def differences(r, p):
    """The compared quantities of a run p against the run r."""
    a, b = r["log"], p["log"]
    d = dict.fromkeys(QUANTITIES, 0.0)
    if a and b:
        nf = r["plan"]["n_free"]
        d.update(err=rel(a[0]["err"], b[0]["err"]), J=rel(a[0]["J"], b[0]["J"]), chi2=rel(a[0]["chi2"], b[0]["chi2"]),
                 b=rel(a[0]["b"], b[0]["b"]), Hdiag=rel(hdiag(a[0]["H"], nf), hdiag(b[0]["H"], nf)),
                 dx=rel(a[0]["dx"], b[0]["dx"]) if a[0]["trials"] == b[0]["trials"] else 0.0)
    d["est"] = rel(r["est"], align(p["est"], r["est"]))
    d["chi2_last"] = rel(r["chi2_last"], p["chi2_last"])
    return d


def measure(names=None, runs=5, seed=2024):
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for name in names or [n for n in CASES if n != "floating"]:
        g, r = case(name)
        for k in range(runs):
            set_math(Ulp(seed + 100 * k + len(name)))
            try:
                p = optimize(g)
            finally:
                set_math(Exact)
            for q, v in differences(r, p).items():
                worst[q] = max(worst[q], v)
    return worst


GOLDEN = ("loop12", "loop13_gap", "band40_fill", "hub130")


def golden_record(name):
    g, r = case(name)
    cor, non = sorted(g["corrected"]), sorted(g["noncorrected"])
    return dict(ids=g["ids"], Tcw=g["Tcw"], edges=g["edges"], loop_kf=np.int32(g["loop_kf"]), cur_kf=np.int32(g["cur_kf"]),
                corrected_kf=np.array(cor, np.int32), corrected=np.array([g["corrected"][k] for k in cor]),
                noncorrected_kf=np.array(non, np.int32), noncorrected=np.array([g["noncorrected"][k] for k in non]),
                est=r["est"], Tcw_out=r["Tcw"], iterations=np.int32(r["iterations"]),
                trials=np.array([x["trials"] for x in r["log"]], np.int32),
                chi2=np.array([x["chi2"] for x in r["log"]]), gain=np.array([x["gain"] for x in r["log"]]),
                chi2_last=r["chi2_last"])


def write_golden(folder):
    """tests/golden/essgraph_<case>.npz: the inputs and the restatement's outputs."""
    for name in GOLDEN:
        np.savez_compressed(folder / f"essgraph_{name}.npz", **golden_record(name))


if __name__ == "__main__":       # with the repository root on PYTHONPATH: the goldens, or `measure`
    import sys
    from pathlib import Path
    if "measure" in sys.argv:
        print(measure())
    else:
        write_golden(Path(__file__).resolve().parent / "golden")
