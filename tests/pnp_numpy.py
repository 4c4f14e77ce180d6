"""A sequential restatement of PnPsolver (src/PnPsolver.cc): the constructor,
SetRansacParameters, iterate as a plain loop with Refine called where the
reference calls it, CheckInliers and EPnP, in float64 / float32 scalars and
element-wise numpy in the defined order.

Every decomposition (the five places the reference goes through OpenCV) is
taken from a `decomp` object: NumpyDecomp (np.linalg in float64) or TapDecomp
(the device's own results, which is how the GPU tests compare byte for byte
without depending on a basis of a null space).
"""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
NAN = float("nan")
DEC = 135          # doubles of decomposition taps per hypothesis
REC = 232          # doubles of one hypothesis record
O_L, O_RHO, O_BETAS, O_R, O_T, O_ERR, O_CHOSEN, O_NPTS = 135, 195, 201, 213, 222, 225, 228, 229


# ---------------------------------------------------------------------------
# constructor and SetRansacParameters
# ---------------------------------------------------------------------------
def construct(keys, pos, valid, sigma2, th2=5.991):
    """(:39-82, :126-128): the correspondences compacted in i order."""
    valid = np.asarray(valid)
    kp = np.flatnonzero(valid != 0).astype(np.int32)
    p2d = np.stack([keys["x"][kp], keys["y"][kp]], 1).astype(np.float32).reshape(-1, 2)
    p3d = np.asarray(pos, np.float32).reshape(-1, 3)[kp]
    s2 = np.asarray(sigma2, np.float32)[keys["octave"][kp]]
    return dict(N=len(kp), kp_index=kp, p2d=p2d, p3d=p3d, max_err=(s2 * f32(th2)).astype(np.float32))


def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """(:93-124) -> (mRansacMinInliers, mRansacMaxIts); the latter 0 when
    N < mRansacMinInliers (no iteration runs; the reference's value there
    comes from a NaN or a negative logarithm)."""
    nmin = int(f32(N) * f32(epsilon))
    nmin = max(nmin, min_inliers, min_set)
    if N < nmin:
        return nmin, 0
    eps = f32(epsilon)
    r = f32(nmin) / f32(N)
    if eps < r:
        eps = r
    if nmin == N:
        nit = 1
    else:
        v = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
        nit = 2147483647 if not v < 2147483647.0 else (1 if v < 1 else int(v))
    return nmin, max(1, min(nit, max_iterations))


def draw_set(N, r4):
    """(:160-173): four picks; the removal writes at the drawn *value*."""
    avail = list(range(N))
    out = []
    for j in range(4):
        size = len(avail)
        randi = int((float(r4[j]) / 2147483648.0) * size)
        idx = avail[randi]
        out.append(idx)
        back = avail[-1]
        if idx < size:
            avail[idx] = back
        avail.pop()          # idx >= size wrote past the live part: never read again
    return out


# ---------------------------------------------------------------------------
# decompositions
# ---------------------------------------------------------------------------
class NumpyDecomp:
    """The five OpenCV places from np.linalg in float64."""

    def begin(self, key):
        pass

    def eig_sym(self, A, which):
        w, v = np.linalg.eigh(np.asarray(A, np.float64))
        order = np.argsort(-np.abs(w), kind="stable")
        return np.abs(w)[order], v.T[order].copy()

    def pinv3(self, cc):
        u, w, vt = np.linalg.svd(np.asarray(cc, np.float64))
        cut = 2 * np.finfo(np.float64).eps * w.sum()
        wi = np.array([1.0 / x if x > cut else 0.0 for x in w])
        return (vt.T * wi) @ u.T

    def solve(self, A, b, which):
        A = np.asarray(A, np.float64)
        u, w, vt = np.linalg.svd(A, full_matrices=False)
        cut = 2 * np.finfo(np.float64).eps * w.sum()
        wi = np.array([1.0 / x if x > cut else 0.0 for x in w])
        return (vt.T * wi) @ (u.T @ np.asarray(b, np.float64))

    def svd3(self, A, which):
        u, w, vt = np.linalg.svd(np.asarray(A, np.float64))
        return u, vt.T.copy()


class TapDecomp:
    """The device's decompositions: dec[key] is one DEC-double record."""

    def __init__(self, records):
        self.records = records
        self.d = None

    def begin(self, key):
        self.d = np.asarray(self.records[key], np.float64)

    def eig_sym(self, A, which):
        if which == 3:
            return self.d[0:3].copy(), self.d[3:12].reshape(3, 3).copy()
        ut = np.full((12, 12), NAN)          # only rows 8..11 are ever read
        ut[8:12] = self.d[21:69].reshape(4, 12)
        return np.full(12, NAN), ut

    def pinv3(self, cc):
        return self.d[12:21].reshape(3, 3).copy()

    def solve(self, A, b, which):
        o, k = {1: (69, 4), 2: (73, 3), 3: (76, 5)}[which]
        return self.d[o:o + k].copy()

    def svd3(self, A, which):
        o = 81 + 18 * (which - 1)
        return self.d[o:o + 9].reshape(3, 3).copy(), self.d[o + 9:o + 18].reshape(3, 3).copy()


# ---------------------------------------------------------------------------
# EPnP (:347-922), FP64, no contraction
# ---------------------------------------------------------------------------
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


def qr_solve(A, b, x, nr=6, nc=4):
    """(:832-922) on lists A (nr*nc, row-major), b (nr); x is left as it was
    by the early return on a zero column."""
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        kk = k * nc + k
        eta = abs(A[kk])
        for i in range(k + 1, nr):     # the reference's walk starts at row k again
            elt = abs(A[kk + (i - k - 1) * nc])
            if eta < elt:
                eta = elt
        if eta == 0:
            return
        inv_eta = 1.0 / eta
        s = 0.0
        for i in range(k, nr):
            A[i * nc + k] *= inv_eta
            s += A[i * nc + k] * A[i * nc + k]
        sigma = math.sqrt(s) if s >= 0 else NAN
        if A[kk] < 0:
            sigma = -sigma
        A[kk] += sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i * nc + k] * A[i * nc + j]
            tau = _div(s, A1[k])
            for i in range(k, nr):
                A[i * nc + j] -= tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i * nc + j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i * nc + j]
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i * nc + j] * x[j]
        x[i] = _div(b[i] - s, A2[i])


def _div(a, b):
    """IEEE division of Python floats."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def compute_pose(pws, us, cam, decomp, log=None):
    """compute_pose (:449-497) over n correspondences (pws n x 3, us n x 2,
    float64; cam fu, fv, uc, vc as the reference names them) -> a REC-double
    record.  n == 0 gives NaNs.  log, a dict, receives the matrices that were
    decomposed."""
    rec = np.full(REC, NAN)
    rec[O_NPTS:] = 0.0
    n = len(pws)
    rec[O_NPTS] = n
    rec[O_CHOSEN] = 0
    if n == 0:
        return rec
    fu, fv, uc, vc = (float(c) for c in cam)
    pws = np.asarray(pws, np.float64)
    us = np.asarray(us, np.float64)
    with np.errstate(all="ignore"):
        # choose_control_points
        c0 = [0.0, 0.0, 0.0]
        for i in range(n):
            for j in range(3):
                c0[j] += pws[i, j]
        for j in range(3):
            c0[j] = _div(c0[j], float(n))
        pw0 = pws - np.array(c0)
        G3 = np.zeros((3, 3))
        for i in range(n):                       # (a): rows in order
            G3 = G3 + np.outer(pw0[i], pw0[i])
        dc, uct = decomp.eig_sym(G3, 3)
        rec[0:3], rec[3:12] = dc, np.asarray(uct).reshape(-1)
        cws = [list(c0)]
        for i in range(1, 4):
            k = _sqrt(_div(dc[i - 1], float(n)))
            cws.append([c0[j] + k * uct[i - 1, j] for j in range(3)])
        # compute_barycentric_coordinates
        cc = np.array([[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)])
        ci = np.asarray(decomp.pinv3(cc), np.float64)
        rec[12:21] = ci.reshape(-1)
        d = pws - np.array(cws[0])
        al = np.zeros((n, 4))
        for j in range(3):
            al[:, 1 + j] = (ci[j, 0] * d[:, 0] + ci[j, 1] * d[:, 1]) + ci[j, 2] * d[:, 2]
        al[:, 0] = ((1.0 - al[:, 1]) - al[:, 2]) - al[:, 3]
        # fill_M and MtM: rows in order, the zero entries multiplied like the rest
        M = np.zeros((2 * n, 12))
        for j in range(4):
            M[0::2, 3 * j] = al[:, j] * fu
            M[0::2, 3 * j + 2] = al[:, j] * (uc - us[:, 0])
            M[1::2, 3 * j + 1] = al[:, j] * fv
            M[1::2, 3 * j + 2] = al[:, j] * (vc - us[:, 1])
        G = np.zeros((12, 12))
        for r in range(2 * n):
            G = G + np.outer(M[r], M[r])
        _, ut = decomp.eig_sym(G, 12)
        rec[21:69] = np.asarray(ut)[8:12].reshape(-1)
        v = [ut[11], ut[10], ut[9], ut[8]]
        # compute_L_6x10, compute_rho
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = [[[v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)] for (a, b) in pairs] for i in range(4)]
        L = np.zeros((6, 10))
        for i in range(6):
            L[i] = [_dot3(dv[0][i], dv[0][i]), 2.0 * _dot3(dv[0][i], dv[1][i]), _dot3(dv[1][i], dv[1][i]),
                    2.0 * _dot3(dv[0][i], dv[2][i]), 2.0 * _dot3(dv[1][i], dv[2][i]), _dot3(dv[2][i], dv[2][i]),
                    2.0 * _dot3(dv[0][i], dv[3][i]), 2.0 * _dot3(dv[1][i], dv[3][i]), 2.0 * _dot3(dv[2][i], dv[3][i]),
                    _dot3(dv[3][i], dv[3][i])]
        rho = [_dist2(cws[a], cws[b]) for (a, b) in pairs]
        rec[O_L:O_L + 60] = L.reshape(-1)
        rec[O_RHO:O_RHO + 6] = rho
        if log is not None:
            log.update(G3=G3, cc=cc, MtM=G, L=L.copy(), rho=np.array(rho), abt=[])
        Rs, ts, errs = [], [], []
        cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}
        for which in (1, 2, 3):
            b = decomp.solve(L[:, cols[which]], np.array(rho), which)
            rec[{1: 69, 2: 73, 3: 76}[which]:][:len(b)] = b
            b = [float(x) for x in b]
            be = [0.0] * 4
            if which == 1:
                if b[0] < 0:
                    be[0] = _sqrt(-b[0])
                    be[1], be[2], be[3] = _div(-b[1], be[0]), _div(-b[2], be[0]), _div(-b[3], be[0])
                else:
                    be[0] = _sqrt(b[0])
                    be[1], be[2], be[3] = _div(b[1], be[0]), _div(b[2], be[0]), _div(b[3], be[0])
            else:
                if b[0] < 0:
                    be[0] = _sqrt(-b[0])
                    be[1] = _sqrt(-b[2]) if b[2] < 0 else 0.0
                else:
                    be[0] = _sqrt(b[0])
                    be[1] = _sqrt(b[2]) if b[2] > 0 else 0.0
                if b[1] < 0:
                    be[0] = -be[0]
                if which == 3:
                    be[2] = _div(b[3], be[0])
            # gauss_newton (:812-830); x starts at zero
            x = [0.0] * 4
            for _ in range(5):
                A, bb = [0.0] * 24, [0.0] * 6
                for i in range(6):
                    r = L[i]
                    A[4 * i] = 2 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3]
                    A[4 * i + 1] = r[1] * be[0] + 2 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3]
                    A[4 * i + 2] = r[3] * be[0] + r[4] * be[1] + 2 * r[5] * be[2] + r[8] * be[3]
                    A[4 * i + 3] = r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2 * r[9] * be[3]
                    bb[i] = rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] +
                                      r[3] * be[0] * be[2] + r[4] * be[1] * be[2] + r[5] * be[2] * be[2] +
                                      r[6] * be[0] * be[3] + r[7] * be[1] * be[3] + r[8] * be[2] * be[3] +
                                      r[9] * be[3] * be[3])
                A = [float(a) for a in A]
                bb = [float(a) for a in bb]
                qr_solve(A, bb, x)
                for i in range(4):
                    be[i] += x[i]
            rec[O_BETAS + 4 * (which - 1):][:4] = be
            # compute_ccs, compute_pcs, solve_for_sign
            ccs = np.zeros((4, 3))
            for i in range(4):
                ccs = ccs + be[i] * np.asarray(v[i], np.float64).reshape(4, 3)
            pcs = np.zeros((n, 3))
            for j in range(3):
                pcs[:, j] = ((al[:, 0] * ccs[0, j] + al[:, 1] * ccs[1, j]) + al[:, 2] * ccs[2, j]) + al[:, 3] * ccs[3, j]
            if pcs[0, 2] < 0.0:
                ccs, pcs = -ccs, -pcs
            # estimate_R_and_t
            pc0, pw00 = [0.0] * 3, [0.0] * 3
            for i in range(n):
                for j in range(3):
                    pc0[j] += pcs[i, j]
                    pw00[j] += pws[i, j]
            for j in range(3):
                pc0[j] = _div(pc0[j], float(n))
                pw00[j] = _div(pw00[j], float(n))
            dc_, dw_ = pcs - np.array(pc0), pws - np.array(pw00)
            abt = np.zeros((3, 3))
            for i in range(n):
                abt = abt + np.outer(dc_[i], dw_[i])
            if log is not None:
                log["abt"].append(abt)
            U, V = decomp.svd3(abt, which)
            rec[81 + 18 * (which - 1):][:18] = np.concatenate([np.asarray(U).reshape(-1), np.asarray(V).reshape(-1)])
            R = [[_dot3(U[i], V[j]) for j in range(3)] for i in range(3)]
            det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                   R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
            if det < 0:
                R[2] = [-R[2][0], -R[2][1], -R[2][2]]
            t = [pc0[i] - _dot3(R[i], pw00) for i in range(3)]
            # reprojection_error
            Xc = ((R[0][0] * pws[:, 0] + R[0][1] * pws[:, 1]) + R[0][2] * pws[:, 2]) + t[0]
            Yc = ((R[1][0] * pws[:, 0] + R[1][1] * pws[:, 1]) + R[1][2] * pws[:, 2]) + t[1]
            iz = 1.0 / (((R[2][0] * pws[:, 0] + R[2][1] * pws[:, 1]) + R[2][2] * pws[:, 2]) + t[2])
            ue = uc + fu * Xc * iz
            ve = vc + fv * Yc * iz
            e = np.sqrt((us[:, 0] - ue) * (us[:, 0] - ue) + (us[:, 1] - ve) * (us[:, 1] - ve))
            s = 0.0
            for i in range(n):
                s += e[i]
            Rs.append(R)
            ts.append(t)
            errs.append(_div(s, float(n)))
        pick = 1
        if errs[1] < errs[0]:
            pick = 2
        if errs[2] < errs[pick - 1]:
            pick = 3
        rec[O_R:O_R + 9] = np.array(Rs[pick - 1]).reshape(-1)
        rec[O_T:O_T + 3] = ts[pick - 1]
        rec[O_ERR:O_ERR + 3] = errs
        rec[O_CHOSEN] = pick
    return rec


# ---------------------------------------------------------------------------
# CheckInliers (:280-311)
# ---------------------------------------------------------------------------
def _fma(a, b, c):
    """Correctly rounded a*b+c of float64 values."""
    a, b, c = float(a), float(b), float(c)
    p = a * b + c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)) or not math.isfinite(p):
        return p
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return p          # the sign of an exact zero is that of the unfused sum
    return float(r)


def _fmaf(a, b, c):
    """Correctly rounded float32 a*b+c of float32 values."""
    a, b, c = float(a), float(b), float(c)
    p = a * b + c
    if not math.isfinite(p) or p == 0:
        return f32(p)
    r = Fraction(a) * Fraction(b) + Fraction(c)
    f = f32(float(r))
    if not np.isfinite(f):
        return f
    best = None
    for cand in (f, np.nextafter(f, f32(-np.inf)), np.nextafter(f, f32(np.inf))):
        if not np.isfinite(cand):
            continue
        key = (abs(Fraction(float(cand)) - r), int(cand.view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, cand)
    return best[1]


def check_inliers(c, cam, R, t, contract=False):
    """-> (count, mask) of the pose R (9), t (3), float64.  Under contract
    the sums of products are fused left to right: fma(c, z, fma(b, y, a*x)) +
    t, fma(fu*Xc, invZc, uc), fmaf(dx, dx, dy*dy)."""
    fu, fv, uc, vc = (float(x) for x in cam)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    P = c["p3d"].astype(np.float64)
    u, v = c["p2d"][:, 0].astype(np.float64), c["p2d"][:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        if not contract:
            row = [((R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1]) + R[i, 2] * P[:, 2]) + t[i] for i in range(3)]
            Xc, Yc = row[0].astype(np.float32), row[1].astype(np.float32)
            iz = (1.0 / row[2]).astype(np.float32)
            ue = uc + fu * Xc.astype(np.float64) * iz.astype(np.float64)
            ve = vc + fv * Yc.astype(np.float64) * iz.astype(np.float64)
            dx, dy = (u - ue).astype(np.float32), (v - ve).astype(np.float32)
            e2 = dx * dx + dy * dy
        else:
            e2 = np.zeros(len(P), np.float32)
            for k in range(len(P)):
                row = [_fma(R[i, 2], P[k, 2], _fma(R[i, 1], P[k, 1], R[i, 0] * P[k, 0])) + t[i] for i in range(3)]
                Xc, Yc, iz = f32(row[0]), f32(row[1]), f32(_div(1.0, row[2]))
                ue = _fma(fu * float(Xc), float(iz), uc)
                ve = _fma(fv * float(Yc), float(iz), vc)
                dx, dy = f32(u[k] - ue), f32(v[k] - ve)
                e2[k] = _fmaf(dx, dx, dy * dy)
        mask = e2 < c["max_err"]
    return int(mask.sum()), mask


def tcw32(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3).astype(np.float32)
    T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T.reshape(-1)


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
class PnPSolver:
    """PnPsolver with its iterate state.  iterate(n_iter, draws) consumes
    four rand() values per iteration from draws (k x 4) and returns the
    call's outputs as a dict; the state lives on in the object."""

    def __init__(self, keys, pos, valid, cam, sigma2, decomp=None, contract=False, **params):
        self.n = len(keys)
        self.cam = np.asarray(cam, np.float32)
        self.epnp_cam = (self.cam[0], self.cam[1], self.cam[2], self.cam[3])
        self.sigma2 = sigma2
        self.keys, self.pos, self.valid = keys, pos, valid
        self.decomp = decomp or NumpyDecomp()
        self.contract = contract
        self.iter_done, self.best_inliers = 0, 0
        self.best_mask = np.zeros(self.n, np.uint8)
        self.best_Tcw = np.zeros(16, np.float32)
        self.slot = 0              # which refit the best state is: 0 incoming, k the k-th record holder of the call
        self.log = None
        self.set_ransac_parameters(**params)

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4,
                              th2=5.991):
        self.c = construct(self.keys, self.pos, self.valid, self.sigma2, th2)
        self.N = self.c["N"]
        self.min_inliers, self.max_its = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set,
                                                           epsilon)

    def set_state(self, iter_done, best_inliers, best_mask, best_Tcw):
        self.iter_done, self.best_inliers = int(iter_done), int(best_inliers)
        self.best_mask = np.array(best_mask, np.uint8)
        self.best_Tcw = np.array(best_Tcw, np.float32).reshape(-1)

    def _pose(self, idx, key):
        self.decomp.begin(key)
        log = None
        if self.log is not None:
            log = {}
            self.log[key] = log
        rec = compute_pose(self.c["p3d"][idx].astype(np.float64), self.c["p2d"][idx].astype(np.float64),
                           (self.cam[0], self.cam[1], self.cam[2], self.cam[3]), self.decomp, log)
        return rec

    def refine(self):
        """(:232-277) -> (ok, count, mask, record)."""
        m = self.best_mask[self.c["kp_index"]] != 0
        rec = self._pose(np.flatnonzero(m), ("refit", self.slot))
        count, mask = check_inliers(self.c, self.cam, rec[O_R:O_R + 9], rec[O_T:O_T + 3], self.contract)
        return count > self.min_inliers, count, mask, rec

    def iterate(self, n_iter, draws):
        draws = np.asarray(draws, np.int64).reshape(-1, 4)
        out = dict(N=self.N, ransac_min_inliers=self.min_inliers, ransac_max_its=self.max_its, iters_run=0, no_more=0,
                   found=0, found_iter=-1, n_inliers=0, refined=0, Tcw=None, inliers=np.zeros(self.n, np.uint8))
        taps = dict(sets=[], rec=[], count=[], refits={})
        self.taps = taps
        self.slot = 0
        if self.N < self.min_inliers:
            out["no_more"] = 1
            return self._finish(out)
        cur = 0
        while self.iter_done < self.max_its or cur < n_iter:
            s = draw_set(self.N, draws[cur])
            it = cur
            cur += 1
            self.iter_done += 1
            rec = self._pose(np.array(s), ("it", it))
            count, mask = check_inliers(self.c, self.cam, rec[O_R:O_R + 9], rec[O_T:O_T + 3], self.contract)
            taps["sets"].append(s)
            taps["rec"].append(rec)
            taps["count"].append(count)
            if count >= self.min_inliers:
                if count > self.best_inliers:
                    self.best_mask = np.zeros(self.n, np.uint8)
                    self.best_mask[self.c["kp_index"][mask]] = 1
                    self.best_inliers = count
                    self.best_Tcw = tcw32(rec[O_R:O_R + 9], rec[O_T:O_T + 3])
                    self.slot += 1
                ok, rcount, rmask, rrec = self.refine()
                taps["refits"][self.slot] = (rrec, rcount)
                if ok:
                    out.update(found=1, found_iter=it, n_inliers=rcount, refined=1,
                               Tcw=tcw32(rrec[O_R:O_R + 9], rrec[O_T:O_T + 3]))
                    out["inliers"][self.c["kp_index"][rmask]] = 1
                    out["iters_run"] = cur
                    return self._finish(out)
        out["iters_run"] = cur
        if self.iter_done >= self.max_its:
            out["no_more"] = 1
            if self.best_inliers >= self.min_inliers:
                out.update(found=1, n_inliers=self.best_inliers, Tcw=self.best_Tcw.copy(),
                           inliers=self.best_mask.copy())
        return self._finish(out)

    def _finish(self, out):
        out.update(iter_done=self.iter_done, best_inliers=self.best_inliers, best_mask=self.best_mask.copy(),
                   best_Tcw=self.best_Tcw.copy(), best_slot=self.slot)
        return out


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAM = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2


def pose_gt(seed):
    rng = np.random.default_rng(1000 + seed)
    w = rng.normal(size=3) * 0.15
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    return R, rng.normal(size=3) * 0.3


def scene(N, seed=0, noise=0.3, outliers=0.2, extra=7):
    """N correspondences among N + extra keypoints (the extra ones without a
    map point): ground-truth projections with pixel noise, a fraction
    `outliers` of them paired with an unrelated point."""
    rng = np.random.default_rng(seed)
    n = N + extra
    R, t = pose_gt(seed)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], 1)
    Xw = (Xc - t) @ R            # R^T (Xc - t)
    uv = np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)
    uv = uv + rng.normal(size=uv.shape) * noise
    keys = np.zeros(n, KEYPOINT)
    keys["x"], keys["y"] = uv[:, 0], uv[:, 1]
    keys["octave"] = rng.integers(0, 8, n)
    valid = np.ones(n, np.uint8)
    valid[rng.choice(n, extra, replace=False)] = 0
    pos = Xw.astype(np.float32)
    good = np.flatnonzero(valid)
    bad = rng.choice(good, int(round(outliers * N)), replace=False)
    pos[bad] = pos[rng.permutation(bad)] + rng.normal(size=(len(bad), 3)).astype(np.float32)
    return dict(keys=keys, pos=pos, valid=valid, cam=CAM.copy(), sigma2=SIGMA2.copy(), R=R, t=t, bad=bad)


def draws_for(seed, k):
    return np.random.default_rng(77 + seed).integers(0, 2 ** 31, size=(k, 4), dtype=np.int64).astype(np.int32)


def frame_of(sc):
    return {k: sc[k] for k in ("keys", "pos", "valid", "cam", "sigma2")}


# Relocalisation's parameters (Tracking.cc:923)
RELOC = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)
# N x total iterations: n_iter = max_iterations = the total (the loop's or runs to the larger)
CASES = [(N, T) for N in (9, 10, 11, 63, 64, 65, 300) for T in (1, 5, 35, 64, 65, 300)]


def case(i):
    """-> (scene, draws, params) of CASES[i]."""
    N, T = CASES[i]
    sc = scene(N, seed=100 + i, noise=0.5)
    return sc, draws_for(i, T), dict(RELOC, max_iterations=T, n_iter=T)


def solver_of(sc, params, decomp=None, contract=False, state=None):
    p = {k: v for k, v in params.items() if k != "n_iter"}
    s = PnPSolver(sc["keys"], sc["pos"], sc["valid"], sc["cam"], sc["sigma2"], decomp=decomp, contract=contract, **p)
    if state is not None:
        s.set_state(state["iter_done"], state["best_inliers"], state["best_mask"], state["best_Tcw"])
    return s


GOLDEN_SCENES = ((0, 40), (1, 120))      # (seed, N)


def golden_run(s, decomp=None):
    """Scene s of the committed fixture and the restatement's first call on
    it (Relocalisation's parameters, iterate(5))."""
    seed, N = GOLDEN_SCENES[s]
    sc = scene(N, seed=500 + seed, noise=0.5)
    d = draws_for(500 + seed, 300)
    sol = solver_of(sc, RELOC, decomp)
    out = sol.iterate(5, d)
    return sc, d, sol, out


def make_golden(path):
    """Writes tests/golden/pnp_ransac.npz: the inputs, the records of every
    iteration and refit of the call (with np.linalg's decompositions in them)
    and the call's outputs."""
    z = {}
    for s in range(len(GOLDEN_SCENES)):
        sc, d, sol, out = golden_run(s)
        p = f"s{s}_"
        for k in ("keys", "pos", "valid", "cam", "sigma2"):
            z[p + k] = sc[k]
        z[p + "draws"] = d
        z[p + "sets"] = np.array(sol.taps["sets"], np.int32)
        z[p + "rec"] = np.array(sol.taps["rec"])
        z[p + "count"] = np.array(sol.taps["count"], np.int32)
        slots = sorted(sol.taps["refits"])
        z[p + "refit_slots"] = np.array(slots, np.int32)
        z[p + "refit_rec"] = np.array([sol.taps["refits"][k][0] for k in slots])
        z[p + "refit_count"] = np.array([sol.taps["refits"][k][1] for k in slots], np.int32)
        for k in ("N", "ransac_min_inliers", "ransac_max_its", "iters_run", "no_more", "found", "found_iter",
                  "n_inliers", "refined", "iter_done", "best_inliers", "best_slot"):
            z[p + k] = np.int32(out[k])
        for k in ("Tcw", "inliers", "best_mask", "best_Tcw"):
            z[p + k] = out[k]
    np.savez_compressed(path, **z)
