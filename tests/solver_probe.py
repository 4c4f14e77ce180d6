"""The probe of the solvers' shared device headers: the build of
tests/solver_probe.hip, the constructed inputs with their census, and the
references (tests/test_solver_probe_numpy.py, tests/test_solver_probe_gpu.py).

The entry points reach orbx_lm.h, orbx_jacobi.h, orbx_linalg.h, orbx_se3.h and
orbx_sim3_dev.h on well-conditioned scenes only; the probe calls each function
of theirs on arrays of inputs, one thread per input, so that the
data-dependent branches (the pivot-swap variants of ldlt_solve and lu3_solve,
qfrom's trace <= 0 side, the 1e-5 thresholds of the exponentials and the
logarithm, the floor and the clamp of the Jacobi core, the LM control's
comparisons) are taken on purpose.

Two kinds of reference:

* the operation order in float64 -- the restatements the suite already holds
  (sim3opt_numpy, essgraph_numpy, test_lba_numpy, init_numpy, sim3_numpy),
  which the device equals byte for byte wherever a function is made of
  + - * / sqrt and compares only.  Four texts are added here because no
  byte-exact one existed: qnormalize and se3_oplus (test_lba_numpy's use
  np.linalg.norm and @, whose summation order is the BLAS build's), the LM
  control (inline in sim3opt_numpy.levenberg) and the Hestenes sweep;
* the mathematical answer in mpmath at 60 digits: the exact solves, the exact
  SVD, 1/x, x^(-1/2), the Jacobi angle, and the closed forms of the SE3 / Sim3
  exponential and logarithm with no small-angle branch.

Where the device goes through a library function (sin, cos, acos, log, pow)
it is compared with the restatement under the bar of tests/essgraph_numpy.py:
8 x the worst relative difference the restatement shows against itself with
those calls moved by -1, 0 or +1 ulp, measured on the CPU on the same inputs
(MEASURED; tests/test_solver_probe_numpy.py asserts that it reproduces).
Nothing is measured against the device.
"""
import ctypes
import functools
import math
import subprocess
from pathlib import Path

import mpmath
import numpy as np

import essgraph_numpy as en
import init_numpy
import sim3_numpy
import sim3opt_numpy as so
import test_lba_numpy as lb
from orb_slam_amd.build import ARCH, COMMON, hipcc

F32, F64 = np.float32, np.float64
HERE = Path(__file__).resolve().parent
SRC = HERE / "solver_probe.hip"
OUT_DIR = HERE / "build_probe"
LIB = OUT_DIR / "libsolver_probe.so"
CSRC = HERE.parent / "orb_slam_amd" / "csrc"
HEADERS = ("orbx_lm.h", "orbx_jacobi.h", "orbx_linalg.h", "orbx_se3.h", "orbx_sim3_dev.h")

DBL_MIN = 2.2250738585072014e-308
DBL_MAX = np.finfo(F64).max
EPS64 = 2.0 ** -52
K_TOL = 8.9e-16          # kInitTol
K_FLOOR = 4.93e-32       # kInitFloor
K_SWEEPS = 40            # kInitSweeps
MP_DIGITS = 60
FACTOR = 8.0

# name: (doubles in, doubles out) per item, as tests/solver_probe.hip lays them out
PROBES = dict(ldlt6=(27, 7), ldlt7=(35, 8), huber=(2, 2), lm_trial=(7, 6), lm_retry=(2, 1), lm_stop=(5, 2),
              lm_scale7=(15, 1), rcp=(1, 1), rsq=(1, 1), jacobi_wants=(4, 1), sym_wants=(2, 1), jacobi_cs=(3, 3),
              hestenes3=(9, 18), hestenes4=(16, 32), null_vector4=(16, 4), linalg3=(23, 36), reproj_e2=(9, 2),
              quat=(20, 24), se3_oplus=(13, 7), se3_map=(10, 3), sim3_exp=(8, 8), sim3_mul=(16, 8),
              sim3_inverse=(8, 8), sim3_map=(11, 3), lu3=(12, 3), sim3_log=(8, 8))
MAX_ITEMS, MAX_ITEMS_MP = 2048, 512


# --- the build -----------------------------------------------------------------------------
def command(out=LIB):
    """The library's compiler and flags (orb_slam_amd.build), as a shared object."""
    return [hipcc(), "-x", "hip", f"--offload-arch={ARCH}", *COMMON, "-shared", str(SRC), "-o", str(out)]


def build():
    """tests/build_probe/libsolver_probe.so, rebuilt when the source or a header is newer."""
    assert "-ffp-contract=off" in COMMON      # what makes the byte comparisons meaningful
    OUT_DIR.mkdir(exist_ok=True)
    deps = [SRC] + sorted(CSRC.glob("*.h"))
    if not LIB.exists() or any(d.stat().st_mtime > LIB.stat().st_mtime for d in deps):
        p = subprocess.run(command(), capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"probe compile failed\n{p.stdout}\n{p.stderr}")
    return LIB


def load():
    lib = ctypes.CDLL(str(build()))
    for name in PROBES:
        f = getattr(lib, "probe_" + name)
        f.argtypes, f.restype = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    return lib


def run(lib, name, inputs):
    """One launch of probe `name` over inputs (n, NI): (n, NO) float64."""
    ni, no = PROBES[name]
    x = np.ascontiguousarray(inputs, F64)
    assert x.ndim == 2 and x.shape[1] == ni and 0 < len(x) <= MAX_ITEMS, (name, x.shape)
    out = np.empty((len(x), no), F64)
    err = getattr(lib, "probe_" + name)(len(x), x.ctypes.data, out.ctypes.data)
    assert err == 0, f"probe_{name}: HIP error {err}"
    return out


# --- comparisons ---------------------------------------------------------------------------
def same_bytes(got, want):
    """Byte for byte; where the reference has a NaN, a NaN of any payload."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def mismatches(got, want):
    """The rows in which same_bytes fails (for the assertion's message)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(np.uint64) != want.view(np.uint64)))
    return np.nonzero(bad.reshape(len(bad), -1).any(1))[0]


def rel_rows(a, b):
    """essgraph_numpy.rel per row over the finite entries; inf where the rows'
    NaNs or infinities differ."""
    a, b = np.asarray(a, F64).reshape(len(a), -1), np.asarray(b, F64).reshape(len(b), -1)
    fin = np.isfinite(a)
    with np.errstate(all="ignore"):
        same = (fin == np.isfinite(b)) & (fin | (np.isnan(a) & np.isnan(b)) | (a == b))
        d = np.where(fin & same, np.abs(a - b) / np.maximum(1.0, np.abs(a)), 0.0)
    return np.where(same.all(1), d.max(1), np.inf)


def ulp_rows(fn, runs=5, seed=2024):
    """Per row, the worst rel_rows of fn() against itself with the library
    calls of essgraph_numpy.MATH (and POW below) moved by an ulp."""
    global POW
    base = fn()
    worst = np.zeros(len(base))
    for k in range(runs):
        u = en.Ulp(seed + 100 * k)
        en.set_math(u)
        POW = lambda x, y, u=u: u._wrap(lambda v: np.power(v, y), x)
        try:
            worst = np.maximum(worst, rel_rows(base, fn()))
        finally:
            en.set_math(en.Exact)
            POW = np.power
    return worst


POW = np.power


# --- LDLT ----------------------------------------------------------------------------------
def pack_lower(H):
    n = len(H)
    return np.array([H[i][j] for i in range(n) for j in range(i + 1)], F64)


def ldlt_pivots(H):
    """The census of one pivoted LDLT: the transpositions tr[k], the sign class
    (0 zero, 1 positive, 2 negative, 3 indefinite) and the pivots, by a
    full-matrix right-looking elimination (not the restatement's order: it
    counts branches, it is no reference)."""
    A = np.array(H, F64)
    A = np.tril(A) + np.tril(A, -1).T
    n = len(A)
    tr, piv, sign = [], [], 0
    with np.errstate(all="ignore"):
        for k in range(n):
            big = k
            for i in range(k + 1, n):
                if abs(A[i, i]) > abs(A[big, big]):
                    big = i
            tr.append(big)
            if big != k:
                A[[k, big]] = A[[big, k]]
                A[:, [k, big]] = A[:, [big, k]]
            akk = A[k, k]
            piv.append(akk)
            if abs(akk) > 0:
                l = A[k + 1:, k] / akk
                A[k + 1:, k + 1:] -= np.outer(l, A[k, k + 1:])
            A[k + 1:, k] = A[k, k + 1:] = 0.0
            if sign == 1:
                sign = 3 if akk < 0 else 1
            elif sign == 2:
                sign = 3 if akk > 0 else 2
            elif sign == 0:
                sign = 1 if akk > 0 else (2 if akk < 0 else 0)
    return tr, sign, piv


def _spd_with_order(rng, n, order):
    """SPD, kappa < 1e3: the diagonal's values descend along `order` (a
    permutation of the positions), by at least a factor 1.3 a step, and the
    couplings are 5 % of sqrt(d_i d_j), so every Schur complement keeps the
    order."""
    v = np.cumprod(np.concatenate([[rng.uniform(40, 60)], 1 / rng.uniform(1.3, 1.6, n - 1)]))
    d = np.empty(n)
    d[np.asarray(order)] = v
    E = rng.uniform(-0.05, 0.05, (n, n))
    E = np.tril(E, -1) + np.tril(E, -1).T
    return np.diag(d) + E * np.sqrt(np.outer(d, d))


@functools.lru_cache(None)
def ldlt_inputs(n):
    """(H (m, n, n), b (m, n), labels): `spd` rows come first."""
    rng = np.random.RandomState(600 + n)
    Hs, bs, labels = [], [], []

    def add(H, b, label):
        Hs.append(np.array(H, F64))
        bs.append(np.array(b, F64))
        labels.append(label)
    for k in range(n - 1):
        for q in range(k + 1, n):
            for _ in range(8):
                # positions 0 .. k-1 hold the largest values in order (no swap before step k), position q the next
                rest = [p for p in range(k, n) if p != q]
                rng.shuffle(rest)
                add(_spd_with_order(rng, n, list(range(k)) + [q] + rest), rng.normal(0, 1, n), "spd")
    for _ in range(40):
        add(_spd_with_order(rng, n, rng.permutation(n)), rng.normal(0, 1, n), "spd")
    for _ in range(24):                                    # dense SPD of a wider condition, kappa <= 1e8
        Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
        w = 10.0 ** rng.uniform(-3, 3, n)
        add((Q * w) @ Q.T, rng.normal(0, 1, n), "spd")
    ones = np.ones(n)
    add(np.zeros((n, n)), rng.normal(0, 1, n), "zero")
    for _ in range(4):
        add(-_spd_with_order(rng, n, rng.permutation(n)), rng.normal(0, 1, n), "negdef")
    first = np.arange(n, 0, -1.0)
    first[1] = -first[1]                                   # the second pivot disagrees with the first
    last = np.arange(n, 0, -1.0)
    last[-1] = -1.0                                        # only the last pivot does
    for d, label in ((first, "indef_first"), (last, "indef_last"), (-last, "indef_last")):
        E = rng.uniform(-0.02, 0.02, (n, n))
        add(np.diag(d) + np.tril(E, -1) + np.tril(E, -1).T, rng.normal(0, 1, n), label)
    # rank n-1: positions 1 and 3 are the same coordinate, with the largest (a power of two) diagonal, so the
    # first pivot's column holds an exact 1, the copy's Schur row is exactly zero and its pivot comes last
    for _ in range(4):
        H = _spd_with_order(rng, n, rng.permutation(n))
        H[3, :], H[:, 3] = H[1, :], H[:, 1]
        H[1, 1] = H[3, 3] = H[1, 3] = H[3, 1] = 64.0
        add(H, rng.normal(0, 1, n), "rank_n-1")
    for _ in range(4):                                     # rank 1: v v^T of signed powers of two, exact
        v = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.randint(-2, 3, n)
        add(np.outer(v, v), rng.normal(0, 1, n), "rank_1")
    v = 2.0 ** np.arange(n)
    v[2] = 0.0
    add(np.outer(v, v), ones, "rank_1")
    for tiny, label in ((DBL_MIN, "pivot_dbl_min"), (-DBL_MIN, "pivot_dbl_min"), (DBL_MIN / 2, "pivot_below"),
                        (5e-324, "pivot_below"), (np.nextafter(DBL_MIN, 1), "pivot_above")):
        for pos in (0, n - 1):
            d = 1.0 + np.arange(n)
            d[pos] = tiny
            add(np.diag(d), ones, label)
    add(4.0 * np.eye(n) + 0.25 * (np.ones((n, n)) - np.eye(n)), rng.normal(0, 1, n), "tie_all")
    for i, j in ((0, 2), (2, 4), (1, n - 1), (n - 2, n - 1)):       # two equal largest entries: the first one wins
        d = 1.0 + np.arange(n) % 3
        d[i] = d[j] = 8.0
        add(np.diag(d) + 0.125 * (np.ones((n, n)) - np.eye(n)), ones, f"tie_{i}_{j}")
    for (i, j), label in (((3, 1), "nan_offdiag"), ((2, 2), "nan_diag"), ((n - 1, n - 1), "nan_diag")):
        H = _spd_with_order(rng, n, rng.permutation(n))
        H[i, j] = H[j, i] = np.nan
        add(H, rng.normal(0, 1, n), label)
    b = rng.normal(0, 1, n)
    b[2] = np.nan
    add(_spd_with_order(rng, n, rng.permutation(n)), b, "nan_b")
    b = rng.normal(0, 1, n)
    b[1] = np.inf
    add(_spd_with_order(rng, n, rng.permutation(n)), b, "inf_b")
    return np.array(Hs), np.array(bs), labels


def ldlt_census(n):
    H, _, labels = ldlt_inputs(n)
    variants, signs, by_label = {}, {}, {}
    for Hk, label in zip(H, labels):
        tr, sign, piv = ldlt_pivots(Hk)
        if not np.isnan(Hk).any():
            for k, q in enumerate(tr):
                if q != k:
                    variants[(k, q)] = variants.get((k, q), 0) + 1
            signs[sign] = signs.get(sign, 0) + 1
        by_label.setdefault(label, []).append((tr, sign, piv))
    return dict(variants=variants, signs=signs, by_label=by_label, n=len(H))


def ldlt_probe_inputs(n):
    H, b, _ = ldlt_inputs(n)
    return np.array([np.concatenate([pack_lower(Hk), bk]) for Hk, bk in zip(H, b)])


@functools.lru_cache(None)
def ldlt_reference(n):
    """sim3opt_numpy.ldlt_solve per input: (m, n + 1), x and the bool."""
    H, b, _ = ldlt_inputs(n)
    out = []
    with np.errstate(all="ignore"):
        for Hk, bk in zip(H, b):
            ok, x = so.ldlt_solve(Hk, bk)
            out.append(np.concatenate([x, [1.0 if ok else 0.0]]))
    return np.array(out)


def mp_solve(A, b):
    """(x*, kappa_2(A)) at MP_DIGITS."""
    with mpmath.workdps(MP_DIGITS):
        M = mpmath.matrix(np.asarray(A, F64).tolist())
        x = mpmath.lu_solve(M, mpmath.matrix([float(v) for v in b]))
        S = mpmath.svd_r(M, compute_uv=False)
        s = [S[i] for i in range(len(S))]
        return [x[i] for i in range(len(b))], max(s) / min(s)


def solve_error(x, exact, kappa):
    """|x - x*| / (|x*| kappa) in the 2-norm, at MP_DIGITS."""
    with mpmath.workdps(MP_DIGITS):
        d = mpmath.sqrt(sum((mpmath.mpf(float(a)) - e) ** 2 for a, e in zip(x, exact)))
        return float(d / (mpmath.sqrt(sum(e ** 2 for e in exact)) * kappa))


@functools.lru_cache(None)
def ldlt_exact(n):
    """The exact solves of the SPD inputs: [(index, x*, kappa)]."""
    H, b, labels = ldlt_inputs(n)
    out = []
    for k, label in enumerate(labels):
        if label == "spd":
            Hs = np.tril(H[k]) + np.tril(H[k], -1).T
            out.append((k,) + mp_solve(Hs, b[k]))
    assert len(out) <= MAX_ITEMS_MP
    return out


# --- LU ------------------------------------------------------------------------------------
def lu3_case(W):
    """The census of one lu3_solve: (first pivot row, second swap, big == 0 in
    the first column, in the second), in the function's own operation order."""
    m = np.array(W, F64).reshape(3, 3).copy()
    with np.errstate(all="ignore"):
        p, big = 0, abs(m[0, 0])
        if abs(m[1, 0]) > big:
            p, big = 1, abs(m[1, 0])
        if abs(m[2, 0]) > big:
            p, big = 2, abs(m[2, 0])
        m[[0, p]] = m[[p, 0]]
        if big != 0.0:
            m[1, 0] /= m[0, 0]
            m[2, 0] /= m[0, 0]
        for i in (1, 2):
            for j in (1, 2):
                m[i, j] -= m[i, 0] * m[0, j]
        swap = bool(abs(m[2, 1]) > abs(m[1, 1]))
        big2 = max(abs(m[1, 1]), abs(m[2, 1]))
    return p, swap, bool(big == 0.0), bool(big2 == 0.0)


@functools.lru_cache(None)
def lu3_inputs():
    """(W (m, 3, 3), t (m, 3), labels): `regular` rows come first."""
    rng = np.random.RandomState(33)
    W = list(rng.normal(0, 1, (384, 3, 3)))
    labels = ["regular"] * 384
    # what Sim3::log builds: A Omega + B Omega^2 + C I, and rows of it permuted
    for k in range(64):
        om = rng.normal(0, 1.5, 3)
        O = lb.skew(om)
        Wk = rng.uniform(0.2, 0.5) * O + rng.uniform(0.05, 0.2) * (O @ O) + rng.uniform(0.8, 1.2) * np.eye(3)
        W.append(Wk[rng.permutation(3)] if k % 2 else Wk)
        labels.append("regular")
    special = [
        (np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4.0]]), "big0_first"),
        (np.array([[1, 0, 0], [0, 0, 1], [0, 0, 2.0]]), "big0_second"),
        (np.array([[2, 4, 1], [1, 2, 3], [4, 8, 5.0]]), "big0_second"),
        (np.array([[1, 2, 3], [4, 5, 6], [5, 7, 9.0]]), "singular"),
        (np.array([[3, 1, 2], [6, 2, 4], [1, 1, 1.0]]), "singular"),
        (np.zeros((3, 3)), "zero"),
        (np.array([[1, 2, 3], [-1, 0.5, 1], [1, 3, 2.0]]), "tie_first"),       # |1| = |-1| = |1|: row 0 stays
        (np.array([[2, 1, 0], [1, 1.5, 1], [1, -0.5, 3.0]]), "tie_second"),    # 1 and -1 after the first column
    ]
    for Wk, label in special:
        W.append(Wk)
        labels.append(label)
    for i, j in ((0, 0), (1, 2), (2, 1)):
        Wk = rng.normal(0, 1, (3, 3))
        Wk[i, j] = np.nan
        W.append(Wk)
        labels.append("nan")
    Wk = rng.normal(0, 1, (3, 3))
    Wk[1, 0] = np.inf
    W.append(Wk)
    labels.append("inf")
    W = np.array(W)
    return W, rng.normal(0, 1, (len(W), 3)), labels


def lu3_census():
    W, _, labels = lu3_inputs()
    cases, big0 = {}, [0, 0]
    for Wk, label in zip(W, labels):
        if np.isfinite(Wk).all():
            p, swap, z1, z2 = lu3_case(Wk)
            cases[(p, swap)] = cases.get((p, swap), 0) + 1
            big0[0] += z1
            big0[1] += z2
    return dict(cases=cases, big0_first=big0[0], big0_second=big0[1], singular=labels.count("singular"), n=len(W))


def lu3_probe_inputs():
    W, t, _ = lu3_inputs()
    return np.concatenate([W.reshape(-1, 9), t], 1)


@functools.lru_cache(None)
def lu3_reference():
    W, t, _ = lu3_inputs()
    return en.lu3_solve([[W[:, i, j] for j in range(3)] for i in range(3)], [t[:, i] for i in range(3)])


@functools.lru_cache(None)
def lu3_exact():
    W, t, labels = lu3_inputs()
    out = [(k,) + mp_solve(W[k], t[k]) for k, label in enumerate(labels) if label == "regular"]
    assert len(out) <= MAX_ITEMS_MP
    return out


# --- quaternions ---------------------------------------------------------------------------
def rodrigues(axis, angle):
    """A rotation matrix in float64 (an input, not a reference)."""
    a = np.asarray(axis, F64)
    a = a / np.sqrt(a @ a)
    K = lb.skew(a)
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def qfrom_branch(m):
    """0: trace > 0; 1, 2, 3: the largest diagonal entry is x, y, z."""
    m = np.asarray(m, F64).reshape(3, 3)
    if m[0, 0] + m[1, 1] + m[2, 2] > 0:
        return 0
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return 1 + i


def qnormalize_ref(q):
    """SE3Quat::normalizeRotation as orbx_se3.h's qnormalize evaluates it."""
    x, y, z, w = (float(v) for v in q)
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    with np.errstate(all="ignore"):
        n = np.sqrt(F64(x * x + y * y + z * z + w * w))
        return np.array([x / n, y / n, z / n, w / n])


@functools.lru_cache(None)
def quat_inputs():
    """(m (n, 9), q1 (n, 4), q2 (n, 4), v (n, 3), labels)."""
    rng = np.random.RandomState(77)
    M, labels = [], []

    def add(m, label):
        M.append(np.asarray(m, F64).reshape(9))
        labels.append(label)
    for k in range(96):                                   # every angle, random axes: mostly trace > 0
        add(rodrigues(rng.normal(0, 1, 3), rng.uniform(0, np.pi)), "random")
    for ax in range(3):                                   # beyond 120 degrees about a dominant axis
        for k in range(32):
            a = 0.25 * rng.normal(0, 1, 3)
            a[ax] = 1.0
            add(rodrigues(a, rng.uniform(2.2, np.pi)), f"dominant_{'xyz'[ax]}")
    h, r3 = 0.5, math.sqrt(3.0) / 2
    add([1, 0, 0, 0, -h, -r3, 0, r3, -h], "120_x")
    add([-h, 0, r3, 0, 1, 0, -r3, 0, -h], "120_y")
    add([-h, -r3, 0, r3, -h, 0, 0, 0, 1], "120_z")
    add([0, 0, 1, 1, 0, 0, 0, 1, 0], "120_diag")           # trace 0 and all three diagonal entries tie
    add([1, 0, 0, 0, -1, 0, 0, 0, -1], "180_x")
    add([-1, 0, 0, 0, 1, 0, 0, 0, -1], "180_y")
    add([-1, 0, 0, 0, -1, 0, 0, 0, 1], "180_z")
    add(2.0 / 3.0 * np.ones((3, 3)) - np.eye(3), "180_diag")
    add([0, 1, 0, 1, 0, 0, 0, 0, -1], "tie_m4_m0")         # 180 degrees about (1, 1, 0): m[4] == m[0] > m[8]
    add([-1, 0, 0, 0, 0, 1, 0, 1, 0], "tie_m8_m4")         # about (0, 1, 1): m[8] == m[4] > m[0]
    add([0, 0, 1, 0, -1, 0, 1, 0, 0], "tie_m8_m0")         # about (1, 0, 1): m[8] == m[0] > m[4]
    for k in range(24):
        a = rng.normal(0, 1, 3)
        add(rodrigues(a, rng.uniform(0, np.pi)) + 1e-6 * rng.normal(0, 1, (3, 3)), "nonorthogonal")
    add(np.eye(3), "identity")
    add(np.zeros(9), "zero")
    for pos in (0, 4, 5):
        m = rodrigues(rng.normal(0, 1, 3), 1.0).reshape(9)
        m[pos] = np.nan
        add(m, "nan")
    n = len(M)
    q1 = rng.normal(0, 1, (n, 4))
    q1[::3] /= np.sqrt((q1[::3] ** 2).sum(1))[:, None]    # a third of them unit
    q1[1] = 0.0                                            # qnormalize of the zero quaternion: 0 / 0
    q1[2] = [0.0, 0.0, 0.0, -2.0]
    q1[3] = [1e-160, 0.0, 0.0, 0.0]                        # the squares underflow
    q1[4, 2] = np.nan
    q2 = rng.normal(0, 1, (n, 4))
    v = rng.normal(0, 3, (n, 3))
    return np.array(M), q1, q2, v, labels


def quat_census():
    M, _, _, _, labels = quat_inputs()
    br = [qfrom_branch(m) for m, label in zip(M, labels) if label != "nan"]
    return dict(branches={b: br.count(b) for b in range(4)}, labels=set(labels), n=len(M))


def quat_probe_inputs():
    M, q1, q2, v, _ = quat_inputs()
    return np.concatenate([M, q1, q2, v], 1)


@functools.lru_cache(None)
def quat_reference():
    M, q1, q2, v, _ = quat_inputs()
    out = []
    with np.errstate(all="ignore"):
        for m, a, b, p in zip(M, q1, q2, v):
            out.append(np.concatenate([lb.matrix_quat(m.reshape(3, 3)), lb.quat_matrix(a).reshape(9), so.quat_mul(a, b),
                                       lb.quat_rotate(a, p), qnormalize_ref(a)]))
    return np.array(out)


# --- SE3 -----------------------------------------------------------------------------------
def se3_oplus_ref(pose, u):
    """VertexSE3Expmap::oplusImpl on (x, y, z, w, tx, ty, tz) in orbx_se3.h's
    operation order: test_lba_numpy.se3_oplus with every sum spelled out (its
    @ and np.linalg.norm leave the order to the BLAS build), sin and cos
    through essgraph_numpy.MATH and the cube through POW."""
    pose, u = np.asarray(pose, F64), np.asarray(u, F64)
    o0, o1, o2 = (float(x) for x in u[:3])
    up = [float(x) for x in u[3:6]]
    with np.errstate(all="ignore"):
        theta = float(np.sqrt(F64(o0 * o0 + o1 * o1 + o2 * o2)))
        O = [[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]]
        O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
        eye = lambda i, j: 1.0 if i == j else 0.0
        if theta < 0.00001:
            R = [[eye(i, j) + O[i][j] + O2[i][j] for j in range(3)] for i in range(3)]
            V = R
        else:
            th = F64(theta)
            s, c = F64(en.MATH.sin(th)), F64(en.MATH.cos(th))
            a, b, d = s / th, (1 - c) / (th * th), (th - s) / F64(POW(th, 3))
            R = [[eye(i, j) + a * O[i][j] + b * O2[i][j] for j in range(3)] for i in range(3)]
            V = [[eye(i, j) + b * O[i][j] + d * O2[i][j] for j in range(3)] for i in range(3)]
        eq = lb.matrix_quat(np.array(R, F64))
        et = [V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2] for i in range(3)]
        eq = qnormalize_ref(eq)
        rt = lb.quat_rotate(eq, pose[4:7])
        nq = qnormalize_ref(so.quat_mul(eq, pose[:4]))
        return np.concatenate([nq, [et[i] + rt[i] for i in range(3)]])


THETA_EDGES = (np.nextafter(1e-5, 0), 1e-5, np.nextafter(1e-5, 1))


def _updates(rng, scale_too):
    """Update vectors (omega, upsilon[, sigma]) and labels: both sides of each
    1e-5 threshold, theta near pi, the zero update, NaN."""
    U, labels = [], []

    def add(om, sigma, label, ups=None):
        ups = rng.normal(0, 1, 3) if ups is None else ups
        U.append(np.concatenate([om, ups, [sigma]] if scale_too else [om, ups]))
        labels.append(label)
    sig_small = (0.0, 3e-6, -7e-6, np.nextafter(1e-5, 0), -np.nextafter(1e-5, 0))
    sig_large = (1e-5, -1e-5, np.nextafter(1e-5, 1), 0.3, -0.2, 2e-5, 1e-3)
    sigmas = (sig_small + sig_large) if scale_too else (0.0,)
    for sigma in sigmas:
        for ax in range(3):                               # sqrt(x * x) = |x|: theta is the entry itself
            for th in THETA_EDGES:
                om = np.zeros(3)
                om[ax] = th if ax != 1 else -th
                add(om, sigma, "theta_edge")
        for k in range(6):
            d = rng.normal(0, 1, 3)
            d /= np.sqrt(d @ d)
            add(10.0 ** rng.uniform(-9, -5.3) * d, sigma, "small")
            add(10.0 ** rng.uniform(-4.7, 0.3) * d, sigma, "regular")
        for th in (np.pi - 1e-3, np.pi - 1e-8, np.pi, 3.0, 2.5):
            for ax in range(3):
                om = 0.1 * rng.normal(0, 1, 3)
                om[ax] = 1.0
                add(th * om / np.sqrt(om @ om), sigma, "near_pi")
        add(np.array([0.0, 0.0, 4.0]), sigma, "beyond_pi")
        add(np.zeros(3), sigma, "zero", np.zeros(3))
    om = rng.normal(0, 0.3, 3)
    om[1] = np.nan
    add(om, 0.1 if scale_too else 0.0, "nan")
    add(np.array([np.nan, 0.0, 0.0]), 0.0, "nan")
    return np.array(U), labels


def _poses(rng, n):
    """Unit quaternions (one in eight off by 1e-8, every fifth with w < 0) and translations."""
    q = rng.normal(0, 1, (n, 4))
    q /= np.sqrt((q ** 2).sum(1))[:, None]
    q[::8] *= 1 + 1e-8
    q[::5] *= np.where(q[::5, 3:4] > 0, -1.0, 1.0)
    q[0] = [0.0, 0.0, 0.0, 1.0]
    return np.concatenate([q, rng.normal(0, 2, (n, 3))], 1)


@functools.lru_cache(None)
def se3_inputs():
    """(pose (n, 7), u (n, 6), labels, branch): branch 0 is theta < 1e-5."""
    rng = np.random.RandomState(91)
    U, labels = _updates(rng, False)
    pose = _poses(rng, len(U))
    theta = np.sqrt(U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2])
    return pose, U, labels, np.where(theta < 1e-5, 0, 1)        # a NaN theta takes the else side, as on the device


def se3_compute():
    pose, U, _, _ = se3_inputs()
    return np.array([se3_oplus_ref(p, u) for p, u in zip(pose, U)])


@functools.lru_cache(None)
def se3_reference():
    return se3_compute()


def se3_groups():
    """The bar of each se3_oplus row: None where the row has no library call."""
    _, _, labels, branch = se3_inputs()
    return [None if b == 0 else ("ulp_se3_edge" if l == "theta_edge" else "ulp_se3") for l, b in zip(labels, branch)]


def se3_map_inputs():
    rng = np.random.RandomState(92)
    pose = _poses(rng, 256)
    pose[3, 1] = np.nan
    return np.concatenate([pose, rng.normal(0, 5, (256, 3))], 1)


def se3_map_reference(x):
    return np.array([lb.quat_rotate(r[:4], r[7:10]) + r[4:7] for r in x])


# --- Sim3 ----------------------------------------------------------------------------------
@functools.lru_cache(None)
def sim3_exp_inputs():
    """(u (n, 7), es (n,), labels, branch): bit 1 |sigma| >= eps, bit 0 theta >= eps."""
    rng = np.random.RandomState(93)
    U, labels = _updates(rng, True)
    with np.errstate(all="ignore"):
        theta = np.sqrt(U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2])
        branch = np.where(np.abs(U[:, 6]) < 1e-5, 0, 2) + np.where(theta < 1e-5, 0, 1)
        return U, np.exp(U[:, 6]), labels, branch


@functools.lru_cache(None)
def sim3_exp_reference():
    """sim3opt_numpy.sim3_exp (math.sin / math.cos) with the probe's es."""
    U, es, _, _ = sim3_exp_inputs()
    with np.errstate(all="ignore"):
        return np.array([so.sim3_exp(u, float(e)) for u, e in zip(U, es)])


def sim3_exp_vector():
    """essgraph_numpy.vexp on the same inputs: the form that goes through MATH."""
    U, es, _, _ = sim3_exp_inputs()
    return en.vexp(U, es)


def sim3_exp_groups():
    _, _, labels, branch = sim3_exp_inputs()
    return [None if b % 2 == 0 else ("ulp_exp_edge" if l == "theta_edge" else "ulp_exp") for l, b in zip(labels, branch)]


def _d_of(q):
    R = en.vqmat(np.asarray(q, F64))
    return float(0.5 * (R[0][0] + R[1][1] + R[2][2] - 1))


def _d_edge(axis):
    """Two half-angles one float apart whose quaternions put d on either side of 1 - 1e-5."""
    def quat(h):
        q = np.zeros(4)
        q[axis], q[3] = math.sin(h), math.cos(h)
        return q
    lo, hi = 1e-3, 3e-3                                   # d(lo) > 1 - eps > d(hi): theta = 2 h = 4.47e-3 at the edge
    assert _d_of(quat(lo)) > 1 - 1e-5 >= _d_of(quat(hi))
    while np.nextafter(lo, 1) < hi:
        mid = 0.5 * (lo + hi)
        if _d_of(quat(mid)) > 1 - 1e-5:
            lo = mid
        else:
            hi = mid
    return quat(lo), quat(hi)


def _s_edge(sign):
    """Two scales one float apart whose log lies on either side of sign * 1e-5."""
    lo, hi = (1.0, 1.0001) if sign > 0 else (0.9999, 1.0)
    inside = lambda s: abs(math.log(s)) < 1e-5
    while np.nextafter(lo, 2) < hi:
        mid = 0.5 * (lo + hi)
        if inside(mid) == inside(lo):
            lo = mid
        else:
            hi = mid
    return (lo, hi) if sign > 0 else (hi, lo)              # (inside, outside)


@functools.lru_cache(None)
def sim3_log_inputs():
    """(Sim3 (n, 8), labels).  The scales next to the sigma threshold are one
    float apart, which moves log(s) by 1e5 of its ulps: any log within an ulp
    takes the same side."""
    rng = np.random.RandomState(94)
    S, labels = [], []

    def add(q, s, label, t=None):
        S.append(np.concatenate([q, rng.normal(0, 1, 3) if t is None else t, [s]]))
        labels.append(label)

    def quat(d, angle):
        d = np.asarray(d, F64)
        d = d / np.sqrt(d @ d)
        return np.concatenate([math.sin(angle / 2) * d, [math.cos(angle / 2)]])
    s_in_p, s_out_p = _s_edge(+1)
    s_in_m, s_out_m = _s_edge(-1)
    scales = (1.0, s_in_p, s_in_m, 1 + 1e-6, 1 - 3e-6, s_out_p, s_out_m, 1.1, 0.8, 1 + 1e-4, 3.0)
    for s in scales:
        for ax in range(3):
            for q in _d_edge(ax):
                add(q, s, "d_edge")
        for k in range(6):
            add(quat(rng.normal(0, 1, 3), 10.0 ** rng.uniform(-8, -2.6)), s, "small")
            add(quat(rng.normal(0, 1, 3), 10.0 ** rng.uniform(-2, 0.4)), s, "regular")
        for ang in (np.pi - 1e-3, np.pi - 1e-6, 3.0):
            add(quat(rng.normal(0, 1, 3), ang), s, "near_pi")
        add(np.array([1.0, 0.0, 0.0, 0.0]), s, "pi")       # d = -1: theta / (2 sqrt(0)) * 0
        add(np.array([0.0, 0.0, 0.0, 1.0]), s, "identity", np.zeros(3))
        add((1 + 1e-8) * quat(rng.normal(0, 1, 3), 1e-4), s, "unnormalised_small")   # d stays above 1 - eps
        add((1 + 1e-8) * quat(rng.normal(0, 1, 3), 0.5), s, "unnormalised")
        add(1.2 * np.array([1.0, 0.0, 0.0, 0.01]), s, "d_below_-1")                  # acos(d < -1): NaN, as in g2o
    add(quat([1, 2, 3], 0.4), 0.0, "s_zero")
    add(quat([1, 2, 3], 0.4), -1.0, "s_negative")
    q = quat([3, 2, 1], 0.2)
    q[2] = np.nan
    add(q, 1.1, "nan")
    return np.array(S), labels


def sim3_log_reference():
    """essgraph_numpy.vlog: (n, 7) and the branch."""
    S, _ = sim3_log_inputs()
    return en.vlog(S)


def sim3_log_groups():
    """Branch 2 takes A and B from differences that cancel to sigma^2 and
    sigma^3 (g2o's text): an ulp of log(s) moves them by 1e-16 / sigma^2, so it
    has a bar of its own.  log(0) = -inf has no neighbour to move to: that row
    is compared as it is and not measured."""
    _, labels = sim3_log_inputs()
    _, branch = sim3_log_reference()
    return [None if l == "s_zero" else ("ulp_log_b2" if b == 2 else "ulp_log") for l, b in zip(labels, branch)]


def sim3_pairs():
    """(a (n, 8), b (n, 8), P (n, 3)) for sim3_mul / sim3_inverse / sim3_map."""
    rng = np.random.RandomState(95)
    n = 256
    a = np.concatenate([_poses(rng, n), rng.uniform(0.5, 2.0, (n, 1))], 1)
    b = np.concatenate([_poses(rng, n), rng.uniform(0.5, 2.0, (n, 1))], 1)
    a[1, 7] = 0.0                                          # inverse: -1 / 0
    a[2, 7] = 5e-324
    a[3, 5] = np.nan
    a[4, 7] = np.inf
    return a, b, rng.normal(0, 4, (n, 3))


# --- mpmath: the exponential and logarithm maps, no small-angle branch -----------------------
def mp_sim3_exp(u):
    """(q (unit, w >= 0), t, s) of Sim3(update) at MP_DIGITS, theta > 0; sigma
    = 0 is SE3's exponential."""
    om = [mpmath.mpf(float(x)) for x in u[:3]]
    ups = [mpmath.mpf(float(x)) for x in u[3:6]]
    sigma = mpmath.mpf(float(u[6])) if len(u) > 6 else mpmath.mpf(0)
    theta = mpmath.sqrt(sum(x * x for x in om))
    s = mpmath.exp(sigma)
    if sigma == 0:
        A, B, C = (1 - mpmath.cos(theta)) / theta ** 2, (theta - mpmath.sin(theta)) / theta ** 3, mpmath.mpf(1)
    else:
        a, b, c = s * mpmath.sin(theta), s * mpmath.cos(theta), theta ** 2 + sigma ** 2
        C = (s - 1) / sigma
        A = (a * sigma + (1 - b) * theta) / (theta * c)
        B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    O = mpmath.matrix([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    W = A * O + B * (O * O) + C * mpmath.eye(3)
    t = W * mpmath.matrix(ups)
    k = mpmath.sin(theta / 2) / theta
    q = [k * om[0], k * om[1], k * om[2], mpmath.cos(theta / 2)]
    if q[3] < 0:
        q = [-x for x in q]
    return [float(x) for x in q] + [float(t[i]) for i in range(3)] + [float(s)]


def mp_sim3_log(a):
    """(omega, upsilon, sigma) of a Sim3 with 0 < theta < pi at MP_DIGITS."""
    q = [mpmath.mpf(float(x)) for x in a[:4]]
    t = mpmath.matrix([mpmath.mpf(float(x)) for x in a[4:7]])
    s = mpmath.mpf(float(a[7]))
    sigma = mpmath.log(s)
    nv = mpmath.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    theta = 2 * mpmath.atan2(nv, q[3])
    om = [theta * x / nv for x in q[:3]]
    if sigma == 0:
        A, B, C = (1 - mpmath.cos(theta)) / theta ** 2, (theta - mpmath.sin(theta)) / theta ** 3, mpmath.mpf(1)
    else:
        sa, sb, c = s * mpmath.sin(theta), s * mpmath.cos(theta), theta ** 2 + sigma ** 2
        C = (s - 1) / sigma
        A = (sa * sigma + (1 - sb) * theta) / (theta * c)
        B = (C - ((sb - 1) * sigma + sa * theta) / c) / theta ** 2
    O = mpmath.matrix([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    W = A * O + B * (O * O) + C * mpmath.eye(3)
    ups = mpmath.lu_solve(W, t)
    return [float(x) for x in om] + [float(ups[i]) for i in range(3)] + [float(sigma)]


def well_conditioned_exp(U, labels):
    """The rows the mpmath comparison runs on: both closed-form branches far
    from their thresholds, theta in [0.01, 3.05]."""
    theta = np.sqrt((U[:, :3] ** 2).sum(1))
    ok = np.array([l == "regular" or l == "near_pi" for l in labels]) & (theta >= 0.01) & (theta <= 3.05)
    if U.shape[1] > 6:
        ok &= (np.abs(U[:, 6]) >= 1e-3) | (U[:, 6] == 0.0)
    return np.nonzero(ok)[0]


# --- Jacobi --------------------------------------------------------------------------------
def col_dot(x, y):
    """orbx_jacobi.h's col_dot: left to right at 3, pairwise at 4."""
    if len(x) == 3:
        return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    return (x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3])


def jacobi_wants_ref(al, be, ga, floor):
    with np.errstate(all="ignore"):
        return bool(ga != 0.0 and ga * ga > (K_TOL * K_TOL) * (al * be) and al >= floor and be >= floor)


def sym_wants_ref(apq, floor):
    with np.errstate(all="ignore"):
        return bool(apq != 0.0 and apq * apq > floor)


def jacobi_cs_ref(al, be, ga):
    """jacobi_cs with 1 / x and 1 / sqrt(x) for fast_rcp and fast_rsq."""
    with np.errstate(all="ignore"):
        zeta = F64(be - al) * (F64(1.0) / F64(2.0 * ga))
        zeta = min(max(zeta, -1e100), 1e100) if not np.isnan(zeta) else F64(-1e100)    # fmax / fmin drop the NaN
        w = 1.0 + zeta * zeta
        t = math.copysign(1.0 / (abs(zeta) + w * (1.0 / np.sqrt(w))), zeta)
        c = 1.0 / np.sqrt(1.0 + t * t)
        return float(c), float(c * t), float(t)


def hestenes_ref(A):
    """One-sided Jacobi in float64, hestenes<N>'s sweep order and tests, on a
    float32 N x N: (a[col][row], v[col][row], sweeps)."""
    A = np.asarray(A, F32).astype(F64)
    n = len(A)
    a = [[float(A[i, j]) for i in range(n)] for j in range(n)]
    v = [[1.0 if i == j else 0.0 for i in range(n)] for j in range(n)]
    with np.errstate(all="ignore"):
        floor = F64(0.0)
        for j in range(n):
            floor = floor + F64(col_dot(a[j], a[j]))
        floor = float(floor * K_FLOOR)
        sweeps = 0
        for sweep in range(K_SWEEPS):
            rot = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    al, be, ga = (float(F64(col_dot(a[i], a[j]))) for i, j in ((p, p), (q, q), (p, q)))
                    if jacobi_wants_ref(al, be, ga, floor):
                        rot = True
                        c, s, _ = jacobi_cs_ref(al, be, ga)
                        for i in range(n):
                            ap, aq, vp, vq = a[p][i], a[q][i], v[p][i], v[q][i]
                            a[p][i], a[q][i] = c * ap - s * aq, s * ap + c * aq
                            v[p][i], v[q][i] = c * vp - s * vq, s * vp + c * vq
            sweeps += 1
            if not rot:
                break
    return np.array(a), np.array(v), sweeps


def _orth(rng, n):
    Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
    return Q


@functools.lru_cache(None)
def hestenes_inputs(n):
    """(A (m, n, n) float32, labels)."""
    rng = np.random.RandomState(400 + n)
    As, labels = [], []

    def add(A, label):
        As.append(np.asarray(A, F64).astype(F32))
        labels.append(label)
    for gap in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6):       # the two smallest singular values differ by gap
        for k in range(6):
            sv = np.sort(rng.uniform(0.5, 2.0, n))[::-1].copy()
            sv[-1] = sv[-2] - gap * sv[0]
            add((_orth(rng, n) * sv) @ _orth(rng, n).T, f"gap_{gap:g}")
    for k in range(12):
        add(rng.normal(0, 1, (n, n)), "random")
    for k in range(6):                                     # rank n - 1, exactly: small integers, the last row a sum
        A = rng.randint(-4, 5, (n, n)).astype(F64)
        A[-1] = A[0] + A[1]
        add(A, "rank_n-1")
        add(np.outer(rng.randint(1, 5, n), rng.randint(-3, 4, n) | 1), "rank_1")
    add(np.zeros((n, n)), "zero")
    sv = np.array([3.0, 3.0, 1.0, 0.5][:n])
    add(np.diag(sv)[rng.permutation(n)], "equal_sv")
    for k in range(4):
        add((_orth(rng, n) * sv) @ _orth(rng, n).T, "equal_sv")
        sv0 = np.array([2.0, 1.0, 0.25, 0.25][4 - n:])     # the two smallest (nearly) equal
        add((_orth(rng, n) * sv0) @ _orth(rng, n).T, "equal_smallest")
    add(np.diag(np.array([2.0, 1.0, 0.5, 0.5][4 - n:])), "equal_smallest")
    for j in range(n):
        A = rng.normal(0, 1, (n, n))
        A[:, j] = 0.0
        add(A, "zero_column")
    add(np.eye(n), "orthogonal")
    add(np.eye(n)[rng.permutation(n)] * np.array([2.0, -1.0, 0.5, 3.0][:n]), "orthogonal")
    add(np.diag(np.arange(1.0, n + 1)), "orthogonal")
    for scale in (1e-18, 1e18):
        for k in range(4):
            add(scale * rng.normal(0, 1, (n, n)), f"scaled_{scale:g}")
    for pos in ((0, 0), (1, 2), (n - 1, n - 1)):
        A = rng.normal(0, 1, (n, n))
        A[pos] = np.nan
        add(A, "nan")
    return np.array(As), labels


def mp_svd(A):
    """(singular values descending, the right singular vectors as rows in that
    order) of a float32 matrix at MP_DIGITS."""
    with mpmath.workdps(MP_DIGITS):
        M = mpmath.matrix(np.asarray(A, F32).astype(F64).tolist())
        U, S, V = mpmath.svd_r(M)
        n = len(S)
        order = sorted(range(n), key=lambda i: -S[i])
        return [float(S[i]) for i in order], np.array([[float(V[i, j]) for j in range(n)] for i in order])


@functools.lru_cache(None)
def hestenes_exact(n):
    A, labels = hestenes_inputs(n)
    return [mp_svd(Ak) if label != "nan" else None for Ak, label in zip(A, labels)]


def hestenes_figures(A, a, v, sv):
    """What a returned (a, v) shows on the float32 A with exact singular values
    sv: |V^T V - I|, |A V - a| / sigma_1, the column norms against sv as sorted
    lists / sigma_1, and whether any pair still wants a rotation."""
    A = np.asarray(A, F32).astype(F64)
    n = len(A)
    s1 = sv[0] if sv[0] > 0 else 1.0
    with np.errstate(all="ignore"):
        orth = float(np.max(np.abs(v @ v.T - np.eye(n))))
        av = float(np.max(np.abs(A @ v.T - a.T))) / s1
        norms = np.sort(np.sqrt((a * a).sum(1)))[::-1]
        svd = float(np.max(np.abs(norms - np.array(sv)))) / s1
        floor = F64(0.0)
        for j in range(n):
            floor = floor + F64(col_dot(A[:, j], A[:, j]))
        floor = float(floor * K_FLOOR)
        wants = any(jacobi_wants_ref(float(col_dot(a[p], a[p])), float(col_dot(a[q], a[q])), float(col_dot(a[p], a[q])), floor)
                    for p in range(n - 1) for q in range(p + 1, n))
    return dict(hest_orth=orth, hest_av=av, hest_sv=svd), wants


def null_select(a, v):
    """null_vector4's choice among hestenes' columns: the v of the smallest
    column, the first one on ties, in float64."""
    best, nv = 0.0, None
    with np.errstate(all="ignore"):
        for j in range(len(a)):
            nj = float(F64(col_dot(a[j], a[j])))
            if j == 0 or nj < best:
                best, nv = nj, v[j]
    return np.asarray(nv, F64)


def null_vector_figure(x, sv, V):
    """How far the unit vector x (float64) lies from the exact null direction,
    in units of eps sigma_1 / gap.  The exact directions are the rows of V whose
    singular values lie within 1e-6 sigma_1 of the smallest (one row where the
    relative gap is at least 1e-6: then this is the distance to +-v); gap is
    from that cluster to the next singular value above it.  Returns (figure,
    |1 - |x||)."""
    x, sv = np.asarray(x, F64), np.asarray(sv, F64)
    s1 = sv[0] if sv[0] > 0 else 1.0
    inside = sv <= sv[-1] + 1e-6 * s1
    unit = abs(1.0 - float(np.sqrt((x * x).sum())))
    if inside.all():
        return 0.0, unit
    gap = (sv[~inside].min() - sv[-1]) / s1
    outside = V[~inside] @ x                              # the components along the other singular vectors
    return float(np.sqrt((outside ** 2).sum()) * gap / EPS64), unit


@functools.lru_cache(None)
def jacobi_inputs():
    """(al, be, ga, floor) rows and labels, for jacobi_wants and jacobi_cs."""
    rng = np.random.RandomState(55)
    rows, labels = [], []

    def add(al, be, ga, floor, label):
        rows.append([al, be, ga, floor])
        labels.append(label)
    for k in range(24):
        al, be = rng.uniform(0.1, 10, 2)
        floor = (al + be) * K_FLOOR
        thr = K_TOL * math.sqrt(al * be)
        for g in (thr, np.nextafter(thr, 0), np.nextafter(thr, 1), thr * (1 - 1e-12), thr * (1 + 1e-12), -thr * 1.001, -thr * 0.999):
            add(al, be, g, floor, "threshold")
        add(al, al, rng.uniform(-1, 1) * al, floor, "al_eq_be")
        add(al, be, rng.uniform(-1, 1) * math.sqrt(al * be), floor, "regular")
        add(al, be, 10.0 ** rng.uniform(-12, -1) * math.sqrt(al * be), floor, "regular")
        add(al, be, (be - al) * 10.0 ** rng.uniform(-130, -101), floor, "clamp")
        add(al, be, 5e-324 * rng.randint(1, 1000), floor, "ga_denormal")
        add(al, be, 0.0, floor, "ga_zero")
        add(al * 1e-40, be, 1e-20 * rng.uniform(-1, 1), floor, "below_floor")
        add(al, floor * (1 - 1e-15), 1e-17, floor, "below_floor")
        add(al, floor, 1e-17, floor, "at_floor")
    add(1.0, 1.0, 0.0, K_FLOOR, "ga_zero")                 # al == be and ga == 0: 0 * inf
    add(1.0, 2.0, np.nan, K_FLOOR, "nan")
    add(np.nan, 2.0, 0.5, K_FLOOR, "nan")
    add(1.0, 2.0, 0.5, np.nan, "nan")
    return np.array(rows), labels


def mp_jacobi(al, be, ga):
    """(c, s, t, zeta) of the exact smaller root of t^2 + 2 zeta t - 1 = 0."""
    with mpmath.workdps(MP_DIGITS):
        zeta = (mpmath.mpf(float(be)) - mpmath.mpf(float(al))) / (2 * mpmath.mpf(float(ga)))
        t = (1 if zeta >= 0 else -1) / (abs(zeta) + mpmath.sqrt(1 + zeta * zeta))
        c = 1 / mpmath.sqrt(1 + t * t)
        return c, c * t, t, zeta


def sym_wants_inputs():
    """(apq, floor) around apq^2 = floor, and the degenerate ones."""
    rng = np.random.RandomState(62)
    rows = []
    for k in range(32):
        f = 10.0 ** rng.uniform(-40, 10)
        r = math.sqrt(f)
        rows += [[r, f], [np.nextafter(r, 0), f], [np.nextafter(r, np.inf), f], [-r * 1.001, f], [-r * 0.999, f], [rng.normal(), f]]
    rows += [[0.0, 0.0], [-0.0, 0.0], [5e-324, 0.0], [1e-200, 0.0], [np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, np.inf]]
    return np.array(rows)


@functools.lru_cache(None)
def rcp_inputs():
    rng = np.random.RandomState(56)
    x = [2.0 ** k for k in range(-500, 501, 25)]
    for c in (1.0, 2.0, 4.0):
        x += [np.nextafter(c, 0), c, np.nextafter(c, 8)]
    x += list(2.0 ** rng.uniform(-500, 500, 400))
    x = np.array(x)
    return np.concatenate([x, -x[::3]])


def rsq_inputs():
    x = rcp_inputs()
    return x[x > 0]


def ulp_error(got, exact_fn, x):
    """|got - exact| in ulps of the exact value, per element, at MP_DIGITS."""
    out = []
    with mpmath.workdps(MP_DIGITS):
        for g, xi in zip(got, x):
            e = exact_fn(mpmath.mpf(float(xi)))
            out.append(float(abs(mpmath.mpf(float(g)) - e) / mpmath.mpf(float(np.spacing(abs(float(e)))))))
    return np.array(out)


# --- the defined float arithmetic --------------------------------------------------------------
@functools.lru_cache(None)
def linalg_inputs():
    """(n, 23) doubles that hold floats: a[9], b[9], v[3], s, t."""
    rng = np.random.RandomState(57)
    x = rng.normal(0, 1, (512, 23)) * 10.0 ** rng.uniform(-3, 3, (512, 1))
    x[0, :9] = [1, 2, 3, 4, 5, 6, 5, 7, 9]                 # singular: det 0, inv 0 / 0 and x / 0
    x[1, :9] = 0.0
    x[2, :9] = np.eye(3).reshape(9)
    x[3, 4] = np.nan
    x[4, 18:21] = 0.0                                      # norm3 of zero
    x[5, :9] *= 1e18                                       # cofactors beyond float, finite in FP64
    x[6, :9] *= 1e-20
    x[7, 18] = np.inf
    x[8, 18:21] = [3e-23, -4e-23, 0.0]                     # squares far below float's range, exact in FP64
    return x.astype(F32).astype(F64)


def linalg_reference(x):
    a, b, v, s, t = x[:, :9], x[:, 9:18], x[:, 18:21], x[:, 21], x[:, 22]
    a3 = a.reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        mul = init_numpy.mul3(a, b).astype(F64)
        smul = np.stack([(s * sim3_numpy.dot3(a3[:, i, :], b.reshape(-1, 3, 3)[:, :, j])).astype(F32)
                         for i in range(3) for j in range(3)], 1).astype(F64)
        mv = np.stack([sim3_numpy.dot3(a3[:, i, :], v).astype(F32) for i in range(3)], 1).astype(F64)
        tmv = np.stack([sim3_numpy.dot3(v, a3[:, :, i]).astype(F32) for i in range(3)], 1).astype(F64)
        aff = (sim3_numpy.dot3(a3[:, 0, :], v) + t).astype(F32).astype(F64)
        nrm = np.sqrt(sim3_numpy.dot3(v, v))
        inv = init_numpy.inv3(a).astype(F64)
        m = a.T
        det = (m[0] * (m[4] * m[8] - m[5] * m[7]) + m[1] * (m[5] * m[6] - m[3] * m[8])) + m[2] * (m[3] * m[7] - m[4] * m[6])
    return np.concatenate([mul, smul, mv, tmv, aff[:, None], nrm[:, None], inv, det[:, None]], 1)


@functools.lru_cache(None)
def reproj_inputs():
    """(n, 9) doubles that hold floats: cam (fx, fy, cx, cy), x, y, z, u, v."""
    rng = np.random.RandomState(58)
    n = 512
    cam = np.array([458.654, 457.296, 367.215, 248.375]) * rng.uniform(0.9, 1.1, (n, 4))
    P = np.concatenate([rng.normal(0, 1, (n, 2)), rng.uniform(0.2, 8, (n, 1))], 1)
    uv = cam[:, 2:] + cam[:, :2] * P[:, :2] / P[:, 2:] + rng.normal(0, 2, (n, 2))
    x = np.concatenate([cam, P, uv], 1)
    x[0, 6] = 0.0                                          # z = 0: 1 / 0
    x[1, 6] = -1.5
    x[2, 6] = 1e-40                                        # a denormal float depth
    x[3, 4] = np.nan
    x[4, 7:9] = cam[4, 2:] + cam[4, :2] * P[4, :2] / P[4, 2:]
    return x.astype(F32).astype(F64)


def reproj_reference(x):
    """reproj_e2 with contract 0 and 1: float operations, the fused ones as
    sim3_numpy._fma (the product of two floats is exact in FP64, and the sum
    of an exact product and a float, rounded to FP64 and then to float, is the
    correctly rounded fma but for double rounding, which these inputs avoid:
    the CPU test checks that against mpmath)."""
    f = x.astype(F32)
    cam, X, Y, Z, u, v = f[:, :4], f[:, 4], f[:, 5], f[:, 6], f[:, 7], f[:, 8]
    with np.errstate(all="ignore"):
        invz = (1.0 / Z.astype(F64)).astype(F32)
        imx, imy = cam[:, 0] * X * invz + cam[:, 2], cam[:, 1] * Y * invz + cam[:, 3]
        ex, ey = imx - u, imy - v
        e0 = ex * ex + ey * ey
        imx = sim3_numpy._fma(cam[:, 0] * X, invz, cam[:, 2])
        imy = sim3_numpy._fma(cam[:, 1] * Y, invz, cam[:, 3])
        ex, ey = imx - u, imy - v
        e1 = sim3_numpy._fma(ex, ex, ey * ey)
    return np.stack([e0, e1], 1).astype(F64)


def fma32_exact(a, b, c):
    """The correctly rounded float fma, through mpmath."""
    with mpmath.workdps(MP_DIGITS):
        out = [mpmath.mpf(float(x)) * mpmath.mpf(float(y)) + mpmath.mpf(float(z)) for x, y, z in zip(a, b, c)]
        return np.array([float(o) if mpmath.isfinite(o) else float("nan") for o in out]).astype(F32)


# --- the LM control --------------------------------------------------------------------------
def lm_trial_ref(row):
    """lm_trial on (lambda, ni, nBad, currentChi, tempChi, ok, scale): the
    lines of simopt_numpy.levenberg's trial, the cube through POW."""
    lam, ni, nbad, chi, tmp, ok, scale = (float(x) for x in row)
    with np.errstate(all="ignore"):
        if not ok:
            tmp = DBL_MAX
        scale = F64(scale) + 1e-3
        rho = float((F64(chi) - F64(tmp)) / scale)
        accept = rho > 0 and np.isfinite(tmp)
        if accept:
            alpha = min(1. - float(POW(F64(2 * rho - 1), 3)), 2. / 3.)
            lam = float(F64(lam) * max(1. / 3., alpha))
            ni = 2.0
            chi = tmp
        else:
            lam = float(F64(lam) * F64(ni))
            ni = float(F64(ni) * 2)
    return [lam, ni, nbad, chi, 1.0 if accept else 0.0, rho]


def lm_retry_ref(row):
    return [1.0 if (row[0] < 0 and row[1] < 10) else 0.0]


def lm_stop_ref(row):
    nbad, qmax, rho, ini, cur = (float(x) for x in row)
    if qmax == 10 or rho == 0:
        return [1.0, nbad]
    with np.errstate(all="ignore"):
        nbad = nbad + 1 if float((F64(ini) - F64(cur)) * 1e3) < ini else 0.0
    return [1.0 if nbad >= 3 else 0.0, nbad]


def lm_scale_ref(row):
    x, lam, b = row[:7], row[7], row[8:15]
    scale = F64(0.0)
    with np.errstate(all="ignore"):
        for j in range(7):
            scale = scale + x[j] * (lam * x[j] + b[j])
    return [float(scale)]


RHO_CROSS = tuple(0.5 * (1 + c ** (1 / 3.0)) for c in (2.0 / 3.0, 1.0 / 3.0))    # 1 - (2 rho - 1)^3 = 1/3, 2/3


@functools.lru_cache(None)
def lm_trial_inputs():
    """rows (lambda, ni, nBad, currentChi, tempChi, ok, scale) and labels."""
    rng = np.random.RandomState(59)
    rows, labels = [], []

    def add(chi, tmp, ok, scale, label, lam=None, ni=None):
        rows.append([rng.uniform(1e-6, 10) if lam is None else lam, 2.0 ** rng.randint(1, 6) if ni is None else ni,
                     float(rng.randint(0, 3)), chi, tmp, ok, scale])
        labels.append(label)
    for k in range(64):
        chi = rng.uniform(1, 100)
        add(chi, chi * rng.uniform(0.2, 1.5), 1.0, rng.uniform(0, 50), "random")
    for k in range(6):
        chi = rng.uniform(1, 100)
        add(chi, chi, 1.0, rng.uniform(0, 5), "rho_zero")
        add(np.inf, np.inf, 1.0, 1.0, "rho_nan")
        add(chi, chi * 0.5, 0.0, 1.0, "not_ok")
        add(chi, np.inf, 1.0, 1.0, "temp_inf")
        add(chi, np.nan, 1.0, 1.0, "temp_nan")
        add(chi, chi * 0.5, 1.0, -1.0, "scale_negative")           # a gain over a negative predicted one: rho < 0
        add(np.inf, chi, 1.0, 1.0, "current_inf")
    assert 0.999 + 1e-3 == 1.0
    for r0 in RHO_CROSS:                                    # scale + 1e-3 = 1 and tempChi = 0: rho = currentChi
        for step in range(-3, 4):
            add(float(r0 + step * np.spacing(r0)), 0.0, 1.0, 0.999, "alpha_cross")
    for r in (1e-3, 0.3, 0.5, 0.75, 0.97, 1.0, 1.5, 40.0, 1e120):
        add(r, 0.0, 1.0, 0.999, "alpha_range")
    add(1.0, 0.5, 1.0, 1.0, "lambda_overflow", lam=1e308, ni=1e10)
    return np.array(rows), labels


def lm_trial_census():
    rows, labels = lm_trial_inputs()
    ref = np.array([lm_trial_ref(r) for r in rows])
    cross = [(r[3], 1. - (2 * r[3] - 1) ** 3) for r, l in zip(rows, labels) if l == "alpha_cross"]
    return dict(labels={l: labels.count(l) for l in set(labels)}, accepted=int(ref[:, 4].sum()), rejected=int((ref[:, 4] == 0).sum()),
                rho_zero=int((ref[:, 5] == 0).sum()), rho_nan=int(np.isnan(ref[:, 5]).sum()),
                below_third=sum(a < 1 / 3 for _, a in cross), above_third=sum(1 / 3 < a < 0.5 for _, a in cross),
                below_two_thirds=sum(0.5 < a < 2 / 3 for _, a in cross), above_two_thirds=sum(a > 2 / 3 for _, a in cross))


@functools.lru_cache(None)
def lm_stop_inputs():
    """rows (nBad, qmax, rho, iniChi, currentChi) and labels.  (ini - cur) 1e3
    == ini at ini = 1000, cur = 999 exactly; a float to either side of cur puts
    the product to either side of ini (the closest the expression can come:
    its step there is 1e3 ulp(cur))."""
    rows, labels = [], []
    assert (1000.0 - 999.0) * 1e3 == 1000.0
    for nbad in (0.0, 1.0, 2.0):
        for cur, label in ((999.0, "gain_equal"), (np.nextafter(999.0, 2000), "gain_below"), (np.nextafter(999.0, 0), "gain_above")):
            rows.append([nbad, 3.0, 0.7, 1000.0, cur])
            labels.append(label)
        for qmax in (9.0, 10.0):
            rows.append([nbad, qmax, 0.7, 1000.0, 500.0])
            labels.append(f"qmax_{int(qmax)}")
            rows.append([nbad, qmax, -0.5, 1000.0, 1000.0])
            labels.append(f"qmax_{int(qmax)}")
        rows.append([nbad, 1.0, 0.0, 1000.0, 1000.0])
        labels.append("rho_zero")
        rows.append([nbad, 1.0, -0.0, 1000.0, 1000.0])
        labels.append("rho_zero")
        rows.append([nbad, 1.0, np.nan, 1000.0, 1000.0])
        labels.append("rho_nan")
        rows.append([nbad, 1.0, 0.5, np.nan, 10.0])
        labels.append("chi_nan")
        rows.append([nbad, 1.0, 0.5, np.inf, 10.0])
        labels.append("chi_inf")
        rows.append([nbad, 1.0, 0.5, 0.0, 0.0])
        labels.append("chi_zero")
    return np.array(rows), labels


def lm_retry_inputs():
    return np.array([[rho, q] for rho in (-1.0, -5e-324, -0.0, 0.0, 5e-324, 0.5, np.nan, -np.inf, np.inf)
                     for q in (0.0, 1.0, 8.0, 9.0, 10.0, 11.0)])


def lm_scale_inputs():
    rng = np.random.RandomState(60)
    x = rng.normal(0, 1, (128, 15)) * 10.0 ** rng.uniform(-8, 8, (128, 1))
    x[:, 7] = 10.0 ** rng.uniform(-16, 4, 128)
    x[0] = 0.0
    x[1, 3] = np.nan
    x[2, :7] = 1e200                                        # lambda x^2 overflows
    return x


def huber_inputs():
    rng = np.random.RandomState(61)
    delta = np.sqrt(np.array([5.991, 7.815, 10.0]))[rng.randint(0, 3, 256)]
    e2 = rng.uniform(0, 30, 256)
    d2 = delta * delta
    e2[:30:3], e2[1:30:3], e2[2:30:3] = d2[:30:3], np.nextafter(d2[1:30:3], 0), np.nextafter(d2[2:30:3], 100)
    e2[30:36] = [0.0, 5e-324, np.inf, np.nan, -1.0, 1e300]
    return np.stack([e2, delta], 1)


def huber_reference(x):
    r0, r1 = so.huber(x[:, 0], x[:, 1])
    return np.stack([r0, r1], 1)


# --- the measured bars -------------------------------------------------------------------------
# ulp_*: the worst rel() of the restatement against itself with sin / cos / acos / log (and the cube of
# se3_oplus and lm_trial) moved by an ulp, on the probe's own inputs; solve_*: the restatement's worst
# |x - x*| / (|x*| kappa) against the exact solve; hest_* / null4: the float64 Hestenes restatement against the
# exact SVD.  The tests' bars are FACTOR x these; tests/test_solver_probe_numpy.py asserts they reproduce.
MEASURED = dict(ulp_se3=9.1e-14, ulp_se3_edge=2.4e-11, ulp_exp=8.8e-12, ulp_exp_edge=2.9e-11, ulp_log=7.2e-14, ulp_log_b2=9.4e-9,
                ulp_lm_lambda=3.9e-16, solve_ldlt6=4.8e-17, solve_ldlt7=3.8e-17, solve_lu3=2.0e-16, hest_orth=1.6e-15,
                hest_av=5.3e-16, hest_sv=8.3e-16, null4=1.2)
TOL = {k: FACTOR * v for k, v in MEASURED.items()}

# The header's promise for fast_rcp / fast_rsq ("a few units of FP64 round-off"), as the maintainers' contract:
RCP_RSQ_MAX_ULP = 8.0


def lm_trial_compute():
    return np.array([lm_trial_ref(r) for r in lm_trial_inputs()[0]])


def measure():
    """MEASURED, again."""
    out = dict.fromkeys(MEASURED, 0.0)
    for fn, groups in ((se3_compute, se3_groups()), (sim3_exp_vector, sim3_exp_groups()),
                       (lambda: sim3_log_reference()[0], sim3_log_groups())):
        for g, w in zip(groups, ulp_rows(fn)):
            if g is not None:
                out[g] = max(out[g], float(w))
    out["ulp_lm_lambda"] = float(ulp_rows(lambda: lm_trial_compute()[:, :1]).max())
    for n in (6, 7):
        ref = ldlt_reference(n)
        out[f"solve_ldlt{n}"] = max(solve_error(ref[k][:n], x, kappa) for k, x, kappa in ldlt_exact(n))
    ref = lu3_reference()
    out["solve_lu3"] = max(solve_error(ref[k], x, kappa) for k, x, kappa in lu3_exact())
    worst = dict(hest_orth=0.0, hest_av=0.0, hest_sv=0.0, null4=0.0)
    for n in (3, 4):
        A, labels = hestenes_inputs(n)
        for Ak, label, exact in zip(A, labels, hestenes_exact(n)):
            if label == "nan":
                continue
            a, v, _ = hestenes_ref(Ak)
            fig, _ = hestenes_figures(Ak, a, v, exact[0])
            for q, val in fig.items():
                worst[q] = max(worst[q], val)
            if n == 4:
                worst["null4"] = max(worst["null4"], null_vector_figure(null_select(a, v), *exact)[0])
    out.update(worst)
    return out
