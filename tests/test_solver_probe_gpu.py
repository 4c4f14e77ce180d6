"""The shared solver headers on the device, one function at a time
(tests/solver_probe.hip through tests/solver_probe.py): byte for byte against
the float64 restatements wherever a function is + - * / sqrt and compares, the
measured bars where it goes through a library function, the exact solves and
the exact SVD from mpmath, and the 8-ulp contract of fast_rcp / fast_rsq.
Every test is one launch of at most 2048 threads (two where two probes share
their inputs); tests/test_solver_probe_numpy.py holds the census of the inputs
and the measurements behind the bars."""
import mpmath
import numpy as np
import pytest

import essgraph_numpy as en
import sim3opt_numpy as so
import solver_probe as sp

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    return sp.load()


def assert_bytes(got, want, what):
    bad = sp.mismatches(got, want)
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(want)} differ; first: got {got[bad[0]]}, want {want[bad[0]]}"


# --- orbx_lm.h -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7])
def test_ldlt_solve(lib, n):
    got = sp.run(lib, f"ldlt{n}", sp.ldlt_probe_inputs(n))
    ref = sp.ldlt_reference(n)
    _, _, labels = sp.ldlt_inputs(n)
    bad = sp.mismatches(got, ref)
    assert len(bad) == 0, f"rows {[(int(k), labels[k]) for k in bad[:8]]}: got {got[bad[0]]}, want {ref[bad[0]]}"
    worst = max(sp.solve_error(got[k][:n], x, kappa) for k, x, kappa in sp.ldlt_exact(n))
    print(f"ldlt{n}: |x - x*| / (|x*| kappa) {worst:.3e}, bar {sp.TOL[f'solve_ldlt{n}']:.3e}")
    assert worst <= sp.TOL[f"solve_ldlt{n}"]


def test_huber(lib):
    x = sp.huber_inputs()
    assert_bytes(sp.run(lib, "huber", x), sp.huber_reference(x), "huber")


def test_lm_trial(lib):
    rows, labels = sp.lm_trial_inputs()
    got, ref = sp.run(lib, "lm_trial", rows), sp.lm_trial_compute()
    assert_bytes(got[:, 1:], ref[:, 1:], "ni, nBad, currentChi, accept, rho")
    rejected = ref[:, 4] == 0
    assert_bytes(got[rejected, :1], ref[rejected, :1], "lambda of the rejected trials")
    d = sp.rel_rows(ref[~rejected, :1], got[~rejected, :1])
    print(f"lambda of the accepted trials: {d.max():.3e}, bar {sp.TOL['ulp_lm_lambda']:.3e}")
    assert d.max() <= sp.TOL["ulp_lm_lambda"]


def test_lm_retry_stop_scale(lib):
    x = sp.lm_retry_inputs()
    assert_bytes(sp.run(lib, "lm_retry", x), np.array([sp.lm_retry_ref(r) for r in x]), "lm_retry")
    x, _ = sp.lm_stop_inputs()
    assert_bytes(sp.run(lib, "lm_stop", x), np.array([sp.lm_stop_ref(r) for r in x]), "lm_stop")
    x = sp.lm_scale_inputs()
    assert_bytes(sp.run(lib, "lm_scale7", x), np.array([sp.lm_scale_ref(r) for r in x]), "lm_scale<7>")


# --- orbx_jacobi.h -------------------------------------------------------------------------------
def test_fast_rcp_rsq_keep_the_eight_ulp_contract(lib):
    x = sp.rcp_inputs()
    e = sp.ulp_error(sp.run(lib, "rcp", x[:, None])[:, 0], lambda v: 1 / v, x)
    print(f"fast_rcp: worst {e.max():.3f} ulp over {len(x)} inputs")
    assert e.max() <= sp.RCP_RSQ_MAX_ULP
    x = sp.rsq_inputs()
    e = sp.ulp_error(sp.run(lib, "rsq", x[:, None])[:, 0], lambda v: 1 / mpmath.sqrt(v), x)
    print(f"fast_rsq: worst {e.max():.3f} ulp over {len(x)} inputs")
    assert e.max() <= sp.RCP_RSQ_MAX_ULP


def test_jacobi_wants_and_sym_wants(lib):
    rows, _ = sp.jacobi_inputs()
    assert_bytes(sp.run(lib, "jacobi_wants", rows), np.array([[float(sp.jacobi_wants_ref(*r))] for r in rows]), "jacobi_wants")
    x = sp.sym_wants_inputs()
    assert_bytes(sp.run(lib, "sym_wants", x), np.array([[float(sp.sym_wants_ref(*r))] for r in x]), "sym_wants")


def test_jacobi_cs(lib):
    rows, labels = sp.jacobi_inputs()
    got = sp.run(lib, "jacobi_cs", rows[:, :3])
    worst_t = worst_cs = 0.0
    with mpmath.workdps(sp.MP_DIGITS):
        for r, l, (c, s, t) in zip(rows, labels, got):
            if l == "nan":
                continue
            assert np.isfinite([c, s, t]).all(), (l, r, c, s, t)          # the clamp: never a NaN
            worst_cs = max(worst_cs, abs(c * c + s * s - 1))
            if l in ("clamp", "ga_denormal"):              # |zeta| held at 1e100: the identity to round-off
                assert abs(c - 1) <= 16 * sp.EPS64 and abs(s) < 1e-99 and abs(t) < 1e-99, (l, r, c, s, t)
            if r[2] != 0.0:
                _, _, te, zeta = sp.mp_jacobi(*r[:3])
                if abs(zeta) < 1e99:                       # at zeta = 0 the roots +-1 are equally small: either sign
                    worst_t = max(worst_t, float(abs((abs(t) if zeta == 0 else t) - te) / abs(te)))
    print(f"jacobi_cs: t {worst_t:.3e} relative, |c2 + s2 - 1| {worst_cs:.3e}")
    assert worst_t <= 1e-12 and worst_cs <= 16 * sp.EPS64


@pytest.mark.parametrize("n", [3, 4])
def test_hestenes(lib, n):
    A, labels = sp.hestenes_inputs(n)
    x = A.astype(F64).reshape(len(A), -1)
    got = sp.run(lib, f"hestenes{n}", x)
    nv = sp.run(lib, "null_vector4", x) if n == 4 else None
    worst = dict.fromkeys(("hest_orth", "hest_av", "hest_sv", "null4"), 0.0)
    for k, (Ak, label, exact) in enumerate(zip(A, labels, sp.hestenes_exact(n))):
        a, v = got[k][:n * n].reshape(n, n), got[k][n * n:].reshape(n, n)
        if label == "nan":                                 # a NaN rotates nothing
            assert np.array_equal(v, np.eye(n)) and sp.same_bytes(a, Ak.astype(F64).T)
        else:
            fig, wants = sp.hestenes_figures(Ak, a, v, exact[0])
            assert not wants, (k, label)
            for q, val in fig.items():
                worst[q] = max(worst[q], val)
                assert val <= sp.TOL[q], (k, label, q, val)
        if n == 4:
            chosen = sp.null_select(a, v)
            assert sp.same_bytes(nv[k], chosen.astype(F32).astype(F64)), (k, label, nv[k], chosen)
            if label != "nan":
                figure, unit = sp.null_vector_figure(chosen, *exact)
                worst["null4"] = max(worst["null4"], figure)
                assert figure <= sp.TOL["null4"] and unit <= 16 * sp.EPS64, (k, label, figure, unit)
    print({q: f"{val:.3e} (bar {sp.TOL[q]:.3e})" for q, val in worst.items()})


# --- orbx_linalg.h -------------------------------------------------------------------------------
def test_linalg3_and_reproj_e2(lib):
    x = sp.linalg_inputs()
    assert_bytes(sp.run(lib, "linalg3", x), sp.linalg_reference(x), "mul3 .. det3")
    x = sp.reproj_inputs()
    assert_bytes(sp.run(lib, "reproj_e2", x), sp.reproj_reference(x), "reproj_e2, contract 0 and 1")


# --- orbx_se3.h ----------------------------------------------------------------------------------
def test_quaternions(lib):
    got, ref = sp.run(lib, "quat", sp.quat_probe_inputs()), sp.quat_reference()
    labels = sp.quat_inputs()[4]
    for name, cols in (("qfrom", slice(0, 4)), ("qmat", slice(4, 13)), ("qmul", slice(13, 17)), ("qrot", slice(17, 20)),
                       ("qnormalize", slice(20, 24))):
        bad = sp.mismatches(got[:, cols], ref[:, cols])
        assert len(bad) == 0, f"{name}: rows {[(int(k), labels[k]) for k in bad[:8]]}: got {got[bad[0], cols]}, want {ref[bad[0], cols]}"


def _bytes_and_bars(got, ref, groups, what):
    """Rows without a library call: bytes.  The others: within their group's bar."""
    worst = {}
    for k, g in enumerate(groups):
        if g is None:
            assert sp.same_bytes(got[k], ref[k]), f"{what}: row {k}: got {got[k]}, want {ref[k]}"
        else:
            d = float(sp.rel_rows(ref[k:k + 1], got[k:k + 1])[0])
            worst[g] = max(worst.get(g, 0.0), d)
            assert d <= sp.TOL[g], f"{what}: row {k} ({g}): {d:.3e} > {sp.TOL[g]:.3e}: got {got[k]}, want {ref[k]}"
    print(what, {g: f"{v:.3e} (bar {sp.TOL[g]:.3e})" for g, v in worst.items()})


def test_se3_oplus_and_map(lib):
    pose, U, _, _ = sp.se3_inputs()
    _bytes_and_bars(sp.run(lib, "se3_oplus", np.concatenate([pose, U], 1)), sp.se3_reference(), sp.se3_groups(), "se3_oplus")
    x = sp.se3_map_inputs()
    assert_bytes(sp.run(lib, "se3_map", x), sp.se3_map_reference(x), "se3_map")


# --- orbx_sim3_dev.h -----------------------------------------------------------------------------
def test_sim3_exp(lib):
    U, es, _, _ = sp.sim3_exp_inputs()
    got = sp.run(lib, "sim3_exp", np.concatenate([U, es[:, None]], 1))
    _bytes_and_bars(got, sp.sim3_exp_reference(), sp.sim3_exp_groups(), "sim3_exp")


def test_sim3_mul_inverse_map(lib):
    a, b, P = sp.sim3_pairs()
    with np.errstate(all="ignore"):
        assert_bytes(sp.run(lib, "sim3_mul", np.concatenate([a, b], 1)), np.array([so.sim3_mul(x, y) for x, y in zip(a, b)]), "sim3_mul")
        assert_bytes(sp.run(lib, "sim3_inverse", a), np.array([so.sim3_inverse(x) for x in a]), "sim3_inverse")
        assert_bytes(sp.run(lib, "sim3_map", np.concatenate([a, P], 1)), np.array([so.sim3_map(x, p) for x, p in zip(a, P)]), "sim3_map")
        assert_bytes(sp.run(lib, "sim3_mul", np.concatenate([a, b], 1)), en.vmul(a, b), "sim3_mul, the vector form")


def test_lu3_solve(lib):
    got, ref = sp.run(lib, "lu3", sp.lu3_probe_inputs()), sp.lu3_reference()
    labels = sp.lu3_inputs()[2]
    bad = sp.mismatches(got, ref)
    assert len(bad) == 0, f"rows {[(int(k), labels[k]) for k in bad[:8]]}: got {got[bad[0]]}, want {ref[bad[0]]}"
    worst = max(sp.solve_error(got[k], x, kappa) for k, x, kappa in sp.lu3_exact())
    print(f"lu3: |x - x*| / (|x*| kappa) {worst:.3e}, bar {sp.TOL['solve_lu3']:.3e}")
    assert worst <= sp.TOL["solve_lu3"]


def test_sim3_log(lib):
    S, labels = sp.sim3_log_inputs()
    got = sp.run(lib, "sim3_log", S)
    ref, branch = sp.sim3_log_reference()
    assert np.array_equal(got[:, 7], branch.astype(F64)), np.nonzero(got[:, 7] != branch)[0]
    # without acos: omega = deltaR / 2 in branches 0 and 2, and in branch 0 (A, B, C constants) upsilon as well
    b0, b2 = branch == 0, branch == 2
    assert_bytes(got[b0, :6], ref[b0, :6], "branch 0: omega, upsilon")
    assert_bytes(got[b2, :3], ref[b2, :3], "branch 2: omega")
    groups = sp.sim3_log_groups()
    worst = {}
    for k, g in enumerate(groups):
        d = float(sp.rel_rows(ref[k:k + 1], got[k:k + 1, :7])[0])
        g = g or "ulp_log"
        worst[g] = max(worst.get(g, 0.0), d)
        assert d <= sp.TOL[g], f"row {k} ({labels[k]}, branch {branch[k]}): {d:.3e} > {sp.TOL[g]:.3e}: got {got[k]}, want {ref[k]}"
    print("sim3_log", {g: f"{v:.3e} (bar {sp.TOL[g]:.3e})" for g, v in worst.items()})
    # fidelity to g2o: acos of d < -1 and theta / sqrt(1 - d^2) at d = -1 are NaN there and here
    for l in ("d_below_-1", "pi"):
        assert np.isnan(got[labels.index(l), :6]).all()
