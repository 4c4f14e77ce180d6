"""The probe of the shared solver headers, on the CPU (tests/solver_probe.py):
the census of every constructed input set -- what keeps
tests/test_solver_probe_gpu.py from silently losing a branch --, the float64
restatements against the mpmath answers on the well-conditioned inputs, the
measurement behind the bars, and the cross-compile of the probe."""
import collections
import math

import mpmath
import numpy as np
import pytest

import essgraph_numpy as en
import solver_probe as sp
import test_lba_numpy as lb

F32, F64 = np.float32, np.float64


# --- the census ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7])
def test_ldlt_inputs_take_every_swap_variant_and_sign_class(n):
    c = sp.ldlt_census(n)
    print(n, "variants", sorted(c["variants"].items()), "signs", c["signs"], "inputs", c["n"])
    want = {(k, q) for k in range(n - 1) for q in range(k + 1, n)}
    assert len(want) == n * (n - 1) // 2 and set(c["variants"]) == want
    assert min(c["variants"].values()) >= 8
    assert set(c["signs"]) == {0, 1, 2, 3} and c["n"] <= sp.MAX_ITEMS
    by = c["by_label"]
    assert all(sign == 0 and tr == list(range(n)) for tr, sign, _ in by["zero"])
    assert all(sign == 2 for _, sign, _ in by["negdef"])
    for tr, sign, piv in by["indef_first"]:                # the second pivot is the first to disagree
        assert sign == 3 and piv[0] > 0 > piv[1]
    for tr, sign, piv in by["indef_last"]:                 # only the last one does
        assert sign == 3 and (np.sign(piv[:-1]) == np.sign(piv[0])).all() and np.sign(piv[-1]) == -np.sign(piv[0])
    for tr, sign, piv in by["rank_n-1"]:
        assert sign == 1 and piv[-1] == 0.0 and all(p > 0 for p in piv[:-1])
    for tr, sign, piv in by["rank_1"]:                     # zero pivots before the last: the column division is skipped
        assert sign == 1 and piv[0] > 0 and all(p == 0.0 for p in piv[1:])
    assert sorted({abs(piv[-1]) for _, _, piv in by["pivot_dbl_min"]}) == [sp.DBL_MIN]
    assert all(0 < abs(piv[-1]) < sp.DBL_MIN for _, _, piv in by["pivot_below"])
    assert all(abs(piv[-1]) > sp.DBL_MIN for _, _, piv in by["pivot_above"])
    assert by["tie_all"][0][0][0] == 0
    for i, j in ((0, 2), (2, 4), (1, n - 1), (n - 2, n - 1)):
        assert by[f"tie_{i}_{j}"][0][0][0] == i             # the first of the two largest wins
    assert {"nan_offdiag", "nan_diag", "nan_b", "inf_b"} <= set(by)
    # the restatement takes the x = 0 line where the census says so
    H, b, labels = sp.ldlt_inputs(n)
    ref = sp.ldlt_reference(n)
    for k, label in enumerate(labels):
        if label in ("zero", "rank_1", "pivot_dbl_min", "pivot_below"):
            assert (ref[k][:n] == 0).any(), label
        if label in ("zero", "spd", "rank_1", "rank_n-1", "tie_all"):
            assert ref[k][n] == 1.0
        if label in ("negdef", "indef_first", "indef_last"):
            assert ref[k][n] == 0.0


def test_lu_inputs_take_every_pivot_case():
    c = sp.lu3_census()
    print(c)
    assert set(c["cases"]) == {(p, s) for p in range(3) for s in (False, True)} and min(c["cases"].values()) >= 32
    assert c["big0_first"] >= 1 and c["big0_second"] >= 2 and c["singular"] >= 2 and c["n"] <= sp.MAX_ITEMS
    W, _, labels = sp.lu3_inputs()
    assert sp.lu3_case(W[labels.index("tie_first")])[0] == 0 and not sp.lu3_case(W[labels.index("tie_second")])[1]
    assert sp.lu3_case(W[labels.index("big0_first")])[2] and sp.lu3_case(W[labels.index("big0_second")])[3]
    assert labels.count("regular") <= sp.MAX_ITEMS_MP and "nan" in labels


def test_quat_inputs_take_every_branch_of_qfrom():
    c = sp.quat_census()
    print(c["branches"])
    assert min(c["branches"].values()) >= 32 and c["n"] <= sp.MAX_ITEMS
    assert {"120_x", "120_y", "120_z", "120_diag", "180_x", "180_y", "180_z", "180_diag", "tie_m4_m0", "tie_m8_m4",
            "nonorthogonal", "nan"} <= c["labels"]
    M, _, _, _, labels = sp.quat_inputs()
    branch = {l: sp.qfrom_branch(m) for m, l in zip(M, labels)}
    assert [branch[f"120_{a}"] for a in "xyz"] == [1, 2, 3] and [branch[f"180_{a}"] for a in "xyz"] == [1, 2, 3]
    assert branch["120_diag"] == 1 and branch["180_diag"] == 1            # all three tie: x
    assert branch["tie_m4_m0"] == 1 and branch["tie_m8_m4"] == 2 and branch["tie_m8_m0"] == 1
    for l in ("120_x", "120_diag"):                                       # trace exactly 0: the else side
        m = M[labels.index(l)]
        assert m[0] + m[4] + m[8] == 0.0


def test_exp_and_log_inputs_take_every_branch_from_both_sides():
    below, at, above = sp.THETA_EDGES
    assert below < 1e-5 == at < above
    pose, U, labels, branch = sp.se3_inputs()
    theta = np.sqrt(U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2])
    assert set(branch) == {0, 1} and len(U) <= sp.MAX_ITEMS
    assert {below, at, above} <= set(theta) and set(branch[theta == below]) == {0} and set(branch[theta == at]) == {1}
    assert "zero" in labels and "near_pi" in labels and np.abs(np.sqrt((pose[:, :4] ** 2).sum(1)) - 1).max() > 5e-9
    U, es, labels, branch = sp.sim3_exp_inputs()
    theta = np.sqrt(U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2])
    count = collections.Counter(branch.tolist())
    print("sim3_exp branches", dict(count))
    assert set(count) == {0, 1, 2, 3} and min(count.values()) >= 32 and len(U) <= sp.MAX_ITEMS
    for side in (0, 2):                                    # the theta edge within either sigma class
        rows = (branch // 2 * 2 == side)
        assert set(branch[rows & (theta == below)]) == {side} and set(branch[rows & (theta == above)]) == {side + 1}
        assert set(branch[rows & (theta == at)]) == {side + 1}
    sig = np.abs(U[:, 6])
    assert set(branch[sig == below] // 2) == {0} and set(branch[sig == at] // 2) == {1} and set(branch[sig == above] // 2) == {1}
    assert {"zero", "near_pi", "nan"} <= set(labels) and np.any(np.abs(es - 1) < 1e-5)
    S, labels = sp.sim3_log_inputs()
    L, branch = sp.sim3_log_reference()
    count = collections.Counter(branch.tolist())
    print("sim3_log branches", dict(count))
    assert set(count) == {0, 1, 2, 3} and min(count.values()) >= 32 and len(S) <= sp.MAX_ITEMS
    edge = np.array([l == "d_edge" for l in labels])
    d = np.array([sp._d_of(q) for q in S[:, :4]])
    assert np.abs(d[edge] - (1 - 1e-5)).max() < 1e-15       # within a few floats of the threshold, on both sides
    for side in (0, 2):
        assert set(branch[edge & (branch // 2 * 2 == side)]) == {side, side + 1}
    for sign in (+1, -1):                                  # two adjacent floats, log on either side of +-1e-5
        s_in, s_out = sp._s_edge(sign)
        assert abs(s_in - s_out) == np.spacing(min(s_in, s_out)) and abs(math.log(s_in)) < 1e-5 <= abs(math.log(s_out))
        assert set(branch[S[:, 7] == s_in] // 2) == {0} and set(branch[S[:, 7] == s_out] // 2) == {1}
    small = np.array([l == "unnormalised_small" for l in labels])
    assert set(branch[small] % 2) == {0}                    # 1e-8 off the unit sphere stays in the small-angle branch
    assert np.isnan(L[labels.index("d_below_-1")][:3]).all() and np.isnan(L[labels.index("pi")][:3]).all()


def test_jacobi_inputs_hold_every_required_case():
    for n in (3, 4):
        A, labels = sp.hestenes_inputs(n)
        assert {"gap_0.1", "gap_0.01", "gap_0.001", "gap_0.0001", "gap_1e-05", "gap_1e-06", "rank_n-1", "rank_1", "zero",
                "equal_sv", "equal_smallest", "zero_column", "orthogonal", "scaled_1e-18", "scaled_1e+18", "nan"} <= set(labels)
        assert len(A) <= sp.MAX_ITEMS_MP and A.dtype == F32
        for Ak, label, exact in zip(A, labels, sp.hestenes_exact(n)):
            if label == "nan":
                continue
            sv = np.array(exact[0])
            if label.startswith("gap_"):
                gap = (sv[-2] - sv[-1]) / sv[0]
                assert 0.5 * float(label[4:]) < gap < 2 * float(label[4:]), (label, gap)
            if label == "rank_n-1":
                assert sv[-1] < 1e-50 * sv[0] < sv[-2]
            if label == "rank_1":
                assert sv[1] < 1e-50 * sv[0]
            if label == "orthogonal":
                assert sp.hestenes_ref(Ak)[2] == 1           # one sweep, no rotation
            if label.startswith("scaled"):
                assert np.isfinite((Ak.astype(F64) ** 2).sum()) and (Ak.astype(F64) ** 2).sum() * sp.K_FLOOR > sp.DBL_MIN
    rows, labels = sp.jacobi_inputs()
    assert {"threshold", "al_eq_be", "clamp", "ga_denormal", "ga_zero", "below_floor", "at_floor", "nan"} <= set(labels)
    wants = [sp.jacobi_wants_ref(*r) for r in rows]
    thr = [w for w, l in zip(wants, labels) if l == "threshold"]
    assert 0.3 < np.mean(thr) < 0.7                        # both sides of |ga| = kInitTol sqrt(al be)
    assert not any(w for w, l in zip(wants, labels) if l in ("ga_zero", "below_floor", "nan"))
    assert all(w for w, l in zip(wants, labels) if l in ("at_floor", "al_eq_be"))
    for r, l in zip(rows, labels):
        if l == "clamp":
            assert abs((r[1] - r[0]) / (2 * r[2])) > 1e100
    x = sp.rcp_inputs()
    assert len(x) <= sp.MAX_ITEMS and {1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 8), 2.0, np.nextafter(2.0, 8), 4.0,
                                       np.nextafter(4.0, 0), 2.0 ** -500, 2.0 ** 500} <= set(x)
    assert x.min() < 0 and sp.rsq_inputs().min() > 0


def test_lm_inputs_hold_every_required_case():
    c = sp.lm_trial_census()
    print(c)
    assert {"rho_zero", "rho_nan", "not_ok", "temp_inf", "alpha_cross", "random"} <= set(c["labels"])
    assert c["rho_zero"] >= 6 and c["rho_nan"] >= 6 and c["accepted"] >= 32 and c["rejected"] >= 32
    assert min(c["below_third"], c["above_third"], c["below_two_thirds"], c["above_two_thirds"]) >= 2
    rows, labels = sp.lm_stop_inputs()
    ref = np.array([sp.lm_stop_ref(r) for r in rows])
    for nbad in (0.0, 1.0, 2.0):
        pick = lambda label: ref[[k for k, (r, l) in enumerate(zip(rows, labels)) if l == label and r[0] == nbad][0]]
        assert pick("gain_equal")[1] == 0 and pick("gain_above")[1] == 0 and pick("gain_below")[1] == nbad + 1
        assert pick("gain_below")[0] == (nbad == 2.0)
    assert {"qmax_9", "qmax_10", "rho_zero", "rho_nan"} <= set(labels)
    assert all(ref[k][0] == 1 for k, l in enumerate(labels) if l in ("qmax_10", "rho_zero"))


# --- the restatements against mpmath ---------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7])
def test_ldlt_restatement_against_the_exact_solve(n):
    ref = sp.ldlt_reference(n)
    worst, kmax = 0.0, 0.0
    for k, x, kappa in sp.ldlt_exact(n):
        worst, kmax = max(worst, sp.solve_error(ref[k][:n], x, kappa)), max(kmax, float(kappa))
    print(f"ldlt{n}: worst |x - x*| / (|x*| kappa) {worst:.3e}, kappa up to {kmax:.3e}")
    assert kmax <= 1e8 and worst <= sp.TOL[f"solve_ldlt{n}"]


def test_lu_restatement_against_the_exact_solve():
    ref = sp.lu3_reference()
    worst, kmax = 0.0, 0.0
    for k, x, kappa in sp.lu3_exact():
        worst, kmax = max(worst, sp.solve_error(ref[k], x, kappa)), max(kmax, float(kappa))
    print(f"lu3: worst {worst:.3e}, kappa up to {kmax:.3e}")
    assert kmax <= 1e8 and worst <= sp.TOL["solve_lu3"]


def _align(q, ref):
    return q if float(np.dot(q[:4], ref[:4])) >= 0 else np.concatenate([-q[:4], q[4:]])


def test_exp_and_log_restatements_against_the_closed_forms():
    with mpmath.workdps(sp.MP_DIGITS):
        U, es, labels, branch = sp.sim3_exp_inputs()
        ref, groups = sp.sim3_exp_reference(), sp.sim3_exp_groups()
        rows = sp.well_conditioned_exp(U, labels)
        assert len(rows) >= 32 and set(branch[rows]) == {1, 3}
        worst = 0.0
        for k in rows:
            exact = np.array(sp.mp_sim3_exp(U[k]))
            d = en.rel(exact, _align(ref[k], exact))
            worst = max(worst, d)
            assert d <= sp.TOL[groups[k]], (k, labels[k], d)
        print(f"sim3_exp against mpmath: {worst:.3e} over {len(rows)} rows")
        pose, U, labels, branch = sp.se3_inputs()
        ref, groups = sp.se3_reference(), sp.se3_groups()
        rows = sp.well_conditioned_exp(U, labels)
        assert len(rows) >= 8
        worst = 0.0
        for k in rows:
            e = np.array(sp.mp_sim3_exp(U[k]))
            # exp(u) * pose in float64 from the exact exponential: the product adds a few roundings of its own
            q = sp.qnormalize_ref(sp.so.quat_mul(e[:4], pose[k][:4]))
            exact = np.concatenate([q, e[4:7] + lb.quat_rotate(e[:4], pose[k][4:7])])
            d = en.rel(exact, _align(ref[k], exact))
            worst = max(worst, d)
            assert d <= max(sp.TOL[groups[k]], 16 * sp.EPS64), (k, labels[k], d)
            d = en.rel(ref[k], np.concatenate(lb.se3_oplus(pose[k][:4], pose[k][4:7], U[k])))
            assert d <= 1e-14                              # test_lba_numpy's form of the same update
        print(f"se3_oplus against mpmath: {worst:.3e} over {len(rows)} rows")
        S, labels = sp.sim3_log_inputs()
        L, branch = sp.sim3_log_reference()
        groups = sp.sim3_log_groups()
        rows = [k for k, l in enumerate(labels) if l in ("regular", "unnormalised") and branch[k] == 3 and abs(L[k][6]) >= 1e-3
                and 0.05 <= np.sqrt((L[k][:3] ** 2).sum()) <= 3.0]
        assert len(rows) >= 12
        worst = 0.0
        for k in rows:
            d = en.rel(np.array(sp.mp_sim3_log(S[k])), L[k])
            worst = max(worst, d)
            # an unnormalised quaternion scales g2o's rotation matrix by |q|^2: 1e-8 off is 2e-8 in the logarithm
            assert d <= (1e-7 if labels[k] == "unnormalised" else sp.TOL[groups[k]]), (k, labels[k], d)
        print(f"sim3_log against mpmath: {worst:.3e} over {len(rows)} rows")


def test_jacobi_restatements_against_mpmath():
    rows, labels = sp.jacobi_inputs()
    worst_t = worst_cs = 0.0
    with mpmath.workdps(sp.MP_DIGITS):
        for r, l in zip(rows, labels):
            if l == "nan" or r[2] == 0.0:
                continue
            c, s, t = sp.jacobi_cs_ref(*r[:3])
            assert np.isfinite([c, s, t]).all()
            worst_cs = max(worst_cs, abs(c * c + s * s - 1))
            ce, se, te, zeta = sp.mp_jacobi(*r[:3])
            if abs(zeta) < 1e99:                       # at zeta = 0 the roots +-1 are equally small: either sign
                worst_t = max(worst_t, float(abs((abs(t) if zeta == 0 else t) - te) / abs(te)))
    print(f"jacobi_cs restatement: t {worst_t:.3e}, c2 + s2 - 1 {worst_cs:.3e}")
    assert worst_t <= 1e-12 and worst_cs <= 16 * sp.EPS64
    for n in (3, 4):
        A, labels = sp.hestenes_inputs(n)
        for Ak, label, exact in zip(A, labels, sp.hestenes_exact(n)):
            a, v, sweeps = sp.hestenes_ref(Ak)
            if label == "nan":
                assert sweeps == 1 and np.array_equal(v, np.eye(n)) and sp.same_bytes(a, Ak.astype(F64).T)
                continue
            fig, wants = sp.hestenes_figures(Ak, a, v, exact[0])
            assert not wants and sweeps < sp.K_SWEEPS, label
            for q, val in fig.items():
                assert val <= sp.TOL[q], (label, q, val)
            if n == 4:
                figure, unit = sp.null_vector_figure(sp.null_select(a, v), *exact)
                assert figure <= sp.TOL["null4"] and unit <= 16 * sp.EPS64, (label, figure, unit)


def test_fused_restatement_is_the_correctly_rounded_fma():
    """sim3_numpy._fma rounds the FP64 sum to float; on the reprojection inputs
    that equals the float fma (no double rounding), which reproj_e2's contract
    mode relies on."""
    x = sp.reproj_inputs()
    f = x.astype(F32)
    with np.errstate(all="ignore"):
        invz = (1.0 / f[:, 6].astype(F64)).astype(F32)
        a, c = f[:, 0] * f[:, 4], f[:, 2]
        got = sp.sim3_numpy._fma(a, invz, c)
    ok = np.isfinite(got)
    assert ok.sum() >= 500 and np.array_equal(got[ok], sp.fma32_exact(a[ok], invz[ok], c[ok]))
    ref = sp.reproj_reference(x)
    assert np.isfinite(ref[5:]).all() and (ref[5:, 0] != ref[5:, 1]).any()       # the two modes differ somewhere


def test_the_measurement_behind_the_bars_reproduces():
    """MEASURED again: every figure is within its bar, and the recorded one is
    within the same factor of it (tests/test_essgraph_numpy.py's rule)."""
    got = sp.measure()
    for q in sp.MEASURED:
        print(f"{q}: measured {got[q]:.3e}, recorded {sp.MEASURED[q]:.3e}, bar {sp.TOL[q]:.3e}")
    for q in sp.MEASURED:
        assert got[q] <= sp.TOL[q] and sp.MEASURED[q] <= sp.FACTOR * got[q], q
    assert sp.FACTOR < 10 and set(got) == set(sp.MEASURED)


# --- the probe itself ----------------------------------------------------------------------------
def test_probe_cross_compiles_with_the_library_flags():
    cmd = sp.command()
    assert "-ffp-contract=off" in cmd and f"--offload-arch={sp.ARCH}" in cmd and "-shared" in cmd
    text = sp.SRC.read_text()
    for h in sp.HEADERS:
        assert (sp.CSRC / h).exists()
    for name, (ni, no) in sp.PROBES.items():
        assert f"PROBE({name}, {ni}, {no})" in text
    lib = sp.load()                                        # builds when the source or a header is newer
    assert sp.LIB.exists() and all(hasattr(lib, "probe_" + name) for name in sp.PROBES)
