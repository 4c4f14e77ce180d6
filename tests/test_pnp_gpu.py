"""orbx_pnp_ransac on the device against the numpy restatement
(tests/pnp_numpy.py), in two layers.

Layer 1, byte for byte.  The restatement is fed the device's decomposition
taps (FP64, as the device computed them: the 3x3 eigenvectors and values,
CC_inv, rows 8..11 of Ut, the three cvSolve results, U and V of ABt, of every
minimal solve and every refit).  Given those, the correspondences, the sets,
L_6x10, rho, the betas after gauss_newton, R, t, the three reprojection
errors and the choice of every iteration the call could run, the counts, the
record holders, every refit, and every output and state field of the call
must be the device's bytes (NaNs equal NaNs), in both contraction modes.

Layer 2.  Each decomposition tap on its own, by properties that do not depend
on a basis: orthonormality, the residual of the factorisation, the order, the
null residual of rows 8..11 and the distance of their projector to
np.linalg.eigh's where the spectrum has a gap, the least-squares solutions
against np.linalg.lstsq where the matrix is well conditioned.  The bound of
each figure is 8 x np.linalg's own figure on the same matrices (both are a
few round-offs, neither is exact); a test prints what it measured.
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import pnp_numpy as pn

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=2)
    yield c
    c.close()


def canon(a):
    """Bytes of a float array with every NaN as one pattern."""
    a = np.array(a)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a.tobytes()


def records_of(dev):
    r = {("it", i): dev["rec"][i] for i in range(len(dev["rec"]))}
    r.update({("refit", s): dev["refit_rec"][s] for s in range(len(dev["refit_rec"]))})
    return r


STATE = ("iter_done", "best_inliers")
OUT_INTS = ("N", "ransac_min_inliers", "ransac_max_its", "iters_run", "no_more", "found", "found_iter", "n_inliers",
            "refined", "best_slot") + STATE


def same_call(dev, want):
    """The out and state fields of one call."""
    for k in OUT_INTS:
        assert dev[k] == want[k], (k, dev[k], want[k])
    assert (dev["Tcw"] is None) == (want["Tcw"] is None)
    if want["Tcw"] is not None:
        assert canon(dev["Tcw"]) == canon(want["Tcw"])
    assert dev["inliers"].tobytes() == want["inliers"].tobytes()
    assert dev["best_mask"].tobytes() == want["best_mask"].tobytes()
    assert canon(dev["best_Tcw"]) == canon(want["best_Tcw"])


def layer1(dev, sc, draws, params, state=None, contract=False, logs=None):
    """The bit-exact layer of one device result (with taps).  Returns the
    restatement's call."""
    draws = np.asarray(draws).reshape(-1, 4)
    dec = pn.TapDecomp(records_of(dev))
    s = pn.solver_of(sc, params, dec, contract, state)
    c = s.c
    assert dev["N"] == c["N"]
    assert dev["kp_index"].tobytes() == c["kp_index"].tobytes()
    for k in ("p2d", "p3d", "max_err"):
        assert canon(dev[k]) == canon(c[k]), k
    iter_done = 0 if state is None else state["iter_done"]
    best_in = 0 if state is None else state["best_inliers"]
    run = c["N"] >= s.min_inliers
    E = max(params["n_iter"], s.max_its - iter_done) if run else 0
    assert E <= len(draws)
    # every iteration the call could run
    counts, masks = [], []
    for it in range(E):
        st = pn.draw_set(c["N"], draws[it])
        assert dev["sets"][it].tolist() == st, it
        dec.begin(("it", it))
        log = None
        if logs is not None:
            log = {}
            logs[("it", it)] = log
        rec = pn.compute_pose(c["p3d"][st].astype(np.float64), c["p2d"][st].astype(np.float64), s.epnp_cam, dec, log)
        assert canon(rec) == canon(dev["rec"][it]), (it, np.flatnonzero(~((rec == dev["rec"][it]) | (np.isnan(rec) & np.isnan(dev["rec"][it])))))
        n, m = pn.check_inliers(c, s.cam, rec[pn.O_R:pn.O_R + 9], rec[pn.O_T:pn.O_T + 3], contract)
        assert dev["count"][it] == n, it
        counts.append(n)
        masks.append(m)
    assert not dev["sets"][E:].any() and not dev["count"][E:].any() and not dev["rec"][E:].any()
    # the strict record holders and every refit
    best, holders = best_in, []
    for it in range(E):
        if counts[it] >= s.min_inliers and counts[it] > best:
            best = counts[it]
            holders.append(it)
    assert dev["n_records"] == len(holders)
    assert dev["record_iter"][1:1 + len(holders)].tolist() == holders
    slots = [(k + 1, masks[it]) for k, it in enumerate(holders)]
    if best_in > 0 and run:
        slots.insert(0, (0, np.asarray(state["best_mask"])[c["kp_index"]] != 0))
    for slot, m in slots:
        dec.begin(("refit", slot))
        log = None
        if logs is not None:
            log = {}
            logs[("refit", slot)] = log
        idx = np.flatnonzero(m)
        rec = pn.compute_pose(c["p3d"][idx].astype(np.float64), c["p2d"][idx].astype(np.float64), s.epnp_cam, dec, log)
        assert canon(rec) == canon(dev["refit_rec"][slot]), slot
        n, _ = pn.check_inliers(c, s.cam, rec[pn.O_R:pn.O_R + 9], rec[pn.O_T:pn.O_T + 3], contract)
        assert dev["refit_count"][slot] == n, slot
    # the call, as the sequential loop replays it
    want = s.iterate(params["n_iter"], draws)
    same_call(dev, want)
    return want


def run_case(ctx, sc, draws, params, state=None, contract=False, logs=None):
    dev = ctx.pnp_ransac(pn.frame_of(sc), draws, taps=True, state=state, **params)
    return dev, layer1(dev, sc, draws, params, state, contract, logs)


@pytest.mark.parametrize("i", range(len(pn.CASES)), ids=[f"N{c[0]}-it{c[1]}" for c in pn.CASES])
def test_ransac_against_the_restatement(ctx, i):
    sc, d, params = pn.case(i)
    N, T = pn.CASES[i]
    dev, want = run_case(ctx, sc, d, params)
    assert dev["N"] == N and not sc["valid"].all()
    if N == 9:
        assert dev["no_more"] == 1 and dev["iters_run"] == 0 and dev["found"] == 0
    print(f"N={N} T={T}: iters_run={dev['iters_run']} found={dev['found']} refined={dev['refined']} "
          f"inliers={dev['n_inliers']} records={dev['n_records']}")


def test_several_record_holders_occur(ctx):
    """The scenes are noisy enough that the device lists more than one
    record holder in at least a few of the cases (their refits are all
    compared above)."""
    several = 0
    for i, (N, T) in enumerate(pn.CASES):
        if N >= 63 and T >= 35:
            sc, d, params = pn.case(i)
            several += ctx.pnp_ransac(pn.frame_of(sc), d, **params)["n_records"] > 1
    assert several >= 3, several


@pytest.mark.parametrize("seed", range(8))
def test_noise_free_scene_returns_the_ground_truth(ctx, seed):
    """The scenes and bounds of tests/test_pnp_numpy.py on the device, with
    the device's own null-space bases: the call returns from a set without
    an unrelated partner, the first iteration that reaches min_inliers, with
    the ground-truth pose and every true correspondence as an inlier."""
    from test_pnp_numpy import TOL_R, TOL_T
    sc = pn.scene(60, seed=40 + seed, noise=0.0, outliers=0.3)
    dev = ctx.pnp_ransac(pn.frame_of(sc), pn.draws_for(40 + seed, 300), taps=True, **dict(pn.RELOC, n_iter=5))
    assert dev["found"] and dev["refined"]
    good = np.ones(len(sc["keys"]), bool)
    good[sc["bad"]] = False
    it = dev["found_iter"]
    assert all(good[dev["kp_index"][i]] for i in dev["sets"][it]) and len(set(dev["sets"][it].tolist())) == 4
    assert dev["count"][it] >= dev["ransac_min_inliers"] and (dev["count"][:it] < dev["ransac_min_inliers"]).all()
    T = dev["Tcw"].reshape(4, 4).astype(np.float64)
    eR, et = np.abs(T[:3, :3] - sc["R"]).max(), np.abs(T[:3, 3] - sc["t"]).max()
    print(f"seed {seed}: returned at {it}, |dR| {eR:.2e} |dt| {et:.2e}")
    assert eR <= TOL_R and et <= TOL_T
    assert dev["n_inliers"] == int(good[dev["kp_index"]].sum())


def test_more_than_one_check_tile(ctx):
    sc = pn.scene(1030, seed=7, noise=0.5)
    d = pn.draws_for(7, 12)
    run_case(ctx, sc, d, dict(pn.RELOC, max_iterations=12, n_iter=12))


def test_refit_of_a_large_set(ctx):
    """A refit of more points than the 64 lanes of the refine workgroup
    compact at once, and of more than one check tile."""
    sc = pn.scene(1100, seed=8, noise=0.2, outliers=0.05)
    d = pn.draws_for(8, 8)
    dev, _ = run_case(ctx, sc, d, dict(pn.RELOC, max_iterations=8, n_iter=8))
    assert dev["found"] and dev["refined"] and dev["n_inliers"] > 1024


def test_min_inliers_4_refits_of_4_and_5_points(ctx):
    """min_inliers down at 4: refits of four and of five inliers."""
    seen = set()
    for seed in range(12):
        sc = pn.scene(12, seed=300 + seed, noise=0.3, outliers=0.6)
        d = pn.draws_for(300 + seed, 40)
        params = dict(pn.RELOC, min_inliers=4, epsilon=0.1, max_iterations=40, n_iter=40)
        dev, _ = run_case(ctx, sc, d, params)
        for s in range(1, dev["n_records"] + 1):
            seen.add(int(dev["refit_rec"][s][pn.O_NPTS]))
        if {4, 5} <= seen:
            break
    assert {4, 5} <= seen, seen


def test_fp_contract_mode(ctx):
    sc, d, params = pn.case(pn.CASES.index((65, 35)))
    try:
        ctx.set_fp_contract(1)
        run_case(ctx, sc, d, params, contract=True)
    finally:
        ctx.set_fp_contract(0)
    run_case(ctx, sc, d, params, contract=False)
    # more than one check tile, and a refit of more than a thousand points
    sc = pn.scene(1030, seed=7, noise=0.5)
    d = pn.draws_for(7, 6)
    try:
        ctx.set_fp_contract(1)
        run_case(ctx, sc, d, dict(pn.RELOC, max_iterations=6, n_iter=6), contract=True)
    finally:
        ctx.set_fp_contract(0)


def test_resumption_as_relocalisation_drives_it(ctx):
    """Call, take the returned pose, call again with the out state and the
    following draws, until no_more: the restatement's successive iterate(5)
    calls, field for field."""
    sc = pn.scene(100, seed=5, noise=0.5)
    params = dict(pn.RELOC, n_iter=5)
    d = pn.draws_for(5, 2048)
    ref = pn.solver_of(sc, params)       # one object through all calls: its state is the reference's members
    state, o, calls, returned = None, 0, 0, 0
    while True:
        dd = d[o:o + 300]
        dev = ctx.pnp_ransac(pn.frame_of(sc), dd, taps=True, state=state, **params)
        layer1(dev, sc, dd, params, state)
        ref.decomp = pn.TapDecomp(records_of(dev))
        same_call(dev, ref.iterate(5, dd))
        state = dev
        o += dev["iters_run"]
        calls += 1
        returned += dev["found"]
        if dev["no_more"]:
            break
        assert calls < 200
    assert calls > 2 and returned >= 2
    print(f"{calls} calls, {returned} returned a pose, {o} iterations")


def test_batch_equals_single_calls(ctx):
    picks = [pn.CASES.index(c) for c in ((9, 5), (11, 35), (64, 64), (300, 35), (65, 300))]
    qs = [pn.case(i) for i in picks]
    singles = [ctx.pnp_ransac(pn.frame_of(sc), d, taps=True, **p) for sc, d, p in qs]
    batch = ctx.pnp_ransac_batch([(pn.frame_of(sc), d, p) for sc, d, p in qs], taps=True)
    for a, b in zip(singles, batch):
        same_call(a, b)
        for k in ("sets", "count", "rec", "refit_rec", "refit_count", "record_iter", "p2d", "p3d", "max_err", "kp_index"):
            assert canon(a[k]) == canon(b[k]), k


def forced_draws(N, sets):
    """rand() values that make draw_set return the given picks (as values of
    RandomInt, before the quirk's remapping)."""
    out = np.zeros((len(sets), 4), np.int32)
    for r, s in enumerate(sets):
        for j, v in enumerate(s):
            size = N - j
            x = int(np.ceil(v * 2147483648.0 / size))
            while int((float(x) / 2147483648.0) * size) < v:
                x += 1
            assert int((float(x) / 2147483648.0) * size) == v
            out[r, j] = x
    return out


def test_forced_degenerate_sets(ctx):
    """A repeated correspondence, four coplanar and four collinear points:
    the outputs equal the restatement fed the taps (NaNs equal NaNs), and
    the neighbouring iterations are what they are without them."""
    sc = pn.scene(40, seed=11, noise=0.3)
    good = np.flatnonzero(sc["valid"])
    R, t = sc["R"], sc["t"]

    def place(k, Xc):
        i = good[k]
        sc["pos"][i] = ((Xc - t) @ R).astype(np.float32)
        sc["keys"]["x"][i] = pn.CAM[0] * Xc[0] / Xc[2] + pn.CAM[2]
        sc["keys"]["y"][i] = pn.CAM[1] * Xc[1] / Xc[2] + pn.CAM[3]
    for k, Xc in enumerate([(-1, -1, 4.0), (1, -1, 4.0), (1, 1, 4.0), (-1, 1, 4.0)]):      # coplanar
        place(k, np.array(Xc))
    for k, a in enumerate((0.0, 0.3, 0.7, 1.0)):                                           # collinear
        place(4 + k, np.array([-1.0, 0.5, 3.0]) + a * np.array([2.0, -1.0, 2.0]))
    N = len(good)
    # drawing place 1 three times: the first removal writes N - 1 at place 1 (value
    # and place still agree), the second writes at the drawn value N - 1, past the
    # live part, so place 1 still holds N - 1 for the third pick
    assert pn.draw_set(N, forced_draws(N, [(1, 1, 1, 2)])[0]) == [1, N - 1, N - 1, 2]
    plain = pn.draws_for(11, 6)
    special = np.array(plain)
    special[1] = forced_draws(N, [(1, 1, 1, 2)])[0]
    special[2] = forced_draws(N, [(0, 1, 2, 3)])[0]
    special[4] = forced_draws(N, [(4, 5, 6, 7)])[0]
    params = dict(pn.RELOC, min_inliers=N, epsilon=1.0, max_iterations=6, n_iter=6)   # never returns: all six run
    a = ctx.pnp_ransac(pn.frame_of(sc), plain, taps=True, **params)
    b = ctx.pnp_ransac(pn.frame_of(sc), special, taps=True, **params)
    layer1(b, sc, special, params)
    assert len(set(b["sets"][1].tolist())) < 4
    assert b["sets"][2].tolist() == [0, 1, 2, 3] and b["sets"][4].tolist() == [4, 5, 6, 7]
    for it in (0, 3, 5):
        assert canon(a["rec"][it]) == canon(b["rec"][it]) and a["count"][it] == b["count"][it], it
    print("degenerate counts", b["count"][:6].tolist(), "chosen", b["rec"][:6, pn.O_CHOSEN].tolist())


def test_argument_rules_and_the_timer(ctx):
    sc, d, params = pn.case(pn.CASES.index((11, 5)))
    f = pn.frame_of(sc)

    def code(frame=f, draws=d, **kw):
        p = dict(params)
        p.update(kw)
        try:
            ctx.pnp_ransac(frame, draws, **p)
        except ox.OrbxError as e:
            return e.code
        return 0
    assert code() == 0
    assert code(min_set=5) == ERR_UNSUPPORTED and code(min_set=3) == ERR_UNSUPPORTED
    assert code(draws=d[:4]) == ERR_ARG                       # n_draws < max(n_iter, max_iterations - iter_done)
    assert code(draws=pn.draws_for(0, 1025), n_iter=1025, max_iterations=1025) == ERR_ARG
    bad = np.array(d)
    bad[2, 1] = -1
    assert code(draws=bad) == ERR_ARG
    assert code(probability=1.0) == ERR_ARG and code(probability=0.0) == ERR_ARG
    assert code(n_iter=0) == ERR_ARG and code(max_iterations=0) == ERR_ARG and code(min_inliers=0) == ERR_ARG
    assert code(epsilon=1.5) == ERR_ARG and code(th2=0.0) == ERR_ARG
    g = dict(f, keys=f["keys"].copy())
    g["keys"]["octave"][3] = len(f["sigma2"])
    assert code(frame=g) == ERR_ARG
    g = dict(f, sigma2=-f["sigma2"])
    assert code(frame=g) == ERR_ARG
    q, keep = ox.pnp_query(f, d, **params)
    q.cap = q.n - 1
    assert ox.lib().orbx_pnp_ransac(ctx._h, ctypes.byref(q)) == ERR_CAPACITY
    big = pn.scene(4097 - 7, seed=1)
    assert code(frame=pn.frame_of(big)) == ERR_UNSUPPORTED
    # one "pnp" region per call, each part once in it
    try:
        for name in ("pnp", "pnp.prepare", "pnp.solve", "pnp.check", "pnp.refine"):
            ctx.timing(True, only=name)
            before = ctx.kernel_time(name)[0]
            ctx.pnp_ransac(f, d, **params)
            ctx.pnp_ransac_batch([(f, d, params), (f, d, params)])
            n, avg, tot = ctx.kernel_time(name)
            assert n - before == 2 and tot > 0, name
    finally:
        ctx.timing(False)


# ---------------------------------------------------------------------------
# layer 2
# ---------------------------------------------------------------------------
def fro(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


class Worst:
    """Worst figures of the device and of np.linalg per property.  A figure
    that is not finite is an error: a NaN must not hide in a maximum."""

    def __init__(self):
        self.dev, self.ref, self.skipped, self.total = {}, {}, {}, {}

    def add(self, name, dev, ref):
        assert np.isfinite(dev) and np.isfinite(ref), (name, dev, ref)
        self.dev[name] = max(self.dev.get(name, 0.0), float(dev))
        self.ref[name] = max(self.ref.get(name, 0.0), float(ref))

    def cut(self, name, skipped):
        self.total[name] = self.total.get(name, 0) + 1
        self.skipped[name] = self.skipped.get(name, 0) + bool(skipped)

    def check(self):
        for k in sorted(self.dev):
            print(f"layer2 {k}: device {self.dev[k]:.3e}  np.linalg {self.ref[k]:.3e}")
        for k in sorted(self.total):
            print(f"layer2 {k}: left out {self.skipped[k]} of {self.total[k]}")
            assert self.skipped[k] <= 0.05 * self.total[k], k
        for k in self.dev:
            assert self.dev[k] <= 8 * self.ref[k], (k, self.dev[k], self.ref[k])


def usable(A):
    return A is not None and bool(np.isfinite(A).all()) and fro(A) > 0


def layer2(w, d, log, minimal):
    """The decomposition taps d (ORBX_PNP_DEC doubles) of one hypothesis
    against the matrices `log` that were decomposed.  Every tap of a finite,
    non-zero matrix must be finite."""
    ref = pn.NumpyDecomp()
    I3 = np.eye(3)
    # the symmetric 3x3
    G = log["G3"]
    assert usable(G)
    dc, U = d[0:3], d[3:12].reshape(3, 3)
    assert np.isfinite(dc).all() and np.isfinite(U).all()
    assert dc[0] >= dc[1] >= dc[2] >= 0
    dr, Ur = ref.eig_sym(G, 3)
    w.add("eig3 orthonormality", fro(U @ U.T - I3), fro(Ur @ Ur.T - I3))
    w.add("eig3 residual", fro(G - U.T @ np.diag(dc) @ U) / fro(G), fro(G - Ur.T @ np.diag(dr) @ Ur) / fro(G))
    # CC_inv: the pseudo-inverse's defining residual, where cc is well conditioned
    cc = log["cc"]
    assert usable(cc)
    ci = d[12:21].reshape(3, 3)
    assert np.isfinite(ci).all()
    cond = np.linalg.cond(cc)
    w.cut("cc_inv", not cond < 1e8)
    if cond < 1e8:
        w.add("cc_inv residual", fro(cc @ ci - I3), fro(cc @ ref.pinv3(cc) - I3))
    # rows 8..11 of Ut
    M = log["MtM"]
    assert usable(M)
    V = d[21:69].reshape(4, 12)
    assert np.isfinite(V).all()
    lam, Q = np.linalg.eigh(M)
    Vr = Q[:, 3::-1].T                       # the four smallest, descending like rows 8..11
    w.add("ut orthonormality", fro(V @ V.T - np.eye(4)), fro(Vr @ Vr.T - np.eye(4)))
    if minimal:          # an exact null space before rounding: the residual is that of the Gram matrix itself
        w.add("ut null residual (minimal sets)", fro(M @ V.T) / fro(M), fro(M @ Vr.T) / fro(M))
    # eigenvalues descending: the Rayleigh quotients of rows 8..11 do not increase.  Two rows count as separated
    # when their quotients differ by more than 100 eps |MtM|_F: a quotient of unit vectors carries a round-off of
    # about 12 eps |MtM|_F from the product alone, and the device orders by diagonal entries that a few sweeps of
    # rotations have touched, so differences below that are not an order.
    q = np.array([V[k] @ M @ V[k] for k in range(4)])
    sep = 100 * EPS * fro(M)
    for k in range(3):
        separated = abs(q[k] - q[k + 1]) > sep
        if not minimal:      # a refit has no exact null space: there the order defines v[0..3]
            w.cut("order of a refit's rows", not separated)
        if separated:
            assert q[k] > q[k + 1], (q, sep)
    gap = (lam[4] - lam[3]) / lam[-1]
    w.cut("projector", not gap >= 1e-4)
    if gap >= 1e-4:
        # Davis-Kahan: |P1 - P2| <= (r1 + r2) / gap, r the residuals |M V - V (V^T M V)|
        def res(X):
            return fro(M @ X.T - X.T @ (X @ M @ X.T)) / lam[-1]
        w.add("ut projector distance", fro(V.T @ V - Vr.T @ Vr), (res(V) + res(Vr)) / gap)
    # the three least-squares solutions
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}
    for which, (o, k) in {1: (69, 4), 2: (73, 3), 3: (76, 5)}.items():
        A, b = log["L"][:, cols[which]], log["rho"]
        assert usable(A) and np.isfinite(b).all()
        x = d[o:o + k]
        assert np.isfinite(x).all(), which
        cond = np.linalg.cond(A)
        w.cut("lstsq", not cond < 1e8)
        if cond < 1e8:
            xr = np.linalg.lstsq(A, b, rcond=None)[0]

            def normal(z):
                return fro(A.T @ (A @ z - b)) / (fro(A) * (fro(A) * fro(z) + fro(b)))
            w.add("lstsq normal-equation residual", normal(x), normal(xr))
    # U and V of ABt
    assert len(log["abt"]) == 3
    for which in (1, 2, 3):
        A = log["abt"][which - 1]
        if not usable(A):          # a beta set that ended in NaNs upstream (its betas are compared in layer 1)
            w.cut("abt", True)
            continue
        w.cut("abt", False)
        o = 81 + 18 * (which - 1)
        U, V = d[o:o + 9].reshape(3, 3), d[o + 9:o + 18].reshape(3, 3)
        assert np.isfinite(U).all() and np.isfinite(V).all(), which
        Ur, Vr = ref.svd3(A, which)

        def offdiag(U_, V_):
            D = U_.T @ A @ V_
            return fro(D - np.diag(np.diag(D))) / fro(A)
        w.add("abt orthonormality", max(fro(U.T @ U - I3), fro(V.T @ V - I3)), max(fro(Ur.T @ Ur - I3), fro(Vr.T @ Vr - I3)))
        w.add("abt off-diagonal", offdiag(U, V), offdiag(Ur, Vr))


@pytest.mark.parametrize("N,T", [(11, 35), (65, 64), (300, 65)])
def test_decompositions_on_their_own(ctx, N, T):
    sc, d, params = pn.case(pn.CASES.index((N, T)))
    logs = {}
    dev, _ = run_case(ctx, sc, d, params, logs=logs)
    w = Worst()
    for key, log in logs.items():
        if "MtM" not in log:
            continue
        rec = dev["rec"][key[1]] if key[0] == "it" else dev["refit_rec"][key[1]]
        layer2(w, rec[:pn.DEC], log, minimal=key[0] == "it")
    w.check()


# ---------------------------------------------------------------------------
# device-resident frame
# ---------------------------------------------------------------------------
W, H, NF = 640, 480, 1000
SLOT_CAM = np.array([520.0, 520.0, 320.0, 240.0], np.float32)


def test_slot_form_equals_search_then_batch():
    from orb_slam_amd import synth
    from test_dev_bow_gpu import create_vocab, level_sigma2, read_bow, view
    from vocab_data import make_vocab
    c = ox.Context(nfeatures=NF, max_w=W, max_h=H, slots=4)
    voc = None
    try:
        c.upload(np.stack(synth.sequence(W, H, 4, seed=23)), 0)
        c.extract(0, 4)
        c.sync()
        voc = create_vocab(c, make_vocab(k=10, L=4, seed=3))
        assert ox.lib().orbx_dev_compute_bow(c.handle, voc, 0, 4, 2) == 0
        feats = [c.features(s) for s in range(4)]
        fk = feats[0][0]
        n1 = len(fk)
        rng = np.random.default_rng(5)
        sigma2 = level_sigma2()
        views, keep, mps = [], [], []
        for s in (1, 2, 3):
            kk, kd = feats[s]
            mp = rng.choice(3, len(kk), p=(0.1, 0.8, 0.1)).astype(np.uint8)
            if s == 3:
                mp[12:] = 0                      # a candidate with few map points: below min_matches
            v, a = view(kk, kd, mp, read_bow(c, s, len(kk)))
            views.append(v)
            keep.append(a)
            mps.append(mp)
        m_f, nm = c.search_by_bow(0, views)
        # map points that make the matches a scene: the frame's pose is the identity
        pos = []
        for k in range(3):
            p = rng.normal(size=(views[k].n, 3)).astype(np.float32) + np.float32([0, 0, 5])
            i = np.flatnonzero(m_f[k][:n1] >= 0)
            z = rng.uniform(3.0, 8.0, len(i))
            good = np.stack([(fk["x"][i] - SLOT_CAM[2]) / SLOT_CAM[0] * z, (fk["y"][i] - SLOT_CAM[3]) / SLOT_CAM[1] * z, z], 1)
            ok = rng.random(len(i)) > 0.2
            p[m_f[k][i][ok]] = good[ok]
            pos.append(p)
        draws = [pn.draws_for(40 + k, 300) for k in range(3)]
        par = dict(pn.RELOC, n_iter=5)
        c.timing(True, only="pnp")
        dev = c.dev_pnp_candidates(0, views, pos, SLOT_CAM, sigma2, draws, min_matches=15, taps=True, **par)
        assert c.kernel_time("pnp")[0] == 1
        c.timing(False)
        print(f"n1 {n1}, matches {nm.tolist()}, discarded {dev['discarded'].tolist()}, "
              f"N {[x['N'] for x in dev['results']]}, found {[x['found'] for x in dev['results']]}")
        assert dev["n_matches"].tolist() == nm.tolist()
        assert dev["discarded"].tolist() == [int(x < 15) for x in nm] and dev["discarded"][2] == 1 and nm[0] >= 15
        qs = []
        for k in range(3):
            assert dev["matches_f"][k].tobytes() == m_f[k].tobytes()
            m = m_f[k][:n1]
            valid = (m >= 0).astype(np.uint8)
            valid[m >= 0] = mps[k][m[m >= 0]] == 1
            assert valid.sum() == nm[k]
            qs.append((dict(keys=fk, pos=pos[k][np.maximum(m, 0)], valid=valid, cam=SLOT_CAM, sigma2=sigma2), draws[k], par))
        host = c.pnp_ransac_batch(qs, taps=True)
        assert host[0]["found"] and host[0]["refined"]
        for k in range(3):
            d = dev["results"][k]
            if dev["discarded"][k]:
                assert d["N"] == 0 and not d["found"] and d["iters_run"] == 0 and not d["no_more"]
                assert not d["count"].any() and not d["inliers"].any()
                continue
            assert not d["inliers"][n1:].any() and not d["best_mask"][n1:].any()
            d = dict(d, inliers=d["inliers"][:n1], best_mask=d["best_mask"][:n1])
            same_call(d, host[k])
            for key in ("sets", "count", "rec", "refit_rec", "refit_count", "record_iter", "p2d", "p3d", "max_err",
                        "kp_index"):
                assert canon(d[key]) == canon(host[k][key]), key
        # the candidates resumed from the state the first call left (its pose, say, failed PoseOptimization):
        # the incoming mask is uploaded per candidate and refitted through the match vector
        states = dev["results"]
        draws2 = [draws[k][states[k]["iters_run"]:] for k in range(3)]
        dev2 = c.dev_pnp_candidates(0, views, pos, SLOT_CAM, sigma2, draws2, min_matches=15, states=states, taps=True, **par)
        host2 = c.pnp_ransac_batch([(qs[k][0], draws2[k], dict(par, state=dict(host[k]))) for k in range(3)], taps=True)
        resumed = 0
        for k in range(3):
            if dev2["discarded"][k]:
                continue
            d = dev2["results"][k]
            assert not d["inliers"][n1:].any() and not d["best_mask"][n1:].any()
            d = dict(d, inliers=d["inliers"][:n1], best_mask=d["best_mask"][:n1])
            same_call(d, host2[k])
            for key in ("sets", "count", "rec", "refit_rec", "refit_count", "record_iter"):
                assert canon(d[key]) == canon(host2[k][key]), key
            assert d["iter_done"] > states[k]["iter_done"] > 0
            resumed += int(d["refit_rec"][0][pn.O_NPTS] > 0)      # slot 0: the incoming set was refitted
        assert resumed >= 1
    finally:
        if voc:
            ox.lib().orbx_vocab_destroy(voc)
        c.close()


def test_batch_of_packed_lengths_in_either_order(ctx):
    """Three candidates in one batch whose arrays have 17, 0 and 31 entries
    (draws included): nothing but the 16-byte draws is a multiple of the
    packing step and an empty candidate lies between the others; the first
    asks for taps, the others do not.  Every result is the single call's, the
    tapped one passes layer 1, in either order."""
    scs = [pn.scene(10, seed=40), None, pn.scene(24, seed=41)]
    scs[1] = {k: (v[:0] if k in ("keys", "pos", "valid") else v) for k, v in pn.frame_of(scs[0]).items()}
    assert [len(s["keys"]) for s in scs] == [17, 0, 31]
    T = (17, 1, 31)
    draws = [pn.draws_for(50 + k, T[k]) for k in range(3)]
    params = [dict(pn.RELOC, max_iterations=T[k], n_iter=T[k]) for k in range(3)]
    taps = (True, False, False)
    frames = [pn.frame_of(s) if "R" in s else s for s in scs]
    single = [ctx.pnp_ransac(frames[k], draws[k], taps=taps[k], **params[k]) for k in range(3)]
    assert [r["N"] for r in single] == [10, 0, 24]
    for order in ((0, 1, 2), (2, 1, 0)):
        built = [ox.pnp_query(frames[k], draws[k], taps=taps[k], **params[k]) for k in order]
        arr = (ox.PnpQuery * 3)(*[b[0] for b in built])
        assert ox.lib().orbx_pnp_ransac_batch(ctx.handle, 3, arr) == 0
        for pos, k in enumerate(order):
            r = ox.pnp_result(arr[pos], built[pos][1], taps[k])
            same_call(r, single[k])
            if taps[k]:
                for name in ("sets", "count", "rec", "refit_rec", "refit_count", "record_iter", "p2d", "p3d", "max_err",
                             "kp_index"):
                    assert canon(r[name]) == canon(single[k][name]), name
                layer1(r, scs[k], draws[k], params[k])
            if k == 1:
                assert r["no_more"] == 1 and r["iters_run"] == 0 and not r["found"]
