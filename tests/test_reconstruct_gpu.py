"""orbx_init_reconstruct on the device against the numpy restatement
(tests/reconstruct_numpy.py), in two layers.

Layer 1, byte for byte: fed the device's own decompositions (the svd and v4
taps) the restatement must give the device's ok, n_hyp, best, R21, t21,
n_good, R_all, t_all, cos_parallax, p3d and triangulated.  parallax goes
through acos and must be within one float32 ulp of the restatement's; ok (and
what hangs on it) is compared whenever no hypothesis' parallax is within that
ulp of min_parallax.  NaNs compare equal to NaNs.

Layer 2, the two decompositions against np.linalg.svd in float64 wherever the
relative singular gaps are at least 1e-4, within one float32 ulp of the
compared matrix's largest entry after aligning the unspecified signs: U, w, Vt
for the homography; for the essential matrix, whose two leading singular
values coincide, t, the leading pair after aligning its rotation, and the
products U W Vt, U Wt Vt (at the bound the rounding of the tap implies); the
4x4 null vectors as tests/test_newpoints_gpu.py compares them.
"""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import reconstruct_numpy as rn

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4
GOLDEN = Path(__file__).resolve().parent / "golden" / "init_reconstruct.npz"
F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=6)
    yield c
    c.close()


def canon(a):
    """Bytes of a float32 array with every NaN as one pattern."""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def within_one_ulp(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        near = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))
    return bool(np.all(both_nan | near))


def assert_layer1(dev, args, contract=0, **kw):
    """The restatement fed the device's decompositions gives the device's
    bytes.  Returns the restatement's result."""
    r = rn.reconstruct(*args, svd=dev["svd"], v4=dev["v4"] if dev["n_hyp"] else None, contract=contract, **kw)
    nh = r["n_hyp"]
    assert dev["n_hyp"] == nh and dev["n_inliers"] == r["n_inliers"]
    assert canon(dev["R_all"]) == canon(r["R_all"]) and canon(dev["t_all"]) == canon(r["t_all"])
    assert dev["n_good"].tobytes() == r["n_good"].tobytes(), (dev["n_good"], r["n_good"])
    assert dev["cos_parallax"].shape == r["cos_parallax"].shape
    assert canon(dev["cos_parallax"]) == canon(r["cos_parallax"])
    print(f"parallax: device {dev['parallax'][:nh].tolist()} restatement {r['parallax'][:nh].tolist()}")
    assert within_one_ulp(dev["parallax"], r["parallax"])
    assert not dev["parallax"][nh:].any() and not dev["n_good"][nh:].any()
    inl = np.asarray(args[3][:r["N"]]).astype(bool)
    if nh:
        assert not dev["v4"][:, ~inl].any() and np.isnan(dev["cos_parallax"][:, ~inl]).all()
    min_par = F32(kw.get("min_parallax", 1.0))
    par = r["parallax"][:nh]
    with np.errstate(all="ignore"):
        decided = bool(np.all(~(np.abs(par.astype(np.float64) - np.float64(min_par)) <= np.spacing(np.abs(par)))))
    if decided:
        assert dev["ok"] == r["ok"] and dev["best"] == r["best"]
        assert dev["p3d"].tobytes() == r["p3d"].tobytes()
        assert dev["triangulated"].tobytes() == r["triangulated"].tobytes()
        if r["ok"]:
            assert dev["R21"].tobytes() == r["R21"].tobytes() and dev["t21"].tobytes() == r["t21"].tobytes()
        else:
            assert dev["R21"] is None and dev["best"] == -1
    if not dev["ok"]:
        assert not dev["p3d"].any() and not dev["triangulated"].any()
    # unmatched and non-inlier keypoints
    m = np.asarray(args[2])
    touched = np.zeros(len(m), bool)
    touched[r["pairs"][inl, 0]] = True
    assert not dev["p3d"][~touched].any() and not dev["triangulated"][~touched].any()
    return r


@pytest.mark.parametrize("name", sorted(rn.CASES))
def test_layer1_cases_bit_for_bit(ctx, name):
    """Both models, an accepted and every rejected branch of each, N = 64,
    65, 256, 257 (a wave, a workgroup) and 300, n1 > N throughout."""
    a, ref = rn.case(name)
    assert len(a[0]) > ref["N"] and (a[2] < 0).any()
    dev = ctx.init_reconstruct(*a[:7], taps=True, **a[8])
    r = assert_layer1(dev, a[:7], **a[8])
    assert dev["ok"] == rn.CASES[name]["ok"] == r["ok"]


@pytest.mark.parametrize("want", [1, 50, 51, 52])
@pytest.mark.parametrize("name", ["F-300", "H-300"])
def test_layer1_min_50_clamp(ctx, name, want):
    """A subset of inlier flags that makes the winner's nGood 1, 50, 51 and
    52: the index min(50, size - 1) of the sorted cosines."""
    a, _ = rn.case(name)
    inl = rn.inliers_for_n_good(name, want)
    args = a[:3] + (inl,) + a[4:7]
    dev = ctx.init_reconstruct(*args, taps=True)
    r = assert_layer1(dev, args)
    assert int(dev["n_good"].max()) == want and r["n_inliers"] == int(inl.sum())


def test_identity_homography_returns_early(ctx):
    a, _ = rn.case("H-65")
    args = a[:4] + (0, np.eye(3, dtype=F32).reshape(9), rn.CAM)
    dev = ctx.init_reconstruct(*args, taps=True)
    assert dev["n_hyp"] == 0 and dev["ok"] == 0 and dev["best"] == -1 and not dev["p3d"].any()
    assert dev["v4"].size == 0 and not dev["n_good"].any()
    assert_layer1(dev, args)


def test_sigma_and_thresholds_other_than_default(ctx):
    a, _ = rn.case("F-65")
    for kw in (dict(sigma=0.4), dict(min_triangulated=70), dict(min_parallax=2.0)):
        dev = ctx.init_reconstruct(*a[:7], taps=True, **kw)
        assert_layer1(dev, a[:7], **kw)


def _svd64(model, M21):
    X = rn.svd_input(model, M21, rn.CAM).astype(np.float64).reshape(3, 3)
    u, w, vt = np.linalg.svd(X)
    if w[2] <= rn.RANK_CUT * w[0]:
        u[:, 2] = np.cross(u[:, 0], u[:, 1])
    return u, w, vt


def _ulp_of_largest(m):
    return np.spacing(F32(np.abs(m).max()))


def _align_pair(ref_u, ref_v, dev_u, dev_v):
    """The 2x2 orthogonal Q (signs, and the rotation inside a pair of equal
    singular values) that takes the reference's leading columns of U and V
    onto the device's, both by the same Q: the orthogonal polar factor of
    ref_u' dev_u + ref_v' dev_v."""
    a, _, bt = np.linalg.svd(ref_u.T @ dev_u + ref_v.T @ dev_v)
    return a @ bt


# The products U W Vt are formed here from the tap's floats.  Each entry sums three terms of two rounded factors;
# a factor below 1 is off by at most 2^-25, and the absolute entries of a unit column sum to at most sqrt(3), so
# the rounding of the tap alone moves a product entry by up to 2 sqrt(3) 2^-25 -- more than one ulp (2^-24) of an
# entry below 1, whatever the solve's accuracy (one motion below measures 1.005 ulp).  The solves' own error
# (eps64 over the gap between sigma2 and sigma3, about 1e-15) is far below either.
PRODUCT_BOUND = 2 * np.sqrt(3.0) * 2.0 ** -25 + 2.0 ** -40


def test_layer2_svd_against_float64(ctx):
    """The svd tap against np.linalg.svd in float64.  Homography: every
    singular pair whose relative gaps are at least 1e-4, signs aligned,
    within one float32 ulp of the matrix's largest entry.  Essential matrix
    (sigma1 = sigma2 to float round-off, sigma3 = 0): t = U's third column
    and, after aligning the leading pair's rotation, the other columns of U
    and V at the same bound; the products U W Vt and U Wt Vt, which do not
    depend on that rotation, at PRODUCT_BOUND."""
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    compared = equal = 0
    # the cases, and further motions and planes (20 matches each: only the decomposition is looked at)
    rng = np.random.default_rng(8)
    inputs = [(name, rn.case(name)[0]) for name in sorted(rn.CASES)]
    for k in range(8):
        model = k % 2
        plane = dict(normal=(rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), 1.0), d=rng.uniform(4, 8)) if model == 0 else None
        k1, k2, m, truth = rn.scene(300 + k, 20, plane=plane, angle=rng.uniform(-0.2, 0.2), t=tuple(rng.uniform(-0.6, 0.6, 3)))
        inputs.append((f"motion-{k}", (k1, k2, m, np.ones(20, np.uint8), model, rn.true_model(model, truth, plane), rn.CAM,
                                       truth, {})))
    for name, a in inputs:
        model, M21 = a[4], a[5]
        dev = ctx.init_reconstruct(*a[:7], taps=True, **a[8])
        S = dev["svd"].astype(np.float64)
        U, w, Vt = S[:9].reshape(3, 3), S[9:12], S[12:].reshape(3, 3)
        u, s, vt = _svd64(model, M21)
        assert within_one_ulp(dev["svd"][9:11], s[:2].astype(F32)), name
        assert np.abs(U.T @ U - np.eye(3)).max() < 1e-6 and np.abs(Vt @ Vt.T - np.eye(3)).max() < 1e-6
        if model == 1:
            sign = np.sign(U[:, 2] @ u[:, 2])
            d_t = np.abs(U[:, 2] - sign * u[:, 2]).max()
            d_v3 = min(np.abs(Vt[2] - vt[2]).max(), np.abs(Vt[2] + vt[2]).max())
            Q = _align_pair(u[:, :2], vt[:2].T, U[:, :2], Vt[:2].T)
            d_u = np.abs(U[:, :2] - u[:, :2] @ Q).max()
            d_v = np.abs(Vt[:2].T - vt[:2].T @ Q).max()
            got = [U @ w_ @ Vt for w_ in (W, W.T)]
            want = [u @ w_ @ vt for w_ in (W, W.T)]
            got = [g * np.sign(np.linalg.det(g)) for g in got]
            want = [g * np.sign(np.linalg.det(g)) for g in want]
            d_p = [min(np.abs(g - x).max() for x in want) for g in got]
            print(f"{name}: in ulps of the largest entry: t {d_t / _ulp_of_largest(u[:, 2]):.2f}, v3 "
                  f"{d_v3 / _ulp_of_largest(vt):.2f}, U pair {d_u / _ulp_of_largest(u):.2f}, V pair "
                  f"{d_v / _ulp_of_largest(vt):.2f}, products {[round(float(d / _ulp_of_largest(u)), 2) for d in d_p]}")
            assert d_t <= _ulp_of_largest(u[:, 2]), name
            assert d_v3 <= _ulp_of_largest(vt) and d_u <= _ulp_of_largest(u) and d_v <= _ulp_of_largest(vt), name
            assert max(d_p) <= PRODUCT_BOUND, name
            compared += 3
            continue
        if (s[0] - s[1]) / s[0] < rn.CUT or (s[1] - s[2]) / s[0] < rn.CUT:
            continue
        assert within_one_ulp(dev["svd"][11:12], s[2:].astype(F32)), name
        for k in range(3):
            sign = np.sign(U[:, k] @ u[:, k])
            du, dv = np.abs(U[:, k] - sign * u[:, k]).max(), np.abs(Vt[k] - sign * vt[k]).max()
            assert du <= _ulp_of_largest(u) and dv <= _ulp_of_largest(vt), (name, k, du, dv)
            compared += 1
            equal += int(np.array_equal(dev["svd"][k:9:3], (sign * u[:, k]).astype(F32)) and
                         np.array_equal(dev["svd"][12 + 3 * k:15 + 3 * k], (sign * vt[k]).astype(F32)))
    print(f"3x3 decompositions: {compared} singular pairs compared, {equal} of the homographies' bit-equal to float64")
    assert compared >= 40


@pytest.mark.parametrize("name", ["F-300", "H-300"])
def test_layer2_null_vectors(ctx, name):
    """Above the cut (s3 - s4) / s1 >= 1e-4 both solves are accurate to about
    eps64 s1 / gap, so they differ in the final rounding at most: within one
    float32 ulp of the vector's largest entry after sign alignment."""
    a, _ = rn.case(name)
    dev = ctx.init_reconstruct(*a[:7], taps=True)
    r = rn.reconstruct(*a[:7], svd=dev["svd"])
    ran = ~np.isnan(r["gap"])
    ok = ran & (r["gap"] >= rn.CUT)
    x, y = dev["v4"][ok], r["v4"][ok]
    sign = np.sign(np.sum(x.astype(np.float64) * y.astype(np.float64), axis=1, keepdims=True))
    assert np.all(sign != 0)
    d = np.abs(x.astype(np.float64) - sign * y.astype(np.float64)).max(axis=1)
    ulp = np.spacing(np.abs(y).max(axis=1).astype(F32))
    print(f"null vectors: {int(ran.sum())} solved, {int(ok.sum())} above the cut, "
          f"{int(np.count_nonzero(d == 0))} bit-equal to the float64 SVD")
    assert np.all(d <= ulp), float((d / ulp).max())
    assert np.all(np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1) < 1e-6)
    assert ran.sum() >= 4 * 300 and ok.sum() >= 0.95 * ran.sum()


def test_fp_contract_modes_on_a_match_built_for_the_device(ctx):
    """CheckRT's fused forms.  The coinciding leading singular pair of an
    essential matrix lets the device's R differ from the fixture's in the last
    bits, which moves the reprojection threshold, so the match is built here
    for the device's own motion: the winning hypothesis' R and t are read
    from the taps of the base scene, the restatement bisects frame 2's
    keypoint of one match to that motion's threshold until its two modes
    decide differently, and the device, called in both modes on that one
    inlier, must count what the restatement counts in each mode -- 1 in one,
    0 in the other."""
    k1, k2, m, M21, S, _ = rn.contract_base()
    base = ctx.init_reconstruct(k1, k2, m, np.ones(rn.CONTRACT_N, np.uint8), 1, M21, rn.CAM, taps=True)
    assert base["ok"] == 1
    h = base["best"]
    edit = rn.find_contract_edit(base["R_all"][h], base["t_all"][h])
    assert edit is not None
    args = rn.contract_case(edit)
    want = {c: rn.reconstruct(*args, svd=base["svd"], contract=c)["n_good"] for c in (0, 1)}
    assert {int(want[0][h]), int(want[1][h])} == {0, 1}
    got = {}
    try:
        for c in (1, 0):
            ctx.set_fp_contract(c)
            dev = ctx.init_reconstruct(*args, taps=True)
            assert dev["svd"].tobytes() == base["svd"].tobytes() and dev["R_all"].tobytes() == base["R_all"].tobytes()
            assert_layer1(dev, args, contract=c)
            got[c] = dev["n_good"]
            print(f"match {edit[0]} at y = {edit[1]!r}, mode {c}: n_good {dev['n_good'][:4].tolist()}")
    finally:
        ctx.set_fp_contract(0)
    for c in (0, 1):
        assert got[c].tobytes() == want[c].tobytes(), (c, got[c], want[c])
    assert got[0][h] != got[1][h]


def test_fp_contract_modes_on_the_fixture_and_the_homography(ctx):
    """Layer 1 in each mode on the fixture's constructed match, and on
    ReconstructH's own expressions (:606-614, :649-651): among the plane cases
    at least one has hypotheses whose bits differ between the restatement's
    two modes on the device's own decomposition, and the device gives each
    mode's bytes."""
    G = np.load(GOLDEN)
    args = (G["f_keys1"], G["f_keys2"], G["f_matches12"], G["f_inliers"], 1, G["f_M21"], G["cam"])
    differ = 0
    try:
        for c in (1, 0):
            ctx.set_fp_contract(c)
            assert_layer1(ctx.init_reconstruct(*args, taps=True), args, contract=c)
            for name in ("H-65", "H-64", "H-256", "H-ambiguous-65"):
                a, _ = rn.case(name)
                dev = ctx.init_reconstruct(*a[:7], taps=True, **a[8])
                assert_layer1(dev, a[:7], contract=c, **a[8])      # compares R_all and t_all byte for byte
                other = rn.faugeras(dev["svd"], 1 - c)
                differ += any(R.tobytes() != dev["R_all"][k].tobytes() or t.tobytes() != dev["t_all"][k].tobytes()
                              for k, (R, t) in enumerate(other))
    finally:
        ctx.set_fp_contract(0)
    print(f"plane cases whose hypotheses differ between the modes: {differ} of 8")
    assert differ >= 1


def same_result(a, b, n1=None):
    for k in ("ok", "n_inliers", "n_hyp", "best"):
        assert a[k] == b[k], k
    for k in ("R21", "t21"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or canon(a[k]) == canon(b[k])), k
    assert a["n_good"].tobytes() == b["n_good"].tobytes() and canon(a["parallax"]) == canon(b["parallax"])
    for k in ("p3d", "triangulated"):
        assert a[k][:n1].tobytes() == b[k][:n1].tobytes(), k
    for k in ("svd", "R_all", "t_all", "v4", "cos_parallax"):
        assert canon(a[k]) == canon(b[k]), k


def test_batch_equals_single_calls(ctx):
    """Three queries of mixed models and one without a match."""
    qs = [rn.case(n)[0][:7] for n in ("F-65", "H-300", "F-noisy")]
    a = qs[0]
    qs.insert(2, (a[0], a[1], np.full(len(a[0]), -1, np.int32), np.zeros(0, np.uint8), 0, a[5], a[6]))
    out = ctx.init_reconstruct_batch(qs, taps=True)
    for q, r in zip(qs, out):
        same_result(r, ctx.init_reconstruct(*q, taps=True))
    assert out[2]["ok"] == 0 and out[2]["n_hyp"] == 0 and out[2]["n_inliers"] == 0 and not out[2]["p3d"].any()
    assert [r["ok"] for r in out] == [1, 1, 0, 0]


def test_argument_rules(ctx):
    a, _ = rn.case("F-65")
    lib = ox.lib()

    def call(**kw):
        v = dict(keys1=a[0], keys2=a[1], matches12=a[2], inliers=a[3], model=a[4], M21=a[5], cam=a[6], sigma=1.0,
                 cap=None)
        v.update(kw)
        q, keep = ox.reconstruct_query(v["keys1"], v["keys2"], v["matches12"], v["inliers"], v["model"], v["M21"],
                                       v["cam"], sigma=v["sigma"], cap=v["cap"])
        for name in kw.get("null", ()):
            setattr(q, name, None)
        return lib.orbx_init_reconstruct(ctx.handle, ctypes.byref(q))

    assert call() == 0
    assert lib.orbx_init_reconstruct(None, None) == ERR_ARG
    assert lib.orbx_init_reconstruct(ctx.handle, None) == ERR_ARG
    for name in ("keys1", "keys2", "matches12", "inliers", "M21", "cam", "p3d", "triangulated"):
        assert call(null=(name,)) == ERR_ARG, name
    assert call(model=2) == ERR_ARG and call(model=-1) == ERR_ARG
    assert call(sigma=0.0) == ERR_ARG and call(sigma=-1.0) == ERR_ARG
    far = a[2].copy()
    far[np.nonzero(far >= 0)[0][0]] = len(a[1])
    assert call(matches12=far) == ERR_ARG
    assert call(cap=len(a[0]) - 1) == ERR_CAPACITY
    assert call(cap=len(a[0])) == 0
    big = np.zeros(4097, ox.KEYPOINT)
    assert call(keys1=big, matches12=np.full(4097, -1, np.int32), inliers=np.zeros(1, np.uint8)) == ERR_UNSUPPORTED
    assert call(keys2=big) == ERR_UNSUPPORTED
    # N == 0
    q = ctx.init_reconstruct(a[0], a[1], np.full(len(a[0]), -1, np.int32), np.zeros(0, np.uint8), 1, a[5], a[6])
    assert q["ok"] == 0 and q["n_hyp"] == 0
    # the device-resident form before a models run
    cam = np.array([120, 120, 80, 60], F32)
    assert lib.orbx_dev_init_reconstruct(ctx.handle, 0, 6, 3, ox._ptr(cam), 0.4, 1.0, 50) == ERR_ARG
    assert lib.orbx_dev_init_reconstruct(ctx.handle, 0, 6, 3, None, 0.4, 1.0, 50) == ERR_ARG


SLOT_CAM = np.array([120.0, 120.0, 80.0, 60.0], F32)


@pytest.mark.parametrize("async_match", [0, 1])
def test_device_resident_pairs(async_match):
    from orb_slam_amd import synth
    import init_numpy as inp
    M = 32
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=6)
    try:
        c.upload(synth.sequence(160, 120, 6, seed=9))
        c.set_async_match(async_match)
        draws = np.stack([inp.make_draws(70 + s, M) for s in range(6)])
        c.extract_match(0, 6, seq_len=3)
        with pytest.raises(ox.OrbxError) as e:
            c.dev_init_reconstruct(0, 6, 3, SLOT_CAM)      # before a models run
        assert e.value.code == ERR_ARG
        c.dev_init_models(0, 6, 3, draws, max_iter=M)
        with pytest.raises(ox.OrbxError) as e:
            c.read_init_reconstruct(1)                      # before a run
        assert e.value.code == ERR_ARG
        with pytest.raises(ox.OrbxError):
            c.dev_init_reconstruct(0, 5, 3, SLOT_CAM)      # not the models run's range
        # thresholds low enough for these small frames to reach every stage
        kw = dict(min_parallax=0.05, min_triangulated=8)
        models = {s: c.read_init_models(s) for s in (1, 2, 4, 5)}
        # a ratio threshold of 0.60 sends these pairs (image shifts: RH = 0.5) through ReconstructF
        c.dev_init_reconstruct(0, 6, 3, SLOT_CAM, rh_threshold=0.60, **kw)
        for s in (1, 2, 4, 5):
            mo = models[s]
            r = c.read_init_reconstruct(s, taps=True, n_matches=mo["n_matches"])
            model = 0 if mo["RH"] > F32(0.60) else 1
            assert r["model"] == model
            if mo["n_matches"] < 8 or mo["best_h"] < 0 or mo["best_f"] < 0:
                assert r["ok"] == 0 and r["n_hyp"] == 0
                continue
            k1, k2 = c.features(s - 1)[0], c.features(s)[0]
            args = (k1, k2, c.matches(s)[0][:len(k1)], mo["inliers_f"] if model else mo["inliers_h"], model,
                    mo["F21"] if model else mo["H21"], SLOT_CAM)
            same_result(r, c.init_reconstruct(*args, taps=True, **kw), n1=len(k1))
        c.timing(True, only="reconstruct")
        c.dev_init_reconstruct(0, 6, 3, SLOT_CAM, rh_threshold=0.40, **kw)
        got = {s: c.read_init_reconstruct(s, taps=True, n_matches=models[s]["n_matches"]) for s in (1, 2, 4, 5)}
        for s in (0, 3, 6):
            with pytest.raises(ox.OrbxError) as e:
                c.read_init_reconstruct(s)
            assert e.value.code == ERR_ARG
        n, _, total = c.kernel_time("reconstruct")
        assert n == 1 and total > 0   # one timed region for the one run
        c.timing(False)
        for s in (1, 2, 4, 5):
            k1, k2 = c.features(s - 1)[0], c.features(s)[0]
            m = c.matches(s)[0][:len(k1)]
            mo, r = models[s], got[s]
            model = 0 if mo["RH"] > F32(0.40) else 1
            assert r["model"] == model
            print(f"slot {s}: n1 {len(k1)} N {mo['n_matches']} RH {mo['RH']:.3f} model {model} ok {r['ok']} "
                  f"n_good {r['n_good'][:r['n_hyp']].tolist()}")
            if mo["n_matches"] < 8 or mo["best_h"] < 0 or mo["best_f"] < 0:
                assert r["ok"] == 0 and r["n_hyp"] == 0
                continue
            args = (k1, k2, m, mo["inliers_f"] if model else mo["inliers_h"], model, mo["F21"] if model else mo["H21"],
                    SLOT_CAM)
            host = c.init_reconstruct(*args, taps=True, **kw)
            same_result(r, host, n1=len(k1))
            assert not r["p3d"][len(k1):].any() and not r["triangulated"][len(k1):].any()
            assert_layer1(host, args, **kw)
        # a new models run invalidates the reconstruction
        c.dev_init_models(0, 6, 3, draws, max_iter=M)
        with pytest.raises(ox.OrbxError):
            c.read_init_reconstruct(1)
    finally:
        c.close()


def test_batch_of_packed_lengths_in_either_order(ctx):
    """Three queries in one batch with 17, 0 and 31 matches (a homography and
    a fundamental matrix at the ends): nothing is a multiple of the 16-byte
    packing step and an empty query lies between the others.  Every result
    is the single call's and the outer ones pass layer 1, in either order."""
    def query(seed, N, model, plane=None):
        k1, k2, m, truth = rn.scene(seed, N, plane=plane, extra1=0, extra2=5)
        return (k1, k2, m, np.ones(N, np.uint8), model, rn.true_model(model, truth, plane), rn.CAM)

    a, b = query(130, 17, 1), query(131, 31, 0, rn.PLANE_CLEAR)
    none = (a[0][:0], a[1][:0], np.zeros(0, np.int32), np.zeros(0, np.uint8), 1, a[5], a[6])
    qs = [a, none, b]
    single = [ctx.init_reconstruct(*q, taps=True) for q in qs]
    assert [r["n_inliers"] for r in single] == [17, 0, 31]
    for order in ((0, 1, 2), (2, 1, 0)):
        out = ctx.init_reconstruct_batch([qs[k] for k in order], taps=True)
        for r, k in zip(out, order):
            same_result(r, single[k])
            if k != 1:
                assert_layer1(r, qs[k])
        assert out[1]["ok"] == 0 and out[1]["n_hyp"] == 0 and not out[1]["p3d"].any()
