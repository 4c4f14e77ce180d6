"""orbx_init_models on the device against the numpy restatement
(tests/init_numpy.py), in two layers.

Layer 1, bit for bit, every iteration: sets, T1, T2, N; the restatement's
CheckHomography / CheckFundamental fed the device's own matrices give the
device's scores; the selection; the defined-order products and inverses from
the device's Hn / Fn.  (The compaction order has no tap of its own: the float
score sums run in that order and the inlier vectors are indexed by it, and
both must equal the restatement's.)  NaNs compare equal to NaNs: IEEE leaves
their payload open and the host's default NaN differs from the device's.

Layer 2, the two null-vector solves: on the iterations that pass the
conditioning cut (computed by the restatement) every entry of Hn / Fn agrees
within one float32 ulp of the matrix's largest entry after aligning sign, and
where the matrices are the same bits the end-to-end scores are too (at least
90 % of the considered iterations must be).  Each case prints its counts; on
an MI355X every considered iteration of all 16 cases was bit-equal up to sign
(H: all iterations considered; F: between 191 of 200 and all).
"""
import ctypes

import numpy as np
import pytest

import init_numpy as inp
import orb_slam_amd as ox

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -1, -3


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


def same_result(a, b, taps=True):
    for k in ("n_matches", "best_h", "best_f"):
        assert a[k] == b[k], k
    for k in ("SH", "SF", "RH"):
        assert canon([a[k]]) == canon([b[k]]), k
    for k in ("H21", "F21"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or canon(a[k]) == canon(b[k])), k
    for k in ("inliers_h", "inliers_f"):
        assert a[k].tobytes() == b[k].tobytes(), k
    if taps:
        assert a["sets"].tobytes() == b["sets"].tobytes()
        for k in ("Hn", "Fn", "H21_all", "H12_all", "F21_all", "score_h", "score_f", "T1", "T2"):
            assert canon(a[k]) == canon(b[k]), k


def layer1(dev, k1, k2, m, d, M, sigma=1.0):
    """The bit-exact layer of one device result (with taps)."""
    p = inp.prepare(k1, k2, m, d, M)
    assert dev["n_matches"] == p["N"]
    assert dev["sets"].tobytes() == p["sets"].tobytes()
    assert canon(dev["T1"]) == canon(p["T1"]) and canon(dev["T2"]) == canon(p["T2"])
    if p["N"] < 8:
        assert dev["best_h"] == dev["best_f"] == -1 and dev["SH"] == 0 and dev["SF"] == 0 and np.isnan(dev["RH"])
        assert dev["H21"] is None and dev["F21"] is None
        assert not dev["inliers_h"].any() and not dev["inliers_f"].any()
        return p
    # the defined products and inverses, from the device's Hn / Fn
    H21, H12 = inp.denorm_h(dev["Hn"], p["T1"], p["T2"])
    F21 = inp.denorm_f(dev["Fn"], p["T1"], p["T2"])
    assert canon(H21) == canon(dev["H21_all"])
    assert canon(H12) == canon(dev["H12_all"])
    assert canon(F21) == canon(dev["F21_all"])
    # the checks, fed the device's matrices, in the restatement's match order
    sh, ih = inp.check_homography(dev["H21_all"], dev["H12_all"], p["xy"], sigma)
    sf, jf = inp.check_fundamental(dev["F21_all"], p["xy"], sigma)
    assert canon(sh) == canon(dev["score_h"])
    assert canon(sf) == canon(dev["score_f"])
    want = inp.finish(p, dev["score_h"], ih, dev["H21_all"], dev["score_f"], jf, dev["F21_all"])
    for k in ("best_h", "best_f"):
        assert dev[k] == want[k], k
    for k in ("SH", "SF", "RH"):
        assert canon([dev[k]]) == canon([want[k]]), k
    for k in ("H21", "F21"):
        assert (dev[k] is None) == (want[k] is None) and (want[k] is None or canon(dev[k]) == canon(want[k])), k
    assert dev["inliers_h"].tobytes() == want["inliers_h"].tobytes()
    assert dev["inliers_f"].tobytes() == want["inliers_f"].tobytes()
    return p


@pytest.mark.parametrize("i", range(len(inp.CASES)), ids=[f"N{c[0]}-it{c[1]}" for c in inp.CASES])
def test_models_against_the_restatement(ctx, i):
    (k1, k2, m, d, M), ref = inp.case(i)
    assert len(k1) != len(k2) and (m < 0).any()   # Normalize sees unmatched keypoints
    dev = ctx.init_models(k1, k2, m, d, 1.0, M, taps=True)
    layer1(dev, k1, k2, m, d, M)
    # layer 2
    ok_h, ok_f = inp.considered(ref)
    for name, ok, score in (("Hn", ok_h, "score_h"), ("Fn", ok_f, "score_f")):
        assert (~ok).sum() <= 0.05 * M, (name, int((~ok).sum()))
        a, b = dev[name][ok], ref[name][ok]
        b = b * np.where((a * b).sum(1, keepdims=True) < 0, np.float32(-1), np.float32(1))
        ulp = np.spacing(np.abs(b).max(1, keepdims=True).astype(np.float32))
        worst = float((np.abs(a - b) / ulp).max()) if ok.any() else 0.0
        same = (a == b).all(1)
        print(f"{name}: {int(ok.sum())}/{M} considered, worst {worst:.2f} ulp, {int(same.sum())} bit-equal up to sign")
        assert worst <= 1.0, (name, worst)
        assert canon(dev[score][ok][same]) == canon(ref[score][ok][same]), score
        assert same.sum() >= 0.9 * ok.sum(), (name, int(same.sum()), int(ok.sum()))


def small_pair(seed, N, M=16, **kw):
    k1, k2, m = inp.scene(seed, N, **kw)
    return k1, k2, m, inp.make_draws(seed + 1, M), 1.0, M


def test_batch_with_short_pairs(ctx):
    """N = 7 and N = 0 beside a normal pair: no fault, and the normal pair's
    result is the single call's."""
    qs = [small_pair(40, 7), small_pair(41, 0), small_pair(42, 65)]
    out = ctx.init_models_batch(qs, taps=True)
    for q, r, n in zip(qs, out, (7, 0, 65)):
        assert r["n_matches"] == n
        layer1(r, *q[:4], q[5])
    assert not out[0]["score_h"].any() and not out[0]["sets"].any()
    same_result(out[2], ctx.init_models(*qs[2], taps=True))


def test_argument_rules(ctx):
    k1, k2, m, d, sigma, M = small_pair(43, 20)
    lib = ox.lib()

    def call(**kw):
        a = dict(keys1=k1, keys2=k2, matches12=m, draws=d, sigma=sigma, max_iter=M, cap=None)
        a.update(kw)
        q, keep = ox.init_query(a["keys1"], a["keys2"], a["matches12"], a["draws"], a["sigma"], a["max_iter"],
                                cap=a["cap"])
        return lib.orbx_init_models(ctx.handle, ctypes.byref(q))

    assert call() == 0
    assert call(cap=19) == ERR_CAPACITY
    assert call(cap=20) == 0
    bad = d.copy()
    bad[3, 5] = -1
    assert call(draws=bad) == ERR_ARG
    assert call(max_iter=0) == ERR_ARG
    assert call(max_iter=1025, draws=inp.make_draws(1, 1025)) == ERR_ARG
    assert call(max_iter=1024, draws=inp.make_draws(1, 1024)) == 0
    assert call(sigma=0.0) == ERR_ARG
    assert lib.orbx_init_models(ctx.handle, None) == ERR_ARG
    far = m.copy()
    far[np.nonzero(m >= 0)[0][0]] = len(k2)
    assert call(matches12=far) == ERR_ARG
    draws6 = np.zeros((6, 4, 8), np.int32)
    assert lib.orbx_dev_init_models(ctx.handle, 0, 7, 3, 1.0, 4, draws6.ctypes.data) == ERR_ARG
    assert lib.orbx_dev_init_models(ctx.handle, 0, 6, 3, 1.0, 0, draws6.ctypes.data) == ERR_ARG
    assert lib.orbx_dev_init_models(ctx.handle, 0, 6, 3, 0.0, 4, draws6.ctypes.data) == ERR_ARG
    draws6[5, 3, 7] = -5
    assert lib.orbx_dev_init_models(ctx.handle, 0, 6, 3, 1.0, 4, draws6.ctypes.data) == ERR_ARG


def test_pure_outliers(ctx):
    k1, k2, m, d, sigma, M = small_pair(44, 65, M=65, outliers=1.0)
    layer1(ctx.init_models(k1, k2, m, d, sigma, M, taps=True), k1, k2, m, d, M)


def test_sigma_other_than_one(ctx):
    k1, k2, m, d, _, M = small_pair(46, 65, M=32)
    layer1(ctx.init_models(k1, k2, m, d, 1.5, M, taps=True), k1, k2, m, d, M, sigma=1.5)


def test_identical_reference_keypoints(ctx):
    """Two matched keypoints of the reference frame at the same coordinates
    (sets that draw both have a repeated row in A)."""
    k1, k2, m, d, sigma, M = small_pair(45, 9, M=65)
    i = np.nonzero(m >= 0)[0]
    k1["x"][i[1]], k1["y"][i[1]] = k1["x"][i[0]], k1["y"][i[0]]
    layer1(ctx.init_models(k1, k2, m, d, sigma, M, taps=True), k1, k2, m, d, M)


def test_batch_equals_single_calls(ctx):
    qs = [small_pair(50 + k, N, M=M, planar=bool(k & 1)) for k, (N, M) in
          enumerate([(300, 24), (9, 65), (65, 8), (8, 1), (120, 40)])]
    out = ctx.init_models_batch(qs, taps=True)
    for q, r in zip(qs, out):
        same_result(r, ctx.init_models(*q, taps=True))


@pytest.mark.parametrize("async_match", [0, 1])
def test_device_resident_pairs(async_match):
    from orb_slam_amd import synth
    M = 32
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=6)
    try:
        c.upload(synth.sequence(160, 120, 6, seed=9))
        c.set_async_match(async_match)
        with pytest.raises(ox.OrbxError):
            c.read_init_models(1)   # before a run
        draws = np.stack([inp.make_draws(70 + s, M) for s in range(6)])
        c.timing(True, only="init")
        c.extract_match(0, 6, seq_len=3)
        c.dev_init_models(0, 6, 3, draws, max_iter=M)
        got = {s: c.read_init_models(s, taps=True) for s in (1, 2, 4, 5)}
        for s in (0, 3):
            with pytest.raises(ox.OrbxError) as e:
                c.read_init_models(s)
            assert e.value.code == ERR_ARG
        n, _, total = c.kernel_time("init")
        assert n == 1 and total > 0   # one timed region for the one run
        c.timing(False)
        for s in (1, 2, 4, 5):
            k1, k2 = c.features(s - 1)[0], c.features(s)[0]
            m = c.matches(s)[0][:len(k1)]
            print(f"slot {s}: n1 {len(k1)} n2 {len(k2)} N {got[s]['n_matches']}")
            same_result(got[s], c.init_models(k1, k2, m, draws[s], 1.0, M, taps=True))
            layer1(got[s], k1, k2, m, draws[s], M)
    finally:
        c.close()


def test_batch_of_packed_lengths_in_either_order(ctx):
    """Three pairs in one batch whose first frames have 17, 0 and 31
    keypoints and which draw 17, 1 and 31 sets: nothing is a multiple of the
    16-byte packing step and an empty pair lies between the others.  Every
    result is the single call's and the outer ones pass layer 1, in either
    order."""
    qs = [small_pair(60, 10, M=17), small_pair(61, 0, M=1, extra1=0, extra2=0), small_pair(62, 24, M=31)]
    assert [len(q[0]) for q in qs] == [17, 0, 31]
    single = [ctx.init_models(*q, taps=True) for q in qs]
    assert [r["n_matches"] for r in single] == [10, 0, 24]
    for order in ((0, 1, 2), (2, 1, 0)):
        out = ctx.init_models_batch([qs[k] for k in order], taps=True)
        for r, k in zip(out, order):
            same_result(r, single[k])
            if k != 1:
                layer1(r, *qs[k][:4], qs[k][5])
        assert out[1]["best_h"] == out[1]["best_f"] == -1 and out[1]["H21"] is None and out[1]["F21"] is None
