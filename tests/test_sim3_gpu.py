"""orbx_sim3_ransac on the device against the numpy restatement
(tests/sim3_numpy.py), in two layers.

Layer 1, byte for byte, every iteration: N, indices1, x3dc1 / 2, p1im1 /
p2im2, the limits and the sets; the restatement's computeT fed the device's
own rotation gives the device's scale, T12 and T21; its CheckInliers fed the
device's T12 / T21 gives the device's counts and the returned mask; the replay
of iterate's bookkeeping over the device's counts gives every output.  NaNs
compare equal to NaNs.

Between the quaternion and the rotation stand the FP64 atan2, sin, cos and
sqrt of two libraries, which differ by a few FP64 ulps: the restatement fed
the device's q must give the device's R within one float32 ulp of 1.0 (the
bit-equal count is printed; where R is the same bits, so is everything after
it by the comparison above).

Layer 2, the eigenvector: on the iterations that pass the eigen-gap cut
(computed by the restatement) q agrees with np.linalg.eigh in float64 within
one float32 ulp of its largest entry after aligning sign, and at least 90 %
are bit-equal.  Each case prints its counts.
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import sim3_numpy as s3

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4
ULP1 = float(np.spacing(np.float32(1.0)))


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=2)
    yield c
    c.close()


def canon(a):
    """Bytes of a float32 array with every NaN as one pattern."""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def opt_same(a, b):
    return (a is None) == (b is None) and (a is None or canon(a) == canon(b))


OUT_INTS = ("N", "ransac_max_its", "iters_run", "no_more", "found", "found_iter", "n_inliers", "best_inliers_out", "best_iter")
ITER_TAPS = ("q", "R", "scale", "T12_all", "T21_all")
CORR_TAPS = ("x3dc1", "x3dc2", "p1im1", "p2im2")


def same_result(a, b, taps=True):
    for k in OUT_INTS:
        assert a[k] == b[k], k
    for k in ("T12", "R12", "t12", "s12"):
        assert opt_same(a[k], b[k]), k
    n = min(len(a["inliers"]), len(b["inliers"]))
    assert a["inliers"][:n].tobytes() == b["inliers"][:n].tobytes()
    assert not a["inliers"][n:].any() and not b["inliers"][n:].any()
    if taps:
        for k in ("sets", "count", "indices1", "max_err1", "max_err2"):
            assert a[k].tobytes() == b[k].tobytes(), k
        for k in ITER_TAPS + CORR_TAPS:
            assert canon(a[k]) == canon(b[k]), k


def layer1(dev, kf1, kf2, m, d, kw, contract=False):
    """The bit-exact layer of one device result (with taps); returns the
    restatement's correspondences and the count of bit-equal rotations."""
    kw = dict(kw)
    idx1 = kw.pop("idx1", None)
    mi, prob, mx = kw.get("min_inliers", 20), kw.get("probability", 0.99), kw.get("max_iterations", 300)
    M = len(np.asarray(d).reshape(-1, 3)) if kw.get("n_iter") is None else kw["n_iter"]
    n1 = len(kf1["keys"])
    c = s3.construct(kf1, kf2, m, idx1, contract)
    N = c["N"]
    assert dev["N"] == N
    assert dev["ransac_max_its"] == s3.ransac_max_its(N, mi, prob, mx)
    for k in ("indices1", "max_err1", "max_err2"):
        assert dev[k].tobytes() == c[k].tobytes(), k
    for k in CORR_TAPS:
        assert canon(dev[k]) == canon(c[k]), k
    if N < mi:
        want = s3.iterate_select([], N, mi, 0, kw.get("iter_done", 0), kw.get("best_inliers", 0))
        for k in want:
            assert dev[k] == want[k], k
        assert dev["T12"] is None and dev["R12"] is None and not dev["inliers"].any()
        assert not dev["sets"].any() and not dev["count"].any() and not dev["T12_all"].any()
        return c, 0
    sets = s3.make_sets(N, np.asarray(d).reshape(-1, 3)[:M])
    assert dev["sets"].tobytes() == sets.tobytes()
    # the rotation from the device's q: two FP64 maths libraries apart
    R = s3.rotation(dev["q"])
    both = np.isnan(R) & np.isnan(dev["R"])
    diff = np.where(both, 0.0, np.abs(R.astype(np.float64) - dev["R"].astype(np.float64)))
    assert not (np.isnan(diff)).any()          # a NaN on one side only
    assert diff.max() <= ULP1, diff.max()
    same_R = int(((R == dev["R"]) | both).all(1).sum())
    # everything after the rotation, from the device's R
    t = s3.compute_t(c, sets, q=dev["q"], R=dev["R"])
    for k in ("scale", "T12_all", "T21_all"):
        assert canon(t[k]) == canon(dev[k]), k
    count, mask = s3.check_inliers(c, kf1, kf2, dev["T12_all"], dev["T21_all"], contract)
    assert dev["count"].tobytes() == count.tobytes()
    sel = s3.iterate_select(dev["count"], N, mi, dev["ransac_max_its"], kw.get("iter_done", 0), kw.get("best_inliers", 0))
    want = s3.outputs(c, sel, dict(T12_all=dev["T12_all"], R=dev["R"], scale=dev["scale"]), mask, n1)
    for k in sel:
        assert dev[k] == want[k], k
    for k in ("T12", "R12", "t12", "s12"):
        assert opt_same(dev[k], want[k]), k
    assert dev["inliers"].tobytes() == want["inliers"].tobytes()
    return c, same_R


@pytest.mark.parametrize("i", range(len(s3.CASES)), ids=[f"N{c[0]}-it{c[1]}" for c in s3.CASES])
def test_ransac_against_the_restatement(ctx, i):
    (kf1, kf2, m, d, kw), ref = s3.case(i)
    N, M = s3.CASES[i][:2]
    assert len(kf1["keys"]) != len(kf2["keys"]) and (m < 0).any() and not kf1["valid"].all()
    dev = ctx.sim3_ransac(kf1, kf2, m, d, taps=True, **kw)
    c, same_R = layer1(dev, kf1, kf2, m, d, kw)
    assert dev["N"] == N
    # layer 2
    ok = s3.considered(ref)
    assert (~ok).sum() <= 0.05 * M, int((~ok).sum())
    a, b = dev["q"][ok], ref["q"][ok]
    b = b * np.where((a * b).sum(1, keepdims=True) < 0, np.float32(-1), np.float32(1))
    ulp = np.spacing(np.abs(b).max(1, keepdims=True).astype(np.float32))
    worst = float((np.abs(a - b) / ulp).max()) if ok.any() else 0.0
    same = (a == b).all(1)
    print(f"q: {int(ok.sum())}/{M} considered, worst {worst:.2f} ulp, {int(same.sum())} bit-equal; "
          f"R from q: {same_R}/{M} bit-equal; found_iter {dev['found_iter']}, n_inliers {dev['n_inliers']}")
    assert worst <= 1.0, worst
    assert same.sum() >= 0.9 * ok.sum(), (int(same.sum()), int(ok.sum()))
    assert (dev["q"][ok][:, 0] >= 0).all()          # the fixed sign


def pair(seed, N, M=16, **kw):
    kf1, kf2, m, idx1 = s3.scene(seed, N, use_idx1=bool(seed & 1))
    return kf1, kf2, m, s3.make_draws(seed + 1, M), dict(idx1=idx1, **kw)


def test_resumption_in_chunks_of_five(ctx):
    """iterate(5) after iterate(5), carrying mnIterations and mnBestInliers
    and going on after every return, against calls that take all the remaining
    iterations at once: the same returns at the same iterations with the same
    results.  The scene returns more than once, and after the first return a
    later iteration returns only if its count reaches the carried best."""
    kf1, kf2, m, idx1 = s3.scene(77, 120, noise=0.02)
    M = 300
    draws = s3.make_draws(78, M)
    kw = dict(idx1=idx1, min_inliers=20)

    def walk(chunk):
        events, done, best = [], 0, 0
        while done < M:
            n = min(chunk, M - done)
            r = ctx.sim3_ransac(kf1, kf2, m, draws[done:done + n], n_iter=n, iter_done=done, best_inliers=best, **kw)
            if r["found"]:
                events.append((done + r["found_iter"], r["n_inliers"], canon(r["T12"]), r["inliers"].tobytes()))
            if r["best_iter"] >= 0:
                state = (done + r["best_iter"], canon(r["R12"]), canon(r["t12"]), canon([r["s12"]]))
            assert r["iters_run"] >= 1 or r["no_more"]
            if r["iters_run"] == 0:
                break
            done, best = done + r["iters_run"], r["best_inliers_out"]
            last = r
        return events, done, best, state, last["no_more"]

    whole, by5 = walk(M), walk(5)
    assert whole == by5
    events, done, best = whole[:3]
    assert len(events) >= 2 and done == ref_max_its(kf1, kf2, m, idx1)
    counts = [e[1] for e in events]
    assert counts == sorted(counts)       # a later return needs count >= the carried best
    print(f"returns at {[e[0] for e in events]} with {counts} inliers; {done} iterations")


def ref_max_its(kf1, kf2, m, idx1):
    return min(300, s3.ransac_max_its(s3.construct(kf1, kf2, m, idx1)["N"]))


def test_batch_equals_single_calls(ctx):
    """With a pair of N < min_inliers and a pair of N = 0 beside normal ones."""
    qs = [pair(50, 300, M=24), pair(51, 10, M=8), pair(52, 65, M=65, min_inliers=6), pair(53, 64, M=1)]
    kf1, kf2, m, d, kw = pair(54, 30, M=5)
    qs.append((kf1, kf2, np.full(len(m), -1, np.int32), d, kw))
    out = ctx.sim3_ransac_batch(qs, taps=True)
    for q, r, n in zip(qs, out, (300, 10, 65, 64, 0)):
        assert r["N"] == n
        same_result(r, ctx.sim3_ransac(*q[:4], taps=True, **q[4]))
        layer1(r, *q)
    assert out[1]["no_more"] == 1 and out[1]["iters_run"] == 0 and not out[1]["found"]
    assert out[4]["no_more"] == 1 and out[4]["ransac_max_its"] == 0
    assert out[0]["found"] and out[2]["found"]


def test_forced_repeated_correspondence(ctx):
    """Draws that make the second and third pick hit the first's position: the
    set holds the back of the list twice (the removal cannot produce three
    equal picks: tests/test_sim3_numpy.py enumerates every outcome).  The call
    returns ORBX_OK, the iteration is the restatement's bit for bit, and the
    other iterations are what they are without it.  Its count is 2, not 0:
    two distinct correspondences fit a similarity exactly whatever they are,
    so both pass CheckInliers in the reference as well, and the rotation about
    the line through them is arbitrary for everything else.  The count of 0 is
    the NaN flavour of a degenerate iteration, test_zero_rotation_gives_nans."""
    kf1, kf2, m, idx1 = s3.scene(60, 64)
    d = s3.make_draws(61, 8)
    forced = d.copy()
    N = 64
    forced[3] = [int((10.5 / N) * 2**31), int((10.5 / (N - 1)) * 2**31), int((10.5 / (N - 2)) * 2**31)]
    kw = dict(idx1=idx1)
    a = ctx.sim3_ransac(kf1, kf2, m, d, taps=True, **kw)
    b = ctx.sim3_ransac(kf1, kf2, m, forced, taps=True, **kw)
    assert b["sets"][3].tolist() == [10, 63, 63]
    layer1(b, kf1, kf2, m, forced, kw)
    print(f"count of the repeated set: {b['count'][3]}")
    assert b["count"][3] == 2
    keep = np.arange(8) != 3
    for k in ("sets", "count"):
        assert a[k][keep].tobytes() == b[k][keep].tobytes(), k
    for k in ITER_TAPS:
        assert canon(a[k][keep]) == canon(b[k][keep]), k
    for k in OUT_INTS:                        # both return at iteration 1, before the forced one
        assert a[k] == b[k], k
    assert a["found_iter"] < 3


def test_zero_rotation_gives_nans(ctx):
    """The same map seen from the same pose on both sides: M is symmetric, N
    is diag(tr M) beside a 3x3 block of smaller eigenvalues, q is (1, 0, 0, 0)
    exactly, norm(vec) is 0 and 2*ang*vec/norm(vec) is 0 * inf.  Every
    iteration is NaNs, counts 0 inliers (err < limit is false) and nothing
    returns; the NaNs compare as NaNs."""
    kf1, kf2, m, idx1 = s3.scene(66, 40)
    n1 = len(kf1["keys"])
    keys2 = s3.make_keys(n1, kf1["keys"]["octave"])
    same = dict(kf1, keys=keys2)
    ident = np.arange(n1, dtype=np.int32)
    d = s3.make_draws(67, 65)
    kw = dict(min_inliers=6)
    dev = ctx.sim3_ransac(kf1, same, ident, d, taps=True, **kw)
    assert dev["N"] == int(kf1["valid"].sum()) >= 40
    assert np.isnan(dev["T12_all"]).any(1).all() and not dev["count"].any()
    assert dev["q"][:, 0].tolist() == [1.0] * 65 and not dev["q"][:, 1:].any()
    assert not dev["found"] and dev["iters_run"] == 65 and dev["best_iter"] == 64 and not dev["inliers"].any()
    layer1(dev, kf1, same, ident, d, kw)


def test_fp_contract_mode(ctx):
    kf1, kf2, m, d, kw = pair(62, 65, M=32)
    try:
        ctx.set_fp_contract(1)
        layer1(ctx.sim3_ransac(kf1, kf2, m, d, taps=True, **kw), kf1, kf2, m, d, kw, contract=True)
    finally:
        ctx.set_fp_contract(0)


def test_more_than_one_tile_of_correspondences(ctx):
    """N above the 1024 correspondences staged at a time."""
    kf1, kf2, m, d, kw = pair(64, 1100, M=9)
    dev = ctx.sim3_ransac(kf1, kf2, m, d, taps=True, **kw)
    assert dev["N"] == 1100 and dev["found"]
    layer1(dev, kf1, kf2, m, d, kw)


def test_argument_rules(ctx):
    kf1, kf2, m, d, kw = pair(70, 30, M=16)
    lib = ox.lib()

    def call(kf1=kf1, kf2=kf2, m=m, d=d, null=None, **over):
        a = dict(kw)
        a.update(over)
        q, keep = ox.sim3_query(kf1, kf2, m, d, **a)
        if null:
            setattr(q, null, None)
        return lib.orbx_sim3_ransac(ctx.handle, ctypes.byref(q))

    assert call() == 0
    assert lib.orbx_sim3_ransac(None, ctypes.byref(ox.Sim3Query())) == ERR_ARG
    assert lib.orbx_sim3_ransac(ctx.handle, None) == ERR_ARG
    for name in ("keys1", "keys2", "matches12", "pos1", "valid1", "pos2", "valid2", "T1w", "T2w", "cam1", "cam2",
                 "sigma2_1", "sigma2_2", "draws", "inliers"):
        assert call(null=name) == ERR_ARG, name
    assert call(n_iter=0) == ERR_ARG
    assert call(d=s3.make_draws(1, 1025), n_iter=1025) == ERR_ARG
    assert call(d=s3.make_draws(1, 1024), n_iter=1024) == 0
    bad = d.copy()
    bad[7, 2] = -1
    assert call(d=bad) == ERR_ARG
    assert call(min_inliers=2) == ERR_ARG
    assert call(min_inliers=3) == 0
    assert call(probability=0.0) == ERR_ARG
    assert call(probability=1.0) == ERR_ARG
    assert call(max_iterations=0) == ERR_ARG
    k = dict(kf1, keys=kf1["keys"].copy())
    k["keys"]["octave"][4] = s3.NLEVELS
    assert call(kf1=k) == ERR_ARG
    k2 = dict(kf2, keys=kf2["keys"].copy())
    k2["keys"]["octave"][0] = -1
    assert call(kf2=k2) == ERR_ARG
    far = m.copy()
    far[np.nonzero(m >= 0)[0][0]] = len(kf2["keys"])
    assert call(m=far) == ERR_ARG
    assert call(cap=len(m) - 1) == ERR_CAPACITY
    assert call(kf1=dict(kf1, sigma2=-kf1["sigma2"])) == ERR_ARG
    big = 4097
    kb = dict(keys=s3.make_keys(big, 0), pos=np.zeros((big, 3), np.float32), valid=np.zeros(big, np.uint8),
              Tcw=np.eye(4, dtype=np.float32), cam=s3.CAM, sigma2=s3.SIGMA2)
    assert call(kf1=kb, m=np.full(big, -1, np.int32), idx1=None) == ERR_UNSUPPORTED
    q, keep = ox.sim3_query(kf1, kf2, m, d, **kw)
    assert lib.orbx_sim3_ransac_batch(ctx.handle, 0, ctypes.byref(q)) == ERR_ARG
    assert lib.orbx_dev_sim3_candidates(None, 0, None, 1, None, None, 0.75, 1, 20, 0.99, 20, 300, 5, None, None, 0,
                                        None, None, None) == ERR_ARG


def test_timer_counts_one_region_per_call(ctx):
    kf1, kf2, m, d, kw = pair(71, 64, M=16)
    try:
        ctx.timing(True, only="sim3")
        ctx.sim3_ransac(kf1, kf2, m, d, **kw)
        n, avg, tot = ctx.kernel_time("sim3")
        assert n == 1 and tot > 0
    finally:
        ctx.timing(False)


# ---------------------------------------------------------------------------
# device-resident frames
# ---------------------------------------------------------------------------
W, H, NF = 640, 480, 1000
SLOT_CAM = np.array([520.0, 520.0, 320.0, 240.0], np.float32)


def test_slot_form_equals_search_then_batch():
    from orb_slam_amd import synth
    from test_dev_bow_gpu import create_vocab, level_sigma2, search_kf
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
        rng = np.random.default_rng(5)
        sigma2 = level_sigma2()
        kfs = []
        for s in range(4):
            keys = feats[s][0]
            n = len(keys)
            depth = rng.uniform(3.0, 8.0, n)
            pos = np.stack([(keys["x"] - SLOT_CAM[2]) / SLOT_CAM[0] * depth, (keys["y"] - SLOT_CAM[3]) / SLOT_CAM[1] * depth,
                            depth], 1).astype(np.float32)
            T = np.eye(4, dtype=np.float32)
            T[:3, 3] = [0.05 * s, -0.02 * s, 0.01 * s]
            mp = rng.choice(3, n, p=(0.1, 0.8, 0.1)).astype(np.uint8)
            kfs.append(dict(keys=keys, mp=mp, pos=pos, Tcw=T, cam=SLOT_CAM, sigma2=sigma2))
        kfs[3]["mp"][12:] = 0                      # a candidate with few map points: below min_matches
        slots2, M = [1, 2, 3], 40
        draws = np.stack([s3.make_draws(90 + k, M) for k in range(3)])
        par = dict(min_inliers=6, probability=0.99, max_iterations=300)
        c.timing(True, only="sim3")
        dev = c.dev_sim3_candidates(0, kfs[0], slots2, [kfs[s] for s in slots2], draws, min_matches=20, taps=True, **par)
        assert c.kernel_time("sim3")[0] == 1
        c.timing(False)
        r, m12, nm = search_kf(c, 1, 0, kfs[0]["mp"], slots2, [kfs[s]["mp"] for s in slots2], cap=NF)
        assert r == 0
        n1 = len(feats[0][0])
        print(f"n1 {n1}, matches {nm.tolist()}, discarded {dev['discarded'].tolist()}, "
              f"N {[x['N'] for x in dev['results']]}")
        assert dev["n_matches"].tolist() == nm.tolist()
        assert dev["discarded"].tolist() == [int(x < 20) for x in nm] and dev["discarded"][2] == 1 and nm[0] >= 20
        qs = []
        for k, s in enumerate(slots2):
            assert dev["matches12"][k].tobytes() == m12[k].tobytes()
            side = lambda f: dict(f, valid=(f["mp"] == 1).astype(np.uint8))
            qs.append((side(kfs[0]), side(kfs[s]), m12[k][:n1], draws[k], par))
        host = c.sim3_ransac_batch(qs, taps=True)
        for k in range(3):
            d = dev["results"][k]
            if dev["discarded"][k]:
                assert d["N"] == 0 and not d["found"] and d["iters_run"] == 0 and not d["no_more"]
                assert not d["count"].any() and not d["inliers"].any()
                continue
            assert d["N"] >= 6
            same_result(d, host[k])
    finally:
        if voc:
            ox.lib().orbx_vocab_destroy(voc)
        c.close()


def test_batch_of_packed_lengths_in_either_order(ctx):
    """Three pairs in one batch whose arrays have 17, 0 and 31 entries (draws
    included): nothing is a multiple of the 16-byte packing step and an empty
    pair lies between the others; the first has idx1, the last does not.
    Every result is the single call's and passes layer 1, in either order."""
    a, b = s3.scene(60, 11, use_idx1=True, unmatched=2, invalid=1), s3.scene(61, 27, unmatched=2, invalid=1)
    assert len(a[0]["keys"]) == 17 and len(b[0]["keys"]) == 31 and a[3] is not None and b[3] is None

    def none_of(kf):
        return dict(kf, keys=kf["keys"][:0], pos=kf["pos"][:0], valid=kf["valid"][:0])

    qs = [(a[0], a[1], a[2], s3.make_draws(62, 17), dict(idx1=a[3], min_inliers=6)),
          (none_of(a[0]), none_of(a[1]), np.zeros(0, np.int32), s3.make_draws(63, 1), dict(idx1=None, min_inliers=6)),
          (b[0], b[1], b[2], s3.make_draws(64, 31), dict(idx1=None, min_inliers=6))]
    single = [ctx.sim3_ransac(*q[:4], taps=True, **q[4]) for q in qs]
    assert [r["N"] for r in single] == [11, 0, 27]
    for order in ((0, 1, 2), (2, 1, 0)):
        out = ctx.sim3_ransac_batch([qs[k] for k in order], taps=True)
        for r, k in zip(out, order):
            same_result(r, single[k])
            if k != 1:
                layer1(r, *qs[k])
        e = out[1]
        assert e["no_more"] == 1 and e["iters_run"] == 0 and e["ransac_max_its"] == 0 and not e["found"]
