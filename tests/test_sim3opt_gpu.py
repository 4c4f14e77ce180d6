"""Optimizer::OptimizeSim3 on the device (orbx_optimize_sim3) against the numpy
restatement tests/sim3opt_numpy.py.  The reference cannot be built next to the
tests, so the comparison has two layers, like tests/test_sim3_gpu.py.

Layer 1, byte for byte, each step fed the DEVICE's own state:
* the correspondence indices and the camera-frame points;
* for every LM iteration the device ran, linearize() at the device's estimate
  gives the device's chi2, H and b; for the first iteration also every edge's
  error and Jacobian entry (the whole linearisation needs + - * /, sqrt and two
  constant exponentials only);
* each check's per-edge chi2 from the estimate of the round's last trial, est
  (+) dx of the tapped last trial: byte for byte.  That update goes through
  exp / sin / cos of two maths libraries, so the device also taps the estimate
  it tested at (check_est): the chi2 are recomputed byte for byte from it as
  well, which holds whatever the libraries return, and check_est is held to
  numpy's est (+) dx within 1e-13 max(1, |x|);
* the flags, n_bad, n_in, the early exit and the return value follow from those
  chi2 by the reference's rule (a NaN keeps the pair).

Layer 2, end to end against the restatement's own run: matches12, n_corr,
n_bad, n_in, returned_early and round 0's iteration and trial counts identical;
q12 (sign-aligned), t12d and s12d within 1e-6 max(1, |x|), the bar of
tests/test_pose_numpy.py (only the FP64 sin / cos / exp of two libraries in the
LM update stand between the runs; the worst difference is printed per case and
recorded in DESIGN.md section 4).  Later rounds restart near convergence,
where accept / reject turns on rounding: their counts are printed, not
compared.  The float R12 / t12 / s12 equal the conversion of the device's
doubles byte for byte.

The cases (sim3opt_numpy.CASES) are the smallest at which each path can go
wrong; tests/test_sim3opt_numpy.py asserts on the CPU that every tested chi2
of every case lies outside th2 (1 +- 1e-3).
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import sim3opt_numpy as so
from test_lba_numpy import quat_matrix

pytestmark = pytest.mark.gpu
TH2 = so.TH2


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=2)
    yield c
    c.close()


def run(ctx, name, taps=True):
    (kf1, kf2, m, init), ref = so.case(name)
    return ctx.optimize_sim3(kf1, kf2, m, *init, th2=TH2, taps=taps), ref, (kf1, kf2, m, init)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def is_bad(c):
    with np.errstate(invalid="ignore"):
        return (c[:, 0] > TH2) | (c[:, 1] > TH2)   # a NaN keeps the pair


@pytest.mark.parametrize("name", list(so.CASES))
def test_layer1_every_step_from_the_device_state(ctx, name):
    d, _, (kf1, kf2, m, init) = run(ctx, name)
    pb = so.build_problem(kf1, kf2, m, TH2)
    n = len(pb["idx"])
    assert d["n_corr"] == n == so.CASES[name][0]
    assert bits(d["corr_index"]) == bits(pb["idx"])
    assert bits(d["x3dc1"]) == bits(pb["x3dc1"]) and bits(d["x3dc2"]) == bits(pb["x3dc2"])
    expect = np.array(m, np.int32)
    if n == 0:
        assert d["returned_early"] == 1 and d["n_in"] == 0 and d["n_lm"] == 0 and d["q12"] is None
        assert bits(d["matches12"]) == bits(expect)
        return
    it0 = d["iterations"][0]
    assert d["n_lm"] == it0 + d["iterations"][1] and 1 <= it0 <= 5

    def last_trial_estimate(k):
        return so.oplus(d["it_est"][k], d["it_dx"][k][d["it_trials"][k] - 1])

    def check(r, k_last, tested):
        want = last_trial_estimate(k_last)
        got = d["check_est"][r]
        assert np.all(np.abs(want - got) <= 1e-13 * np.maximum(1, np.abs(got)))
        c = so.stored_chi2(got, pb)
        assert bits(d["edge_chi2"][r][tested]) == bits(c[tested])
        # and from est (+) dx as numpy forms it: the same bytes wherever the two libraries' exp / sin / cos
        # agree at the update's arguments, which they do for every case here
        assert bits(d["edge_chi2"][r][tested]) == bits(so.stored_chi2(want, pb)[tested])
        assert np.isnan(d["edge_chi2"][r][~tested]).all()
        return tested & is_bad(c)

    def linearise_round(first, count):
        for k in range(first, first + count):
            chi, h, b, err, J = so.linearize(d["it_est"][k], pb)
            assert bits(d["it_chi2"][k]) == bits(np.float64(chi)), (k, chi, d["it_chi2"][k])
            assert bits(d["it_H"][k]) == bits(h) and bits(d["it_b"][k]) == bits(b), k
            if k == 0:
                assert bits(d["edge_err"]) == bits(err)
                assert bits(d["edge_J"]) == bits(J)
            assert 1 <= d["it_trials"][k] <= 10

    linearise_round(0, it0)
    bad0 = check(0, it0 - 1, np.ones(n, bool))
    expect[pb["idx"][bad0]] = -1
    assert d["n_bad"] == int(bad0.sum())
    if n - d["n_bad"] < 10:
        assert d["returned_early"] == 1 and d["n_in"] == 0 and d["iterations"][1] == 0
        assert d["q12"] is None and d["R12"] is None
        assert np.isnan(d["edge_chi2"][1]).all()
    else:
        assert d["returned_early"] == 0
        pb["active"] = ~bad0
        assert 1 <= d["iterations"][1] <= (10 if d["n_bad"] else 5)
        linearise_round(it0, d["iterations"][1])
        bad1 = check(1, d["n_lm"] - 1, ~bad0)
        expect[pb["idx"][bad1]] = -1
        assert d["n_in"] == int((~bad0 & ~bad1).sum())
    assert bits(d["matches12"]) == bits(expect)
    # the skipped entries stay as they were
    skipped = np.setdiff1d(np.arange(len(m)), pb["idx"])
    assert bits(d["matches12"][skipped]) == bits(np.asarray(m, np.int32)[skipped])


@pytest.mark.parametrize("name", list(so.CASES))
def test_layer2_against_the_restatement(ctx, name):
    d, ref, _ = run(ctx, name)
    assert bits(d["matches12"]) == bits(ref["matches12"])
    for k in ("n_corr", "n_bad", "n_in", "returned_early"):
        assert d[k] == ref[k], k
    assert d["iterations"][0] == ref["iterations"][0] and d["trials"][0] == ref["trials"][0]
    print(f"{name}: round 1 iterations / trials device {d['iterations'][1]} / {d['trials'][1]}, "
          f"restatement {ref['iterations'][1]} / {ref['trials'][1]}; LDLT failures {d['not_posdef']}")
    if ref["returned_early"]:
        assert d["q12"] is None and d["t12"] is None
        return
    est = np.concatenate([d["q12"], d["t12d"], [d["s12d"]]])
    want = ref["est"].copy()
    if est[:4] @ want[:4] < 0:
        want[:4] = -want[:4]
    rel = np.abs(est - want) / np.maximum(1, np.abs(want))
    print(f"{name}: worst |device - restatement| / max(1, |x|) = {rel.max():.3e}")
    assert rel.max() <= 1e-6
    assert bits(d["R12"]) == bits(quat_matrix(est[:4]).astype(np.float32))
    assert bits(d["t12"]) == bits(est[4:7].astype(np.float32)) and bits(d["s12"]) == bits(np.float32(est[7]))


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), k
        else:
            assert a[k] == b[k], k


MIXED = ("n40_gross", "n0", "n12_gross3", "n65", "n9", "n130_clean", "behind", "n10")


def test_batch_equals_single_calls_in_either_order(ctx):
    args = [so.case(name)[0] for name in MIXED]
    args = [(a[0], a[1], a[2], *a[3]) for a in args]
    single = [ctx.optimize_sim3(*a, th2=TH2, taps=True) for a in args]
    for order in (list(range(8)), list(range(7, -1, -1))):
        batch = ctx.optimize_sim3_batch([args[k] for k in order], th2=TH2, taps=True)
        for pos, k in enumerate(order):
            same(batch[pos], single[k])
    assert any(s["returned_early"] for s in single) and any(s["n_in"] >= 20 for s in single)


def test_two_runs_are_byte_equal_with_and_without_taps(ctx):
    a, _, _ = run(ctx, "n257")
    b, _, _ = run(ctx, "n257")
    same(a, b)
    c, _, _ = run(ctx, "n257", taps=False)
    for k in c:
        if isinstance(c[k], np.ndarray):
            assert bits(c[k]) == bits(a[k]), k
        else:
            assert c[k] == a[k], k


def test_refused_call_leaves_the_callers_arrays(ctx):
    (kf1, kf2, m, init), _ = so.case("n40_gross")
    lib = ox.lib()
    for breakage in ("th2", "s12", "index", "octave", "nlevels"):
        q, keep = ox.sim3_opt_query(kf1, kf2, m, *init, th2=TH2, taps=True)
        if breakage == "th2":
            q.th2 = -1.0
        elif breakage == "s12":
            q.s12 = float("nan")
        elif breakage == "index":
            keep["matches12"][np.argmax(keep["matches12"] >= 0)] = q.n2
        elif breakage == "octave":
            keep["keys2"] = keep["keys2"].copy()      # the case's arrays are shared
            keep["keys2"]["octave"][3] = q.nlevels
            q.keys2 = keep["keys2"].ctypes.data
        else:
            q.nlevels = 17
        before = {k: v.copy() for k, v in keep.items()}
        r12 = list(q.R12)
        assert lib.orbx_optimize_sim3(ctx.handle, ctypes.byref(q)) == -1, breakage
        for k, v in keep.items():
            assert bits(v) == bits(before[k]), (breakage, k)
        assert list(q.R12) == r12
    for field, value, code in (("n1", 4097, -4), ("n2", 4097, -4), ("n1", -1, -1), ("pos2", None, -1),
                               ("inv_sigma2_1", None, -1), ("matches12", None, -1)):
        q, keep = ox.sim3_opt_query(kf1, kf2, m, *init, th2=TH2)
        setattr(q, field, value)
        assert lib.orbx_optimize_sim3(ctx.handle, ctypes.byref(q)) == code, field
        assert bits(keep["matches12"]) == bits(np.asarray(m, np.int32))
    q, keep = ox.sim3_opt_query(kf1, kf2, m, *init, th2=TH2, taps=True, cap=39)
    assert lib.orbx_optimize_sim3(ctx.handle, ctypes.byref(q)) == -3
    assert bits(keep["matches12"]) == bits(np.asarray(m, np.int32))


def test_timer_counts_one_region_per_call(ctx):
    (kf1, kf2, m, init), _ = so.case("n64")
    try:
        ctx.timing(True, only="sim3opt")
        ctx.optimize_sim3(kf1, kf2, m, *init, th2=TH2)
        n, avg, tot = ctx.kernel_time("sim3opt")
        assert n == 1 and tot > 0
    finally:
        ctx.timing(False)


# ---------------------------------------------------------------------------
# device-resident frames
# ---------------------------------------------------------------------------
W, H, NF = 640, 480, 1000
SLOT_CAM = np.array([520.0, 520.0, 320.0, 240.0], np.float32)


def test_slot_form_equals_the_host_array_form():
    from orb_slam_amd import synth
    from test_dev_bow_gpu import level_sigma2
    c = ox.Context(nfeatures=NF, max_w=W, max_h=H, slots=3)
    try:
        c.upload(np.stack(synth.sequence(W, H, 3, seed=29)), 0)
        c.extract(0, 3)
        c.sync()
        feats = [c.features(s)[0] for s in range(3)]
        rng = np.random.default_rng(6)
        sigma2 = level_sigma2()
        inv = (np.float32(1) / sigma2).astype(np.float32)
        kfs = []
        for s in range(3):
            keys = feats[s]
            n = len(keys)
            depth = rng.uniform(3.0, 8.0, n)
            pos = np.stack([(keys["x"] - SLOT_CAM[2]) / SLOT_CAM[0] * depth, (keys["y"] - SLOT_CAM[3]) / SLOT_CAM[1] * depth,
                            depth], 1).astype(np.float32)
            mp = rng.choice(3, n, p=(0.1, 0.8, 0.1)).astype(np.uint8)
            kfs.append(dict(keys=keys, mp=mp, pos=pos, Tcw=np.eye(4, dtype=np.float32), cam=SLOT_CAM, sigma2=sigma2,
                            inv_sigma2=inv))
        n1 = len(feats[0])
        # candidate 0: the keyframe against itself (every point its own partner, so the identity fits);
        # candidate 1, 2: unrelated partners (every pair gross: the early exit)
        slots2 = [0, 1, 2]
        m12 = []
        for s in slots2:
            n2 = len(feats[s])
            m = np.where(np.arange(n1) < n2, np.arange(n1), -1).astype(np.int32) if s == 0 else \
                rng.integers(0, n2, n1).astype(np.int32)
            m[rng.choice(n1, n1 // 5, replace=False)] = -1
            m[rng.choice(n1, 7, replace=False)] = -2
            m12.append(m)
        sims = [(so._rot([0.01, -0.02, 0.015]).astype(np.float32), np.array([0.05, -0.03, 0.04], np.float32),
                 np.float32(1.03))] * 3
        dev = c.dev_optimize_sim3(0, kfs[0], slots2, [kfs[s] for s in slots2], m12, sims, th2=TH2, taps=True)
        side = lambda f: dict(f, valid=(f["mp"] == 1).astype(np.uint8))
        host = c.optimize_sim3_batch([(side(kfs[0]), side(kfs[s]), m12[k], *sims[k]) for k, s in enumerate(slots2)],
                                     th2=TH2, taps=True)
        print([(x["n_corr"], x["n_bad"], x["n_in"], x["returned_early"]) for x in dev])
        for k in range(3):
            same(dev[k], host[k])
        assert dev[0]["n_in"] >= 100 and not dev[0]["returned_early"]
        assert abs(dev[0]["s12d"] - 1) < 0.03     # the start is 3 % off
        assert dev[1]["returned_early"] and dev[1]["n_corr"] > 100
    finally:
        c.close()


def test_batch_of_packed_lengths_in_either_order(ctx):
    """Three candidates in one batch whose keyframes have 17, 0 and 31
    keypoints: nothing is a multiple of the 16-byte packing step and an empty
    candidate lies between the others; the first asks for taps, the others do
    not.  Every result is the single call's, in either order."""
    kw = dict(null=2, invalid=2, unobserved=2, extra2=6, gross=0.2)
    args = [so.scene(520, 9, **kw), None, so.scene(521, 23, **kw)]
    kf1, kf2 = args[0][:2]

    def none_of(kf):
        return dict(kf, keys=kf["keys"][:0], pos=kf["pos"][:0], valid=kf["valid"][:0])

    args[1] = (none_of(kf1), none_of(kf2), np.zeros(0, np.int32), args[0][3])
    args = [(a[0], a[1], a[2], *a[3]) for a in args]
    assert [len(a[0]["keys"]) for a in args] == [17, 0, 31]
    taps = (True, False, False)
    single = [ctx.optimize_sim3(*args[k], th2=TH2, taps=taps[k]) for k in range(3)]
    assert [s["n_corr"] for s in single] == [9, 0, 23]
    for order in ((0, 1, 2), (2, 1, 0)):
        built = [ox.sim3_opt_query(*args[k], th2=TH2, taps=taps[k]) for k in order]
        arr = (ox.Sim3OptQuery * 3)(*[b[0] for b in built])
        assert ox.lib().orbx_optimize_sim3_batch(ctx.handle, 3, arr) == 0
        for pos, k in enumerate(order):
            same(ox.sim3_opt_result(arr[pos], built[pos][1], taps[k]), single[k])
    pb = so.build_problem(args[0][0], args[0][1], args[0][2], TH2)
    assert bits(single[0]["corr_index"]) == bits(pb["idx"]) and bits(single[0]["x3dc1"]) == bits(pb["x3dc1"])
    assert single[1]["returned_early"] == 1 and single[1]["n_in"] == 0
