"""New map points on the device (orbx_triangulate_matches,
orbx_create_new_map_points, orbx_dev_create_new_map_points) against the numpy
restatement (tests/newpoints_numpy.py) and the oracle's
SearchForTriangulation, in two layers: fed the device's null vectors (the v4
tap) the restatement must give the device's status and xyz bytes; the null
vectors themselves must agree with a float64 SVD to the final rounding
wherever the singular values separate them."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import newpoints_numpy as npn
import orb_slam_amd as ox
from orb_slam_amd import synth

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 500


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=NF, max_w=W, max_h=H, slots=6)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big():
    """The scene the shape cases are cut from (computed once)."""
    return npn.scene(31, 300, 3)


@pytest.fixture(scope="module")
def chain_case():
    return npn.unpack(np.load(Path(__file__).resolve().parent / "golden" / "new_points.npz"), "c_",
                      npn.CHAIN_CASE["n"])


def cut(S, n1, n):
    """The first n1 KF1 keypoints and n neighbours of a scene, with its truth matches."""
    return (S["keys1"][:n1], S["g1"], S["keys2"][:n], S["g2"][:n], [t[:n1] for t in S["truth"][:n]])


def assert_layer1(dev, keys1, g1, keys2, g2s, matches, contract=0):
    """The restatement fed the device's null vectors gives the device's bytes."""
    for k in range(len(keys2)):
        r = npn.triangulate(keys1, g1, keys2[k], g2s[k], matches[k], v4=dev["v4"][k], contract=contract)
        assert dev["status"][k].tobytes() == r["status"].tobytes(), (k, np.flatnonzero(dev["status"][k] != r["status"]))
        assert dev["xyz"][k].tobytes() == r["xyz"].tobytes(), k
        assert dev["n_created"][k] == r["n_created"], k
        ran = (r["status"] != 0) & (r["status"] != 2)
        assert not dev["v4"][k][~ran].any(), k       # the tap is written where the solve ran only


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n1", [1, 64, 65, 300])
def test_layer1_gates_bit_for_bit(ctx, big, n1, n):
    keys1, g1, keys2, g2s, m = cut(big, n1, n)
    if n1 == 1:
        m = [np.array([max(int(big["truth"][k].max()), 0)], np.int32) for k in range(n)]   # a match for the one keypoint
    dev = ctx.triangulate_matches(keys1, g1, keys2, g2s, m, v4=True)
    assert_layer1(dev, keys1, g1, keys2, g2s, m)
    if n1 >= 64:
        assert sum(dev["n_created"]) > 0


def test_no_matches_and_no_keypoints(ctx, big):
    keys1, g1, keys2, g2s, m = cut(big, 65, 3)
    dev = ctx.triangulate_matches(keys1, g1, keys2, g2s, [np.full(65, -1, np.int32)] * 3, v4=True)
    assert not any(s.any() for s in dev["status"]) and not dev["n_created"].any()
    assert not any(x.any() for x in dev["xyz"]) and not any(v.any() for v in dev["v4"])
    # n1 = 0 (and n = 0): ORBX_OK, nothing touched
    dev = ctx.triangulate_matches(keys1[:0], g1, keys2, g2s, [np.zeros(0, np.int32)] * 3)
    assert dev["n_created"].tolist() == [0, 0, 0]
    assert ctx.triangulate_matches(keys1, g1, [], [], [])["n_created"].size == 0


def test_layer2_null_vectors(ctx, big):
    """Above the cut (s3 - s4) / s1 >= 1e-4 both solves are accurate to about
    eps64 s1 / gap = 2e-12 relative, so they differ in the final rounding at
    most: within one float32 ulp of the vector's largest entry after sign
    alignment."""
    keys1, g1, keys2, g2s, m = cut(big, 300, 3)
    dev = ctx.triangulate_matches(keys1, g1, keys2, g2s, m, v4=True)
    solved = above = equal = 0
    for k in range(3):
        r = npn.triangulate(keys1, g1, keys2[k], g2s[k], m[k])
        ran = ~np.isnan(r["gap"])
        ok = ran & (r["gap"] >= 1e-4)
        solved, above = solved + int(ran.sum()), above + int(ok.sum())
        a, b = dev["v4"][k][ok], r["v4"][ok]
        sign = np.sign(np.sum(a.astype(np.float64) * b.astype(np.float64), axis=1, keepdims=True))
        assert np.all(sign != 0)
        d = np.abs(a.astype(np.float64) - sign * b.astype(np.float64)).max(axis=1)
        ulp = np.spacing(np.abs(b).max(axis=1).astype(np.float32))
        equal += int(np.count_nonzero(d == 0))
        assert np.all(d <= ulp), (k, float((d / ulp).max()))
        # unit vectors
        assert np.all(np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1) < 1e-6)
    print(f"null vectors: {solved} solved, {above} above the cut, {equal} bit-equal to the float64 SVD")
    assert solved > 300 and above >= 0.95 * solved


def test_both_fp_contract_modes(ctx, big):
    keys1, g1, keys2, g2s, m = cut(big, 300, 3)
    try:
        ctx.set_fp_contract(1)
        dev = ctx.triangulate_matches(keys1, g1, keys2, g2s, m, v4=True)
        assert_layer1(dev, keys1, g1, keys2, g2s, m, contract=1)
    finally:
        ctx.set_fp_contract(0)
    dev = ctx.triangulate_matches(keys1, g1, keys2, g2s, m, v4=True)
    assert_layer1(dev, keys1, g1, keys2, g2s, m, contract=0)


def test_fp_contract_modes_on_matches_where_they_differ(ctx):
    """The fixture's three matches at the reprojection threshold, on which the
    restatement's two modes give different statuses: layer 1 in each mode,
    so a kernel that ignored the mode would miss one of them."""
    G = np.load(Path(__file__).resolve().parent / "golden" / "new_points.npz")
    keys1, g1, keys2, g2, m = npn.unpack_contract(G)
    st = []
    try:
        for c in (1, 0):
            ctx.set_fp_contract(c)
            dev = ctx.triangulate_matches(keys1, g1, [keys2], [g2], [m], v4=True)
            assert_layer1(dev, keys1, g1, [keys2], [g2], [m], contract=c)
            st.append(dev["status"][0])
            print(f"mode {c}: status {dev['status'][0].tolist()}, null vectors equal to the fixture's up to sign: "
                  f"{int(np.count_nonzero((np.abs(dev['v4'][0]) == np.abs(G['f_v4'])).all(axis=1)))} of {len(m)}")
    finally:
        ctx.set_fp_contract(0)
    # the statuses are decided on the device's own null vectors; where those are the fixture's (up to the
    # unspecified sign), so are the statuses, which differ between the modes
    if np.array_equal(np.abs(dev["v4"][0]), np.abs(G["f_v4"])):
        assert st[0].tobytes() == G["f_status1"].tobytes() and st[1].tobytes() == G["f_status0"].tobytes()


def search_batch(ctx, V1, V2s, F12s, sigma2s, nlevels, check_ori):
    n = len(V2s)
    outs = [np.zeros(V1.n, np.int32) for _ in range(n)]
    nm = np.zeros(n, np.int32)
    arr = (type(V1) * n)(*V2s)
    F = np.ascontiguousarray(np.concatenate(F12s), np.float32)
    s2 = np.ascontiguousarray(np.concatenate(sigma2s), np.float32)
    r = ox.lib().orbx_search_for_triangulation_batch(ctx.handle, ctypes.byref(V1), n, arr, ox._ptr(F), ox._ptr(s2),
                                                     nlevels, check_ori, ox._ptr_array(outs), ox._ptr(nm))
    assert r == 0, r
    return outs, nm


def assert_same_result(a, b, n, length=None):
    for k in range(n):
        for name in ("matches12", "status", "xyz", "v4"):
            x, y = a[name][k], b[name][k]
            if length is not None:
                x, y = x[:length], y[:length]
            assert x.tobytes() == y.tobytes(), (name, k)
    assert np.array_equal(a["n_matches"], b["n_matches"]) and np.array_equal(a["n_created"], b["n_created"])


@pytest.mark.parametrize("check_ori", [0, 1])
def test_unchained_equals_search_then_triangulate(ctx, chain_case, check_ori):
    S = chain_case
    V1, V2s, keep = npn.views(S)
    dev = ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], np.concatenate(S["F12"]), check_ori=check_ori,
                                    chain=False, v4=True)
    m, nm = search_batch(ctx, V1, V2s, S["F12"], [g["level_sigma2"] for g in S["g2"]], npn.NLEVELS, check_ori)
    tri = ctx.triangulate_matches(S["keys1"], S["g1"], S["keys2"], S["g2"], m, v4=True)
    tri["matches12"], tri["n_matches"] = m, nm
    assert_same_result(dev, tri, len(V2s))
    assert nm.min() > 50 and dev["n_created"].min() > 20


def test_chained_equals_the_reference_loop(ctx, chain_case):
    S = chain_case
    n = len(S["keys2"])
    V1, V2s, keep = npn.views(S)
    F = np.concatenate(S["F12"])
    dev = ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], F, chain=True, v4=True)
    ref = npn.replay(S, 1, v4s=dev["v4"])
    for k, r in enumerate(ref):
        assert dev["matches12"][k].tobytes() == r["matches12"].tobytes(), k
        assert dev["n_matches"][k] == r["n_matches"], k
        assert dev["status"][k].tobytes() == r["status"].tobytes(), k
        assert dev["xyz"][k].tobytes() == r["xyz"].tobytes(), k
        assert dev["n_created"][k] == r["n_created"], k
    # the caller's states are not written, and the unchained call differs
    assert S["mp1"].tobytes() == keep[0]["mp"].tobytes()
    flat = ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], F, chain=False)
    assert np.array_equal(flat["matches12"][0], dev["matches12"][0])
    assert any(not np.array_equal(flat["matches12"][k], dev["matches12"][k]) for k in range(1, n))
    freed = (dev["matches12"][1] >= 0) & (dev["matches12"][1] != flat["matches12"][1])
    assert freed.any()


def test_batch_equals_single_neighbour_calls(ctx, chain_case):
    S = chain_case
    V1, V2s, keep = npn.views(S)
    both = ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], np.concatenate(S["F12"]), chain=False, v4=True)
    for k in range(len(V2s)):
        one = ctx.create_new_map_points(V1, S["g1"], [V2s[k]], [S["g2"][k]], S["F12"][k], chain=False, v4=True)
        for name in ("matches12", "status", "xyz", "v4"):
            assert one[name][0].tobytes() == both[name][k].tobytes(), (name, k)
        assert one["n_matches"][0] == both["n_matches"][k] and one["n_created"][0] == both["n_created"][k]


# ---------------------------------------------------------------------------
# device-resident frames
# ---------------------------------------------------------------------------
SLOT_CAM = np.array([120.0, 120.0, 80.0, 60.0], np.float32)


@pytest.fixture(scope="module")
def slots(ctx):
    """Four extracted frames with their BoW on the device, their read-back
    features and FeatureVectors, and synthetic poses with the F12 of each
    neighbour."""
    from test_dev_bow_gpu import create_vocab, read_bow
    from vocab_data import make_vocab
    frames = synth.sequence(W, H, 4, seed=17)
    ctx.upload(np.stack(frames), 0)
    ctx.extract(0, 4)
    ctx.sync()
    V = make_vocab(k=10, L=4, seed=3)
    voc = create_vocab(ctx, V)
    assert ox.lib().orbx_dev_compute_bow(ctx.handle, voc, 0, 4, 2) == 0
    feats = [ctx.features(s) for s in range(4)]
    bows = [read_bow(ctx, s, len(feats[s][0])) for s in range(4)]
    rng = np.random.default_rng(4)
    geoms = [npn.make_geom(npn._rot(rng.normal(0, 0.01, 3)), np.array([-0.2 * s, 0.01 * s, 0.0]), cam=SLOT_CAM)
             for s in range(4)]
    yield dict(feats=feats, bows=bows, geoms=geoms)
    ox.lib().orbx_vocab_destroy(voc)


@pytest.mark.parametrize("chain", [0, 1])
def test_slot_form_equals_host_form(ctx, slots, chain):
    from test_dev_bow_gpu import view
    feats, bows, geoms = slots["feats"], slots["bows"], slots["geoms"]
    rng = np.random.default_rng(9)
    mps = [rng.choice(3, len(f[0]), p=(0.85, 0.1, 0.05)).astype(np.uint8) for f in feats]
    slots2 = [1, 2, 3]
    F = np.concatenate([npn.compute_f12(geoms[0], geoms[s]) for s in slots2])
    dev = ctx.dev_create_new_map_points(0, mps[0], geoms[0], slots2, [mps[s] for s in slots2],
                                        [geoms[s] for s in slots2], F, chain=chain, v4=True)
    vs = [view(feats[s][0], feats[s][1], mps[s], bows[s]) for s in range(4)]
    host = ctx.create_new_map_points(vs[0][0], geoms[0], [vs[s][0] for s in slots2], [geoms[s] for s in slots2], F,
                                     chain=chain, v4=True)
    n1 = len(feats[0][0])
    assert n1 > 50
    assert_same_result(dev, host, 3, length=n1)
    for k in range(3):
        assert np.all(dev["matches12"][k][n1:] == -1) and not dev["status"][k][n1:].any()
    print(f"slot form, chain {chain}: matches {dev['n_matches'].tolist()}, created {dev['n_created'].tolist()}")


def code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except ox.OrbxError as e:
        return e.code
    return 0


def test_argument_rules(ctx, big, chain_case, slots):
    keys1, g1, keys2, g2s, m = cut(big, 65, 2)
    tri = ctx.triangulate_matches
    L = ox.lib()
    assert L.orbx_triangulate_matches(None, None, 1, None, 1, None, None, None, None, None, None, None, None) == -1
    assert L.orbx_triangulate_matches(ctx.handle, ox._ptr(keys1), 65, None, 2, None, None, None, None, None, None, None,
                                      None) == -1                                   # a null required pointer
    assert code(tri, keys1, dict(g1, nlevels=1), keys2, g2s, m) == -1
    assert code(tri, keys1, g1, keys2, [g2s[0], dict(g2s[1], nlevels=17)], m) == -1
    bad = keys1.copy()
    bad["octave"][3] = npn.NLEVELS
    assert code(tri, bad, g1, keys2, g2s, m) == -1
    bad2 = keys2[1].copy()
    bad2["octave"][0] = -1
    assert code(tri, keys1, g1, [keys2[0], bad2], g2s, m) == -1
    mm = m[1].copy()
    mm[5] = len(keys2[1])
    assert code(tri, keys1, g1, keys2, g2s, [m[0], mm]) == -1
    assert code(tri, keys1, g1, keys2, g2s, m) == 0
    # the loop forms
    S = chain_case
    V1, V2s, keep = npn.views(S)
    F = np.concatenate(S["F12"])
    cnp = ctx.create_new_map_points
    assert L.orbx_create_new_map_points(None, None, None, 1, None, None, None, 0, 1, None, None, None, None, None,
                                        None) == -1
    assert code(cnp, V1, S["g1"], [V2s[0], V2s[0]], S["g2"][:2], F[:18], chain=True) == -1     # a KF2 listed twice
    assert code(cnp, V1, S["g1"], [V2s[0], V2s[0]], S["g2"][:2], F[:18], chain=False) == 0
    assert code(cnp, V1, dict(S["g1"], nlevels=1), V2s, S["g2"], F) == -1
    assert cnp(V1, S["g1"], [], [], np.zeros(0, np.float32))["n_created"].size == 0             # n = 0
    # the slot form
    geoms = slots["geoms"]
    mp = np.zeros(NF, np.uint8)
    dnp = ctx.dev_create_new_map_points
    F2 = np.concatenate([npn.compute_f12(geoms[0], geoms[s]) for s in (1, 2)])
    args = (0, mp, geoms[0], [1, 2], [mp, mp], [geoms[1], geoms[2]], F2)
    assert code(dnp, *args) == 0
    assert code(dnp, *args, cap=NF - 1) == -3
    assert code(dnp, 0, mp, geoms[0], [1, 1], [mp, mp], [geoms[1], geoms[1]], F2, chain=True) == -1   # a slot twice
    assert code(dnp, 0, mp, geoms[0], [1, 1], [mp, mp], [geoms[1], geoms[1]], F2, chain=False) == 0
    g7 = npn.make_geom(np.eye(3), [0, 0, 0], cam=SLOT_CAM, nlevels=7)
    assert code(dnp, 0, mp, g7, [1, 2], [mp, mp], [geoms[1], geoms[2]], F2) == -1            # not the extractor's nlevels
    assert code(dnp, 0, mp, geoms[0], [1, 6], [mp, mp], [geoms[1], geoms[2]], F2) == -1      # no such slot
    assert code(dnp, 0, mp, geoms[0], [], [], [], np.zeros(0, np.float32)) == 0


def test_timer_counts_the_launches(ctx, chain_case):
    S = chain_case
    V1, V2s, keep = npn.views(S)
    F = np.concatenate(S["F12"])
    try:
        ctx.timing(True, only="triangulate")
        ctx.triangulate_matches(S["keys1"], S["g1"], S["keys2"], S["g2"], S["truth"])
        n, avg, tot = ctx.kernel_time("triangulate")
        assert n == 1 and tot > 0
        ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], F, chain=False)
        assert ctx.kernel_time("triangulate")[0] == 1
        ctx.create_new_map_points(V1, S["g1"], V2s, S["g2"], F, chain=True)
        assert ctx.kernel_time("triangulate")[0] == len(V2s)
    finally:
        ctx.timing(False)


def test_neighbours_of_packed_lengths_in_either_order(ctx, big):
    """Three neighbours in one call with 31, 0 and 17 keypoints against 17 of
    KF1: nothing is a multiple of the 16-byte packing step and an empty
    neighbour lies between the others.  The outer ones pass layer 1, the empty
    one creates nothing, and every neighbour's result is its single call's, in
    either order."""
    keys1, g1, keys2, g2s, m = cut(big, 17, 3)
    keys2 = [keys2[0][:31], keys2[1][:0], keys2[2][:17]]
    m = [np.where(t < len(k), t, -1).astype(np.int32) for t, k in zip(m, keys2)]
    assert [len(k) for k in keys2] == [31, 0, 17] and (m[0] >= 0).any() and (m[2] >= 0).any()
    single = [ctx.triangulate_matches(keys1, g1, [keys2[k]], [g2s[k]], [m[k]], v4=True) for k in range(3)]
    for order in ((0, 1, 2), (2, 1, 0)):
        dev = ctx.triangulate_matches(keys1, g1, [keys2[k] for k in order], [g2s[k] for k in order],
                                      [m[k] for k in order], v4=True)
        for pos, k in enumerate(order):
            for name in ("status", "xyz", "v4"):
                assert dev[name][pos].tobytes() == single[k][name][0].tobytes(), (name, k)
            assert dev["n_created"][pos] == single[k]["n_created"][0]
        assert not dev["status"][1].any() and dev["n_created"][1] == 0 and not dev["xyz"][1].any()
    for k in (0, 2):
        assert_layer1(single[k], keys1, g1, [keys2[k]], [g2s[k]], [m[k]])
