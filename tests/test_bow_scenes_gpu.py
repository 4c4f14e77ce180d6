"""The vocabulary-node searches on the device at every gate's edge: the
hand-built scenes of tests/bow_scenes.py through the single-call and batch
entry points, against the oracle (oracle/ref_bow.cpp) and the vector written
in the scene; and the device-slot forms on what can be steered there -- a
one-node vocabulary (the widest node a slot can have), map-point states taken
from the oracle's own first pass, and a frame past the 2048-candidate limit.
Every comparison is exact: the match vector and n_matches."""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import bow_scenes as bs
from orb_slam_amd import synth
from bow_data import BowView
from test_bow_gpu import run_gpu
from test_bow_oracle import run_ref
from test_bow_scenes_numpy import wrong_rows
from test_dev_bow_gpu import create_vocab, level_sigma2, search, search_kf, translation_f12, view
from vocab_data import make_vocab, run_ref as ref_transform

pytestmark = pytest.mark.gpu

W, H = 640, 480
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=100, max_w=64, max_h=64, slots=1)
    yield c
    c.close()


# ---------------------------------------------------------------------------
# single-call entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", bs.CASES, ids=[f"{n}-m{m}" for n, m in bs.CASES])
def test_scene_single_call(ctx, name, mode):
    S = bs.scene(name, mode)
    go, gn = run_gpu(ctx, mode, S, S["nnratio"], S["check_ori"])
    ro, rn = run_ref(mode, S, S["nnratio"], S["check_ori"])
    assert not wrong_rows(S, go), wrong_rows(S, go)
    assert np.array_equal(go, ro) and gn == rn
    assert np.array_equal(go.astype(np.int64), S["want"]) and gn == S["n_want"]


def test_too_wide_node_is_unsupported(ctx):
    """2049 candidates in one node: ORBX_ERR_UNSUPPORTED, outputs untouched;
    2048 is served (widths2048 above)."""
    L = ox.lib()
    for mode in (0, 1, 2):
        S = bs.too_wide(mode)
        out = np.full(S["V2"].n if mode == 0 else S["V1"].n, 77, np.int32)
        n = ctypes.c_int(123)
        V1, V2 = ctypes.byref(S["V1"]), ctypes.byref(S["V2"])
        if mode == 0:
            r = L.orbx_search_by_bow_frame(ctx.handle, V1, V2, 0.75, 0, ox._ptr(out), ctypes.byref(n))
        elif mode == 1:
            r = L.orbx_search_by_bow_kf(ctx.handle, V1, V2, 0.75, 0, ox._ptr(out), ctypes.byref(n))
        else:
            r = L.orbx_search_for_triangulation(ctx.handle, V1, V2, ox._ptr(S["F12"]), ox._ptr(S["sigma2"]), 8, 0,
                                                ox._ptr(out), ctypes.byref(n))
        assert r == UNSUPPORTED and n.value == 123 and np.all(out == 77), mode


# ---------------------------------------------------------------------------
# batch entry points
# ---------------------------------------------------------------------------
def run_batch(ctx, mode, V1, jobs, nnratio, check_ori, fill=None):
    n = len(jobs)
    KF2s = (BowView * n)(*[S["V2"] for S in jobs])
    outs = [np.zeros(V1.n, np.int32) if fill is None else np.full(V1.n, fill, np.int32) for _ in range(n)]
    outp = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    nm = np.zeros(n, np.int32) if fill is None else np.full(n, fill, np.int32)
    L = ox.lib()
    if mode == 1:
        r = L.orbx_search_by_bow_kf_batch(ctx.handle, ctypes.byref(V1), n, KF2s, nnratio, check_ori, outp, ox._ptr(nm))
    else:
        F = np.ascontiguousarray(np.concatenate([S["F12"] for S in jobs]), np.float32)
        Sg = np.ascontiguousarray(np.concatenate([S["sigma2"] for S in jobs]), np.float32)
        r = L.orbx_search_for_triangulation_batch(ctx.handle, ctypes.byref(V1), n, KF2s, ox._ptr(F), ox._ptr(Sg), 8,
                                                  check_ori, outp, ox._ptr(nm))
    return r, outs, nm


def groups(mode):
    """The scenes of a mode by the arguments a batch call shares (mode 2 has
    no nnratio)."""
    g = {}
    for name, m in bs.CASES:
        if m == mode:
            S = bs.scene(name, mode)
            g.setdefault((S["nnratio"] if mode == 1 else 0.0, S["check_ori"]), []).append(S)
    return g


@pytest.mark.parametrize("mode", [1, 2], ids=["bow_kf", "triangulation"])
def test_scenes_as_batches(ctx, mode):
    """All scenes that share the call's arguments as one batch of unlike
    jobs: their KF1 sides joined into one keyframe, one job per KF2 side
    (each with its own F12 and sigma2), and an empty KF2."""
    seen_f12, seen_sig = set(), set()
    for (nnratio, check_ori), scenes in groups(mode).items():
        V1, keep1, jobs = bs.batch_jobs(scenes)
        E = bs.empty_kf2(mode)
        todo = [S for S, _ in jobs] + [E]
        r, outs, nm = run_batch(ctx, mode, V1, todo, nnratio, check_ori)
        assert r == 0, r
        for k, (S, first) in enumerate(jobs):
            want = np.full(V1.n, -1, np.int64)
            want[first:first + len(S["want"])] = S["want"]
            assert np.array_equal(outs[k].astype(np.int64), want) and nm[k] == S["n_want"], S["name"]
            P = {"V1": V1, "V2": S["V2"], "F12": S["F12"], "sigma2": S["sigma2"]}
            so, sn = run_gpu(ctx, mode, P, nnratio, check_ori)
            assert np.array_equal(outs[k], so) and nm[k] == sn, S["name"]
            seen_f12.add(S["F12"].tobytes())
            seen_sig.add(S["sigma2"].tobytes())
        assert nm[-1] == 0 and np.all(outs[-1] == -1)
    assert mode == 1 or (len(seen_f12) >= 3 and len(seen_sig) >= 2)


@pytest.mark.parametrize("mode", [1, 2], ids=["bow_kf", "triangulation"])
def test_batch_with_too_wide_node_is_unsupported(ctx, mode):
    S = bs.scene("distance", mode)
    V1, keep1, jobs = bs.batch_jobs([S, bs.too_wide(mode)])
    r, outs, nm = run_batch(ctx, mode, V1, [j for j, _ in jobs], 0.9, 0, fill=77)
    assert r == UNSUPPORTED
    assert np.all(nm == 77) and all(np.all(o == 77) for o in outs)


# ---------------------------------------------------------------------------
# device-slot forms
# ---------------------------------------------------------------------------
def one_node_vocab():
    """levelsup = L puts the FeatureVector at the root: the whole frame is
    one node.  No stopped words, so every feature is in it."""
    V = make_vocab(k=10, L=3, seed=21)
    V["weight"][V["weight"] == 0.0] = 1.0
    return V


@pytest.fixture(scope="module")
def dev():
    c = ox.Context(nfeatures=1000, max_w=W, max_h=H, slots=4)
    frames = synth.sequence(W, H, 3, seed=91)
    c.upload(np.stack(frames), 0)
    c.upload(synth.texture_frame(W, H, seed=5), 3)
    c.extract(0, 4)
    c.sync()
    feats = [c.features(s) for s in range(4)]
    V = one_node_vocab()
    voc = create_vocab(c, V)
    assert ox.lib().orbx_dev_compute_bow(c.handle, voc, 0, 4, V["L"]) == 0
    T = [ref_transform(V, d, V["L"]) for _, d in feats]
    for t, (k, _) in zip(T, feats):
        assert t["nf"] == 1 and t["fp"][1] == len(k) > 500          # one node holding every feature
    yield c, feats, T
    ox.lib().orbx_vocab_destroy(voc)
    c.close()


SLOTS2 = [1, 2, 3, 0]       # the next frames, an unrelated frame, the slot itself


def dev_pass(c, feats, T, mode, mps):
    """One device call of slot 0 against SLOTS2 under the map-point states
    mps[slot], checked against the oracle; returns the oracle's vectors."""
    views = [view(feats[s][0], feats[s][1], mps[s], T[s]) for s in range(4)]
    n0 = len(feats[0][0])
    ref = []
    if mode == 0:
        # the slot is F (never asked for states); the others are the keyframes
        r, outs, nm = search(c, 0, [views[s][0] for s in SLOTS2], 0.75, 1)
        assert r == 0, r
        for i, s in enumerate(SLOTS2):
            ro, rn = run_ref(0, {"V1": views[s][0], "V2": views[0][0]}, 0.75, 1)
            assert nm[i] == rn and np.array_equal(outs[i][:n0], ro), (mode, s)
            assert np.all(outs[i][n0:] == -1)
            ref.append((ro, rn))
        return ref
    F12s = np.concatenate([translation_f12(1.0, 0.0 if s == 0 else 0.3 * s) for s in SLOTS2]).astype(np.float32)
    sig = level_sigma2()
    r, outs, nm = search_kf(c, mode, 0, mps[0], SLOTS2, [mps[s] for s in SLOTS2], 0.75, 1, F12s,
                            np.tile(sig, len(SLOTS2)).astype(np.float32))
    assert r == 0, r
    for i, s in enumerate(SLOTS2):
        P = {"V1": views[0][0], "V2": views[s][0], "F12": F12s[9 * i:9 * i + 9].copy(), "sigma2": sig}
        ro, rn = run_ref(mode, P, 0.75, 1)
        assert nm[i] == rn and np.array_equal(outs[i][:n0], ro), (mode, s)
        assert np.all(outs[i][n0:] == -1)
        ref.append((ro, rn))
    return ref


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["bow_frame", "bow_kf", "triangulation"])
def test_dev_one_node_two_passes(dev, mode):
    """The whole frame in one node (16 chunks, the taken-mask in heavy use),
    every feature eligible; then a second pass in which exactly the features
    the oracle matched the first time are ineligible, so every row re-decides
    without its previous winner."""
    c, feats, T = dev
    ok = 0 if mode == 2 else 1
    mps = [np.full(len(k), ok, np.uint8) for k, _ in feats]
    first = dev_pass(c, feats, T, mode, mps)
    n0 = len(feats[0][0])
    # the slot against itself: every feature finds itself at distance 0 (mode
    # 2: a window of 0, on its own epipolar line) before the rotation filter,
    # which keeps all of bin 0
    ro, rn = first[3]
    assert rn > 0.9 * n0 and np.all((ro == np.arange(n0)) | (ro == -1))
    assert all(rn > 50 for _, rn in first[:2])
    # second pass: the first pass's winners get a bad map point (ineligible in
    # every mode) on the side the mode gates: KF2 in modes 1, 2, the
    # keyframe (side 1, the match vector's values) in mode 0
    mp2 = [m.copy() for m in mps]
    for i, s in enumerate(SLOTS2[:3]):
        ro, _ = first[i]
        mp2[s][ro[ro >= 0]] = 2
    second = dev_pass(c, feats, T, mode, mp2)
    for i, s in enumerate(SLOTS2[:3]):
        (ro, _), (so, sn) = first[i], second[i]
        assert sn > 0 and not np.any(np.isin(so[so >= 0], ro[ro >= 0])), (mode, s)


def test_dev_node_past_2048_is_unsupported():
    """A frame of more than 2048 keypoints under the one-node vocabulary: the
    three device forms return ORBX_ERR_UNSUPPORTED before any matching."""
    c = ox.Context(nfeatures=3000, max_w=W, max_h=H, slots=1)
    try:
        c.upload(synth.texture_frame(W, H, seed=5), 0)
        c.extract(0, 1)
        c.sync()
        kps, desc = c.features(0)
        assert len(kps) > 2048
        V = one_node_vocab()
        voc = create_vocab(c, V)
        try:
            assert ox.lib().orbx_dev_compute_bow(c.handle, voc, 0, 1, V["L"]) == 0
            t = ref_transform(V, desc, V["L"])
            assert t["nf"] == 1 and t["fp"][1] == len(kps)
            mp = np.ones(len(kps), np.uint8)
            small, keep = view(kps[:10], desc[:10], mp[:10], ref_transform(V, desc[:10], V["L"]))
            assert search(c, 0, [small], 0.75, 1)[0] == UNSUPPORTED
            assert search_kf(c, 1, 0, mp, [0], [mp])[0] == UNSUPPORTED
            mp0 = np.zeros(len(kps), np.uint8)
            assert search_kf(c, 2, 0, mp0, [0], [mp0], F12s=translation_f12(1.0, 0.0),
                             sigma2s=level_sigma2())[0] == UNSUPPORTED
        finally:
            ox.lib().orbx_vocab_destroy(voc)
    finally:
        c.close()
