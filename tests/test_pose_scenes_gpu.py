"""The device's keyframe projection searches (orbx_kfproj.hip) on the
constructed scenes of tests/pose_scenes.py: general poses, a rejected and an
accepted point at every gate, exact edges, and a searched keyframe of
kMaxFeatures keypoints.

For every scene and entry point the device result is byte for byte the
oracle's (all points, undecided ones included), and the decided points equal
the float64 reference's expectation.  Each case is one small launch.
"""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import pose_scenes as ps
import proj_data as pd
from oracle_lib import ptr
from test_pose_scenes_numpy import CAP, RUN_IDS, RUNS, compare, frustum_scene
from test_proj_oracle import ref_distinctive

pytestmark = pytest.mark.gpu
ORBX_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=100, max_w=64, max_h=64, slots=1)
    yield c
    c.close()


def device_is_oracle(s, entry, scale, orb, ori, handle, nq=None):
    """Byte for byte on every point, then the decided ones against float64."""
    want = ps.run(s, entry, None, scale, orb, ori, nq=nq)
    res, got, share = compare(s, entry, scale, orb, ori, handle, nq=nq)
    assert want[0] == 0
    assert np.array_equal(got[1], want[1])
    if entry in ("fuse0", "fuse1"):
        assert np.array_equal(got[2], want[2])
    else:
        assert got[2] == want[2]
    return res, got, share


@pytest.mark.parametrize("pose,bounds", ps.GATE_SCENES, ids=[f"{p}-{b}" for p, b in ps.GATE_SCENES])
@pytest.mark.parametrize("entry,scale,orb,ori", RUNS, ids=RUN_IDS)
def test_gate_scenes(ctx, pose, bounds, entry, scale, orb, ori):
    s = ps.scene(pose, bounds)
    res, got, share = device_is_oracle(s, entry, scale, orb, ori, ctx.handle)
    assert share <= CAP and res.ori_stable
    if entry == "framekf":       # the point behind the camera is searched at its mirrored projection
        z = s.rows["z"][0]
        assert res.gate[z] == "win" and got[1][res.idx[z]] == z


@pytest.mark.parametrize("entry,scale,orb,ori", RUNS, ids=RUN_IDS)
def test_exact_edges(ctx, entry, scale, orb, ori):
    s = ps.built("exact", ps.exact_scene)
    if entry in ("fuse1", "kfsim3"):
        scale = 2.0 if scale > 1 else 0.5          # exact in float32
    res, got, share = device_is_oracle(s, entry, scale, orb, ori, ctx.handle)
    assert share == 0
    rows = s.exact_rows
    strict = entry != "framekf"
    assert res.gate[rows["u==max_x"]] == ("umax" if strict else "win")
    assert res.gate[rows["v==max_y"]] == ("vmax" if strict else "win")


@pytest.mark.parametrize("entry,scale,orb,ori", RUNS, ids=RUN_IDS)
def test_keyframe_of_max_features(ctx, entry, scale, orb, ori):
    """n = 4096: the index field of the packed key is full (winner 4095 in
    cell 0, winner 0 in cell 3071), and the sequential searches take
    21 n + 192 bytes (86 KB) of dynamic LDS."""
    s = ps.built("size4096", ps.size_scene)
    res, got, share = device_is_oracle(s, entry, scale, orb, ori, ctx.handle)
    assert share == 0
    assert [int(res.idx[p]) for p in s.winners] == list(ps.SIZE_WINNERS)


def test_keyframe_over_max_features_is_an_argument_error(ctx):
    s = ps.built("size4096", ps.size_scene)
    keys = np.concatenate([s.K.keys, s.K.keys[:1]])
    desc = np.ascontiguousarray(np.concatenate([s.K.desc, s.K.desc[:1]]))
    kv = ox.frame_view(keys, desc, ps.W, ps.H)
    assert kv.n == 4097
    for sim3 in (0, 1):
        assert ps.fuse_call(kv, s.cam, s.mp, s.nq, s.T, sim3, ctx.handle)[0] == ORBX_ERR_ARG
    L, h = ox.lib(), ctx.handle
    n = ctypes.c_int()
    mv, small = s.mpview(), s.K.view()
    out = np.full(4097, -1, np.int32)
    taken = np.zeros(4097, np.uint8)
    assert L.orbx_search_by_projection_kf_sim3(h, ctypes.byref(kv), ptr(s.cam), ctypes.byref(mv), ptr(s.skip), ptr(s.T),
                                               6, ptr(out), ctypes.byref(n)) == ORBX_ERR_ARG
    qv = ox.frame_view(s.qkeys, s.mp["desc"], ps.W, ps.H)
    valid = np.ones(s.nq, np.uint8)
    assert L.orbx_search_by_projection_frame_kf(h, ctypes.byref(kv), ctypes.byref(qv), ptr(s.cam), ctypes.byref(mv),
                                                ptr(valid), ptr(taken), ptr(s.T), ps.TH, 100, 0, ptr(out),
                                                ctypes.byref(n)) == ORBX_ERR_ARG
    # SearchBySim3 with the oversized keyframe on either side
    big = {k: np.ascontiguousarray(np.resize(a, (4097,) + a.shape[1:])) for k, a in s.mp.items()}
    bv = ps.mp_view(big, 4097)
    v1, prior, new = np.ones(4097, np.uint8), np.full(4097, -2, np.int32), np.zeros(4097, np.int32)
    R12, t12 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    ok = {k: np.ascontiguousarray(np.resize(a, (s.K.n,) + a.shape[1:])) for k, a in s.mp.items()}
    ov = ps.mp_view(ok, s.K.n)
    # the control: the same call at 4096 on both sides is accepted
    assert L.orbx_search_by_sim3(h, ctypes.byref(small), ctypes.byref(small), ptr(s.cam), ctypes.byref(ov), ptr(v1),
                                 ctypes.byref(ov), ptr(v1), ptr(s.T), ptr(s.T), 1.0, ptr(R12), ptr(t12), ps.TH,
                                 ptr(prior), ptr(new), ctypes.byref(n)) == 0
    for K1, m1, K2, m2 in ((kv, bv, small, ov), (small, ov, kv, bv)):
        assert L.orbx_search_by_sim3(h, ctypes.byref(K1), ctypes.byref(K2), ptr(s.cam), ctypes.byref(m1), ptr(v1),
                                     ctypes.byref(m2), ptr(v1), ptr(s.T), ptr(s.T), 1.0, ptr(R12), ptr(t12), ps.TH,
                                     ptr(prior), ptr(new), ctypes.byref(n)) == ORBX_ERR_ARG


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("entry,scale", [("fuse0", 1.0), ("fuse1", 1.7), ("kfsim3", 0.6)])
def test_point_counts_around_the_workgroup(ctx, entry, scale, nq):
    """A workgroup takes four map points: one, one short of a group, a full
    group, one over, and 64 groups and one."""
    s = ps.scene("axis0.9", "image")
    assert s.nq >= nq
    device_is_oracle(s, entry, scale, 0, 0, ctx.handle, nq=nq)


@pytest.mark.parametrize("sim3", [0, 1])
def test_fuse_batch_of_unlike_jobs(ctx, sim3):
    """Three jobs with different poses and cameras: a gate scene; the
    keyframe of 4096 with the first job's map-point view (uploaded once); a
    keyframe of 5 with the exact scene's camera and points."""
    a, big, ex = ps.scene("x1.2", "undist"), ps.built("size4096", ps.size_scene), ps.built("exact", ps.exact_scene)
    five = ps.Keyframe(ex.K.keys[:5].copy(), ex.K.desc[:5].copy())
    cam2 = np.array([450.0, 470.0, 310.0, 250.0], np.float32)
    scale = 1.7 if sim3 else 1.0
    jobs = [(a.K, a.cam, a.mp, ps.pose32(a.R, a.t, scale)),
            (big.K, cam2, a.mp, ps.pose32(*ps.POSES["z0.4"], scale)),
            (five, ex.cam, ex.mp, ps.pose32(ex.R, ex.t, 2.0 if sim3 else 1.0))]
    views = (ox.FrameView * 3)(*[K.view() for K, _, _, _ in jobs])
    assert [v.n for v in views] == [a.K.n, 4096, 5]
    cams = np.ascontiguousarray(np.concatenate([c for _, c, _, _ in jobs]).astype(np.float32))
    Ts = np.ascontiguousarray(np.concatenate([T.reshape(-1) for _, _, _, T in jobs]))
    shared = ps.mp_view(a.mp, a.nq)
    mvs = [shared, shared, ps.mp_view(ex.mp, ex.nq)]
    mps = (ctypes.c_void_p * 3)(*[ctypes.addressof(m) for m in mvs])
    bi = [np.full(m.n, -9, np.int32) for m in mvs]
    bd = [np.full(m.n, -9, np.int32) for m in mvs]
    pi = (ctypes.c_void_p * 3)(*[b.ctypes.data for b in bi])
    pdist = (ctypes.c_void_p * 3)(*[b.ctypes.data for b in bd])
    assert ox.lib().orbx_fuse_candidates_batch(ctx.handle, 3, views, ptr(cams), mps, ptr(Ts), sim3, ps.TH, pi, pdist) == 0
    found = 0
    for k, (K, cam, mp, T) in enumerate(jobs):
        rc, wi, wd = ps.fuse_call(K.view(), cam, mp, mvs[k].n, T, sim3)
        assert rc == 0 and np.array_equal(bi[k], wi) and np.array_equal(bd[k], wd), k
        found += int((wi >= 0).sum())
    assert found > 60
    # the first job is its scene's own search: the decided points as the float64 reference has them
    entry = "fuse1" if sim3 else "fuse0"
    res, _, _ = ps.reference(a, entry, scale)
    ps.check_decided(a, entry, res, bi[0], bd[0])


@pytest.mark.parametrize("pose,bounds", ps.GATE_SCENES + [("exact", "image"), ("size4096", "image")],
                         ids=[f"{p}-{b}" for p, b in ps.GATE_SCENES] + ["exact", "size4096"])
def test_frustum_and_local_map_search(ctx, pose, bounds):
    """k_frustum and the local-map search behind it (orbx_search_local_map):
    every output bit for bit the oracle's, the decided points as float64."""
    s = frustum_scene(pose, bounds)
    want, got = ps.run_frustum(s), ps.run_frustum(s, ctx.handle)
    assert want[0] == 0 and got[0] == 0
    for w, g in zip(want[1:6], got[1:6]):
        assert np.array_equal(np.ascontiguousarray(w).view(np.uint8), np.ascontiguousarray(g).view(np.uint8))
    assert got[6:] == want[6:] and got[6] >= 5
    assert ps.check_frustum(s, ps.reference_frustum(s), got) <= CAP


@pytest.mark.parametrize("r12,s12", ps.SIM3_CASES)
@pytest.mark.parametrize("bounds", ["image", "undist"])
def test_search_by_sim3(ctx, r12, s12, bounds):
    s = ps.built(("sim3", r12, s12, bounds),
                 lambda: ps.sim3_scene(r12, s12, bounds=ps.BOUNDS_IMAGE if bounds == "image" else ps.BOUNDS_UNDIST))
    new, decided, _, _ = ps.reference_sim3(s)
    rc, want, wn = ps.run_sim3(s)
    rg, got, gn = ps.run_sim3(s, ctx.handle)
    assert rc == 0 and rg == 0
    assert np.array_equal(got, want) and gn == wn and wn >= 20
    assert np.array_equal(got[decided], new[decided])
    print(f"{s.name}: undecided {1 - decided.mean():.4f}")


def test_distinctive_edge_sets(ctx):
    p, d, want, names = pd.distinctive_edge_sets()
    got = np.full(len(want), -9, np.int32)
    assert ox.lib().orbx_distinctive_descriptors(ctx.handle, len(want), ox._ptr(p), ox._ptr(d), ox._ptr(got)) == 0
    assert np.array_equal(got, ref_distinctive(p, d))
    assert got.tolist() == want.tolist(), names
