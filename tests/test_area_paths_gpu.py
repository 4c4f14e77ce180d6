"""Every form of k_area_lists / k_area_replay through the four public area
searches, on the hand-built scenes of tests/area_scenes.py: matches and
counts must equal the oracle's exactly, and the replay's counters
(orbx_debug_area_rounds: parallel rounds used by converged replays, and
sequential fallbacks) must move by what the scene is built for.

The counters are process-wide, so every assertion is on the difference over
one call.  A replay that falls back adds nothing to the rounds counter.

Forms reached (proved from the sizes alone by test_area_paths_numpy.py):
lists of 0, 1, 2..64, 65..128 and over 128 candidates with their exact
boundaries; short lists past the LDS entry budget; the per-query arrays in
LDS (up to the largest sizes that fit) and in global memory with a full and a
shrunk entry budget; more than 1024 queries; chains that converge in exactly
kMaxRounds = 24 rounds and chains that do not (the one-wave sequential
replay, through all three list forms); ties between cells; assigned
candidates, cleared queries, the rotation filter and the ratio test inside
chains.  launch_area_search's ORBX_ERR_UNSUPPORTED cannot be reached at or
below kMaxFeatures keypoints (the fixed LDS part always fits), so no scene
asks for it.
"""
import ctypes

import numpy as np
import pytest

import area_scenes as A
import orb_slam_amd as ox
from oracle_lib import load

pytestmark = pytest.mark.gpu

# (rounds delta, fallback delta) the issue of these tests names, apart from the mirror
NAMED = {"chain10x3": (11, 0), "chain23": (24, 0), "chain24": (0, 1), "chain24x3": (0, 1), "chain40x3": (0, 1)}


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=1000, max_w=A.W, max_h=A.H, slots=2)
    yield c
    c.close()


def oracle_fns():
    L = load()
    L.orbx_ref_search_local_map.argtypes = [ctypes.c_void_p]
    return {"window": L.orbx_ref_window_search, "pair": L.orbx_ref_search_by_projection_pair,
            "motion": L.orbx_ref_search_by_projection_motion, "local": L.orbx_ref_search_by_projection_local,
            "local_map": L.orbx_ref_search_local_map}


def gpu_fns():
    L = ox.lib()
    return {"window": L.orbx_window_search, "pair": L.orbx_search_by_projection_pair,
            "motion": L.orbx_search_by_projection_motion, "local": L.orbx_search_by_projection_local,
            "local_map": L.orbx_search_local_map}


def counters():
    L = ox.lib()
    L.orbx_debug_area_rounds.argtypes = [ctypes.c_void_p]
    out = np.zeros(2, np.uint64)
    assert L.orbx_debug_area_rounds(out.ctypes.data) == 0
    return out.astype(np.int64)


@pytest.mark.parametrize("name,kind", A.CASES)
def test_area_search_equals_oracle(ctx, name, kind):
    s, m = A.scene(name, kind)
    rc, om, on = A.search(s, oracle_fns())
    assert rc == 0
    before = counters()
    rc, gm, gn = A.search(s, gpu_fns(), ctx.handle)
    delta = tuple(int(v) for v in counters() - before)
    assert rc == 0, ox.ERRORS.get(rc, rc)
    print(f"{name}/{kind}: nq {s.nq} n2 {s.n2} matches {gn} (oracle {on}) rounds +{delta[0]} fallbacks +{delta[1]}")
    assert gn == on, (gn, on)
    assert np.array_equal(gm, om), np.nonzero(gm != om)[0][:10]
    for q, c in s.expect.items():     # by construction
        assert np.nonzero(gm == q)[0].tolist() == ([c] if c >= 0 else []), (q, c)
    want = (0, 1) if m["fallback"] else (m["rounds"], 0)
    assert delta == want, (delta, want)
    if name in NAMED:
        assert delta == NAMED[name]


def posed_cases():
    from test_area_paths_numpy import POSED, POSED_IDS
    return dict(argvalues=POSED, ids=POSED_IDS)


@pytest.mark.parametrize("name,kind,pose", **posed_cases())
def test_area_search_under_a_general_pose(ctx, name, kind, pose):
    """The small, tie and extras scenes of the three projection kinds from a
    rotated and translated camera (the local-map kind through isInFrustum):
    the oracle's matches, the construction's, and the unposed scene's rounds."""
    from test_area_paths_numpy import posed_scene
    s, m = posed_scene(name, kind, pose)
    rc, om, on = A.search(s, oracle_fns())
    assert rc == 0
    before = counters()
    rc, gm, gn = A.search(s, gpu_fns(), ctx.handle)
    delta = tuple(int(v) for v in counters() - before)
    assert rc == 0, ox.ERRORS.get(rc, rc)
    print(f"{name}/{kind}/{pose}: matches {gn} (oracle {on}) rounds +{delta[0]} fallbacks +{delta[1]}")
    assert gn == on and np.array_equal(gm, om)
    for q, c in s.expect.items():
        assert np.nonzero(gm == q)[0].tolist() == ([c] if c >= 0 else []), (q, c)
    assert delta == ((0, 1) if m["fallback"] else (m["rounds"], 0))


def test_track_frame_falls_back_inside_its_chain_of_kernels(ctx, ref):
    """orbx_track_frame whose motion search holds a chain of 24 among the
    natural keypoints (area_scenes.track_chain): the shared launch path
    takes the sequential replay once, and the whole tracked frame -- matches,
    counts, outlier flags, pose -- equals the chain over the oracle.  The
    same frame without the chain does not fall back."""
    import track_data as td
    from test_track_gpu import compare, features, px_to_x, run
    seed, shift, err = A.TRACK_CASE
    last, cur = td.images(A.W, A.H, shift, seed)
    kl, dl = features(ctx, last, 0)
    kc, dc = features(ctx, cur, 1)
    scene = td.make_scene(kl, dl, seed)
    Tpred = td.pose_x(px_to_x(shift + err))
    before = counters()
    got = run(ctx, scene, Tpred, slot=1, last_view=ox.frame_view(kl, dl, A.W, A.H))
    plain = counters() - before
    compare(got, td.ref_chain(ref, kl, dl, kc, dc, scene, Tpred), True)
    kl2, dl2, scene2, path = A.track_chain(kl, dl, kc, dc, scene, Tpred)
    m = A.mirror(A.TrackMotion(kl2, dl2, kc, dc, scene2, Tpred))
    assert m["fallback"] == 1 and m["state"][:24].tolist() == path
    before = counters()
    got = run(ctx, scene2, Tpred, slot=1, last_view=ox.frame_view(kl2, dl2, A.W, A.H))
    delta = counters() - before
    print(f"track: plain rounds +{plain[0]} fallbacks +{plain[1]}; chain of 24 rounds +{delta[0]} fallbacks +{delta[1]}")
    exp = td.ref_chain(ref, kl2, dl2, kc, dc, scene2, Tpred)
    assert exp["status"] == 0 and exp["n_local"] > 0
    compare(got, exp, True)
    assert plain[1] == 0 and delta[1] == 1


@pytest.mark.parametrize("kind", A.KINDS)
def test_more_than_max_features_is_an_argument_error(ctx, kind):
    over = A.K_MAX_FEATURES + 1
    s = A.edge(kind, 40, over, per_spot=16)
    before = counters()
    rc, _, _ = A.search(s, gpu_fns(), ctx.handle)
    assert rc == -1      # ORBX_ERR_ARG
    if kind != "local":  # the queries are a frame too
        rc, _, _ = A.search(A.edge(kind, over, 40, per_spot=16), gpu_fns(), ctx.handle)
        assert rc == -1
    assert np.array_equal(counters(), before)
