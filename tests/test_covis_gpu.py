"""The covisibility graph in HBM (orbx_covis_*, orb_slam_amd/csrc/
orbx_covis.hip) against the literal restatement of KeyFrame::UpdateConnections,
the covisibility reads and Tracking::UpdateReference (tests/covis_numpy.py).
Everything is integer work: every comparison is exact, lists in order."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import covis_cases as cc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4
MAX_KEYPOINTS = 300
GOLDEN = Path(__file__).resolve().parent / "golden" / "covis_sequence.npz"


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=320, max_h=240, slots=2)
    yield c
    c.close()


def both(ctx, ops, sizes=None):
    want, _ = cc.run_restatement(ops)
    got = cc.run_device(ox, ctx, ops, sizes)
    cc.assert_same(got, want)
    return got


@pytest.mark.parametrize("name", sorted(cc.rule_cases()))
def test_rule(ctx, name):
    ops, answer = cc.rule_cases()[name]
    cc.check_answers(both(ctx, ops), answer)


def test_golden_sequence(ctx):
    ops, want = cc.decode(np.load(GOLDEN))
    cc.assert_same(cc.run_device(ox, ctx, ops), want)


@pytest.mark.parametrize("members,row_len", [(0, 5), (1, 1), (2, 63), (3, 0), (3, 64), (5, 65), (4, 257),
                                             (3, MAX_KEYPOINTS), (64, 65), (65, 64), (130, 63)])
def test_random_sequences(ctx, members, row_len):
    """Rows and frames of every length around a wavefront and a workgroup, 64
    and 65 keyframes around one wavefront of rows; set_matches, erase_points,
    erase_keyframe and updates in batches of 1, 2 and all, with both reads of
    every keyframe and a frame after each stage."""
    ops = cc.random_ops(1000 * members + row_len, members, row_len)
    kf, mp, kp = cc.sizes_of(ops)
    both(ctx, ops, (kf, mp, MAX_KEYPOINTS if row_len == MAX_KEYPOINTS else kp))


@pytest.mark.parametrize("members", [64, 65, 130])
def test_window_scene(ctx, members):
    """The scene that shows lists with entries below the threshold, fallback
    lists, weight ties, stale entries and neighbour passes that append; the
    batched update takes 65 ids at 130 keyframes."""
    ops = cc.window_scene(members, members)
    assert all(cc.scene_properties(ops).values())
    both(ctx, ops)


def test_unchanged_state_same_answer(ctx):
    """The per-point marks of one call are gone before the next."""
    ops = cc.window_scene(7, 64)
    frame = next(o for o in ops if o["op"] == "reference")["frame"]
    twice = np.concatenate([frame, frame[:7]])   # seven points stand twice
    members = sorted({o["id"] for o in ops if o["op"] == "add"} - {o["id"] for o in ops if o["op"] == "erase_kf"})
    out = []

    def keep(m):
        for _ in range(2):
            out.append(m.update_reference(twice))
            out.append(m.update_connections(members[3:5]))
    kf, mp, kp = cc.sizes_of(ops)
    cc.run_device(ox, ctx, ops, (kf, mp, len(twice)), keep=keep)
    for f in ("frame_erased", "local_kf", "local_mp", "n_voters", "ref_kf"):
        assert np.array_equal(out[0][f], out[2][f]), f
    assert len(out[0]["local_kf"]) > 1 and len(out[0]["local_mp"]) > 60
    assert np.array_equal(out[1][1], out[3][1])


def test_error_returns(ctx):
    lib = ox.lib()
    h = ctypes.c_void_p()
    for args in ((8193, 10, 10), (8, 10, 65536), (8, (1 << 27) + 1, 10)):
        assert lib.orbx_covis_create(ctx.handle, *args, ctypes.byref(h)) == ERR_UNSUPPORTED
    assert lib.orbx_covis_create(ctx.handle, 0, 10, 10, ctypes.byref(h)) == ERR_ARG
    m = ox.CovisibilityMap(ctx, 8, 50, 6)
    try:
        def code(f, *a):
            with pytest.raises(ox.OrbxError) as e:
                f(*a)
            return e.value.code
        m.add_keyframe(0, 77, [1, 2, 3, -1])
        m.add_keyframe(1, 78, [1, 2, 3, 4, 5, 6])
        assert code(m.add_keyframe, 0, 79, [1]) == ERR_ARG          # id in use
        assert code(m.add_keyframe, 8, 79, [1]) == ERR_ARG          # id out of range
        assert code(m.add_keyframe, 2, 77, [1]) == ERR_ARG          # key used
        assert code(m.add_keyframe, 2, 79, [1, 1]) == ERR_ARG       # a point twice
        assert code(m.add_keyframe, 2, 79, [50]) == ERR_ARG         # point out of range
        assert code(m.add_keyframe, 2, 79, [-2]) == ERR_ARG
        assert code(m.add_keyframe, 2, 79, [1] * 7) == ERR_ARG      # longer than max_keypoints
        assert code(m.set_matches, 0, [3], [2]) == ERR_ARG          # 2 stands at index 1
        assert code(m.set_matches, 0, [4], [9]) == ERR_ARG          # index outside the row
        assert code(m.set_matches, 5, [0], [9]) == ERR_ARG          # not a member
        assert code(m.erase_points, [50]) == ERR_ARG
        assert code(m.update_connections, [0, 2]) == ERR_ARG
        assert code(m.update_connections, [0], 0) == ERR_ARG
        assert code(m.connections, 2) == ERR_ARG
        assert code(m.connections, 0, 2) == ERR_ARG
        assert code(m.update_reference, [50]) == ERR_ARG
        assert code(m.update_reference, [1] * 7) == ERR_ARG
        m.set_matches(0, [1, 3], [-1, 2])                           # in order: 2 leaves index 1 first
        m.erase_keyframe(0)
        assert code(m.erase_keyframe, 0) == ERR_ARG
        assert code(m.add_keyframe, 0, 80, [1]) == ERR_ARG          # an erased id is not reused
        assert len(m) == 1
        # capacities: the counts are set, the capacity's worth of entries written
        m.add_keyframe(2, 60, [1, 2, 9])
        m.add_keyframe(3, 61, [1, 9, 10])
        u, f = m.update_connections([1, 2, 3], 1)
        assert u.tolist() == [1, 1, 1] and f.tolist() == [2, 1, 2]   # 2's tie at weight 2: the larger key, 1
        kfs, ws = np.zeros(1, np.int32), np.zeros(1, np.int32)
        n = ctypes.c_int()
        r = lib.orbx_covis_connections(ctx.handle, m.handle, 2, ox.COVIS_ORDERED, kfs.ctypes.data, ws.ctypes.data, 1,
                                       ctypes.byref(n))
        assert (r, n.value, kfs[0], ws[0]) == (ERR_CAPACITY, 2, 1, 2)
        full = m.update_reference([1, 9])
        assert full["local_kf"].tolist() == [2, 3, 1] and full["local_mp"].tolist() == [1, 2, 9, 10, 3, 4, 5, 6]
        part = m.update_reference([1, 9], kf_cap=2, mp_cap=3)
        assert part["code"] == ERR_CAPACITY and (part["n_local_kf"], part["n_voters"], part["n_local_mp"]) == (3, 3, 8)
        assert part["local_kf"].tolist() == [2, 3] and part["local_mp"].tolist() == [1, 2, 9] and part["ref_kf"] == 2
        m.clear()
        assert len(m) == 0
        m.add_keyframe(0, 77, [1])                                   # after clear the id and the key are free
    finally:
        m.close()


def test_kernel_timers(ctx):
    """The four timers of the kfdb kind count their launches."""
    ops = cc.window_scene(3, 64)
    ops = ops[:40] + [cc.reference(ops[0]["row"])]
    names = ("covis_count", "covis_select", "covis_points", "covis_connect")
    ctx.timing(True)
    try:
        before = [ctx.kernel_time(n)[0] for n in names]
        cc.run_device(ox, ctx, ops)
        ctx.sync()
        after = [ctx.kernel_time(n)[0] for n in names]
    finally:
        ctx.timing(False)
    # 20 updates and one frame: a count region each, one select and one points region, 20 connect regions
    assert [a - b for a, b in zip(after, before)] == [21, 1, 1, 20]
