"""LocalMapping's culling on the device covisibility graph
(orbx_covis_set_octaves, orbx_covis_cull_keyframes, orbx_covis_cull_points in
orb_slam_amd/csrc/orbx_covis.hip) against the literal restatement of
KeyFrameCulling and MapPointCulling (tests/culling_numpy.py).  Integer work
plus one FP64 and one FP32 comparison: every comparison is exact, lists in
order."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import orb_slam_amd as ox
import culling_cases as kc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -1, -3
GOLDEN = Path(__file__).resolve().parent / "golden" / "culling_sequence.npz"


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=320, max_h=240, slots=2)
    yield c
    c.close()


def both(ctx, ops, sizes=None):
    want, _ = kc.run_restatement(ops)
    got = kc.run_device(ox, ctx, ops, sizes)
    kc.assert_same(got, want)
    return got


@pytest.mark.parametrize("name", sorted(kc.rule_cases()))
def test_rule(ctx, name):
    ops, answer = kc.rule_cases()[name]
    kc.check_answers(both(ctx, ops), answer)


def test_golden_sequence(ctx):
    ops, want = kc.decode(np.load(GOLDEN))
    kc.assert_same(kc.run_device(ox, ctx, ops), want)


@pytest.mark.parametrize("members,row_len", [(0, 5), (1, 1), (2, 63), (3, 0), (3, 64), (5, 65), (4, 257), (6, 1025)])
def test_random_sequences(ctx, members, row_len):
    """Rows of every length around a wavefront, the 256 threads of the row
    kernels and the 1024 of the walk; both culls interleaved with set_matches,
    erase_points, updates and frames.  After every cull both reads of every
    member and a frame: HBM, the shadow (which checks the later edits) and the
    restatement agree on the state a cull leaves."""
    ops = kc.random_ops(1000 * members + row_len, members, row_len)
    both(ctx, ops)


def scene(members):
    ops, _ = kc.culling_scene(members, members)
    cut = next(k for k, o in enumerate(ops) if o["op"] == "cull_kf")
    return ops, cut


@pytest.mark.parametrize("members", [64, 65, 130])
def test_window_scene(ctx, members):
    ops, cut = scene(members)
    assert all(kc.scene_properties(ops).values())
    both(ctx, ops)


@pytest.mark.parametrize("members", [64, 65, 130])
def test_window_scene_resumed_and_repeated(ctx, members):
    """The scene's KeyFrameCulling driven with max_culls = 1 and resumed over
    the rest of the list: the decisions, the bad points and the state of the
    one unlimited call (which test_window_scene compares with the
    restatement).  Then the same call on the unchanged final state, twice: the
    same answer, so the per-point scratch of a call is clean when it ends."""
    ops, cut = scene(members)
    whole = ops[cut]
    want, _ = kc.run_restatement(ops)
    one = next(r for r in want if r["kind"] == "cull_kf")
    got = {}

    def drive(m):
        r = m.cull_keyframes(whole["cur"], whole["keep"], 1)
        cand = r["cand"]
        dec, mps, red, bad = [list(r[f]) for f in ("decision", "n_mps", "n_redundant", "bad_points")]
        done, calls = r["n_done"], 1
        while done < len(cand):
            r = m.cull_keyframes(-1, whole["keep"], 1, cand[done:])
            assert r["cand"].tolist() == cand[done:].tolist()
            for acc, f in ((dec, "decision"), (mps, "n_mps"), (red, "n_redundant"), (bad, "bad_points")):
                acc += list(r[f])
            done += r["n_done"]
            calls += 1
        got.update(cand=cand, decision=dec, n_mps=mps, n_redundant=red, bad_points=bad, calls=calls)
        b = kc.OnDevice(m)
        got["after"] = [kc.step(b, o) for o in ops[cut + 1:]]
        again = [m.cull_keyframes(whole["cur"], whole["keep"]) for _ in range(2)]
        got["again"] = again

    kc.run_device(ox, ctx, ops[:cut], kc.sizes_of(ops), keep=drive)
    for f in ("cand", "decision", "n_mps", "n_redundant", "bad_points"):
        assert np.array_equal(got[f], one[f]), f
    culls = int((one["decision"] == 1).sum())
    assert culls >= 1 and got["calls"] in (culls, culls + 1)     # the last call holds no cull unless the list ends with one
    at = next(k for k, r in enumerate(want) if r is one)
    kc.assert_same([r for r in got["after"] if r is not None], want[at + 1:])
    a, b = got["again"]
    for f in ("cand", "decision", "n_mps", "n_redundant", "bad_points"):
        assert np.array_equal(a[f], b[f]), f
    assert len(a["cand"]) > 0


def test_error_returns_leave_the_state(ctx):
    """Every ORBX_ERR_ARG and ORBX_ERR_CAPACITY return of the three calls, each
    followed by the reads of the whole state."""
    ops, _ = kc.rule_cases()["two_left_flips_next"]
    build = [o for o in ops if o["op"] in ("add", "octaves")]
    members = sorted(o["id"] for o in build if o["op"] == "add")
    frame = [50, 90, 60, 70]
    m = ox.CovisibilityMap(ctx, 8, 100, 32)
    try:
        b = kc.OnDevice(m)
        for o in build[:-1]:                          # keyframe 6 still without octaves
            kc.step(b, o)
        m.update_connections(members, 1)

        def state():
            return [kc.step(b, o) for o in kc.state_reads(members, frame)]

        def code(f, *a, **kw):
            with pytest.raises(ox.OrbxError) as e:
                f(*a, **kw)
            return e.value.code

        before = state()

        def unchanged():
            kc.assert_same(state(), before)
            assert len(m) == len(members)
            return True

        assert code(m.cull_keyframes, cand=[1, 2]) == ERR_ARG and unchanged()      # a member without octaves
        assert code(m.set_octaves, 7, []) == ERR_ARG                                # not a member
        assert code(m.set_octaves, 6, [0] * 5) == ERR_ARG                           # another n
        lib = ox.lib()
        assert lib.orbx_covis_set_octaves(ctx.handle, m.handle, 6, 29, None) == ERR_ARG
        kc.step(b, build[-1])
        assert code(m.cull_keyframes, 7) == ERR_ARG and code(m.cull_keyframes, 0) == ERR_ARG   # cur no member
        assert code(m.cull_keyframes, -2) == ERR_ARG
        assert code(m.cull_keyframes, cand=[1, 8]) == ERR_ARG                       # a listed id out of range
        assert code(m.cull_keyframes, cand=[1, -1]) == ERR_ARG
        assert code(m.cull_keyframes, cand=[1] * 9) == ERR_ARG                      # longer than kf_capacity
        assert code(m.cull_keyframes, cand=[1, 2], keep=[8]) == ERR_ARG             # a kept id out of range
        assert code(m.cull_keyframes, cand=[1, 2], max_culls=-1) == ERR_ARG
        q = ox.CovisCull()
        q.cur, q.cand_cap, q.bad_cap = 3, 8, 8                                      # null pointers
        assert lib.orbx_covis_cull_keyframes(ctx.handle, m.handle, ctypes.byref(q)) == ERR_ARG
        assert lib.orbx_covis_cull_keyframes(ctx.handle, m.handle, None) == ERR_ARG
        assert unchanged()
        # capacities: the counts are set, the graph as it was
        r = m.cull_keyframes(cand=[1, 2], cand_cap=1)
        assert (r["code"], r["n_cand"]) == (ERR_CAPACITY, 2) and unchanged()
        r = m.cull_keyframes(3, cand_cap=2)                                          # 3's list: 1, 2, 4 and 6
        assert (r["code"], r["n_cand"], len(r["cand"])) == (ERR_CAPACITY, 4, 2) and unchanged()
        r = m.cull_keyframes(cand=[1, 2], bad_cap=1)
        assert (r["code"], r["n_cand"], r["n_done"], r["n_bad"]) == (ERR_CAPACITY, 2, 2, 2)
        assert r["decision"].tolist() == [1, 1] and r["bad_points"].tolist() == [90] and unchanged()
        # MapPointCulling's arguments
        ok = ([50, 60], [1, 1], [1, 1], [3, 3])
        assert code(m.cull_points, 5, [50, 100], *ok[1:]) == ERR_ARG                # an id out of range
        assert code(m.cull_points, 5, [50, -1], *ok[1:]) == ERR_ARG
        assert code(m.cull_points, 5, [50, 50], *ok[1:]) == ERR_ARG                 # listed twice
        assert code(m.cull_points, 5, ok[0], [1, -1], *ok[2:]) == ERR_ARG           # a negative count
        assert code(m.cull_points, 5, ok[0], ok[1], [-1, 1], ok[3]) == ERR_ARG
        assert code(m.cull_points, 5, ok[0], ok[1], ok[2], [3, 6]) == ERR_ARG       # first_kf > cur_kf
        assert lib.orbx_covis_cull_points(ctx.handle, m.handle, 5, -1, None, None, None, None, None) == ERR_ARG
        assert lib.orbx_covis_cull_points(ctx.handle, m.handle, 5, 2, None, None, None, None, None) == ERR_ARG
        assert unchanged()
        # and the same calls with room: the answers of the rule case
        r = m.cull_keyframes(cand=[1, 2], bad_cap=2, cand_cap=2)
        assert r["code"] == 0 and r["decision"].tolist() == [1, 1] and r["bad_points"].tolist() == [90, 50]
        assert len(m) == len(members) - 2
        assert m.cull_points(5, *ok).tolist() == [1, 0]
        m.clear()
        m.add_keyframe(1, 5, [1, 2])
        assert code(m.cull_keyframes, cand=[1]) == ERR_ARG                          # clear took the octaves' flags
    finally:
        m.close()


def test_kernel_timers(ctx):
    """covis_cull_kf and covis_cull_mp count one region per call."""
    ops, _ = kc.rule_cases()["two_left_flips_next"]
    ops = ops + [kc.cull_mp(9, [60, 61], [1, 1], [1, 9], [9, 9])]
    names = ("covis_cull_kf", "covis_cull_mp")
    ctx.timing(True)
    try:
        before = [ctx.kernel_time(n)[0] for n in names]
        kc.run_device(ox, ctx, ops)
        ctx.sync()
        after = [ctx.kernel_time(n)[0] for n in names]
    finally:
        ctx.timing(False)
    assert [a - b for a, b in zip(after, before)] == [1, 1]
