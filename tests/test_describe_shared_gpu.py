"""k_describe with the per-keypoint trigonometry shared by the workgroup and
the window staged in 16-byte pieces.  One wave of each workgroup computes
fastAtan2 and the correctly rounded sin/cos for the workgroup's eight
keypoints between two block barriers, so every wave of a workgroup that has a
keypoint must reach the barriers, also a wave without one; a window row is
three 16-byte pieces from an origin that is 4-byte aligned only.  Everything
is bit-exact against the oracle: every KEYPOINT field (angle included) and
the descriptors.

The inputs are chosen for their keypoint counts modulo 8 (keypoints per
workgroup): 1 and 3 leave a wave with one empty half, 1 and 2 leave empty
waves beside a working one, 0 fills the last workgroup; with 300 / 8 = 38
workgroups per frame every frame also has workgroups without any keypoint.
Their window origins (16 + x - 21) & ~3 cover all four alignment classes
modulo 16.  Both properties are asserted on the oracle's output before any
GPU call.  nfeatures = 300 is the smallest round number the oracle accepts at
these sizes (it returns error -4 at 100 and below).
"""
import numpy as np
import pytest

import orb_slam_amd as ox
from orb_slam_amd import synth
from oracle_lib import RefExtractor

pytestmark = pytest.mark.gpu

N = 300
E = 16         # padded border
WIN_R = 21     # the staged window starts at (X - 21) & ~3
GROUP = 8      # keypoints per k_describe workgroup
DIRECT = (160, 128)   # width a multiple of 16: level 0 read from the frame store
COPY = (181, 120)     # level-0 copy mode
# (size, seed) -> keypoints the oracle returns
INPUTS = {(DIRECT, 21): 269, (DIRECT, 22): 265, (DIRECT, 23): 270,
          (COPY, 21): 256, (COPY, 22): 275, (COPY, 23): 266}

_cache = {}


def image(size, seed):
    key = ("img", size, seed)
    if key not in _cache:
        _cache[key] = synth.noise_frame(size[0], size[1], seed)
    return _cache[key]


def oracle(size, seed, variant="iso", score_type=1):
    """Oracle output for one input, computed once: features and the per-level keys."""
    key = (size, seed, variant, score_type)
    if key not in _cache:
        ref = RefExtractor(N, variant=variant, score_type=score_type)
        k, d = ref(image(size, seed))
        _cache[key] = dict(kps=k, desc=d, keys=[ref.level_keys(l) for l in range(8)])
    return _cache[key]


def origin_classes(keys):
    """Alignment classes modulo 16 of the window origins of one level's keys."""
    x = keys["x"].astype(np.int64)
    return set((((E + x - WIN_R) & ~3) % 16).tolist())


def check_inputs():
    """The properties the cases rely on, on the oracle's own output."""
    if "checked" in _cache:
        return
    residues = set()
    for (size, seed), want in INPUTS.items():
        o = oracle(size, seed)
        n = len(o["kps"])
        assert n == want, (size, seed, n)
        assert sum(len(k) for k in o["keys"]) == n, (size, seed)
        assert -(-n // GROUP) < N // GROUP + (N % GROUP > 0), (size, seed)   # workgroups without a keypoint
        residues.add(n % GROUP)
        lv0 = origin_classes(o["keys"][0])
        upper = set().union(*[origin_classes(k) for k in o["keys"][1:]])
        assert lv0 == {0, 4, 8, 12} and upper == {0, 4, 8, 12}, (size, seed, lv0, upper)
    assert {0, 1, 2, 3} <= residues, residues
    _cache["checked"] = True


def assert_kps_equal(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in ox.KEYPOINT.names:
        assert np.array_equal(a[f], b[f]), (what, f)


def assert_features(got, o, what=""):
    gk, gd = got
    assert_kps_equal(gk, o["kps"], what)
    assert np.array_equal(gd, o["desc"]), what


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("size,seed", sorted(INPUTS))
def test_single_frame(size, seed, contract):
    check_inputs()
    o = oracle(size, seed, "contract" if contract else "iso")
    ctx = ox.Context(nfeatures=N, max_w=size[0], max_h=size[1], slots=1)
    ctx.set_fp_contract(contract)
    ctx.upload(image(size, seed))
    ctx.extract(0, 1)
    ctx.sync()
    assert ctx.level0_direct() is (size == DIRECT)
    assert_features(ctx.features(0), o, (size, seed, contract))
    ctx.close()


def test_batch_of_three():
    """Three slots in one launch: the grid pads to 8 frame columns, so padding
    blocks (which return at once) run beside blocks that reach the barriers."""
    check_inputs()
    seeds = (21, 22, 23)
    ctx = ox.Context(nfeatures=N, max_w=DIRECT[0], max_h=DIRECT[1], slots=3)
    ctx.upload(np.stack([image(DIRECT, s) for s in seeds]))
    ctx.extract(0, 3)
    ctx.sync()
    assert ctx.level0_direct()
    for slot, s in enumerate(seeds):
        assert_features(ctx.features(slot), oracle(DIRECT, s), ("batch", s))
    ctx.close()


def test_single_call_graph():
    """ctx(img): the captured single-frame graph, the cascade with the padded level 0."""
    check_inputs()
    ctx = ox.Context(nfeatures=N, max_w=DIRECT[0], max_h=DIRECT[1], slots=1)
    got = ctx(image(DIRECT, 22))
    assert ctx.level0_direct() is False
    assert_features(got, oracle(DIRECT, 22), "graph")
    ctx.close()


def test_harris_score():
    """The Harris score type: k_describe reads the u64 entries."""
    check_inputs()
    o = oracle(DIRECT, 21, score_type=0)
    ctx = ox.Context(nfeatures=N, score_type=0, max_w=DIRECT[0], max_h=DIRECT[1], slots=1)
    ctx.upload(image(DIRECT, 21))
    ctx.extract(0, 1)
    ctx.sync()
    assert len(o["kps"]) > 50
    assert_features(ctx.features(0), o, "harris")
    ctx.close()
