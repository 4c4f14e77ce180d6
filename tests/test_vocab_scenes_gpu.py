"""DBoW2's transform on the device under the constructed vocabularies of
tests/vocab_scenes.py: the host form (orbx_vocab_transform) at 0, 1, 255, 256,
257 and 2048 features, and the slot form (orbx_dev_compute_bow, whose
k_bow_build sorts and sums on the device) on extracted frames of 64 to 4096
features, so that a thread of k_bow_build holds 1, 2 and 4 keys, with counts
at and one past a power of two.  Every result is held to the scene's pinned
outcome, to the numpy restatement and to the oracle (oracle/ref_vocab.cpp):
integers exactly, float64 as bit patterns.  After a slot call only
bow[:nw], fv_nodes[:nf], fv_ptr[:nf + 1] and fv_feat[:m] are read."""
import ctypes

import numpy as np
import pytest

import orb_slam_amd as ox
import vocab_scenes as vs
from orb_slam_amd import synth
from test_dev_bow_gpu import create_vocab, read_bow
from vocab_data import run_ref

pytestmark = pytest.mark.gpu

W, H, SEED = vs.FRAME
ARG = -1


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=100, max_w=64, max_h=64, slots=1)
    yield c
    c.close()


def host_transform(c, voc, D, levelsup):
    """orbx_vocab_transform into arrays filled with a pattern, so that what
    the call leaves unwritten cannot pass for a result."""
    n = len(D)
    out = {"word": np.full(n, -7, np.int32), "weight": np.full(n, -7.0), "nid": np.full(n, -7, np.int32),
           "bw": np.full(n, 77, np.uint32), "bv": np.full(n, -7.0), "fn": np.full(n, 77, np.uint32),
           "fp": np.full(n + 1, -7, np.int32), "ff": np.full(n, -7, np.int32)}
    nw, nf = ctypes.c_int(-7), ctypes.c_int(-7)
    r = ox.lib().orbx_vocab_transform(c.handle, voc, n, ox._ptr(D) if n else None, levelsup, ox._ptr(out["word"]),
                                      ox._ptr(out["weight"]), ox._ptr(out["nid"]), ox._ptr(out["bw"]),
                                      ox._ptr(out["bv"]), ctypes.byref(nw), ox._ptr(out["fn"]), ox._ptr(out["fp"]),
                                      ox._ptr(out["ff"]), ctypes.byref(nf))
    assert r == 0, r
    out["nw"], out["nf"] = nw.value, nf.value
    return out


def held(S, G, D, what):
    """G against the scene's pin, the restatement and the oracle."""
    G = vs.trim(G)
    S["pin"](G)
    assert not vs.differences(G, S["T"]), (what, "restatement", vs.differences(G, S["T"]))
    R = run_ref(S["V"], D, S["levelsup"])
    assert not vs.differences(G, R), (what, "oracle", vs.differences(G, R))


@pytest.mark.parametrize("name", vs.NAMES)
def test_host_form(ctx, name):
    pool = vs.random_descriptors(4096, 1)
    for n in vs.HOST_SIZES:
        D = np.ascontiguousarray(pool[:n])
        S = vs.scene(name, D)
        voc = create_vocab(ctx, S["V"])
        try:
            assert ox.lib().orbx_vocab_n_words(voc) == S["n_words"]
            G = host_transform(ctx, voc, D, S["levelsup"])
            if n == 0:
                assert G["nw"] == G["nf"] == 0 and G["fp"][0] == 0
            held(S, G, D, (name, n))
        finally:
            ox.lib().orbx_vocab_destroy(voc)


def extracted(nfeatures, nlevels, frames):
    c = ox.Context(nfeatures=nfeatures, nlevels=nlevels, max_w=W, max_h=H, slots=len(frames))
    c.upload(np.stack(frames), 0)
    c.extract(0, len(frames))
    c.sync()
    return c, [np.ascontiguousarray(c.features(s)[1]) for s in range(len(frames))]


def slot_bow(c, S, first, count, read):
    """orbx_dev_compute_bow of slots [first, first + count) under the scene's
    vocabulary; the results of the slots in `read`."""
    voc = create_vocab(c, S["V"])
    try:
        assert ox.lib().orbx_dev_compute_bow(c.handle, voc, first, count, S["levelsup"]) == 0
        return [read_bow(c, s, c.nfeatures) for s in read]
    finally:
        c.sync()
        ox.lib().orbx_vocab_destroy(voc)


def cut(G, n):
    """A slot result read with cap = nfeatures, per-feature arrays cut to the slot's count."""
    G = dict(G)
    for k in ("word", "weight", "nid"):
        G[k] = G[k][:n]
    return G


@pytest.mark.parametrize("nf,nlevels", vs.SLOT_SHAPES)
def test_slot_form(nf, nlevels):
    """Every scene on an extracted frame that fills the quota: n = nfeatures,
    so 1024, 2048 and 4096 sort without padding, 65, 1025 and 2049 with
    nearly a whole power of two of it, and a thread holds 1, 2 or 4 keys.
    The vocabulary is built from the descriptors read back from the slot."""
    c, (D,) = extracted(nf, nlevels, [synth.texture_frame(W, H, seed=SEED)])
    try:
        assert len(D) == nf
        for name in vs.NAMES:
            S = vs.scene(name, D)
            G, = slot_bow(c, S, 0, 1, [0])
            held(S, cut(G, nf), D, (name, nf))
    finally:
        c.close()


def frames_of_three_slots():
    """A flat image (no feature), the full frame, and the frame with texture
    in its top left quarter only (fewer features than the quota)."""
    full = synth.texture_frame(W, H, seed=SEED)
    part = synth.flat_frame(W, H)
    part[:H // 2, :W // 2] = full[:H // 2, :W // 2]
    return [synth.flat_frame(W, H), full, part]


SHARED = ("identity", "three_words", "runs", "stopped_alternate", "levels_1", "root4096")


def test_several_slots_in_one_launch():
    """Slots of 0, 2048 and some hundred features in one call: each equals
    its own single-slot call, the restatement and the oracle, and the empty
    slot reads back nw = nf = 0."""
    c, Ds = extracted(2048, 8, frames_of_three_slots())
    try:
        assert len(Ds[0]) == 0 and len(Ds[1]) == 2048 and 0 < len(Ds[2]) < 1024
        for name in SHARED:
            S = vs.scene(name, Ds[1])
            together = slot_bow(c, S, 0, 3, [0, 1, 2])
            for s in range(3):
                n = len(Ds[s])
                G = vs.trim(cut(together[s], n))
                alone, = slot_bow(c, S, s, 1, [s])
                assert not vs.differences(G, cut(alone, n)), (name, s)
                assert not vs.differences(G, vs.transform(S["V"], Ds[s], S["levelsup"])), (name, s)
                assert not vs.differences(G, run_ref(S["V"], Ds[s], S["levelsup"])), (name, s)
            S["pin"](vs.trim(cut(together[1], 2048)))
            assert together[0]["nw"] == together[0]["nf"] == 0 and together[0]["fp"][0] == 0
    finally:
        c.close()


def test_recompute_carries_nothing_over():
    """The identity vocabulary (2048 words, 2048 nodes), then the one-word
    vocabulary on the same slot: the second result has the small counts and
    is right up to them."""
    c, (D,) = extracted(2048, 8, [synth.texture_frame(W, H, seed=SEED)])
    try:
        first = vs.scene("identity", D)
        G, = slot_bow(c, first, 0, 1, [0])
        assert G["nw"] == G["nf"] == 2048
        second = vs.scene("one_word", D)
        G, = slot_bow(c, second, 0, 1, [0])
        assert G["nw"] == G["nf"] == 1 and G["fp"][1] == 2048 and G["bv"][0] == 1.0
        held(second, cut(G, 2048), D, "recompute")
    finally:
        c.close()


def test_contexts_stop_at_4096_features():
    """orbx_dev_compute_bow sorts at most 4096 keys a slot and documents
    ORBX_ERR_UNSUPPORTED above; no context can ask for it, because
    orbx_create refuses nfeatures = 4097 (4096 runs in test_slot_form)."""
    h = ctypes.c_void_p(0xdead)
    assert ox.lib().orbx_create(ctypes.byref(h), 0, 4097, 1.2, 8, 1, 20, W, H, 1) == ARG
    assert not h.value


def test_vocab_create_rejections(ctx):
    """Every refusal is ORBX_ERR_ARG and leaves *out NULL."""
    V = vs.scene("levels_1", vs.random_descriptors(64, 3))["V"]
    L = ox.lib()

    def create(k=V["k"], Lv=V["L"], n_nodes=len(V["parent"]), parent=V["parent"], is_leaf=V["is_leaf"], desc=V["desc"],
               weight=V["weight"], handle=ctx.handle):
        out = ctypes.c_void_p(0xdead)
        r = L.orbx_vocab_create(handle, k, Lv, n_nodes, ox._ptr(parent), ox._ptr(is_leaf), ox._ptr(desc),
                                ox._ptr(weight), ctypes.byref(out))
        return r, out

    def with_parent(i, p):
        q = V["parent"].copy()
        q[i] = p
        return q

    r, out = create()
    assert r == 0 and out.value
    L.orbx_vocab_destroy(out)
    refused = {
        "parent above": dict(parent=with_parent(4, 9)),         # parent[i] > i
        "parent past the nodes": dict(parent=with_parent(4, 16)),
        "negative parent": dict(parent=with_parent(7, -1)),
        "own parent": dict(parent=with_parent(5, 5)),
        "one node": dict(n_nodes=1),
        "no node": dict(n_nodes=0),
        "k = 0": dict(k=0),
        "L = 0": dict(Lv=0),
        "no context": dict(handle=None),
        "no parent": dict(parent=None),
        "no flags": dict(is_leaf=None),
        "no descriptors": dict(desc=None),
        "no weights": dict(weight=None),
    }
    for what, kw in refused.items():
        r, out = create(**kw)
        assert r == ARG and not out.value, what
    assert L.orbx_vocab_create(ctx.handle, V["k"], V["L"], len(V["parent"]), ox._ptr(V["parent"]),
                               ox._ptr(V["is_leaf"]), ox._ptr(V["desc"]), ox._ptr(V["weight"]), None) == ARG


def test_vocabulary_serves_a_second_context(ctx):
    """A vocabulary created on one context is accepted by another context of the device."""
    D = vs.random_descriptors(257, 9)
    S = vs.scene("levels_1", D)
    voc = create_vocab(ctx, S["V"])
    other = ox.Context(nfeatures=100, max_w=64, max_h=64, slots=1)
    try:
        held(S, host_transform(other, voc, D, S["levelsup"]), D, "second context")
    finally:
        other.close()
        ox.lib().orbx_vocab_destroy(voc)
