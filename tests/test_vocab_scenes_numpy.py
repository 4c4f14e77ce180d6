"""The constructed vocabularies of tests/vocab_scenes.py on the CPU: on random
descriptors and on the oracle's extraction of the frame the device test
uses (the oracle's extraction is bit-exact to the device's, so these are the
descriptors the slots will hold), every builder's property holds, every
scene's pinned outcome holds on the numpy restatement and on the oracle
(oracle/ref_vocab.cpp), and the two are equal, float64 as bit patterns.
The mutation table shows which scenes tell each wrong reading of DBoW2's
transform apart.  This pins the scenes before the device sees them
(test_vocab_scenes_gpu.py)."""
import functools

import numpy as np
import pytest

import vocab_scenes as vs
from oracle_lib import RefExtractor
from orb_slam_amd import synth
from vocab_data import run_ref


@functools.lru_cache(maxsize=None)
def frame_descriptors(nfeatures, nlevels):
    """The oracle's extraction of the synthetic frame under a context's settings."""
    w, h, seed = vs.FRAME
    return RefExtractor(nfeatures=nfeatures, nlevels=nlevels)(synth.texture_frame(w, h, seed=seed))[1]


def sources():
    out = [(f"random{n}", lambda n=n: vs.random_descriptors(4096, 1)[:n]) for n in vs.HOST_SIZES]
    out += [(f"frame{nf}", lambda nf=nf, nl=nl: frame_descriptors(nf, nl)) for nf, nl in vs.SLOT_SHAPES]
    return out


SOURCES = sources()


@pytest.mark.parametrize("source", [s for s, _ in SOURCES])
def test_scene_pins_restatement_oracle_agree(source):
    D = dict(SOURCES)[source]()
    for name in vs.NAMES:
        S = vs.scene(name, D)                       # asserts the builder's property and the pin on the restatement
        R = run_ref(S["V"], D, S["levelsup"])
        S["pin"](vs.trim(R))
        assert not vs.differences(S["T"], R), (name, vs.differences(S["T"], R))


@pytest.mark.parametrize("nf,nlevels", vs.SLOT_SHAPES)
def test_frame_fills_every_quota(nf, nlevels):
    """The texture frame gives exactly nfeatures distinct descriptors under
    every slot shape, so each lands in the keys-per-thread class it is there for."""
    D = frame_descriptors(nf, nlevels)
    assert len(D) == nf and len(vs.distinct_rows(D)) == nf
    assert vs.keys_per_thread(len(D)) == {64: 1, 65: 1, 96: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 4, 4096: 4}[nf]


def test_runs_scene_positions():
    """The runs scene states where in the sorted keys its properties sit, for
    2 and for 4 keys a thread, on every source large enough to have them."""
    for nf, nl in vs.SLOT_SHAPES:
        if nf >= vs.BIG:
            P = vs.scene("runs", frame_descriptors(nf, nl))["positions"]
            for per in (2, 4):
                assert P[per]["starts_inside_chunk"] % per and P[per]["head_last_of_chunk"] % per == per - 1
                assert P[per]["chunk_of_heads"] % per == 0


def test_few_words_tell_the_sum_orders_apart():
    D = frame_descriptors(2048, 8)
    for name in ("two_words", "three_words"):
        T = vs.scene(name, D)["T"]
        assert np.bincount(T["word"]).min() >= 200
        assert any(len(set(vs._three_sums(T["weight"][T["word"] == w]))) == 3 for w in np.unique(T["word"]))


# edit of the restatement -> scenes that must fail under it (DESIGN.md has the full table)
MUTATION_TABLE = {
    "last_min": ["tie_dup_0_1", "tie_dup_first_last", "tie_dup_63_64", "tie_equal", "interleaved"],
    "le": ["tie_dup_0_1", "tie_dup_first_last", "tie_dup_63_64", "tie_equal", "interleaved"],
    "reverse_children": ["tie_dup_0_1", "tie_dup_first_last", "tie_dup_63_64", "tie_equal", "interleaved"],
    "pairwise": ["two_words", "three_words"],
    "count_times_w": ["two_words", "three_words"],
    "norm_feature_order": ["identity", "identity_root"],
    "w_ge_0": ["stopped_all", "stopped_but_one", "stopped_alternate", "stopped_ends"],
    "nid_level_plus_1": ["levels_0", "levels_1", "levels_2", "levels_L", "chain20"],
    "nid_level_minus_1": ["levels_0", "levels_1", "levels_2", "chain20"],
    "shallow_nid_0": ["levels_0", "levels_1"],
    "fv_word_order": ["identity_root", "levels_L", "levels_L_plus_2"],
}


@pytest.mark.parametrize("source", ["random2048", "frame2048"])
@pytest.mark.parametrize("mutation", vs.MUTATIONS)
def test_mutations_are_caught(mutation, source):
    """Every listed edit of the restatement differs from the oracle on each
    scene the table names (and the table names every edit)."""
    assert set(MUTATION_TABLE) == set(vs.MUTATIONS)
    D = dict(SOURCES)[source]()
    for name in MUTATION_TABLE[mutation]:
        S = vs.scene(name, D)
        R = run_ref(S["V"], D, S["levelsup"])
        assert vs.differences(vs.transform(S["V"], D, S["levelsup"], {mutation}), R), (mutation, name)
