"""CIDEr-D on the CPU: the oracle (tests/cider_oracle.py) on hand-checked cases, the package's host document-frequency table and key
packing against it, and the C entry point's limits (checked before any launch, so no GPU is needed)."""
import math
import random

import numpy as np
import pytest

from tests import cider_oracle as O

A, B_, C_, D_, E_, F_ = 10, 11, 12, 13, 14, 15


def test_candidate_equal_to_its_reference_scores_ten():
    corpus = [[[A, B_, C_, D_, E_]], [[20, 21, 22, 23]]]          # every n-gram of image 0 is unique to it
    df, n = O.document_frequency(corpus)
    assert O.cider_d([1, A, B_, C_, D_, E_, 2, 0], corpus[0], df, n) == pytest.approx(10.0, abs=1e-12)


def test_disjoint_captions_score_zero():
    corpus = [[[A, B_, C_]], [[D_, E_, F_]]]
    df, n = O.document_frequency(corpus)
    assert O.cider_d([D_, E_, F_], corpus[0], df, n) == 0.0


def test_length_penalty_closed_form():
    # cand [a a] against ref [a a a]: unigram and bigram vectors are parallel (sim 1 each), no tri- / 4-grams in the candidate;
    # bigram lengths 1 and 2 -> 10 * (1 + 1 + 0 + 0) / 4 * exp(-1 / 72)
    corpus = [[[A, A, A]], [[B_]]]
    df, n = O.document_frequency(corpus)
    assert O.cider_d([A, A], corpus[0], df, n) == pytest.approx(5.0 * math.exp(-1.0 / 72.0), rel=1e-12)


def test_ngram_in_every_image_has_zero_idf():
    corpus = [[[A, B_]], [[A, C_]]]
    df, n = O.document_frequency(corpus)
    assert df[(A,)] == 2 and df[(B_,)] == 1
    # unigram vectors {a: 0, b: log 2} are parallel, the bigram ones equal: 10 * (1 + 1) / 4
    assert O.cider_d([A, B_], corpus[0], df, n) == pytest.approx(5.0, rel=1e-12)
    from gan_image_captioning_amd.cider import CiderD, pack_keys
    sc = CiderD(corpus, 64, "cpu")
    k = int(pack_keys(np.array([[A]]), 1)[0])
    i = int(np.searchsorted(sc.keys.numpy(), k))
    assert sc.keys[i] == k and float(sc.idf[i]) == 0.0


def test_empty_candidate_scores_zero():
    corpus = [[[A, B_, C_]], [[D_]]]
    df, n = O.document_frequency(corpus)
    assert O.cider_d([], corpus[0], df, n) == 0.0
    assert O.cider_d([1, 2, 0, 0], corpus[0], df, n) == 0.0            # all specials


def _random_corpus(rng, images, V, max_refs=5, max_len=20):
    return [[[rng.randrange(0, V) for _ in range(rng.randrange(0, max_len + 1))] for _ in range(rng.randrange(1, max_refs + 1))]
            for _ in range(images)]


@pytest.mark.parametrize("V", [8, 50, 32768])
def test_host_df_table_matches_the_oracle(V):
    from gan_image_captioning_amd.cider import CiderD, document_frequency, unpack_key
    rng = random.Random(V)
    corpus = _random_corpus(rng, 40, V)
    df, n = O.document_frequency(corpus)
    keys, counts = document_frequency(corpus)
    assert np.all(keys[1:] > keys[:-1])
    got = {unpack_key(k): int(c) for k, c in zip(keys, counts)}
    assert got == df
    sc = CiderD(corpus, V, "cpu")
    assert sc.log_n == pytest.approx(math.log(n))
    want = np.array([math.log(n) - math.log(max(1, df[unpack_key(k)])) for k in keys], dtype=np.float32)
    np.testing.assert_array_equal(sc.idf.numpy(), want)


def test_key_packing_round_trips():
    from gan_image_captioning_amd.cider import pack_keys, unpack_key
    rng = np.random.default_rng(0)
    for n in range(1, 5):
        toks = rng.integers(0, 32768, size=(100, n))
        toks[0] = 32767
        keys = pack_keys(toks, n)
        assert all(unpack_key(k) == tuple(int(t) for t in row) for k, row in zip(keys, toks))
        assert int(keys.max()) < 2 ** 62
    # n-gram order of keys: all unigrams before all bigrams, ...
    assert pack_keys(np.array([[32767]]), 1)[0] < pack_keys(np.array([[0, 0]]), 2)[0]


def test_vocabulary_and_lengths_beyond_the_limits_are_refused():
    from gan_image_captioning_amd.cider import CiderD, RefBatch
    with pytest.raises(ValueError, match="32768"):
        CiderD([[[4, 5]]], 32769, "cpu")
    with pytest.raises(ValueError):
        RefBatch.pack([[list(range(4, 4 + 65))]])
    with pytest.raises(ValueError):
        RefBatch.pack([[[4]] * 33])


def test_entry_point_limits_return_unsupported_before_any_launch():
    from gan_image_captioning_amd import _lib
    lib = _lib.load()
    ok = dict(n_cand=4, Lc=20, n_ref=4, Lr=20, B=2, max_refs=2, V=1000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gic_cider_d(None, a["Lc"], None, None, a["n_cand"], a["Lc"], None, a["Lr"], None, None, a["n_ref"], a["Lr"], a["B"],
                               a["max_refs"], None, None, 0, 1.0, a["V"], None, None)

    assert call() == -1                                   # the limits pass; then the NULL pointers are refused
    for kw in ({"V": 32769}, {"Lc": 65}, {"Lr": 65}, {"max_refs": 33}):
        assert call(**kw) == -2, kw
        assert b"cider_d" in lib.gic_last_error()
    for kw in ({"n_cand": -1}, {"B": -1}, {"V": 0}, {"B": 0}):
        assert call(**kw) == -1, kw
    assert call(n_cand=0) == 0                            # nothing to score: no launch
