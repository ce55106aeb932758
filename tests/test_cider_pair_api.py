"""Pairwise CIDEr-D, consensus selection and Self-CIDEr without a GPU: the oracle (tests/cider_pair_oracle.py) against the
multi-reference oracle and against analytic spectra, the error budget of the kernel's lambda_max iteration (restated in float32),
gic_cider_pairwise's argument checks (each returns -1 with a message that names the argument, before any launch), the flags, keywords
and symbols, and the eligibility of the cases whose order tests/test_gpu_cider_pair.py compares."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd.args import default_args
from tests import cider_oracle as CO
from tests import cider_pair_oracle as PO
from tests import test_constrained_api as T


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("seed,V,K", [(0, 8, 2), (1, 8, 5), (2, 30, 7), (3, 300, 3)])
def test_pairwise_oracle_agrees_with_the_multi_reference_oracle(seed, V, K):
    rng = np.random.RandomState(seed)
    caps = [[1] + rng.randint(3, V, size=rng.randint(0, 12)).tolist() + [2] for _ in range(K)]
    caps[-1] = list(caps[0])                                                   # a duplicate
    corpus = [caps] + [[rng.randint(3, V, size=8).tolist() for _ in range(2)] for _ in range(4)]
    df, n = CO.document_frequency(corpus)
    M = PO.pair_matrix(caps, df, n)
    for i in range(K):
        for j in range(K):
            assert M[i, j] == CO.cider_d(caps[i], [caps[j]], df, n)
    cons = PO.consensus(M)
    for i in range(K):
        assert abs(cons[i] - (K * CO.cider_d(caps[i], caps, df, n) - M[i, i]) / (K - 1)) <= 1e-12
    assert M[0, K - 1] == M[0, 0] and (M >= 0).all() and (M <= 10.0 + 1e-12).all()
    S = PO.similarity(M)
    assert np.array_equal(S, S.T) and (np.diag(S) <= 1.0 + 1e-12).all()


def test_diagonal_counts_the_non_zero_vectors():
    corpus = [[[3, 4, 5, 6, 7]], [[3, 8, 9, 10, 11]], [[3, 12, 13, 14, 15]]]     # token 3 is in every image: idf 0
    df, n = CO.document_frequency(corpus)
    caps = [[4, 5, 6, 7, 8], [4, 5, 6], [4, 5], [4], [3], [], [1, 2, 0]]
    assert np.diag(PO.pair_matrix(caps, df, n)).tolist() == pytest.approx([10.0, 7.5, 5.0, 2.5, 0.0, 0.0, 0.0], abs=1e-12)
    assert PO.consensus(np.array([[10.0]])).tolist() == [0.0] and PO.self_cider(np.array([[10.0]])) == 0.0
    assert PO.self_cider(np.zeros((3, 3))) == 0.0


# captions of >= 4 tokens over a corpus of 4 images in which no n-gram is in every image
def _disjoint(K, length=5):
    return [[3 + length * k + t for t in range(length)] for k in range(K)]


def _table(caps):
    corpus = [[c] for c in caps[:3]] + [[[3000, 3001, 3002, 3003]]]
    return CO.document_frequency(corpus)


@pytest.mark.parametrize("K", [2, 5, 8, 32])
def test_analytic_spectra(K):
    caps = _disjoint(K)
    df, n = _table(caps)
    assert n >= 3
    same = PO.pair_matrix([caps[0]] * K, df, n)
    assert np.allclose(same, 10.0, atol=1e-12) and abs(PO.self_cider(same)) <= 1e-12 and PO.self_cider_f32(same) <= 1e-6
    apart = PO.pair_matrix(caps, df, n)
    assert np.allclose(apart, 10.0 * np.eye(K), atol=1e-12) and abs(PO.self_cider(apart) - 1.0) <= 1e-12
    assert abs(PO.self_cider_f32(apart) - 1.0) <= 1e-6
    if K % 2 == 0 and K > 2:
        two = PO.pair_matrix([caps[0]] * (K // 2) + [caps[1]] * (K // 2), df, n)
        assert abs(PO.self_cider(two) - math.log(2) / math.log(K)) <= 1e-12
        assert abs(PO.self_cider_f32(two) - math.log(2) / math.log(K)) <= 1e-6


def test_lambda_max_budget():
    """The measured number: max |self_cider_f32 - self_cider_f64| over the GPU test's problems and the near-degenerate spectra."""
    worst_cases = worst_spectra = 0.0
    for case in PO.CASES:
        _, (M, _, sc) = PO.case_problem(case)
        worst_cases = max([worst_cases] + [abs(PO.self_cider_f32(M[b]) - sc[b]) for b in range(M.shape[0])])
    spectra = PO.near_degenerate_spectra()
    for S in spectra:
        worst_spectra = max(worst_spectra, abs(PO.self_cider_s_f32(S) - PO.self_cider_s(S)))
    print(f"[cider_pair] lambda_max restatement, {PO.SQUARINGS} squarings: max |f32 - f64| self_cider {worst_cases:.3e} over the GPU problems, "
          f"{worst_spectra:.3e} over {len(spectra)} two-cluster spectra; TOL_SELF_CIDER {PO.TOL_SELF_CIDER:.3e}")
    assert PO.SQUARINGS == L.CIDER_PAIR_SQUARINGS
    assert PO.TOL_SELF_CIDER <= 1e-3
    assert max(worst_cases, worst_spectra) <= PO.TOL_SELF_CIDER / 4


def test_the_spectra_are_near_degenerate():
    """The sweep holds what the budget is about: top eigenvalues 1e-5 apart (relative), and equal."""
    gaps = []
    for S in PO.near_degenerate_spectra():
        ev = np.linalg.eigvalsh(S)
        gaps.append((ev[-1] - ev[-2]) / ev[-1])
    gaps = np.array(gaps)
    assert gaps.min() <= 1e-12 and ((gaps > 1e-6) & (gaps < 2e-5)).any() and ((gaps > 2e-5) & (gaps < 2e-4)).any() and gaps.max() > 0.5
    # plain power iteration with a few dozen steps does not meet the budget there: 32 steps from the all-ones vector
    worst = 0.0
    for S in PO.near_degenerate_spectra():
        v = np.ones(S.shape[0])
        for _ in range(32):
            v = S @ v
            v /= np.linalg.norm(v)
        ratio = float(v @ S @ v) / float(np.trace(S))
        worst = max(worst, abs(PO.self_cider_of_ratio(ratio, S.shape[0]) - PO.self_cider_s(S)))
    assert worst > 1e-3


def test_problems_hold_the_edge_cases():
    for case in PO.CASES:
        V, B, K, Lmax = case
        prob, (M, cons, sc) = PO.case_problem(case)
        ids, lengths = prob["ids"], prob["lengths"]
        assert ids.shape == (B, K, Lmax) and lengths.shape == (B, K) and int(ids.max()) < V and int(lengths.max()) <= Lmax
        if K > 1:
            off = M - np.stack([np.diag(np.diag(m)) for m in M])
            assert off.max() > 1.0, "no real match in the problem"
        else:
            assert not cons.any() and not sc.any()
        if K >= 8:
            stripped = [[len(CO.tokens(c)) for c in PO.captions(prob, b)] for b in range(B)]
            assert all(0 in s and {1, 2, 3} & set(s) for s in stripped)                              # empty / specials-only, and 1-3 tokens
            assert any(int(lengths[b, k]) > 0 and stripped[b][k] == 0 for b in range(B) for k in range(K))
            assert any(max(CO.ngrams(CO.tokens(c), 1).values(), default=0) > 1 for b in range(B) for c in PO.captions(prob, b))
        if K >= 3:
            assert any(np.array_equal(M[b][i], M[b][j]) and M[b][i, j] == M[b][i, i] > 0 for b in range(B) for i in range(K) for j in range(i))
        if K == 32:
            assert int(lengths.max()) == 64 and any(len(CO.tokens(c)) == 64 for c in PO.captions(prob, 0))
        if V == 32768:
            assert int(ids.max()) == 32767
    assert not np.allclose(PO.case_problem(PO.FOREIGN_DF)[1][0], 0.0)


# ------------------------------------------------------------------------------------------------ argument checks (host only)
FAKE = [0x10000 * (i + 1) for i in range(8)]          # distinct non-null addresses: never dereferenced (the checks come first)


def _args(**kw):
    a = dict(ids=FAKE[0], ld=20, lengths=FAKE[1], B=4, K=5, L=20, keys=FAKE[2], idf=FAKE[3], n_keys=100, log_n=1.5, V=1000, matrix=FAKE[4],
             consensus=FAKE[5], self_cider=FAKE[6])
    a.update(kw)
    return [a[k] for k in ("ids", "ld", "lengths", "B", "K", "L", "keys", "idf", "n_keys", "log_n", "V", "matrix", "consensus", "self_cider")] + [None]


def _refused(status, *words):
    assert status == -1
    msg = L.load().gic_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_pairwise_argument_checks():
    f = L.load().gic_cider_pairwise
    for K in (0, 33, -1):
        _refused(f(*_args(K=K)), f"K={K}")
    for Lc in (0, 65):
        _refused(f(*_args(L=Lc, ld=80)), f"L={Lc}")
    _refused(f(*_args(V=32769)), "V=32769")
    _refused(f(*_args(V=0)), "V=0")
    _refused(f(*_args(B=0)), "B=0")
    _refused(f(*_args(matrix=None, consensus=None, self_cider=None)), "matrix", "consensus", "self_cider")
    _refused(f(*_args(ids=None)), "ids")
    _refused(f(*_args(lengths=None)), "lengths")
    _refused(f(*_args(keys=None)), "keys")
    _refused(f(*_args(idf=None)), "idf")
    _refused(f(*_args(log_n=float("nan"))), "log_n")
    _refused(f(*_args(log_n=-1.0)), "log_n")
    _refused(f(*_args(ld=19)), "ld_ids=19", "L=20")
    _refused(f(*_args(n_keys=-1)), "n_keys=-1")


# ------------------------------------------------------------------------------------------------ pins
def test_symbol_header_and_abi_version():
    import os
    lib = L.load()
    assert "gic_cider_pairwise" in L.EXPORTED_SYMBOLS and hasattr(lib, "gic_cider_pairwise")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gicap.h")).read()
    assert "int gic_cider_pairwise(" in header and "#define GIC_CIDER_PAIR_MAX_K 32" in header
    assert f"#define GIC_CIDER_PAIR_SQUARINGS {L.CIDER_PAIR_SQUARINGS}" in header
    assert L.CIDER_PAIR_MAX_K == 32
    assert lib.gic_abi_version() == L.ABI_VERSION == 5


def test_flags_and_keywords():
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.cider import CiderD
    from gan_image_captioning_amd.generator import Generator
    from gan_image_captioning_amd.training import GANInstructor
    a = default_args()
    assert (a.eval_consensus_samples, a.eval_consensus_weight) == (0, 1.0)
    p = inspect.signature(Generator.caption).parameters
    assert (p["consensus"].default, p["consensus_weight"].default, p["return_consensus"].default) == (None, 1.0, False)
    assert list(p)[-6:] == ["consensus", "consensus_weight", "return_consensus", "no_repeat_ngram", "min_length", "suppress_tokens"]
    assert list(p).index("return_rerank") == list(p).index("consensus") - 1
    p = inspect.signature(Generator.sample_captions).parameters
    assert (p["consensus"].default, p["consensus_weight"].default) == (None, 1.0)
    assert list(p)[-5:] == ["consensus", "consensus_weight", "no_repeat_ngram", "min_length", "suppress_tokens"]
    assert list(p).index("rerank_weight") == list(p).index("consensus") - 1
    p = inspect.signature(GANInstructor.evaluate_consensus).parameters
    assert list(p)[1:] == ["what", "num_samples", "top_k", "top_p", "temperature", "weight", "seed", "max_caption_len", "batch_size"]
    assert [p[k].default for k in list(p)[1:]] == ["val", 8, 0, 1.0, 1.0, 1.0, 1234, None, None]
    p = inspect.signature(engine.cider_pairwise).parameters
    assert list(p) == ["ids", "lengths", "keys", "idf", "log_n", "V", "want_matrix", "want_consensus", "want_self_cider"]
    assert [p[k].default for k in list(p)[-3:]] == [True, True, True]
    assert list(inspect.signature(CiderD.pairwise).parameters)[:3] == ["self", "ids", "lengths"]
    assert list(inspect.signature(CiderD.self_cider).parameters) == ["self", "ids", "lengths"]


def test_one_reranking_at_a_time_and_return_consensus_needs_consensus():
    """Both refusals come before any device work: the generator below has no decoder and no encoder."""
    import torch
    from gan_image_captioning_amd.generator import Generator
    gen = Generator.__new__(Generator)
    torch.nn.Module.__init__(gen)
    gen.decoder = object()
    with pytest.raises(ValueError, match="one re-ranking at a time"):
        gen.caption(None, consensus=object(), rerank_disc=object())
    with pytest.raises(ValueError, match="one re-ranking at a time"):
        gen.sample_captions(None, consensus=object(), rerank_disc=object())
    with pytest.raises(ValueError, match="return_consensus needs consensus"):
        gen.caption(None, return_consensus=True)


def test_cpu_tensors_are_refused():
    import torch
    from gan_image_captioning_amd import engine
    with pytest.raises(L.GicError, match="not on a GPU"):
        engine.cider_pairwise(torch.zeros(2, 3, 5, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64),
                              torch.zeros(4), 1.0, 50)


# ------------------------------------------------------------------------------------------------ the ordering cases of the GPU test
# (case of tests/test_constrained_api.beam_oracle, [(length_penalty, consensus_weight)]): beam search with k = 4 on the oracles' tiny
# decoders.  The seeds were picked by running the oracles: every image's beam selection is clear (margin >= 1e-4, so the device finds
# the same beams) and its adjacent finals lie more than ORDER_GAP apart under every (length_penalty, weight) listed.
ORDER_GAP = 1e-3
ORDER_CASES = [
    (("generic", 29, 4, 1, 0.0, T.C_NGRAM2), [(0.0, 4.0), (0.7, 2.0), (0.0, -4.0)]),
    (("attn", 75, 4, 1, 0.0, T.C_NGRAM2), [(0.0, 4.0), (0.7, 2.0), (0.0, -4.0)]),
]


def order_table(case):
    """The df table of an ordering case: (corpus, df, N)."""
    V = (T.ATTN_SHAPE if case[0] == "attn" else T.LSTM_SHAPES[case[0]])[2]
    corpus = PO.table_corpus(V)
    return (corpus,) + CO.document_frequency(corpus)


@pytest.mark.parametrize("case,settings", ORDER_CASES, ids=lambda v: T._case_id(v) if isinstance(v, tuple) else None)
def test_ordering_cases_are_eligible(case, settings):
    ids, scores, lengths, margins = T.beam_oracle(case)[:4]
    assert all(sel >= 1e-4 for sel, _ in margins), margins
    _, df, n = order_table(case)
    cons = PO.consensus_of(ids.numpy(), lengths.numpy(), df, n)
    moved = False
    for lp, w in settings:
        order, _, gaps = PO.rerank(scores.numpy(), lengths.numpy(), cons, w, lp)
        assert (gaps > ORDER_GAP).all(), (lp, w, gaps)                           # every image: none is left out
        moved = moved or (order != np.arange(order.shape[1])).any()
    assert moved, "the consensus changes no order: the case shows nothing"
