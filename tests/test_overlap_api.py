"""The n-gram overlap metrics without a GPU: the C ABI of gic_caption_overlap (symbol, argument statuses and limits before any launch),
the float64 oracle (tests/overlap_oracle.py) against utils.bleu_score, brute force and a hand-worked example, metrics.corpus_bleu and
RewardMix's weight validation, the new flags, the default SCST scorer, and the problems of tests/test_gpu_overlap.py: each is checked
here, with the oracle alone, to hold the cases the kernel test relies on."""
import itertools
import os
import random
import re

import pytest

from tests import overlap_oracle as O
from tests.test_gpu_overlap import PROBLEMS, overlap_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- the C ABI
def test_symbol_declared_bound_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    assert re.search(r"\bgic_caption_overlap\(", hdr)
    assert "gic_caption_overlap" in L.EXPORTED_SYMBOLS
    assert lib.gic_caption_overlap is not None
    assert int(re.search(r"#define GIC_OVERLAP_STATS (\d+)", hdr).group(1)) == L.OVERLAP_STATS == 10
    assert lib.gic_abi_version() == 5                      # a backwards-compatible addition


def _call(lib, n_cand=2, Lc=8, n_ref=2, Lr=8, B=2, max_refs=1, V=100, null=(), ld_cand=None, ld_ref=None):
    """One call on fake (non-null, aligned) pointers: every status comes back before any launch."""
    p = {k: 0x1000 * (i + 1) for i, k in enumerate(("cand", "cand_len", "cand_img", "ref", "ref_len", "ref_off", "stats", "rouge", "sbleu"))}
    for k in null:
        p[k] = None
    return lib.gic_caption_overlap(p["cand"], Lc if ld_cand is None else ld_cand, p["cand_len"], p["cand_img"], n_cand, Lc, p["ref"],
                                   Lr if ld_ref is None else ld_ref, p["ref_len"], p["ref_off"], n_ref, Lr, B, max_refs, V, p["stats"],
                                   p["rouge"], p["sbleu"], None)


def test_null_and_negative_arguments_are_invalid():
    _, lib = _lib()
    for name in ("cand", "cand_len", "cand_img", "ref", "ref_len", "ref_off", "stats", "rouge", "sbleu"):
        assert _call(lib, null=(name,)) == -1, name
        assert b"null" in lib.gic_last_error(), name
    for kw in ({"n_cand": -1}, {"Lc": -1}, {"n_ref": -1}, {"Lr": -1}, {"B": -1}, {"max_refs": -1}, {"V": 0}, {"B": 0}, {"ld_cand": 4},
               {"ld_ref": 4}):
        assert _call(lib, **kw) == -1, kw
        assert lib.gic_last_error()
    assert _call(lib, n_cand=0, null=("cand", "stats", "rouge", "sbleu")) == 0        # nothing to score


def test_limits_are_unsupported_without_a_gpu():
    L, lib = _lib()
    assert (L.CIDER_MAX_LEN, L.CIDER_MAX_REFS, L.CIDER_MAX_VOCAB) == (64, 32, 32768)
    for kw in ({"Lc": 65}, {"Lr": 65}, {"max_refs": 33}, {"V": 32769}):
        assert _call(lib, **kw) == L.ERR_UNSUPPORTED, kw
        assert lib.gic_last_error()
    assert _call(lib, Lc=65, null=("cand",)) == L.ERR_UNSUPPORTED             # the limits come first


def test_python_scorer_refuses_what_the_kernel_refuses():
    import torch
    from gan_image_captioning_amd.cider import RefBatch
    from gan_image_captioning_amd.metrics import OverlapScorer
    with pytest.raises(ValueError, match="32768"):
        OverlapScorer(32769)
    refs = RefBatch.pack([[[4, 5]]])
    with pytest.raises(ValueError, match="at most 64"):
        OverlapScorer(100).score(torch.zeros(1, 65, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), refs)
    with pytest.raises(ValueError, match="references for 1"):
        OverlapScorer(100).score(torch.zeros(2, 3, 8, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32), refs)


# ---------------------------------------------------------------- the oracle
def _random_corpus(rng):
    """A few images with 1..5 references each and one candidate per image: lengths 0..64, small vocabularies so that tokens and
    n-grams repeat, specials inside the captions."""
    V = rng.choice((5, 8, 20, 200))
    cands, refs = [], []
    for _ in range(rng.randrange(1, 6)):
        group = [[rng.randrange(0, V) for _ in range(rng.randrange(0, 65))] for _ in range(rng.randrange(1, 6))]
        kind = rng.random()
        if kind < 0.3:
            c = list(rng.choice(group))
        elif kind < 0.6:
            src = rng.choice(group)
            c = src[:rng.randrange(0, len(src) + 1)] + [rng.randrange(0, V) for _ in range(rng.randrange(0, 8))]
        else:
            c = [rng.randrange(0, V) for _ in range(rng.randrange(0, 65))]
        cands.append(c[:64])
        refs.append(group)
    return cands, refs


def test_summed_stats_give_the_corpus_bleu_of_utils():
    from gan_image_captioning_amd.metrics import corpus_bleu
    from gan_image_captioning_amd.utils import bleu_score
    rng = random.Random(0)
    nonzero = [0, 0, 0, 0]
    for _ in range(240):
        cands, refs = _random_corpus(rng)
        total = [sum(col) for col in zip(*(O.stats(c, r) for c, r in zip(cands, refs)))]
        got = corpus_bleu(total)
        words = [O.tokens(c) for c in cands]
        ref_words = [[O.tokens(x) for x in r] for r in refs]
        assert got[3] == pytest.approx(bleu_score(words, ref_words), rel=1e-12, abs=0.0)
        for n in (1, 2, 3):
            assert got[n - 1] == pytest.approx(bleu_score(words, ref_words, max_n=n, weights=(1.0 / n,) * n), rel=1e-12, abs=0.0)
        assert got == pytest.approx(O.corpus_bleu(total), rel=1e-12, abs=0.0)
        nonzero = [k + (g > 0) for k, g in zip(nonzero, got)]
    assert min(nonzero) >= 50                     # BLEU-4 included: the comparison is not between zeros


def test_corpus_bleu_takes_tensors_and_checks_its_input():
    import torch
    from gan_image_captioning_amd.metrics import STAT_COLUMNS, corpus_bleu
    assert len(STAT_COLUMNS) == 10
    s = [5, 4, 3, 2, 6, 5, 4, 3, 6, 7]
    assert corpus_bleu(torch.tensor(s, dtype=torch.int64)) == corpus_bleu(s) == pytest.approx(O.corpus_bleu(s), rel=1e-12)
    assert corpus_bleu([3, 2, 0, 0, 6, 5, 4, 3, 6, 6])[2:] == [0.0, 0.0] and corpus_bleu([0] * 10) == [0.0] * 4
    with pytest.raises(ValueError):
        corpus_bleu(s[:9])


def _lcs_brute(a, b):
    best = 0
    for k in range(len(a), 0, -1):
        for idx in itertools.combinations(range(len(a)), k):
            sub = [a[i] for i in idx]
            it = iter(b)
            if all(any(t == u for u in it) for t in sub):
                return k
    return best


def test_lcs_table_equals_brute_force_enumeration():
    rng = random.Random(1)
    seen = set()
    for _ in range(400):
        a = [rng.randrange(3, 7) for _ in range(rng.randrange(0, 9))]
        b = [rng.randrange(3, 7) for _ in range(rng.randrange(0, 9))]
        want = _lcs_brute(a, b)
        assert O.lcs(a, b) == want == O.lcs(b, a)
        seen.add(want)
    assert {0, 1, 2, 3, 4, 5} <= seen


def test_rouge_l_hand_worked_example():
    """candidate  c  = 4 5 6 7 8      (len 5; <S> = 1 and <E> = 2 around it are dropped)
       reference r1 = 4 6 5 7 9 8    (len 6): LCS = 4 (4 5 7 8, or 4 6 7 8)     -> lcs/len_c = 4/5, lcs/len_r = 4/6
       reference r2 = 7 8            (len 2): LCS = 2 (7 8)                      -> lcs/len_c = 2/5, lcs/len_r = 2/2
       P = max(4/5, 2/5) = 0.8, R = max(4/6, 1) = 1, beta^2 = 1.44
       ROUGE-L = (1 + 1.44) * 0.8 * 1 / (1 + 1.44 * 0.8) = 1.952 / 2.152 = 0.90706319...
       stats: unigrams 4 5 6 7 8 all in r1 -> 5 of 5; bigrams (7 8) in r2 only -> 1 of 4; no common 3- / 4-gram -> 0 of 3, 0 of 2;
       closest length: |5 - 6| = 1 < |5 - 2| -> 6
       sbleu = exp(1 - 6/5) * (5/5 * 2/5 * 1/4 * 1/3)^(1/4) = exp(-0.2) * (1/30)^(1/4)"""
    c, r1, r2 = [1, 4, 5, 6, 7, 8, 2], [4, 6, 5, 7, 9, 8], [7, 8]
    assert O.lcs(O.tokens(c), r1) == 4 and O.lcs(O.tokens(c), r2) == 2
    assert O.rouge_l(c, [r1, r2]) == pytest.approx(1.952 / 2.152, rel=1e-12)
    assert O.rouge_l(c, [r1, r2]) == pytest.approx(0.90706319, abs=1e-8)
    assert O.stats(c, [r1, r2]) == [5, 1, 0, 0, 5, 4, 3, 2, 5, 6]
    assert O.sbleu(c, [r1, r2]) == pytest.approx(2.718281828459045 ** -0.2 * (1.0 / 30.0) ** 0.25, rel=1e-12)
    assert O.rouge_l([1, 2], [r1]) == 0.0 and O.rouge_l(c, [[0, 1]]) == 0.0 and O.rouge_l(c, []) == 0.0
    assert O.stats(c, []) == [0] * 10 and O.sbleu(c, []) == 0.0 and O.sbleu([9, 9], [[4, 5]]) == 0.0
    assert O.stats([4, 4, 4], [[4, 4], [4, 5, 6, 7]])[:4] == [2, 1, 0, 0]                      # clipped by the best single reference
    assert O.stats([4, 5, 6], [[4] * 5, [7]])[9] == 1 and O.stats([4, 5, 6], [[4] * 2, [7] * 4])[9] == 2      # ties: the shorter


@pytest.mark.parametrize("V,images,max_refs", PROBLEMS)
def test_gpu_problems_hold_the_cases_the_kernel_test_needs(V, images, max_refs):
    corpus, cands, cimg = overlap_problem(V, images, max_refs)
    per = [corpus[b] for b in cimg]
    stats, rouge, sbleu = O.score_all(cands, per)
    assert max(len(r) for r in corpus) == max_refs and min(len(r) for r in corpus) >= 1
    lens = {s[8] for s in stats}
    assert 0 in lens and max(lens) == 64
    assert any(c and not O.tokens(c) for c in cands)                                          # specials only
    assert any(s[3] > 0 for s in stats)                                                       # a shared 4-gram
    assert any(r > 0.5 for r in rouge) and any(0.0 < r < 0.5 for r in rouge)
    assert any(0.0 < x < 0.999 for x in sbleu)
    assert any(s[0] > max(O.lcs(O.tokens(r), O.tokens(c)) for r in refs) for s, c, refs in zip(stats, cands, per))   # order matters
    def tie_to_shorter(s, refs):
        ls = [len(O.tokens(r)) for r in refs]
        return any(l > s[9] and abs(l - s[8]) == abs(s[9] - s[8]) for l in ls)
    assert any(tie_to_shorter(s, refs) for s, refs in zip(stats, per))
    assert all(0 <= s[n] <= s[4 + n] for s in stats for n in range(4))


# ---------------------------------------------------------------- rewards, flags, the default scorer
class _Fixed:
    def __init__(self, *vals):
        self.vals, self.calls = vals, 0

    def score(self, cand_ids, cand_lengths, refs, cand_img=None):
        self.calls += 1
        return self.vals if len(self.vals) > 1 else self.vals[0]


def test_reward_mix_validates_its_weights_and_skips_unweighted_scorers():
    import torch
    from gan_image_captioning_amd.metrics import RewardMix
    for w in ((-1.0, 0.0, 0.0), (1.0, -0.5, 0.0), (1.0, 0.0, float("nan")), (float("inf"), 0.0, 0.0), (0.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            RewardMix(object(), object(), *w)
    with pytest.raises(ValueError):
        RewardMix(None, object(), 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        RewardMix(object(), None, 1.0, 0.5, 0.0)
    c, r, b = torch.tensor([2.0, 4.0]), torch.tensor([0.5, 0.25]), torch.tensor([0.125, 1.0])
    cider, overlap = _Fixed(c), _Fixed(None, r, b)
    got = RewardMix(cider, overlap, 1.0, 0.5, 0.25).score(None, None, None)
    assert torch.equal(got, c + 0.5 * b + 0.25 * r) and (cider.calls, overlap.calls) == (1, 1)
    cider, overlap = _Fixed(c), _Fixed(None, r, b)
    assert torch.equal(RewardMix(cider, overlap, 2.0, 0.0, 0.0).score(None, None, None), 2.0 * c) and overlap.calls == 0
    assert torch.equal(RewardMix(None, overlap, 0.0, 0.0, 1.0).score(None, None, None), r) and cider.calls == 1


def test_flags_parse_with_their_defaults():
    from gan_image_captioning_amd.args import build_parser
    a = build_parser().parse_args([])
    assert (a.scst_cider_weight, a.scst_bleu_weight, a.scst_rouge_weight, a.eval_metrics_beam_size) == (1.0, 0.0, 0.0, 0)
    a = build_parser().parse_args(["--scst-cider-weight", "1", "--scst-bleu-weight", "0.5", "--scst-rouge-weight", "0.25",
                                   "--eval-metrics-beam-size", "3"])
    assert (a.scst_cider_weight, a.scst_bleu_weight, a.scst_rouge_weight, a.eval_metrics_beam_size) == (1.0, 0.5, 0.25, 3)


def test_default_flags_build_a_plain_cider_scorer():
    import inspect
    from gan_image_captioning_amd import training
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.cider import CiderD
    from gan_image_captioning_amd.metrics import RewardMix
    corpus = [[[4, 5, 6], [4, 6]], [[7, 8]]]
    sc = training.scst_reward_scorer(default_args(device="cpu", vocab_size=16), corpus)
    assert type(sc) is CiderD
    mix = training.scst_reward_scorer(default_args(device="cpu", vocab_size=16, scst_bleu_weight=0.5, scst_rouge_weight=0.5), corpus)
    assert type(mix) is RewardMix and type(mix.cider) is CiderD and mix.overlap is not None
    only = training.scst_reward_scorer(default_args(device="cpu", vocab_size=16, scst_cider_weight=0.0, scst_rouge_weight=1.0), corpus)
    assert only.cider is None                     # no table is built for a scorer that is never launched
    with pytest.raises(ValueError):
        training.scst_reward_scorer(default_args(device="cpu", vocab_size=16, scst_cider_weight=0.0), corpus)
    src = inspect.getsource(training.GANInstructor.scst_train)
    assert "scst_reward_scorer(args, groups.references())" in src and "RewardMix" not in src
