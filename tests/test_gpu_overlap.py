"""gic_caption_overlap (csrc/overlap.hip) against the float64 CPU oracle (tests/overlap_oracle.py) on the problem family of
tests/test_gpu_cider.py -- vocabulary sizes up to the 15-bit limit, caption lengths 0..64, 1..32 references per image, exact-reference,
prefix-plus-noise, specials-only, empty and length-64 candidates -- plus, per problem, a reversed reference (the LCS falls below the
unigram overlap) and a candidate midway between two reference lengths (the closest-length tie); bit-identical repeats in and out of
deterministic mode; the documented limits; GANInstructor.evaluate_metrics against evaluate / evaluate_cider / the oracle; SCST steps with
mixed rewards against the oracles, and with default weights against a step driven by a bare CiderD.

PROBLEMS and overlap_problem are shared with tests/test_overlap_api.py, which checks on the CPU, with the oracle alone, that every
problem holds the cases the kernel test relies on."""
import random

import numpy as np
import pytest
import torch

from tests import cider_oracle as CO
from tests import overlap_oracle as O
from tests.test_gpu_cider import _problem

PROBLEMS = [(50, 24, 5), (10000, 40, 32), (32768, 16, 7), (8, 12, 3)]          # V, images, max_refs: those of tests/test_gpu_cider.py


def overlap_problem(V, images, max_refs):
    """The CIDEr-D problem of the same parameters and seed, with two more candidates per problem: the first reference with >= 4 distinct
    tokens reversed, and -- for the first image with two references whose stripped lengths la < lb differ by an even amount and no
    reference closer to their midpoint -- the first (la + lb) / 2 tokens of the longer one."""
    corpus, cands, cimg = _problem(V + images, V, images, max_refs)
    cands, cimg = list(cands), list(cimg)
    for b, refs in enumerate(corpus):
        pick = next((O.tokens(r) for r in refs if len(set(O.tokens(r))) >= 4), None)
        if pick is not None:
            cands.append(pick[::-1])
            cimg.append(b)
            break
    for b, refs in enumerate(corpus):
        toks = sorted((O.tokens(r) for r in refs), key=len)
        tie = next(((x, y) for i, x in enumerate(toks) for y in toks[i + 1:]
                    if len(y) > len(x) and (len(y) - len(x)) % 2 == 0
                    and all(abs(len(t) - (len(x) + len(y)) // 2) >= (len(y) - len(x)) // 2 for t in toks)), None)
        if tie is not None:
            cands.append(tie[1][:(len(tie[0]) + len(tie[1])) // 2])
            cimg.append(b)
            break
    return corpus, cands, cimg


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _score(corpus, cands, cimg, V, dev):
    from gan_image_captioning_amd.cider import RefBatch
    from gan_image_captioning_amd.metrics import OverlapScorer
    refs = RefBatch.pack(corpus).to(dev)
    Lc = max([len(c) for c in cands] + [1])
    ids = torch.zeros(len(cands), Lc, dtype=torch.int64)
    for i, c in enumerate(cands):
        ids[i, :len(c)] = torch.tensor(c, dtype=torch.int64)
    lens = torch.tensor([len(c) for c in cands], dtype=torch.int32)
    return OverlapScorer(V, dev).score(ids.to(dev), lens.to(dev), refs, cand_img=torch.tensor(cimg, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("V,images,max_refs", PROBLEMS)
def test_kernel_matches_the_oracle(dev, V, images, max_refs):
    corpus, cands, cimg = overlap_problem(V, images, max_refs)
    stats, rouge, sbleu = _score(corpus, cands, cimg, V, dev)
    want_stats, want_rouge, want_sbleu = O.score_all(cands, [corpus[b] for b in cimg])
    got_stats = stats.cpu().numpy()
    rouge, sbleu = rouge.cpu().double().numpy(), sbleu.cpu().double().numpy()
    print("max |rouge - oracle| %.3g, max |sbleu - oracle| %.3g" % (np.abs(rouge - np.array(want_rouge)).max(),
                                                                 np.abs(sbleu - np.array(want_sbleu)).max()))
    assert got_stats.dtype == np.int32 and got_stats.shape == (len(cands), 10)
    assert np.array_equal(got_stats, np.array(want_stats, dtype=np.int32))
    np.testing.assert_allclose(rouge, np.array(want_rouge), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sbleu, np.array(want_sbleu), rtol=1e-5, atol=1e-5)


def test_image_grouped_batch_form_and_images_without_references(dev):
    """score() on [B, n, L] candidates (n per image, image-major) equals the oracle; an image without references scores zeros."""
    from gan_image_captioning_amd.cider import RefBatch
    from gan_image_captioning_amd.metrics import OverlapScorer
    rng = random.Random(3)
    V, B, n, L = 30, 6, 4, 16
    corpus = [[[rng.randrange(0, V) for _ in range(rng.randrange(1, L))] for _ in range(5)] for _ in range(B)]
    corpus[2] = []
    ids = torch.randint(0, V, (B, n, L))
    lens = torch.randint(0, L + 1, (B, n), dtype=torch.int32)
    stats, rouge, sbleu = OverlapScorer(V, dev).score(ids.to(dev), lens.to(dev), RefBatch.pack(corpus).to(dev))
    assert stats.shape == (B, n, 10) and rouge.shape == (B, n) and sbleu.shape == (B, n)
    cands = [ids[b, j, :int(lens[b, j])].tolist() for b in range(B) for j in range(n)]
    want_stats, want_rouge, want_sbleu = O.score_all(cands, [corpus[b] for b in range(B) for _ in range(n)])
    assert np.array_equal(stats.cpu().numpy().reshape(-1, 10), np.array(want_stats))
    np.testing.assert_allclose(rouge.cpu().double().numpy().reshape(-1), np.array(want_rouge), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sbleu.cpu().double().numpy().reshape(-1), np.array(want_sbleu), rtol=1e-5, atol=1e-5)
    assert not stats[2].any() and not rouge[2].any() and not sbleu[2].any()
    assert max(want_rouge) > 0 and max(want_sbleu) > 0


def test_candidates_outside_the_batch_and_broken_offsets(dev):
    """CIDEr-D's rule: a cand_img outside [0, B), more references than max_refs or offsets outside [0, n_ref] give NaN scores and
    stats -1; the other candidates are scored."""
    from gan_image_captioning_amd import engine
    ids = torch.tensor([[4, 5, 6, 7], [4, 5, 6, 7], [4, 5, 6, 7], [4, 5, 6, 7]], device=dev)
    lens = torch.full((4,), 4, dtype=torch.int32, device=dev)
    ref_ids = torch.tensor([[4, 5, 6, 7], [4, 5, 9, 9], [8, 8, 8, 8]], device=dev)
    ref_len = torch.full((3,), 4, dtype=torch.int32, device=dev)
    img = torch.tensor([0, 1, 2, -1], dtype=torch.int32, device=dev)
    off = torch.tensor([0, 1, 3], dtype=torch.int32, device=dev)          # image 1 holds 2 references: more than max_refs = 1
    stats, rouge, sbleu = engine.caption_overlap(ids, lens, img, ref_ids, ref_len, off, 1, 16)
    assert stats[0].tolist() == [4, 3, 2, 1, 4, 3, 2, 1, 4, 4] and float(rouge[0]) == 1.0 and float(sbleu[0]) == pytest.approx(1.0, abs=1e-6)
    for c in (1, 2, 3):
        assert stats[c].tolist() == [-1] * 10 and torch.isnan(rouge[c]) and torch.isnan(sbleu[c])
    off = torch.tensor([0, 1, 7], dtype=torch.int32, device=dev)          # past n_ref = 3
    stats, rouge, _ = engine.caption_overlap(ids, lens, img, ref_ids, ref_len, off, 8, 16)
    assert stats[0, 0] == 4 and stats[1].tolist() == [-1] * 10 and torch.isnan(rouge[1])


def test_repeat_calls_and_deterministic_mode_give_the_same_bits(dev):
    from gan_image_captioning_amd import engine
    corpus, cands, cimg = _problem(11, 10000, 64, 5)
    a = _score(corpus, cands, cimg, 10000, dev)
    b = _score(corpus, cands, cimg, 10000, dev)
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        c = _score(corpus, cands, cimg, 10000, dev)
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert float(a[1].max()) > 0.5


def test_limits_are_refused_before_any_launch(dev):
    from gan_image_captioning_amd import engine
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    base = dict(cand_ids=z(2, 8, dt=torch.int64), cand_len=z(2), cand_img=z(2), ref_ids=z(2, 8, dt=torch.int64), ref_len=z(2),
                ref_off=torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), max_refs=1, V=100)
    stats, rouge, sbleu = engine.caption_overlap(**base)
    torch.cuda.synchronize()
    assert stats.shape == (2, 10) and rouge.shape == (2,) and sbleu.shape == (2,)
    for kw in ({"V": 32769}, {"cand_ids": z(2, 65, dt=torch.int64)}, {"ref_ids": z(2, 65, dt=torch.int64)}, {"max_refs": 33}):
        with pytest.raises(NotImplementedError, match="status -2"):
            engine.caption_overlap(**dict(base, **kw))


# ---------------------------------------------------------------- evaluation and SCST
def _instructor(train=None, dev=None, **over):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    kw = dict(device="cuda", log_file=None, model_dir=None, save_dir=None, compute_dtype="fp32", vocab_size=64, gen_embed_dim=16,
              gen_hidden_dim=32, image_size=32, attn_dim=32, num_workers=0)
    kw.update(over)
    args = default_args(**kw)
    return GANInstructor(args, train, dev), args


@pytest.mark.parametrize("cgan", [0, 1])
def test_evaluate_metrics_equals_the_single_metric_evaluations(cgan):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.utils import bleu_score
    V = 64
    train = SyntheticCaptionData(8, V, 32, 8, seed=1, ragged=True)
    val = SyntheticCaptionData(10, V, 32, 8, seed=2, ragged=True)
    inst, _ = _instructor(train, val, conditional_gan=cgan, vocab_size=V, adv_eval_batch_size=4, max_seq_len=10)
    got = inst.evaluate_metrics("val", beam_size=2)
    assert set(got) == {"bleu1", "bleu2", "bleu3", "bleu4", "rouge_l", "cider_d"}
    assert got["bleu4"] == pytest.approx(inst.evaluate("val", beam_size=2), rel=1e-6)
    assert got["cider_d"] == inst.evaluate_cider("val", beam_size=2)
    cands, refs = [], []
    for ids, lengths, caps in inst._beam_decode("val", 2):
        ids, lengths = ids.cpu(), lengths.cpu()
        cands += [ids[b, :int(lengths[b])].tolist() for b in range(len(caps))]
        refs += caps
    assert got["rouge_l"] == pytest.approx(float(np.mean([O.rouge_l(c, r) for c, r in zip(cands, refs)])), rel=1e-5, abs=1e-6)
    stripped, stripped_refs = [O.tokens(c) for c in cands], [[O.tokens(x) for x in r] for r in refs]
    for n in (1, 2, 3, 4):
        assert got[f"bleu{n}"] == pytest.approx(bleu_score(stripped, stripped_refs, max_n=n, weights=(1.0 / n,) * n), rel=1e-6)


def test_evaluate_metrics_accumulates_over_batches_of_matching_captions():
    """An untrained generator shares next to nothing with its references, so the numbers above are near zero.  Here the decode is
    replaced, for all three evaluations alike, by each image's reference with every third caption perturbed: BLEU-4 is far from 0
    and from 1, and the sums run over three batches."""
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    V = 64
    train = SyntheticCaptionData(8, V, 32, 8, seed=1, ragged=True)
    val = SyntheticCaptionData(10, V, 32, 8, seed=2, ragged=True)
    inst, args = _instructor(train, val, conditional_gan=1, vocab_size=V, adv_eval_batch_size=4, max_seq_len=10)
    real = inst._beam_decode

    def decode(what, beam_size, max_caption_len=None, batch_size=None):
        k = 0
        for ids, lengths, caps in real(what, beam_size, max_caption_len, batch_size):
            rows = []
            for group in caps:
                c = list(group[0])
                if k % 3 == 1:
                    c[len(c) // 2] = 4 + (c[len(c) // 2] + 7) % (V - 4)          # one token replaced
                if k % 3 == 2:
                    c = c[1:] + c[:1]                                            # rotated: the order changes, the tokens stay
                rows.append([1] + c + [2])
                k += 1
            out = torch.zeros(len(rows), ids.shape[1], dtype=torch.int64)
            for i, r in enumerate(rows):
                out[i, :len(r)] = torch.tensor(r)
            yield out.to(ids.device), torch.tensor([len(r) for r in rows], dtype=lengths.dtype, device=ids.device), caps

    inst._beam_decode = decode
    got = inst.evaluate_metrics("val", beam_size=2)
    assert 0.05 < got["bleu4"] < 0.95 and got["bleu1"] > got["bleu2"] > got["bleu3"] > got["bleu4"]
    assert got["bleu4"] == pytest.approx(inst.evaluate("val", beam_size=2), rel=1e-6)
    assert got["cider_d"] == inst.evaluate_cider("val", beam_size=2) and got["cider_d"] > 0
    cands, refs = [], []
    for ids, lengths, caps in decode("val", 2):
        ids, lengths = ids.cpu(), lengths.cpu()
        cands += [ids[b, :int(lengths[b])].tolist() for b in range(len(caps))]
        refs += caps
    want = float(np.mean([O.rouge_l(c, r) for c, r in zip(cands, refs)]))
    assert 0.5 < want < 1.0 and got["rouge_l"] == pytest.approx(want, rel=1e-5, abs=1e-6)
    total = [sum(col) for col in zip(*(O.stats(c, r) for c, r in zip(cands, refs)))]
    assert [got[f"bleu{n}"] for n in (1, 2, 3, 4)] == pytest.approx(O.corpus_bleu(total), rel=1e-12)


def _corpus(rng, B, V, max_refs=4, max_len=7):
    return [[[rng.randrange(3, V) for _ in range(rng.randrange(1, max_len + 1))] for _ in range(rng.randrange(1, max_refs + 1))]
            for _ in range(B)]


def _scst_step(weights, baseline="greedy"):
    """One SCST step (no update) with the mixed reward of ``weights`` and a fixed draw; returns (out, corpus, df_corpus, B, n)."""
    from gan_image_captioning_amd.cider import CiderD, RefBatch
    from gan_image_captioning_amd.metrics import OverlapScorer, RewardMix
    from gan_image_captioning_amd.scst import SCSTStep
    torch.manual_seed(5)
    B, n, L, V = 6, 3, 9, 64
    inst, args = _instructor(decoder="lstm", conditional_gan=1, vocab_size=V)
    dev = args.device
    rng = random.Random(7)
    corpus = _corpus(rng, B, V)
    df_corpus = corpus + _corpus(rng, 10, V)
    mix = RewardMix(CiderD(df_corpus, V, dev) if weights[0] else None, OverlapScorer(V, dev), *weights)
    step = SCSTStep(inst, mix, n, baseline)
    images = torch.randn(B, 3, 32, 32, device=dev)
    noise = torch.rand(L, B * n, V, generator=torch.Generator().manual_seed(11)).to(dev)
    inst.gen.train()
    out = step(images, RefBatch.pack(corpus).to(dev), L, opt_step=False, noise_u=noise)
    torch.cuda.synchronize()
    return out, corpus, df_corpus, B, n


def _sampled(out, B, n):
    ids, lengths = out["ids"].cpu(), out["lengths"].cpu()
    return [ids[b, j, :int(lengths[b, j])].tolist() for b in range(B) for j in range(n)]


def test_scst_rewards_with_rouge_alone_are_the_oracles_rouge():
    out, corpus, _, B, n = _scst_step((0.0, 0.0, 1.0))
    cands = _sampled(out, B, n)
    want = np.array([O.rouge_l(c, corpus[i // n]) for i, c in enumerate(cands)]).reshape(B, n)
    np.testing.assert_allclose(out["rewards"].cpu().double().numpy(), want, rtol=1e-5, atol=1e-5)
    assert want.max() > 0


def test_scst_rewards_with_mixed_weights_are_the_weighted_sum_of_the_oracles():
    out, corpus, df_corpus, B, n = _scst_step((1.0, 0.5, 0.5), baseline="mean")
    cands = _sampled(out, B, n)
    per = [corpus[i // n] for i in range(B * n)]
    cider = np.array(CO.corpus_scores(cands, per, df_corpus))
    sb = np.array([O.sbleu(c, r) for c, r in zip(cands, per)])
    rl = np.array([O.rouge_l(c, r) for c, r in zip(cands, per)])
    want = (1.0 * cider + 0.5 * sb + 0.5 * rl).reshape(B, n)
    np.testing.assert_allclose(out["rewards"].cpu().double().numpy(), want, rtol=1e-5, atol=1e-5)
    base = (want.sum(1, keepdims=True) - want) / (n - 1)
    np.testing.assert_allclose(out["baselines"].cpu().double().numpy(), base, rtol=1e-5, atol=1e-5)
    assert sb.max() > 0 and rl.max() > 0


def test_default_weights_step_is_bit_identical_to_a_bare_cider_step():
    """With the default weights training.py hands SCSTStep a plain CiderD: loss, rewards and the updated generator arena have the bits
    of a step driven by a CiderD built by hand (deterministic mode, so that two steps from the same state can be compared at all)."""
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.cider import CiderD, RefBatch
    from gan_image_captioning_amd.scst import SCSTStep
    from gan_image_captioning_amd.training import scst_reward_scorer
    B, n, L, V = 6, 3, 9, 64
    rng = random.Random(7)
    corpus = _corpus(rng, B, V)
    df_corpus = corpus + _corpus(rng, 10, V)
    noise = torch.rand(L, B * n, V, generator=torch.Generator().manual_seed(11))

    def run(make_scorer):
        torch.manual_seed(5)
        inst, args = _instructor(decoder="lstm", conditional_gan=0, vocab_size=V)
        step = SCSTStep(inst, make_scorer(args), n, "greedy", lr=1e-3)
        inst.gen.train()
        out = step(None, RefBatch.pack(corpus).to(args.device), L, noise_u=noise.to(args.device))
        torch.cuda.synchronize()
        return out["loss"].clone(), out["rewards"].clone(), inst.gen_arena.flat.clone()

    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        got = run(lambda args: scst_reward_scorer(args, df_corpus))
        want = run(lambda args: CiderD(df_corpus, V, args.device))
    finally:
        engine.set_deterministic(was)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert float(got[1].abs().max()) > 0
