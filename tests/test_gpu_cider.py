"""gic_cider_d (csrc/cider.hip) against the float64 CPU oracle (tests/cider_oracle.py) on random corpora: vocabulary sizes up to the
15-bit limit, caption lengths 0..64, 1..32 references per image, repeated tokens and all-special candidates; bit-identical repeats in and
out of deterministic mode; the documented limits refused before any launch."""
import random

import numpy as np
import pytest
import torch

from tests import cider_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _caption(rng, V, n, repeat=False):
    if repeat:                                   # a few distinct tokens repeated: counts > 1 and n-grams that recur
        pool = [rng.randrange(3, V) for _ in range(3)]
        return [rng.choice(pool) for _ in range(n)]
    return [rng.randrange(0, V) for _ in range(n)]       # specials included: the scorer drops them


def _problem(seed, V, images, max_refs, max_len=64, n_per_image=3):
    rng = random.Random(seed)
    corpus, cands, cimg = [], [], []
    for b in range(images):
        R = rng.randrange(1, max_refs + 1) if b else max_refs
        refs = [_caption(rng, V, rng.randrange(0, max_len + 1), repeat=rng.random() < 0.2) for _ in range(R)]
        corpus.append(refs)
        for j in range(n_per_image):
            kind = rng.random()
            if kind < 0.15:
                c = list(rng.choice(refs))                                   # an exact reference
            elif kind < 0.3 and any(refs):
                src = rng.choice([r for r in refs if r] or [[4]])
                c = src[:rng.randrange(0, len(src) + 1)] + _caption(rng, V, rng.randrange(0, 8))   # a prefix plus noise
            elif kind < 0.4:
                c = [rng.choice((0, 1, 2)) for _ in range(rng.randrange(0, 10))]          # specials only
            else:
                c = _caption(rng, V, rng.randrange(0, max_len + 1), repeat=rng.random() < 0.3)
            cands.append(c[:max_len])
            cimg.append(b)
    if images > 1:
        cands.append([])                                                     # an empty candidate
        cimg.append(images - 1)
        cands.append(list(range(3, 3 + max_len)) if V > 3 + max_len else [5] * max_len)    # exactly at the length limit
        cimg.append(0)
    return corpus, cands, cimg


def _score(corpus, cands, cimg, V, dev, df_corpus=None):
    from gan_image_captioning_amd.cider import CiderD, RefBatch
    sc = CiderD(df_corpus if df_corpus is not None else corpus, V, dev)
    refs = RefBatch.pack(corpus).to(dev)
    Lc = max([len(c) for c in cands] + [1])
    ids = torch.zeros(len(cands), Lc, dtype=torch.int64)
    for i, c in enumerate(cands):
        ids[i, :len(c)] = torch.tensor(c, dtype=torch.int64)
    lens = torch.tensor([len(c) for c in cands], dtype=torch.int32)
    return sc, sc.score(ids.to(dev), lens.to(dev), refs, cand_img=torch.tensor(cimg, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("V,images,max_refs", [(50, 24, 5), (10000, 40, 32), (32768, 16, 7), (8, 12, 3)])
def test_kernel_matches_the_oracle(dev, V, images, max_refs):
    corpus, cands, cimg = _problem(V + images, V, images, max_refs)
    _, got = _score(corpus, cands, cimg, V, dev)
    want = O.corpus_scores(cands, [corpus[b] for b in cimg], corpus)
    got = got.cpu().double().numpy()
    np.testing.assert_allclose(got, np.array(want), rtol=1e-5, atol=1e-5)
    assert max(want) > 1.0                      # the problem has real matches, not only zeros


def test_df_from_another_corpus_and_unseen_ngrams(dev):
    """Rewards take df from the training split, evaluation from the evaluated split: n-grams outside the table get idf log N."""
    V = 300
    corpus, cands, cimg = _problem(5, V, 10, 5)
    df_corpus, _, _ = _problem(6, V, 30, 5)
    _, got = _score(corpus, cands, cimg, V, dev, df_corpus=df_corpus)
    want = O.corpus_scores(cands, [corpus[b] for b in cimg], df_corpus)
    np.testing.assert_allclose(got.cpu().double().numpy(), np.array(want), rtol=1e-5, atol=1e-5)


def test_repeat_calls_and_deterministic_mode_give_the_same_bits(dev):
    from gan_image_captioning_amd import engine
    corpus, cands, cimg = _problem(11, 10000, 64, 5)
    _, a = _score(corpus, cands, cimg, 10000, dev)
    _, b = _score(corpus, cands, cimg, 10000, dev)
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        _, c = _score(corpus, cands, cimg, 10000, dev)
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_image_grouped_batch_form(dev):
    """score() on [B, n, L] candidates (n per image, image-major) equals the flat form."""
    from gan_image_captioning_amd.cider import CiderD, RefBatch
    rng = random.Random(3)
    V, B, n, L = 100, 6, 4, 16
    corpus = [[_caption(rng, V, rng.randrange(1, L)) for _ in range(5)] for _ in range(B)]
    ids = torch.randint(0, V, (B, n, L))
    lens = torch.randint(0, L + 1, (B, n), dtype=torch.int32)
    sc = CiderD(corpus, V, dev)
    got = sc.score(ids.to(dev), lens.to(dev), RefBatch.pack(corpus).to(dev))
    assert got.shape == (B, n)
    want = O.corpus_scores([ids[b, j, :int(lens[b, j])].tolist() for b in range(B) for j in range(n)],
                           [corpus[b] for b in range(B) for _ in range(n)], corpus)
    np.testing.assert_allclose(got.cpu().double().numpy().reshape(-1), np.array(want), rtol=1e-5, atol=1e-5)


def test_limits_are_refused_before_any_launch(dev):
    from gan_image_captioning_amd import _lib, engine
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    keys, idf = z(1, dt=torch.int64), z(1, dt=torch.float32)
    base = dict(cand_ids=z(2, 8, dt=torch.int64), cand_len=z(2), cand_img=z(2), ref_ids=z(2, 8, dt=torch.int64), ref_len=z(2),
                ref_off=torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), max_refs=1, keys=keys, idf=idf, log_n=1.0, V=100)
    out = engine.cider_d(**base)
    torch.cuda.synchronize()
    assert out.shape == (2,)
    for kw in ({"V": 32769}, {"cand_ids": z(2, 65, dt=torch.int64)}, {"ref_ids": z(2, 65, dt=torch.int64)}, {"max_refs": 33}):
        with pytest.raises(NotImplementedError, match="status -2"):
            engine.cider_d(**dict(base, **kw))
    with pytest.raises(ValueError):
        engine.cider_d(**dict(base, log_n=float("nan")))
    assert _lib.CIDER_MAX_LEN == 64 and _lib.CIDER_MAX_REFS == 32 and _lib.CIDER_MAX_VOCAB == 32768
