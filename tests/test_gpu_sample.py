"""Caption sampling on the GPU (gic_sample_logits, gic_decoder_sample_captions, gic_attn_sample_captions and the Python layers
above them) against the CPU oracle (tests/sample_oracle.py), the roll-out, beam search and teacher-forced rescoring."""
import math

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import sample_oracle as SO

pytestmark = pytest.mark.gpu

CFG4 = (32, 20, 10000, 512, 512, 2048, 49, 512)          # B, L, V, E, H, C, P, A: cfg4's per-GPU attention shape


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _eng(V, E, H, NL, dt):
    from gan_image_captioning_amd import engine
    return engine.DecoderEngine(V, E, H, NL, dt)


def _aeng(V, E, H, C, P, A, dt):
    from gan_image_captioning_amd import engine
    return engine.AttnDecoderEngine(V, E, H, C, P, A, dt)


def _mask_after_eos(ids, eos=2, pad=0):
    out = ids.clone()
    for b in range(ids.shape[0]):
        hit = (ids[b] == eos).nonzero()
        if len(hit):
            out[b, int(hit[0]) + 1:] = pad
    return out


def _check_rows(ids, lengths, L, eos=2, pad=0):
    """PAD after each row's length, <E> at its last position unless it ran L steps, no earlier <E>."""
    ids, lengths = ids.cpu(), lengths.cpu().long()
    pos = torch.arange(L)[None, None]
    assert (ids[pos.expand_as(ids) >= lengths[..., None]] == pad).all()
    last = ids.gather(2, (lengths - 1).clamp(min=0)[..., None])[..., 0]
    assert ((last == eos) | (lengths == L)).all()
    early = (ids == eos) & (pos < (lengths[..., None] - 1))
    assert not early.any()


# ---------------------------------------------------------------- gic_sample_logits
def _crafted(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(rows, V, generator=g) * 2.0
    for r in range(0, rows, 4):                                 # ties: a block of equal values around the 5th / 50th largest
        srt = torch.sort(l[r], descending=True)
        k = 5 if r % 8 == 0 else min(50, V - 1)
        l[r, srt.indices[k - 2:k + 2]] = srt.values[k - 1]
    for r in range(1, rows, 4):                                 # coarse values: ties everywhere
        l[r] = torch.round(l[r])
    return l


@pytest.mark.parametrize("V", [50, 9999, 10000, 20011])
@pytest.mark.parametrize("opts", [(0, 1.0, 1.0), (5, 1.0, 1.0), (50, 1.0, 0.7), (0, 0.9, 1.0), (50, 0.9, 1.3), (0, 0.5, 0.6), (1, 1.0, 1.0)],
                         ids=["off", "k5", "k50_t07", "p09", "k50_p09_t13", "p05_t06", "k1"])
def test_sample_logits_matches_oracle(dev, V, opts):
    from gan_image_captioning_amd import engine
    top_k, top_p, tau = opts
    top_k = min(top_k, V)
    rows = 24
    l = _crafted(rows, V, V + top_k)
    u = torch.rand(rows, V, generator=torch.Generator().manual_seed(7))
    pad = torch.zeros(rows, V + 3)                              # a leading dimension beyond V
    pad[:, :V] = l
    ids, logp, kept = engine.sample_logits(pad.to(dev)[:, :V], top_k, top_p, tau, noise_u=u.to(dev))
    torch.cuda.synchronize()
    checked = 0
    for r in range(rows):
        tok, lp, nk, dm, pm = SO.draw(l[r], u[r], top_k, top_p, tau)
        assert float(logp[r]) == pytest.approx(float(l[r].double()[int(ids[r])] - torch.logsumexp(l[r].double(), 0)), abs=1e-5)
        if pm > 1e-5:
            assert int(kept[r]) == nk, r
            if dm > 1e-5:
                assert int(ids[r]) == tok, r
                assert float(logp[r]) == pytest.approx(lp, abs=1e-5)
                checked += 1
    # at V = 20011 with top_p = 0.9 the nucleus boundary falls between tokens of probability ~1e-5, so most rows are near-ties there
    assert checked >= (rows // 2 if V <= 10000 or top_p == 1.0 else 4)


@pytest.mark.parametrize("opts", [(0, 1.0, 1.0), (10, 1.0, 1.0), (0, 0.8, 1.0), (20, 0.7, 0.5), (0, 0.95, 2.0)])
def test_philox_draws_follow_the_truncated_distribution(dev, opts):
    from gan_image_captioning_amd import engine
    top_k, top_p, tau = opts
    V, rows = 64, 65536
    l = torch.randn(V, generator=torch.Generator().manual_seed(1)) * 1.5
    keep, _ = SO.truncate(l, top_k, top_p, tau)
    p = torch.where(keep, torch.softmax(l.double() / tau, 0), torch.zeros(V, dtype=torch.float64))
    p = p / p.sum()
    ids, _, kept = engine.sample_logits(l.to(dev).expand(rows, V).contiguous(), top_k, top_p, tau, seed=1234, stream_id=3)
    counts = torch.bincount(ids.cpu(), minlength=V).double()
    assert (counts[~keep] == 0).all()
    assert (kept.cpu() == int(keep.sum())).all()
    sd = torch.sqrt(rows * p * (1 - p))
    assert ((counts - rows * p).abs() <= 5 * sd + 1e-9).all(), ((counts - rows * p).abs() / sd.clamp(min=1e-9)).max()


# ---------------------------------------------------------------- the LSTM decoder
LSTM_SHAPES = {"cfg1": (8, 10, 64, 32, 512, 1), "generic_v50": (6, 8, 50, 8, 16, 2), "generic_rows": (130, 6, 52, 8, 16, 1)}


def _lstm_problem(shape, seed, dev, eos_bias=0.0):
    B, L, V, E, H, NL = shape
    params = BO.random_params(V, E, H, NL, seed=seed, scale=3.0)
    params[-1] = params[-1].clone()
    params[-1][2] += eos_bias
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(seed + 1))
    return [p.to(dev) for p in params], feats.to(dev), params, feats


@pytest.mark.parametrize("case", list(LSTM_SHAPES))
@pytest.mark.parametrize("opts", [(0, 1.0, 1.0), (5, 1.0, 0.8), (0, 0.9, 1.0), (8, 0.8, 1.5)], ids=["off", "k5", "p09", "k8p08"])
def test_lstm_f32_matches_oracle(dev, case, opts):
    shape = LSTM_SHAPES[case]
    B, L, V, E, H, NL = shape
    n = 3 if case != "generic_rows" else 4                     # 130 * 4 = 520 rows: beyond the fused kernels' 512
    params, feats, p_cpu, f_cpu = _lstm_problem(shape, B + V, dev, eos_bias=1.0)
    eng = _eng(V, E, H, NL, 0)
    u = torch.rand(L, B * n, V, generator=torch.Generator().manual_seed(5))
    ids, scores, lengths = eng.sample_captions(params, feats, L, n, *opts, noise_u=u.to(dev))
    torch.cuda.synchronize()
    _check_rows(ids, lengths, L)
    rid, rsc, rlen, margin = SO.decode(p_cpu, f_cpu, n, L, u, *opts)
    ok = margin > 1e-5
    assert ok.float().mean() > 0.5, margin
    assert torch.equal(ids.cpu()[ok], rid[ok])
    assert torch.equal(lengths.cpu().long()[ok], rlen[ok])
    torch.testing.assert_close(scores.cpu().double()[ok], rsc[ok], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("case", ["cfg1", "generic_v50"])
def test_lstm_n1_equals_the_rollout(dev, case):
    B, L, V, E, H, NL = LSTM_SHAPES[case]
    params, feats, *_ = _lstm_problem(LSTM_SHAPES[case], 3 * B, dev)
    eng = _eng(V, E, H, NL, 0)
    u = torch.rand(L, B, V, generator=torch.Generator().manual_seed(9)).to(dev)
    _, ref, _ = eng.sample_fwd(params, feats, L, 1.0, pretrain=False, noise_u=u)
    ids, _, lengths = eng.sample_captions(params, feats, L, 1, noise_u=u)
    torch.cuda.synchronize()
    assert torch.equal(ids[:, 0].cpu(), _mask_after_eos(ref.cpu()))


@pytest.mark.parametrize("case", ["cfg1", "generic_v50", "generic_rows"])
def test_lstm_top_k_1_equals_beam_1(dev, case):
    B, L, V, E, H, NL = LSTM_SHAPES[case]
    if case == "generic_rows":
        B = 520                                                 # beam k = 1 over the same 520 rows
    params, feats, *_ = _lstm_problem((B, L, V, E, H, NL), 7 + B, dev, eos_bias=1.0)
    eng = _eng(V, E, H, NL, 0)
    ids, scores, lengths = eng.sample_captions(params, feats, L, 1, top_k=1, seed=5)
    bid, bsc, blen = eng.beam_search(params, feats, L, 1)
    torch.cuda.synchronize()
    assert eng.beam_fused(B, 1) == (case == "cfg1")
    assert torch.equal(ids, bid) and torch.equal(lengths, blen)
    torch.testing.assert_close(scores, bsc, rtol=1e-5, atol=1e-6)


def _decoder(dev, V, E, H, L, dtype, seed=11):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Decoder
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, gen_num_layers=1, compute_dtype=dtype, max_seq_len=L,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(seed)
    dec = Decoder(args).to(dev)
    with torch.no_grad():
        dec.linear.weight.mul_(8.0)
        dec.linear.bias[2] += 2.0
    return dec


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scores_equal_teacher_forced_rescoring(dev, dtype):
    B, L, V, E, H, n = 16, 20, 10000, 512, 512, 5
    dec = _decoder(dev, V, E, H, L, dtype)
    feats = torch.randn(B, E, device=dev)
    ids, scores, lengths = dec.sample_captions(feats, num_samples=n, top_k=50, top_p=0.95, seed=3)
    torch.cuda.synchronize()
    assert ids.shape == (B, n, L) and scores.shape == (B, n) and lengths.shape == (B, n)
    _check_rows(ids, lengths, L)
    tol = (1e-4, 1e-4) if dtype == "fp32" else (1e-2, 1e-2)
    for j in range(n):
        row, k = ids[:, j], lengths[:, j].long()
        pred, _ = dec(feats, row[:, :-1].contiguous(), k.cpu(), pretrain=True)
        logp = torch.log_softmax(pred.float(), dim=-1)
        tok = row[:, :pred.shape[1]]
        lp = logp.gather(2, tok[..., None])[..., 0]
        pos = torch.arange(pred.shape[1], device=dev)[None]
        lp = torch.where(pos < k[:, None], lp, torch.zeros_like(lp))
        torch.testing.assert_close(lp.sum(1), scores[:, j], rtol=tol[0], atol=tol[1])


def test_sequence_behaviour(dev):
    from gan_image_captioning_amd import engine
    B, L, V, E, H, n = 8, 30, 64, 32, 512, 8
    params, feats, *_ = _lstm_problem((B, L, V, E, H, 1), 21, dev, eos_bias=4.0)
    eng = _eng(V, E, H, 1, 0)
    a = eng.sample_captions(params, feats, L, n, seed=77)
    b = eng.sample_captions(params, feats, L, n, seed=77)
    c = eng.sample_captions(params, feats, L, n, seed=78)
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        d = eng.sample_captions(params, feats, L, n, seed=77)
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    ids, scores, lengths = a
    _check_rows(ids, lengths, L)
    assert int(lengths.max()) < L                               # every row finished: the decode stopped early, PAD behind
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a, d):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0])
    distinct = [len({tuple(ids[i, j].tolist()) for j in range(n)}) for i in range(B)]
    assert max(distinct) > 1, distinct                          # the samples of an image differ
    assert (scores <= 0).all()


def test_rows_are_independent_of_the_batch(dev):
    """Philox is keyed by (seed, t, row): the first image's samples do not change when the batch grows."""
    B, L, V, E, H, n = 6, 12, 64, 32, 512, 3
    params, feats, *_ = _lstm_problem((B, L, V, E, H, 1), 5, dev, eos_bias=0.5)
    eng = _eng(V, E, H, 1, 0)
    full = eng.sample_captions(params, feats, L, n, seed=9)
    part = eng.sample_captions(params, feats[:2].contiguous(), L, n, seed=9)
    torch.cuda.synchronize()
    assert torch.equal(full[0][:2], part[0][:2]) and torch.equal(full[2][:2], part[2][:2])


# ---------------------------------------------------------------- the attention decoder
def _attn_problem(shape, seed, dev, eos_bias=0.0, out_scale=1.0, scale=6.0):
    B, L, V, E, H, C, P, A = shape
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=scale)
    params[5] = params[5] * out_scale
    params[6] = params[6].clone()
    params[6][2] += eos_bias
    return [p.to(dev) for p in params], feats.to(dev), fmap.to(dev), params, feats, fmap


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 52, 8, 16, 24, 9, 16), CFG4], ids=["s1", "cfg4"])
def test_attn_top_k_1_equals_beam_1(dev, dt, shape):
    B, L = shape[:2]
    cfg4 = shape == CFG4
    params, feats, fmap, *_ = _attn_problem(shape, sum(shape), dev, eos_bias=1.0, out_scale=20.0 if cfg4 else 1.0, scale=1.0 if cfg4 else 6.0)
    eng = _aeng(*shape[2:], dt)
    ids, scores, lengths = eng.sample_captions(params, feats, fmap, L, 1, top_k=1, seed=2)
    bid, bsc, blen = eng.beam_search(params, feats, fmap, L, 1)
    torch.cuda.synchronize()
    assert torch.equal(ids, bid) and torch.equal(lengths, blen)
    torch.testing.assert_close(scores, bsc, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_attn_scores_equal_teacher_forced_rescoring(dev, dt):
    shape = (8, 12, 10000, 512, 512, 2048, 49, 512)
    B, L = shape[:2]
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _attn_problem(shape, 4, dev, eos_bias=3.0, out_scale=20.0, scale=1.0)
    eng = _aeng(*shape[2:], dt)
    ids, scores, lengths = eng.sample_captions(params, feats, fmap, L, 4, top_k=50, top_p=0.9, seed=8)
    torch.cuda.synchronize()
    _check_rows(ids, lengths, L)
    ref = AO.sequence_logprob(p_cpu, f_cpu, m_cpu, ids.cpu(), lengths.cpu())
    got = scores.cpu().double()
    tol = (1e-4 * ref.abs() + 1e-4) if dt == 0 else (2e-2 * ref.abs() + 0.05 * lengths.cpu().double())
    assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()


def test_attn_bits_and_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    shape = (6, 10, 64, 16, 32, 40, 9, 24)
    params, feats, fmap, *_ = _attn_problem(shape, 3, dev, eos_bias=1.0)
    eng = _aeng(*shape[2:], 0)
    runs = [eng.sample_captions(params, feats, fmap, shape[1], 5, top_p=0.9, seed=4) for _ in range(2)]
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        runs.append(eng.sample_captions(params, feats, fmap, shape[1], 5, top_p=0.9, seed=4))
    finally:
        engine.set_deterministic(was)
    other = eng.sample_captions(params, feats, fmap, shape[1], 5, top_p=0.9, seed=5)
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)
    assert not torch.equal(runs[0][0], other[0])
    _check_rows(runs[0][0], runs[0][2], shape[1])


# ---------------------------------------------------------------- end to end
def _gen_args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64,
                conditional_gan=1, max_seq_len=8, adv_eval_batch_size=4, num_workers=0, device="cuda", log_file=None, model_dir=None,
                save_dir=None)
    base.update(kw)
    return default_args(**base)


_ATTN = dict(decoder="attention", encoder_arch="resnet18", gen_embed_dim=16, gen_hidden_dim=32, attn_dim=24)


@pytest.mark.parametrize("kind", ["lstm", "lstm_uncond", "attention"])
def test_generator_sample_captions(dev, kind):
    from gan_image_captioning_amd.generator import Generator
    kw = {"lstm": {}, "lstm_uncond": dict(conditional_gan=0), "attention": _ATTN}[kind]
    torch.manual_seed(4)
    gen = Generator(_gen_args(**kw)).to(dev)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    ids, scores, lengths = gen.sample_captions(images, num_samples=3, top_k=10, top_p=0.9, seed=6)
    again = gen.sample_captions(images, num_samples=3, top_k=10, top_p=0.9, seed=6)
    torch.cuda.synchronize()
    assert ids.shape == (4, 3, 8) and scores.shape == (4, 3) and lengths.shape == (4, 3)
    for x, y in zip((ids, scores, lengths), again):
        assert torch.equal(x, y)
    _check_rows(ids, lengths, 8)
    with torch.no_grad():
        if kind == "attention":
            feats, fmap = gen.encoder.forward_with_map(images)
            direct = gen.decoder.sample_captions(feats, fmap, num_samples=3, top_k=10, top_p=0.9, seed=6)
        elif kind == "lstm":
            direct = gen.decoder.sample_captions(gen.encoder(images), num_samples=3, top_k=10, top_p=0.9, seed=6)
        else:
            feats = gen.decoder.embed(torch.ones(4, dtype=torch.long, device=dev))
            direct = gen.decoder.sample_captions(feats, num_samples=3, top_k=10, top_p=0.9, seed=6)
    assert torch.equal(direct[0], ids)


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_evaluate_diversity(dev, kind):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    kw = _ATTN if kind == "attention" else {}
    args = _gen_args(eval_num_samples=4, **kw)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    out = inst.evaluate_diversity("val", num_samples=4, top_p=0.95)
    assert set(out) == {"bleu4", "mbleu4", "distinct1", "distinct2", "vocab"}
    for k in ("bleu4", "mbleu4", "distinct1", "distinct2"):
        assert 0.0 <= out[k] <= 1.0, (k, out[k])
    assert isinstance(out["vocab"], int) and 0 <= out["vocab"] <= 64
    assert [t for t, _ in seen] == ["BLEU4S_val", "mBLEU4_val", "Distinct1_val", "Distinct2_val", "Vocab_val"]
    assert out == inst.evaluate_diversity("val", num_samples=4, top_p=0.95)
