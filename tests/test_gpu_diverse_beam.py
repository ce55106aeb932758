"""Diverse beam search on the GPU (gic_decoder_diverse_beam_search, gic_attn_diverse_beam_search, the decoders' and Generator.caption's
beam_groups / diversity, GANInstructor.evaluate_diverse_beam) against the float64 oracle (tests/diverse_beam_oracle.py), plain beam
search, teacher-forced rescoring and itself."""
import math

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import diverse_beam_oracle as DO
from tests.golden_io import Golden, initial_params
from tests.gpu_util import dec_params

pytestmark = pytest.mark.gpu


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


def _golden_problem(case, seed, dev, eos_bias=1.5):
    g = Golden(case)
    gp, m = initial_params(g)[0], g.meta
    params = dec_params(gp, dev)
    params[-1] = params[-1].clone()
    params[-1][2] += eos_bias
    feats = torch.randn(m["B"], m["E"], generator=torch.Generator().manual_seed(seed)).to(dev) * 0.5
    return m, params, feats


def _attn_problem(shape, seed, dev, eos_bias=0.0, out_scale=1.0, scale=6.0):
    B, L, V, E, H, C, P, A = shape
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=scale)
    params[5] = params[5] * out_scale
    params[6] = params[6].clone()
    params[6][2] += eos_bias
    return [p.to(dev) for p in params], feats.to(dev), fmap.to(dev), params, feats, fmap


def _compare(got, want, margins, k, G, alphas=None, ralphas=None):
    """Images whose selections (penalty included) are decided by >= 1e-4 at every step: the same beams in every group, in the same
    order where the group orders are decided by >= 1e-4 too (else as sets per group).  Returns the number of images compared."""
    ids, sc, ln = got[0].cpu(), got[1].cpu().double(), got[2].cpu().long()
    rid, rsc, rlen = want
    kg = k // G
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    for b in ok:
        for g in range(G):
            s = slice(g * kg, (g + 1) * kg)
            if margins[b][1] >= 1e-4:
                assert torch.equal(ids[b, s], rid[b, s]), (b, g)
                assert torch.equal(ln[b, s], rlen[b, s]), (b, g)
                torch.testing.assert_close(sc[b, s], rsc[b, s], rtol=1e-4, atol=1e-5)
            else:
                assert sorted(zip(ids[b, s].tolist(), ln[b, s].tolist())) == sorted(zip(rid[b, s].tolist(), rlen[b, s].tolist())), (b, g)
                torch.testing.assert_close(sc[b, s].sort().values, rsc[b, s].sort().values, rtol=1e-4, atol=1e-5)
            if alphas is not None:
                for j in range(g * kg, (g + 1) * kg):
                    r = next(i for i in range(g * kg, (g + 1) * kg) if torch.equal(rid[b, i], ids[b, j]))
                    torch.testing.assert_close(alphas[b, j].cpu().double(), ralphas[b, r], rtol=1e-4, atol=1e-6)
    return len(ok)


def _group_order(scores, lengths, G, alpha):
    """Within each group the returned beams are sorted by score / length**alpha."""
    k = scores.shape[1]
    kg = k // G
    norm = scores.cpu().double() / lengths.cpu().double() ** alpha
    for g in range(G):
        n = norm[:, g * kg:(g + 1) * kg]
        assert (n[:, :-1] >= n[:, 1:] - 1e-6 * n.abs()[:, 1:]).all()


LSTM_CASES = [(2, 2, 0.5, 0.0), (4, 2, 1.0, 0.7), (4, 4, 0.3, 0.0), (6, 3, 2.0, 0.7), (6, 2, 0.8, 0.0), (8, 4, 0.5, 0.7),
              (8, 2, 3.0, 0.0)]


@pytest.mark.parametrize("k,G,lam,alpha", LSTM_CASES, ids=[f"k{c[0]}g{c[1]}l{c[2]}a{c[3]}" for c in LSTM_CASES])
@pytest.mark.parametrize("case", ["tiny_scaled", "cfg1"], ids=["generic", "fused"])
def test_lstm_f32_matches_oracle(dev, case, k, G, lam, alpha):
    m, params, feats = _golden_problem(case, 10 * k + G, dev)
    eng = _eng(m["V"], m["E"], m["H"], m["NL"], 0)
    assert eng.beam_fused(m["B"], k) == (case == "cfg1")
    L = 12
    got = eng.diverse_beam_search(params, feats, L, k, G, lam, length_penalty=alpha)
    torch.cuda.synchronize()
    assert got[0].shape == (m["B"], k, L)
    _group_order(got[1], got[2], G, alpha)
    rid, rsc, rlen, margins = DO.diverse_beam_search([p.cpu() for p in params], feats.cpu(), k, G, lam, L, length_penalty=alpha)
    n = _compare(got, (rid, rsc, rlen), margins, k, G)
    # (at least 3/4 of the batch: the oracle gives every image but for 3 of 4 at generic (8, 4) and 6 of 8 at fused (6, 2), (8, 4))
    assert 4 * n >= 3 * m["B"], f"{n} of {m['B']} images with a clear selection to compare: margins {margins}"


ATTN_CASES = [(2, 2, 1.0, 0.0), (4, 2, 0.5, 0.7), (6, 3, 2.0, 0.0), (8, 8, 0.7, 0.7), (8, 4, 1.5, 0.0)]


@pytest.mark.parametrize("k,G,lam,alpha", ATTN_CASES, ids=[f"k{c[0]}g{c[1]}l{c[2]}a{c[3]}" for c in ATTN_CASES])
def test_attn_f32_matches_oracle(dev, k, G, lam, alpha):
    shape = (6, 10, 64, 16, 32, 40, 49, 24)
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _attn_problem(shape, 200 + k + G, dev, eos_bias=1.5)
    eng = _aeng(*shape[2:], 0)
    L = shape[1]
    got = eng.diverse_beam_search(params, feats, fmap, L, k, G, lam, length_penalty=alpha, want_alphas=True)
    torch.cuda.synchronize()
    _group_order(got[1], got[2], G, alpha)
    rid, rsc, rlen, ral, margins = DO.attn_diverse_beam_search(p_cpu, f_cpu, m_cpu, k, G, lam, L, length_penalty=alpha)
    n = _compare(got, (rid, rsc, rlen), margins, k, G, got[3], ral)
    assert 4 * n >= 3 * shape[0], f"{n} of {shape[0]} images with a clear selection to compare: margins {margins}"


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 10, 64, 32, 512, 1), (64, 20, 10000, 512, 512, 1), (16, 8, 1001, 64, 64, 2)],
                         ids=["cfg1", "cfg2", "generic"])
def test_one_group_is_beam_search_bit_for_bit(dev, dt, shape):
    B, L, V, E, H, NL = shape
    eng = _eng(V, E, H, NL, dt)
    assert eng.beam_fused(B, 4) == (V != 1001)
    params = [t.to(dev) for t in BO.random_params(V, E, H, NL, seed=B + V, scale=3.0)]
    params[-1][2] += 1.0
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(4)).to(dev)
    for k, lam, alpha in ((4, 0.0, 0.0), (4, 2.5, 0.7), (7, 1.0, 0.0)):
        want = eng.beam_search(params, feats, L, k, length_penalty=alpha)
        got = eng.diverse_beam_search(params, feats, L, k, 1, lam, length_penalty=alpha)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), (k, lam, alpha)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_attn_one_group_is_beam_search_bit_for_bit(dev, dt):
    shape = (6, 10, 64, 16, 32, 40, 49, 24)
    params, feats, fmap, *_ = _attn_problem(shape, 7, dev, eos_bias=1.0)
    eng = _aeng(*shape[2:], dt)
    for k, lam, alpha in ((3, 0.0, 0.0), (5, 2.0, 0.7)):
        want = eng.beam_search(params, feats, fmap, shape[1], k, length_penalty=alpha, want_alphas=True)
        got = eng.diverse_beam_search(params, feats, fmap, shape[1], k, 1, lam, length_penalty=alpha, want_alphas=True)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), (k, lam, alpha)


def test_zero_penalty_one_beam_per_group_is_beam_1(dev):
    m, params, feats = _golden_problem("cfg1", 3, dev)
    eng = _eng(m["V"], m["E"], m["H"], m["NL"], 0)
    one = eng.beam_search(params, feats, 12, 1)
    shape = (5, 10, 64, 16, 32, 40, 9, 24)
    ap, af, am, *_ = _attn_problem(shape, 11, dev, eos_bias=1.0)
    aeng = _aeng(*shape[2:], 0)
    aone = aeng.beam_search(ap, af, am, shape[1], 1)
    for k in (2, 4, 8):
        ids, scores, lengths = eng.diverse_beam_search(params, feats, 12, k, k, 0.0)
        aids, ascores, alengths = aeng.diverse_beam_search(ap, af, am, shape[1], k, k, 0.0)
        torch.cuda.synchronize()
        for j in range(k):
            assert torch.equal(ids[:, j], one[0][:, 0]) and torch.equal(lengths[:, j], one[2][:, 0]), (k, j)
            assert torch.equal(aids[:, j], aone[0][:, 0]) and torch.equal(alengths[:, j], aone[2][:, 0]), (k, j)
            torch.testing.assert_close(scores[:, j], one[1][:, 0], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(ascores[:, j], aone[1][:, 0], rtol=1e-5, atol=1e-6)


def test_large_penalty_makes_first_tokens_distinct(dev):
    """lambda = 1e4, far above any logit gap: with one beam per group every group starts with a token no earlier group took."""
    m, params, feats = _golden_problem("cfg1", 5, dev)
    eng = _eng(m["V"], m["E"], m["H"], m["NL"], 1)
    shape = (4, 8, 64, 16, 32, 40, 9, 24)
    ap, af, am, *_ = _attn_problem(shape, 12, dev)
    aeng = _aeng(*shape[2:], 0)
    for k in (4, 8):
        ids = eng.diverse_beam_search(params, feats, 10, k, k, 1e4)[0].cpu()
        aids = aeng.diverse_beam_search(ap, af, am, shape[1], k, k, 1e4)[0].cpu()
        for t in (ids, aids):
            for b in range(t.shape[0]):
                assert len(set(t[b, :, 0].tolist())) == k, (k, t[b, :, 0])


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
    B, L, V, E, H, k, G = 16, 20, 10000, 512, 512, 6, 3
    dec = _decoder(dev, V, E, H, L, dtype)
    feats = torch.randn(B, E, device=dev)
    ids, scores, lengths = dec.beam_search(feats, beam_size=k, return_beams=True, beam_groups=G, diversity=0.7)
    torch.cuda.synchronize()
    assert ids.shape == (B, k, L)
    pos = torch.arange(L, device=dev)[None, None]
    assert (ids[pos.expand_as(ids) >= lengths[..., None].long()] == 0).all()
    tol = (1e-4, 1e-4) if dtype == "fp32" else (1e-2, 1e-2)
    for j in range(k):
        row, n = ids[:, j], lengths[:, j].long()
        pred, _ = dec(feats, row[:, :-1].contiguous(), n.cpu(), pretrain=True)
        logp = torch.log_softmax(pred.float(), dim=-1)
        lp = logp.gather(2, row[:, :pred.shape[1], None])[..., 0]
        lp = torch.where(pos[0, :, :pred.shape[1]] < n[:, None], lp, torch.zeros_like(lp))
        torch.testing.assert_close(lp.sum(1), scores[:, j], rtol=tol[0], atol=tol[1])


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_attn_scores_equal_teacher_forced_rescoring(dev, dt):
    shape = (8, 12, 10000, 512, 512, 2048, 49, 512)
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _attn_problem(shape, 4, dev, eos_bias=3.0, out_scale=20.0, scale=1.0)
    eng = _aeng(*shape[2:], dt)
    ids, scores, lengths = eng.diverse_beam_search(params, feats, fmap, shape[1], 4, 2, 1.0)
    torch.cuda.synchronize()
    ref = AO.sequence_logprob(p_cpu, f_cpu, m_cpu, ids.cpu(), lengths.cpu())
    got = scores.cpu().double()
    tol = (1e-4 * ref.abs() + 1e-4) if dt == 0 else (2e-2 * ref.abs() + 0.05 * lengths.cpu().double())
    assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()


def test_bits_and_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    B, L, V, E, H = 64, 20, 10000, 512, 512
    eng = _eng(V, E, H, 1, 1)
    params = [t.to(dev) for t in BO.random_params(V, E, H, 1, seed=3, scale=3.0)]
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(2)).to(dev)
    shape = (8, 12, 10000, 512, 512, 2048, 49, 512)
    ap, af, am, *_ = _attn_problem(shape, 9, dev, eos_bias=2.0, out_scale=20.0, scale=1.0)
    aeng = _aeng(*shape[2:], 1)

    def both():
        return (eng.diverse_beam_search(params, feats, L, 8, 4, 0.5),
                aeng.diverse_beam_search(ap, af, am, shape[1], 6, 3, 0.5, want_alphas=True))

    runs = [both(), both()]
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        runs.append(both())
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            for a, b in zip(x, y):
                assert torch.equal(a, b)


def test_early_stop(dev):
    """An <E>-biased b_out: every beam of every group ends early, the search stops, PAD behind, and the result is the oracle's."""
    m, params, feats = _golden_problem("tiny_scaled", 6, dev, eos_bias=4.0)
    eng = _eng(m["V"], m["E"], m["H"], m["NL"], 0)
    shape = (4, 12, 64, 16, 32, 40, 9, 24)
    ap, af, am, p_cpu, f_cpu, m_cpu = _attn_problem(shape, 5, dev, eos_bias=4.0)
    aeng = _aeng(*shape[2:], 0)
    for k, G in ((4, 2), (6, 6)):
        got = eng.diverse_beam_search(params, feats, 12, k, G, 0.5)
        agot = aeng.diverse_beam_search(ap, af, am, shape[1], k, G, 0.5, want_alphas=True)
        torch.cuda.synchronize()
        want = DO.diverse_beam_search([p.cpu() for p in params], feats.cpu(), k, G, 0.5, 12)
        awant = DO.attn_diverse_beam_search(p_cpu, f_cpu, m_cpu, k, G, 0.5, shape[1])
        assert 4 * _compare(got, want[:3], want[3], k, G) >= 3 * m["B"]
        assert 4 * _compare(agot, awant[:3], awant[4], k, G, agot[3], awant[3]) >= 3 * shape[0]
        for ids, lengths in ((got[0], got[2]), (agot[0], agot[2])):
            assert int(lengths.max()) < ids.shape[2], lengths
            pos = torch.arange(ids.shape[2], device=dev)[None, None]
            assert (ids[pos.expand_as(ids) >= lengths[..., None].long()] == 0).all()


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
def test_generator_caption(dev, kind):
    from gan_image_captioning_amd.generator import Generator
    kw = {"lstm": {}, "lstm_uncond": dict(conditional_gan=0), "attention": _ATTN}[kind]
    torch.manual_seed(4)
    gen = Generator(_gen_args(**kw)).to(dev)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    plain = gen.caption(images, beam_size=4, return_beams=True)
    one = gen.caption(images, beam_size=4, return_beams=True, beam_groups=1, diversity=1.5)
    beams = gen.caption(images, beam_size=4, return_beams=True, beam_groups=2, diversity=0.5)
    best = gen.caption(images, beam_size=4, beam_groups=2, diversity=0.5)
    torch.cuda.synchronize()
    for a, b in zip(plain, one):
        assert torch.equal(a, b)
    assert [t.shape for t in beams] == [(4, 4, 8), (4, 4), (4, 4)]
    assert torch.equal(best[0], beams[0][:, 0]) and torch.equal(best[1], beams[1][:, 0])
    with torch.no_grad():
        if kind == "attention":
            feats, fmap = gen.encoder.forward_with_map(images)
            direct = gen.decoder.beam_search(feats, fmap, beam_size=4, return_beams=True, beam_groups=2, diversity=0.5,
                                             return_alphas=True)
            alphas = gen.caption(images, beam_size=4, return_beams=True, return_alphas=True, beam_groups=2, diversity=0.5)[3]
            assert torch.equal(direct[3], alphas)
        elif kind == "lstm":
            direct = gen.decoder.beam_search(gen.encoder(images), beam_size=4, return_beams=True, beam_groups=2, diversity=0.5)
        else:
            feats = gen.decoder.embed(torch.ones(4, dtype=torch.long, device=dev))
            direct = gen.decoder.beam_search(feats, beam_size=4, return_beams=True, beam_groups=2, diversity=0.5)
    for a, b in zip(beams, direct):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_evaluate_diverse_beam(dev, kind):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    kw = _ATTN if kind == "attention" else {}
    args = _gen_args(eval_diverse_beam_size=4, **kw)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    out = inst.evaluate_diverse_beam("val", beam_size=4, groups=2, diversity=0.5)
    assert set(out) == {"bleu4", "mbleu4", "distinct1", "distinct2", "vocab"}
    for k in ("bleu4", "mbleu4", "distinct1", "distinct2"):
        assert math.isfinite(out[k]) and 0.0 <= out[k] <= 1.0, (k, out[k])
    assert isinstance(out["vocab"], int) and 0 <= out["vocab"] <= 64
    assert [t for t, _ in seen] == ["BLEU4DBS_val", "mBLEU4DBS_val", "Distinct1DBS_val", "Distinct2DBS_val", "VocabDBS_val"]
    assert out == inst.evaluate_diverse_beam("val", beam_size=4, groups=2, diversity=0.5)
