"""Beam search with the attention decoder on the GPU (gic_attn_beam_search, AttnDecoder.beam_search, Generator.caption,
GANInstructor.evaluate) against the library's greedy attention roll-out and the float64 oracle (tests/attn_beam_oracle.py)."""
import pytest
import torch

from oracle import cpu_attention as CA
from tests import attn_beam_oracle as AO

pytestmark = pytest.mark.gpu

CFG4 = (32, 20, 10000, 512, 512, 2048, 49, 512)          # B, L, V, E, H, C, P, A: BASELINE config 4 per GPU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _engine(V, E, H, C, P, A, dt):
    from gan_image_captioning_amd import engine
    return engine.AttnDecoderEngine(V, E, H, C, P, A, dt)


def _problem(shape, seed, dev, eos_bias=0.0, out_scale=1.0, scale=6.0):
    B, L, V, E, H, C, P, A = shape
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=scale)
    params[5] = params[5] * out_scale
    params[6] = params[6].clone()
    params[6][2] += eos_bias
    return [p.to(dev) for p in params], feats.to(dev), fmap.to(dev), params, feats, fmap


def _mask_after_eos(ids, eos=2, pad=0):
    out = ids.clone()
    for b in range(ids.shape[0]):
        hit = (ids[b] == eos).nonzero()
        if len(hit):
            out[b, int(hit[0]) + 1:] = pad
    return out


def _check_alphas(alphas, lengths):
    """Rows t < length sum to 1, rows past the length are zero."""
    L = alphas.shape[-2]
    live = torch.arange(L, device=alphas.device)[None, None] < lengths[..., None].long()
    sums = alphas.double().sum(-1)
    torch.testing.assert_close(sums[live], torch.ones_like(sums[live]), rtol=0, atol=1e-5)
    assert (alphas[~live] == 0).all()


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 52, 8, 16, 24, 9, 16), (5, 4, 64, 16, 32, 40, 49, 24), (70, 3, 132, 8, 16, 16, 4, 8), CFG4],
                         ids=["s1", "s2", "s70", "cfg4"])
def test_k1_equals_greedy_rollout(dev, dt, shape):
    """k = 1 gives sample_fwd(pretrain=True)'s ids with PAD after <E>.  The roll-out's hp product may split K and the search's does
    not, and the search sums the context over positions in another order, so a step whose top-2 logit gap (float64 oracle on the
    roll-out's own ids) is below 1e-3 (f32) or 3e-2 (bf16, where z is rounded to 8 bits) may legitimately pick the other token: where
    a caption first differs from the roll-out's, that step must be such a near-tie (and the rest of the caption is not compared)."""
    B, L = shape[:2]
    cfg4 = shape == CFG4
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _problem(shape, sum(shape), dev, out_scale=20.0 if cfg4 else 1.0,
                                                        scale=1.0 if cfg4 else 6.0)
    eng = _engine(*shape[2:], dt)
    _, greedy, _ = eng.sample_fwd(params, feats, fmap, L, 1.0, pretrain=True)
    ids, scores, lengths = eng.beam_search(params, feats, fmap, L, 1)
    torch.cuda.synchronize()
    greedy = greedy.cpu()
    logits, _, _ = CA.attn_decoder_sample(AO.as_dict(p_cpu), f_cpu.double(), m_cpu.double(), L, 1.0, pretrain=True, force_ids=greedy)
    top2 = logits.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    thr = 1e-3 if dt == 0 else 3e-2
    want, got = _mask_after_eos(greedy), ids[:, 0].cpu()
    compared = 0
    for b in range(B):
        diff = (got[b] != want[b]).nonzero()
        n = int(diff[0]) if len(diff) else L
        assert n == L or gap[b, n] < thr, (b, n, float(gap[b, n]), got[b], want[b])
        compared += n
    assert compared >= B * L // 2, f"too few decided steps to compare: {compared} of {B * L}"


def _check_vs_oracle(eng, params, feats, fmap, p_cpu, f_cpu, m_cpu, L, k, alpha=0.0):
    ids, scores, lengths, alphas = eng.beam_search(params, feats, fmap, L, k, length_penalty=alpha, want_alphas=True)
    torch.cuda.synchronize()
    rid, rsc, rlen, ral, margins = AO.beam_search(p_cpu, f_cpu, m_cpu, k, L, length_penalty=alpha)
    _check_alphas(alphas, lengths)
    ids_c, sc_c, len_c, al_c = ids.cpu(), scores.cpu().double(), lengths.cpu().long(), alphas.cpu().double()
    norm = sc_c / len_c.double() ** alpha
    assert (norm[:, :-1] >= norm[:, 1:] - 1e-6 * norm.abs()[:, 1:]).all()
    # (at least 3/4 of the batch: every case of this file has a clear selection in every image of the oracle's run)
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    assert 4 * len(ok) >= 3 * len(margins), f"{len(ok)} of {len(margins)} images with a clear selection to compare: margins {margins}"
    for b in ok:
        if margins[b][1] >= 1e-4:
            assert torch.equal(ids_c[b], rid[b]), b
            assert torch.equal(len_c[b], rlen[b]), b
            torch.testing.assert_close(sc_c[b], rsc[b], rtol=1e-4, atol=1e-6)
            torch.testing.assert_close(al_c[b], ral[b], rtol=1e-4, atol=1e-6)
        else:
            mine = sorted(zip(ids_c[b].tolist(), len_c[b].tolist()))
            want = sorted(zip(rid[b].tolist(), rlen[b].tolist()))
            assert mine == want, b
            torch.testing.assert_close(sc_c[b].sort().values, rsc[b].sort().values, rtol=1e-4, atol=1e-6)
            for j in range(k):                           # each returned beam's maps are those of the oracle's beam with its ids
                r = next(i for i in range(k) if torch.equal(rid[b, i], ids_c[b, j]))
                torch.testing.assert_close(al_c[b, j], ral[b, r], rtol=1e-4, atol=1e-6)
    return ids, lengths, len(ok)


ORACLE_SHAPE = (6, 10, 64, 16, 32, 40, 49, 24)
# P = 70: no multiple of the 8-position energy group, more than a wave; C = 136: a partial last attn_step_ctx workgroup; A = 264: a
# second width pass of the energy kernel (f32), K hp rows of 264 floats staged in LDS
WIDE_SHAPE = (3, 6, 64, 8, 16, 136, 70, 264)


@pytest.mark.parametrize("k,alpha,shape", [(k, a, ORACLE_SHAPE) for a in (0.0, 0.7) for k in (2, 3, 5, 8)] + [(2, 0.0, WIDE_SHAPE), (8, 0.0, WIDE_SHAPE)],
                         ids=[f"{k}-{a}" for a in (0.0, 0.7) for k in (2, 3, 5, 8)] + ["2-0.0-wide", "8-0.0-wide"])
def test_f32_matches_oracle(dev, k, alpha, shape):
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _problem(shape, 100 + k, dev, eos_bias=1.5)
    eng = _engine(*shape[2:], 0)
    ids, lengths, _ = _check_vs_oracle(eng, params, feats, fmap, p_cpu, f_cpu, m_cpu, shape[1], k, alpha)
    assert ids.shape == (shape[0], k, shape[1])


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_k8_at_the_widest_attention(dev, dt):
    """k = 8 at A = 2048: attn_step_energy stages 8 hp rows of 2048 floats, the 64 KB LDS request.  The call returns its status cleanly
    and every live alpha row sums to 1."""
    shape = (1, 3, 64, 8, 16, 16, 3, 2048)
    params, feats, fmap, *_ = _problem(shape, 2048, dev)
    eng = _engine(*shape[2:], dt)
    ids, scores, lengths, alphas = eng.beam_search(params, feats, fmap, shape[1], 8, want_alphas=True)
    torch.cuda.synchronize()
    assert ids.shape == (1, 8, 3) and alphas.shape == (1, 8, 3, 3) and bool(torch.isfinite(scores).all())
    assert int(lengths.min()) >= 1
    _check_alphas(alphas, lengths)


def test_more_than_512_rows(dev):
    """B = 72, k = 8: 576 rows through the step kernels (no generic path)."""
    shape = (72, 6, 52, 8, 16, 24, 9, 16)
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _problem(shape, 72, dev, eos_bias=1.0)
    eng = _engine(*shape[2:], 0)
    _, _, n_ok = _check_vs_oracle(eng, params, feats, fmap, p_cpu, f_cpu, m_cpu, shape[1], 8)
    assert n_ok >= 36, n_ok


def test_early_stop(dev):
    """An <E>-biased b_out: every beam ends early, the search stops, and ids (PAD after <E>), lengths, scores and maps are the
    oracle's."""
    shape = (4, 12, 64, 16, 32, 40, 9, 24)
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _problem(shape, 5, dev, eos_bias=4.0)
    eng = _engine(*shape[2:], 0)
    for k in (1, 3):
        ids, lengths, n_ok = _check_vs_oracle(eng, params, feats, fmap, p_cpu, f_cpu, m_cpu, shape[1], k)
        assert n_ok == shape[0]
        assert (lengths < 4).all(), lengths
        assert (ids.cpu()[:, :, 4:] == 0).all()


@pytest.mark.parametrize("k", [3, 5])
def test_bf16_cfg4_rescored(dev, k):
    """bf16 at cfg4's shape: each returned score equals the float64 log-probability of its own ids (teacher-forced) within
    rtol 2e-2 + 0.05 per token (bf16 rounds every operand to 8 bits); beams in order, maps normalised."""
    B, L = CFG4[:2]
    params, feats, fmap, p_cpu, f_cpu, m_cpu = _problem(CFG4, k, dev, eos_bias=3.0, out_scale=20.0, scale=1.0)
    eng = _engine(*CFG4[2:], 1)
    ids, scores, lengths, alphas = eng.beam_search(params, feats, fmap, L, k, want_alphas=True)
    torch.cuda.synchronize()
    assert ids.shape == (B, k, L) and scores.shape == (B, k) and alphas.shape == (B, k, L, CFG4[6])
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    _check_alphas(alphas, lengths)
    pos = torch.arange(L, device=dev)[None, None]
    assert (ids[pos.expand_as(ids) >= lengths[..., None].long()] == 0).all()
    ref = AO.sequence_logprob(p_cpu, f_cpu, m_cpu, ids.cpu(), lengths.cpu())
    got = scores.cpu().double()
    tol = 2e-2 * ref.abs() + 0.05 * lengths.cpu().double()
    assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()


def test_bits_and_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    params, feats, fmap, *_ = _problem(CFG4, 9, dev, eos_bias=2.0, out_scale=20.0, scale=1.0)
    eng = _engine(*CFG4[2:], 1)
    runs = [eng.beam_search(params, feats, fmap, CFG4[1], 5, want_alphas=True) for _ in range(2)]
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        runs.append(eng.beam_search(params, feats, fmap, CFG4[1], 5, want_alphas=True))
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def _attn_args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=16, gen_hidden_dim=32, conditional_gan=1, encoder_arch="resnet18", decoder="attention",
                attn_dim=24, compute_dtype="fp32", image_size=64, max_seq_len=8, device="cuda", log_file=None, model_dir=None, save_dir=None)
    base.update(kw)
    return default_args(**base)


def test_caption_module_api(dev):
    from gan_image_captioning_amd.generator import Generator
    torch.manual_seed(4)
    gen = Generator(_attn_args()).to(dev)
    with torch.no_grad():
        for p in gen.decoder.parameters():
            p.mul_(8.0)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    ids, scores, lengths, alphas = gen.caption(images, beam_size=3, return_alphas=True)
    feats, fmap = gen.encoder.forward_with_map(images)
    ids2, scores2, lengths2, alphas2 = gen.decoder.beam_search(feats, fmap, beam_size=3, return_alphas=True)
    torch.cuda.synchronize()
    assert ids.shape == (4, 8) and alphas.shape == (4, 8, 4)            # 64x64 images: a 2x2 map
    for a, b in zip((ids, scores, lengths, alphas), (ids2, scores2, lengths2, alphas2)):
        assert torch.equal(a, b)
    _check_alphas(alphas[:, None], lengths[:, None])
    beams = gen.caption(images, beam_size=3, return_beams=True)
    assert [t.shape for t in beams] == [(4, 3, 8), (4, 3), (4, 3)]
    assert torch.equal(beams[0][:, 0], ids)


def test_evaluate_bleu_with_attention(dev):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    args = _attn_args(eval_beam_size=3, adv_eval_batch_size=4, num_workers=0)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    score = inst.evaluate("val", beam_size=args.eval_beam_size)
    assert isinstance(score, float) and 0.0 <= score <= 1.0
    assert seen and seen[0][0] == "BLEU4_val" and seen[0][1] == score
