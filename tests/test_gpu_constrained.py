"""Decode constraints on the GPU (gic_*_constrained_beam_search, gic_*_constrained_sample_captions; the engines', decoders' and
Generator's no_repeat_ngram / min_length / suppress_tokens; the --eval-* flags) against the float64 oracle
(tests/constrained_oracle.py) on the cases that tests/test_constrained_api.py pins, the invariants of every returned caption,
teacher-forced rescoring, the unconstrained calls and itself."""
import math

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import test_constrained_api as T
from tests.test_gpu_diverse_beam import _compare

pytestmark = pytest.mark.gpu

CONS = dict(no_repeat_ngram=2, min_length=5, suppress_tokens=(1, 3))
CFG4 = (32, 20, 10000, 512, 512, 2048, 49, 512)          # B, L, V, E, H, C, P, A: the largest shape of tests/test_gpu_attn_beam.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _eng(which, dt=0):
    from gan_image_captioning_amd import engine
    if which == "attn":
        return engine.AttnDecoderEngine(*T.ATTN_SHAPE[2:], dt)
    B, L, V, E, H, NL = T.LSTM_SHAPES[which]
    return engine.DecoderEngine(V, E, H, NL, dt)


def _gpu_beam(case, dev, constrained=True):
    which, seed, k, G, lam, cons = case
    kw = cons if constrained else {}
    eng = _eng(which)
    if which == "attn":
        params, feats, fmap = T.attn_problem(seed)
        return eng.diverse_beam_search([p.to(dev) for p in params], feats.to(dev), fmap.to(dev), T.ATTN_SHAPE[1], k, G, lam,
                                       want_alphas=True, **kw)
    params, feats = T.lstm_problem(which, seed)
    B, L = T.LSTM_SHAPES[which][:2]
    assert eng.beam_fused(B, k) == (which == "fused")
    return eng.diverse_beam_search([p.to(dev) for p in params], feats.to(dev), L, k, G, lam, **kw)


def _gpu_sample(case, dev, constrained=True):
    which, seed, n, opts, cons = case
    kw = cons if constrained else {}
    eng = _eng(which)
    u = T.case_noise(which, seed, n).to(dev)
    if which == "attn":
        params, feats, fmap = T.attn_problem(seed)
        return eng.sample_captions([p.to(dev) for p in params], feats.to(dev), fmap.to(dev), T.ATTN_SHAPE[1], n, *opts, noise_u=u, **kw)
    params, feats = T.lstm_problem(which, seed)
    return eng.sample_captions([p.to(dev) for p in params], feats.to(dev), T.LSTM_SHAPES[which][1], n, *opts, noise_u=u, **kw)


def _check(ids, lengths, cons):
    T.check_invariants(ids.cpu(), lengths.cpu().long(), ids.shape[-1], cons["no_repeat_ngram"], cons["min_length"],
                       cons["suppress_tokens"])


# ---------------------------------------------------------------- 1. f32 against the oracle, on the pinned cases
@pytest.mark.parametrize("case", T.BEAM_CASES, ids=T._case_id)
def test_beam_f32_matches_oracle(dev, case):
    which, seed, k, G, lam, cons = case
    B = (T.ATTN_SHAPE if which == "attn" else T.LSTM_SHAPES[which])[0]
    got = _gpu_beam(case, dev)
    torch.cuda.synchronize()
    _check(got[0], got[2], cons)
    want = T.beam_oracle(case)
    if which == "attn":
        n = _compare(got, want[:3], want[3], k, G, got[3], want[4])
    else:
        n = _compare(got, want[:3], want[3], k, G)
    print(f"{T._case_id(case)}: {n} of {B} images compared; margins {want[3]}")
    assert 4 * n >= 3 * B, f"{n} of {B} images with a clear selection: margins {want[3]}"


@pytest.mark.parametrize("case", T.SAMPLE_CASES, ids=T._case_id)
def test_sample_f32_matches_oracle(dev, case):
    which, seed, n, opts, cons = case
    ids, scores, lengths = _gpu_sample(case, dev)
    torch.cuda.synchronize()
    _check(ids, lengths, cons)
    rid, rsc, rlen, margin = T.sample_oracle(case)
    ok = margin > 1e-5
    print(f"{T._case_id(case)}: {int(ok.sum())} of {ok.numel()} rows compared")
    assert 4 * int(ok.sum()) >= 3 * ok.numel(), margin
    assert torch.equal(ids.cpu()[ok], rid[ok])
    assert torch.equal(lengths.cpu().long()[ok], rlen[ok])
    torch.testing.assert_close(scores.cpu().double()[ok], rsc[ok], rtol=1e-5, atol=1e-4)


# ---------------------------------------------------------------- 2. invariants of every returned caption, and its score
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


def _rescore(dec, feats, ids, scores, lengths, tol):
    """Each score is the teacher-forced log-probability of the returned ids (the rescoring of tests/test_gpu_beam.py)."""
    L = ids.shape[-1]
    pos = torch.arange(L, device=ids.device)[None]
    for j in range(ids.shape[1]):
        row, n = ids[:, j], lengths[:, j].long()
        pred, _ = dec(feats, row[:, :-1].contiguous(), n.cpu(), pretrain=True)
        logp = torch.log_softmax(pred.float(), dim=-1)
        lp = logp.gather(2, row[:, :pred.shape[1], None])[..., 0]
        lp = torch.where(pos[:, :pred.shape[1]] < n[:, None], lp, torch.zeros_like(lp))
        torch.testing.assert_close(lp.sum(1), scores[:, j], rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(64, 20, 10000, 512, 512), (16, 12, 1001, 256, 256)], ids=["cfg2", "generic"])
def test_lstm_invariants_and_scores(dev, shape, dtype):
    B, L, V, E, H = shape
    dec = _decoder(dev, V, E, H, L, dtype)
    feats = torch.randn(B, E, device=dev)
    tol = 1e-4 if dtype == "fp32" else 1e-2
    assert dec.engine().beam_fused(B, 6) == (V == 10000)
    free = dec.beam_search(feats, beam_size=5, return_beams=True)
    assert T._violations(free[0].cpu(), free[2].cpu(), CONS) >= 1            # (the constraints bind at this shape)
    runs = [dec.beam_search(feats, beam_size=5, return_beams=True, **CONS),
            dec.beam_search(feats, beam_size=6, return_beams=True, beam_groups=3, diversity=0.7, **CONS),
            dec.sample_captions(feats, num_samples=5, top_k=50, top_p=0.95, seed=3, **CONS)]
    torch.cuda.synchronize()
    for ids, scores, lengths in runs:
        _check(ids, lengths, CONS)
        _rescore(dec, feats, ids, scores, lengths, tol)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_attn_invariants_and_scores(dev, dt):
    from gan_image_captioning_amd import engine
    B, L = CFG4[:2]
    p_cpu, f_cpu, m_cpu = AO.random_problem(B, *CFG4[2:], seed=4, scale=1.0)
    p_cpu[5] = p_cpu[5] * 20.0
    p_cpu[6] = p_cpu[6].clone()
    p_cpu[6][2] += 3.0
    params, feats, fmap = [p.to(dev) for p in p_cpu], f_cpu.to(dev), m_cpu.to(dev)
    eng = engine.AttnDecoderEngine(*CFG4[2:], dt)
    runs = [eng.beam_search(params, feats, fmap, L, 3, **CONS),
            eng.diverse_beam_search(params, feats, fmap, L, 4, 2, 1.0, **CONS),
            eng.sample_captions(params, feats, fmap, L, 2, top_k=50, top_p=0.9, seed=8, **CONS)]
    torch.cuda.synchronize()
    for ids, scores, lengths in runs:
        _check(ids, lengths, CONS)
        ref = AO.sequence_logprob(p_cpu, f_cpu, m_cpu, ids.cpu(), lengths.cpu())
        got = scores.cpu().double()
        tol = (1e-4 * ref.abs() + 1e-4) if dt == 0 else (2e-2 * ref.abs() + 0.05 * lengths.cpu().double())
        assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()


# ---------------------------------------------------------------- 3. constraints off: the unconstrained call, bit for bit
@pytest.fixture
def through_new_entry_points(monkeypatch):
    """The engines call the constrained entry points even with every constraint off (they otherwise call the unconstrained ones)."""
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    calls = []
    lib = L.load()
    for name in ("gic_decoder_constrained_beam_search", "gic_attn_constrained_beam_search", "gic_decoder_constrained_sample_captions",
                 "gic_attn_constrained_sample_captions"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(fn, name))
    real = engine.decode_constraints
    monkeypatch.setattr(engine, "decode_constraints", lambda *a: real(*a) or L.DecodeConstraints())
    return calls


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 10, 64, 32, 512, 1), (64, 20, 10000, 512, 512, 1), (16, 8, 1001, 64, 64, 2)],
                         ids=["cfg1", "cfg2", "generic"])
def test_lstm_constraints_off_is_bit_for_bit(dev, dt, shape, monkeypatch, request):
    from gan_image_captioning_amd import engine
    B, L, V, E, H, NL = shape
    eng = engine.DecoderEngine(V, E, H, NL, dt)
    assert eng.beam_fused(B, 4) == (V != 1001)
    params = [t.to(dev) for t in BO.random_params(V, E, H, NL, seed=B + V, scale=3.0)]
    params[-1][2] += 1.0
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(4)).to(dev)

    def runs():
        return [eng.beam_search(params, feats, L, 4, length_penalty=0.7), eng.beam_search(params, feats, L, 7),
                eng.diverse_beam_search(params, feats, L, 6, 3, 0.8), eng.sample_captions(params, feats, L, 3, 8, 0.9, 0.8, seed=5)]

    want = runs()
    calls = request.getfixturevalue("through_new_entry_points")
    got = runs()
    torch.cuda.synchronize()
    assert calls == ["gic_decoder_constrained_beam_search"] * 3 + ["gic_decoder_constrained_sample_captions"]
    for x, y in zip(got, want):
        for a, b in zip(x, y):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_attn_constraints_off_is_bit_for_bit(dev, dt, request):
    from gan_image_captioning_amd import engine
    shape = T.ATTN_SHAPE
    p_cpu, f_cpu, m_cpu = AO.random_problem(shape[0], *shape[2:], seed=7, scale=6.0)
    p_cpu[6] = p_cpu[6].clone()
    p_cpu[6][2] += 1.0
    params, feats, fmap = [p.to(dev) for p in p_cpu], f_cpu.to(dev), m_cpu.to(dev)
    eng = engine.AttnDecoderEngine(*shape[2:], dt)

    def runs():
        return [eng.beam_search(params, feats, fmap, shape[1], 5, length_penalty=0.7, want_alphas=True),
                eng.diverse_beam_search(params, feats, fmap, shape[1], 6, 3, 2.0, want_alphas=True),
                eng.sample_captions(params, feats, fmap, shape[1], 3, 8, 0.9, 0.8, seed=5)]

    want = runs()
    calls = request.getfixturevalue("through_new_entry_points")
    got = runs()
    torch.cuda.synchronize()
    assert calls == ["gic_attn_constrained_beam_search"] * 2 + ["gic_attn_constrained_sample_captions"]
    for x, y in zip(got, want):
        for a, b in zip(x, y):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. the same bits twice, and in the deterministic mode
def test_bits_and_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    B, L, V, E, H = 64, 20, 10000, 512, 512
    eng = engine.DecoderEngine(V, E, H, 1, 1)
    gen = engine.DecoderEngine(1001, 64, 64, 2, 1)
    params = [t.to(dev) for t in BO.random_params(V, E, H, 1, seed=3, scale=3.0)]
    gparams = [t.to(dev) for t in BO.random_params(1001, 64, 64, 2, seed=4, scale=3.0)]
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(2)).to(dev)
    gfeats = torch.randn(16, 64, generator=torch.Generator().manual_seed(3)).to(dev)
    shape = (8, 12, 10000, 512, 512, 2048, 49, 512)
    p_cpu, f_cpu, m_cpu = AO.random_problem(shape[0], *shape[2:], seed=9, scale=1.0)
    p_cpu[5] = p_cpu[5] * 20.0
    ap, af, am = [p.to(dev) for p in p_cpu], f_cpu.to(dev), m_cpu.to(dev)
    aeng = engine.AttnDecoderEngine(*shape[2:], 1)

    def all_heads():
        return (eng.beam_search(params, feats, L, 5, **CONS), eng.diverse_beam_search(params, feats, L, 8, 4, 0.5, **CONS),
                eng.sample_captions(params, feats, L, 5, 50, 0.95, seed=7, **CONS),
                gen.diverse_beam_search(gparams, gfeats, 8, 6, 2, 0.5, **CONS), gen.sample_captions(gparams, gfeats, 8, 3, seed=7, **CONS),
                aeng.diverse_beam_search(ap, af, am, shape[1], 6, 3, 0.5, want_alphas=True, **CONS),
                aeng.sample_captions(ap, af, am, shape[1], 3, 50, 0.9, seed=7, **CONS))

    runs = [all_heads(), all_heads()]
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        runs.append(all_heads())
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            for a, b in zip(x, y):
                assert torch.equal(a, b)
    for out in runs[0]:
        _check(out[0], out[2], CONS)


# ---------------------------------------------------------------- 5. the constraints bind on the device
@pytest.mark.parametrize("case", [T.BEAM_CASES[0], T.BEAM_CASES[6], T.BEAM_CASES[13]], ids=T._case_id)
def test_beam_constraints_bind_on_the_device(dev, case):
    cons = case[5]
    free = _gpu_beam(case, dev, constrained=False)
    held = _gpu_beam(case, dev)
    torch.cuda.synchronize()
    assert T._violations(free[0].cpu(), free[2].cpu(), cons) >= 1
    assert T._violations(held[0].cpu(), held[2].cpu(), cons) == 0
    assert not torch.equal(free[0], held[0])


@pytest.mark.parametrize("case", [T.SAMPLE_CASES[1], T.SAMPLE_CASES[3], T.SAMPLE_CASES[5]], ids=T._case_id)
def test_sample_constraints_bind_on_the_device(dev, case):
    cons = case[4]
    free = _gpu_sample(case, dev, constrained=False)
    held = _gpu_sample(case, dev)
    torch.cuda.synchronize()
    assert T._violations(free[0].cpu(), free[2].cpu(), cons) >= 1
    assert T._violations(held[0].cpu(), held[2].cpu(), cons) == 0


# ---------------------------------------------------------------- 6. through the public interface
def _gen_args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64,
                conditional_gan=1, max_seq_len=8, adv_eval_batch_size=4, num_workers=0, device="cuda", log_file=None, model_dir=None,
                save_dir=None)
    base.update(kw)
    return default_args(**base)


_ATTN = dict(decoder="attention", encoder_arch="resnet18", gen_embed_dim=16, gen_hidden_dim=32, attn_dim=24)


@pytest.mark.parametrize("kind", ["lstm", "lstm_uncond", "attention"])
def test_generator_caption_and_sample_captions(dev, kind):
    from gan_image_captioning_amd.generator import Generator
    kw = {"lstm": {}, "lstm_uncond": dict(conditional_gan=0), "attention": _ATTN}[kind]
    torch.manual_seed(4)
    gen = Generator(_gen_args(**kw)).to(dev)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    plain = gen.caption(images, beam_size=4, return_beams=True)
    off = gen.caption(images, beam_size=4, return_beams=True, no_repeat_ngram=0, min_length=0, suppress_tokens=())
    beams = gen.caption(images, beam_size=4, return_beams=True, **CONS)
    best = gen.caption(images, beam_size=4, **CONS)
    groups = gen.caption(images, beam_size=4, return_beams=True, beam_groups=2, diversity=0.5, **CONS)
    draws = gen.sample_captions(images, num_samples=3, top_k=20, seed=5, **CONS)
    again = gen.sample_captions(images, num_samples=3, top_k=20, seed=5, **CONS)
    torch.cuda.synchronize()
    for a, b in zip(plain, off):
        assert torch.equal(a, b)
    assert [t.shape for t in beams] == [(4, 4, 8), (4, 4), (4, 4)] and [t.shape for t in draws] == [(4, 3, 8), (4, 3), (4, 3)]
    assert torch.equal(best[0], beams[0][:, 0]) and torch.equal(best[1], beams[1][:, 0])
    for out in (beams, groups, draws):
        _check(out[0], out[2], CONS)
    for a, b in zip(draws, again):
        assert torch.equal(a, b)
    if kind == "attention":
        al = gen.caption(images, beam_size=4, return_beams=True, return_alphas=True, **CONS)
        assert torch.equal(al[0], beams[0]) and al[3].shape == (4, 4, 8, al[3].shape[-1])
    with pytest.raises(ValueError, match="infeasible|min_length"):
        gen.caption(images, beam_size=4, min_length=9)


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_evaluate_with_the_flags(dev, kind):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    kw = _ATTN if kind == "attention" else {}
    args = _gen_args(eval_no_repeat_ngram=2, eval_min_length=5, eval_suppress_tokens=[1, 3], **kw)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen, decoded = [], []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    cap, smp = inst.gen.caption, inst.gen.sample_captions
    inst.gen.caption = lambda *a, **k: (decoded.append(cap(*a, **k)), decoded[-1])[1]
    inst.gen.sample_captions = lambda *a, **k: (decoded.append(smp(*a, **k)), decoded[-1])[1]
    bleu = inst.evaluate("val", beam_size=3)
    cider = inst.evaluate_cider("val", beam_size=3)
    div = inst.evaluate_diversity("val", num_samples=3, top_k=20)
    dbs = inst.evaluate_diverse_beam("val", beam_size=4, groups=2, diversity=0.5)
    assert math.isfinite(bleu) and 0.0 <= bleu <= 1.0 and math.isfinite(cider) and cider >= 0.0
    for out in (div, dbs):
        assert set(out) == {"bleu4", "mbleu4", "distinct1", "distinct2", "vocab"}
    assert {"BLEU4_val", "CIDErD_val", "mBLEU4_val", "mBLEU4DBS_val"} <= {t for t, _ in seen}
    assert len(decoded) >= 4 * 2                               # six images in batches of four, four evaluations
    for ids, _, lengths in decoded:
        _check(ids, lengths, CONS)
    assert bleu == inst.evaluate("val", beam_size=3)
