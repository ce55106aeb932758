"""Caption log-likelihood scoring and the masked, label-smoothed pre-training loss at the module level: Decoder / AttnDecoder
.log_likelihood against the torch.log_softmax rescoring of the decoder's own forward output and against the scores beam search and sampling
return, Generator.score_captions, GANInstructor.pretrain_step with --pretrain-ignore-pad / --label-smoothing against F.cross_entropy on the
module's own predictions (values and decoder gradients), the untouched default path, and evaluate_perplexity."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import close
from tests.rerank_cases import spread

pytestmark = pytest.mark.gpu

V, L, B = 64, 12, 4
TOL = {"fp32": 1e-4, "bf16": 1e-2}                       # the figures of the existing teacher-forced rescoring (_rescore)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _gen(dev, kind, dtype="fp32", cgan=1, seed=4):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Generator
    kw = dict(decoder="attention", attn_dim=16) if kind == "attention" else dict(gen_num_layers=1)
    args = default_args(vocab_size=V, gen_embed_dim=32, gen_hidden_dim=64, compute_dtype=dtype, image_size=64, conditional_gan=cgan,
                        encoder_arch="resnet18", max_seq_len=L, device="cuda", log_file=None, model_dir=None, save_dir=None, **kw)
    torch.manual_seed(seed)
    gen = Generator(args).to(dev).eval()
    spread(gen)
    return gen


def _images(dev, n=B, seed=9):
    return torch.randn(n, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(dev)


def _maps(fmap):
    return () if fmap is None else (fmap,)


def _rescore(dec, features, fmap, ids, lengths):
    """sum_{t < length} log_softmax(forward(features[, fmap], ids[:, :-1], lengths, pretrain=True))[t, ids[t]] with torch."""
    n = lengths.long()
    pred = dec(features, *_maps(fmap), ids[:, :-1].contiguous(), n.cpu(), pretrain=True)[0]
    lp = torch.log_softmax(pred.float(), -1).gather(2, ids[:, :pred.shape[1], None])[..., 0]
    pos = torch.arange(pred.shape[1], device=ids.device)[None]
    return torch.where(pos < n[:, None], lp, torch.zeros_like(lp)).sum(1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_log_likelihood_is_the_rescoring_of_forward(dev, kind, dtype):
    gen = _gen(dev, kind, dtype)
    dec = gen.decoder
    with torch.no_grad():
        features, fmap = gen._features(_images(dev))
        g = torch.Generator().manual_seed(3)
        ids = torch.randint(3, V, (B, L), generator=g).to(dev)
        lengths = torch.tensor([L, L - 3, 2, 1], dtype=torch.int32, device=dev)
        want = _rescore(dec, features, fmap, ids, lengths)
        logp, tokens = dec.log_likelihood(features, *_maps(fmap), ids, lengths)
    torch.cuda.synchronize()
    assert logp.dtype == torch.float32 and tokens.dtype == torch.int32 and logp.shape == tokens.shape == (B,)
    assert torch.equal(tokens, lengths)
    torch.testing.assert_close(logp, want, rtol=TOL[dtype], atol=TOL[dtype])
    assert bool((logp < 0).all())
    # lengths as a list and on the CPU are the same call
    again = dec.log_likelihood(features, *_maps(fmap), ids, lengths.tolist())[0]
    assert torch.equal(again, logp)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_log_likelihood_of_decoded_captions_is_their_score(dev, kind, dtype):
    gen = _gen(dev, kind, dtype)
    dec = gen.decoder
    K = 3
    with torch.no_grad():
        features, fmap = gen._features(_images(dev))
        runs = [dec.beam_search(features, *_maps(fmap), beam_size=K, max_caption_len=L, return_beams=True)[:3],
                dec.sample_captions(features, *_maps(fmap), num_samples=K, temperature=1.0, max_caption_len=L, seed=5)]
        for ids, scores, lengths in runs:
            assert ids.shape == (B, K, L)
            for k in range(K):
                logp, tokens = dec.log_likelihood(features, *_maps(fmap), ids[:, k].contiguous(), lengths[:, k])
                assert torch.equal(tokens, lengths[:, k])
                torch.testing.assert_close(logp, scores[:, k], rtol=TOL[dtype], atol=TOL[dtype])
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,cgan", [("lstm", 1), ("attention", 1), ("lstm", 0)])
def test_score_captions_with_k_captions_per_image(dev, kind, cgan):
    gen = _gen(dev, kind, "fp32", cgan=cgan)
    images = _images(dev)
    K = 3
    ids, scores, lengths = gen.sample_captions(images, num_samples=K, max_caption_len=L, seed=7)
    logp, tokens = gen.score_captions(images, ids, lengths)
    torch.cuda.synchronize()
    assert logp.shape == tokens.shape == (B, K) and torch.equal(tokens, lengths)
    torch.testing.assert_close(logp, scores, rtol=1e-4, atol=1e-4)
    for k in range(K):
        one, tok = gen.score_captions(images, ids[:, k].contiguous(), lengths[:, k])
        assert one.shape == (B,) and torch.equal(tok, lengths[:, k])
        torch.testing.assert_close(one, logp[:, k], rtol=1e-4, atol=1e-4)
    if not cgan:                                         # the start feature is embed(<S>), as the trainer forms it
        feats = gen.decoder.embed(torch.ones(B, dtype=torch.long, device=dev)).detach()
        want = gen.decoder.log_likelihood(feats, ids[:, 0].contiguous(), lengths[:, 0])[0]
        torch.testing.assert_close(logp[:, 0], want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="score_captions"):
        gen.score_captions(images, ids, lengths[:, 0])


# ------------------------------------------------------------------------------------------ the instructor
def _instructor(decoder, mode, **kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    dims = dict(gen_embed_dim=16, gen_hidden_dim=32, attn_dim=24) if decoder == "attention" else dict(gen_embed_dim=32, gen_hidden_dim=64)
    base = dict(vocab_size=V, conditional_gan=1, encoder_arch="resnet18", compute_dtype="fp32", image_size=64, device="cuda", log_file=None,
                model_dir=None, save_dir=None, decoder=decoder, pretrain_mode="teacher" if mode == "scheduled" else mode,
                scheduled_sampling_prob=0.5 if mode == "scheduled" else 0.0, max_seq_len=L, **dims)
    base.update(kw)
    torch.manual_seed(12)
    inst = GANInstructor(default_args(**base), None, None)
    with torch.no_grad():
        for q in inst.gen.decoder.parameters():
            q.mul_(8.0)
    return inst


def _captions(lens, seed=2):
    """Hand-made captions in tasks.collate_fn's layout: <S> body <E>, then <PAD> = 0."""
    g = torch.Generator().manual_seed(seed)
    caps = torch.zeros(len(lens), L, dtype=torch.int64)
    for b, n in enumerate(lens):
        caps[b, :n] = torch.cat([torch.ones(1, dtype=torch.int64), torch.randint(3, V, (n - 2,), generator=g), torch.full((1,), 2)])
    return caps, torch.tensor(lens, dtype=torch.int32)


def _capture_pred(inst, monkeypatch, seen):
    """Record the prediction tensor pretrain_step computes its loss on (the decoder's own output, attached to its autograd graph), and
    ``seen["again"]``: the same decode once more, with the same device draws -- a decode's backward runs once, so the gradients of a
    second loss need a second graph."""
    from gan_image_captioning_amd.generator import SEEDS
    dec = inst.gen.decoder
    for name in ("forward", "sample", "forward_scheduled"):
        inner = getattr(dec, name)

        def wrapped(*a, _inner=inner, **kw):
            n0 = SEEDS._n
            res = _inner(*a, **kw)
            seen["pred"] = res[0]

            def again():
                n1 = SEEDS._n
                SEEDS.reset(n0)
                try:
                    return _inner(*a, **kw)[0]
                finally:
                    SEEDS.reset(n1)
            seen["again"] = again
            return res
        monkeypatch.setattr(dec, name, wrapped)


@pytest.mark.parametrize("mode", ["teacher", "sample", "scheduled"])
@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_pretrain_step_with_the_flags_is_torch_cross_entropy(dev, decoder, mode, monkeypatch):
    """Values and decoder gradients of --pretrain-ignore-pad 1 --label-smoothing 0.1 on captions of lengths (L, L-3, 2): a training batch
    is F.cross_entropy(pred, targets, ignore_index=pad, label_smoothing=0.1) of the module's own pred, a validation batch the same
    without smoothing (only training batches are smoothed)."""
    inst = _instructor(decoder, mode, pretrain_ignore_pad=1, label_smoothing=0.1)
    assert (inst.ignore_pad, inst.label_smoothing) == (True, 0.1)
    caps, lengths = _captions([L, L - 3, 2])
    images = _images(dev, 3)
    params = list(inst.gen.decoder.parameters())
    seen = {}
    _capture_pred(inst, monkeypatch, seen)
    monkeypatch.setattr(inst, "optimize", lambda opt, loss, model=None, retain_graph=False: seen.update(
        grads=torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)))

    def torch_loss(eps, pred=None):
        pred = seen["pred"] if pred is None else pred
        return F.cross_entropy(pred.float().reshape(-1, V), caps.to(dev)[:, :pred.shape[1]].reshape(-1), ignore_index=0, label_smoothing=eps)

    inst.gen.train()
    with torch.enable_grad():
        loss = inst.pretrain_step(images, caps.to(dev), L, train=True, lengths=lengths)
        want = torch_loss(0.1)
        pred2 = seen["again"]()                           # the same decode, for torch's loss to back-propagate through
        torch.testing.assert_close(pred2, seen["pred"], rtol=1e-5, atol=1e-5)
        gw = torch.autograd.grad(torch_loss(0.1, pred2), params, allow_unused=True)
    torch.cuda.synchronize()
    assert float(loss.detach()) == pytest.approx(float(want.detach()), rel=1e-5)
    for (n, _), got, w in zip(inst.gen.decoder.named_parameters(), seen["grads"], gw):
        assert (got is None) == (w is None), n
        if w is not None:
            close(got, w, rtol=2e-3, atol_scale=1e-4, what=f"{decoder} {mode} {n}")
    if mode != "scheduled":
        inst.gen.eval()
        with torch.no_grad():
            val = inst.pretrain_step(images, caps.to(dev), L, train=False, lengths=lengths)
            assert float(val) == pytest.approx(float(torch_loss(0.0)), rel=1e-5)
        assert abs(float(torch_loss(0.1)) - float(torch_loss(0.0))) > 1e-3 * abs(float(val))      # (smoothing does move this loss)


@pytest.mark.parametrize("mode", ["teacher", "sample"])
@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_default_flags_leave_the_step_as_it_was(dev, decoder, mode, monkeypatch):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.training import _XentFn
    inst = _instructor(decoder, mode)
    assert (inst.ignore_pad, inst.label_smoothing) == (False, 0.0)
    caps, lengths = _captions([L, L - 3, 2])
    images = _images(dev, 3)
    seen = {}
    _capture_pred(inst, monkeypatch, seen)

    def never(*a, **kw):
        raise AssertionError("engine.xent_seq ran with the flags at their defaults")
    monkeypatch.setattr(engine, "xent_seq", never)
    monkeypatch.setattr(inst, "optimize", lambda opt, loss, model=None, retain_graph=False: seen.update(
        dpred=torch.autograd.grad(loss, seen["pred"], retain_graph=True)[0]))
    inst.gen.train()
    with torch.enable_grad():
        loss = inst.pretrain_step(images, caps.to(dev), L, train=True, lengths=lengths)
        pred = seen["pred"]
        flat = pred.reshape(-1, V)
        targets = caps.to(dev)[:, :pred.shape[1]].reshape(-1)
        old = _XentFn.apply(flat, targets)                 # the step's loss as it was before the flags existed
        old_d = torch.autograd.grad(old, pred)[0]
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), old.detach()) and torch.equal(seen["dpred"], old_d)
    assert float(loss.detach()) == pytest.approx(float(F.cross_entropy(flat.detach().float(), targets)), rel=1e-5)


@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_evaluate_perplexity(dev, decoder):
    inst = _instructor(decoder, "teacher", eval_perplexity=1)
    inst.gen.eval()
    batches = []
    for i, lens in enumerate(([L, L - 3, 2], [5, 9, 3, 7])):
        caps, lengths = _captions(lens, seed=20 + i)
        batches.append((_images(dev, len(lens), seed=30 + i).cpu(), caps, lengths, L))
    inst.pre_eval_loader = batches
    nll, tokens = 0.0, 0
    with torch.no_grad():
        for images, caps, lengths, _ in batches:
            feats = inst._features(images.to(dev), caps.shape[0])
            feats = feats if isinstance(feats, tuple) else (feats,)
            logp, tok = inst.gen.decoder.log_likelihood(*feats, caps.to(dev), lengths)
            assert torch.equal(tok.cpu(), lengths)
            nll += float(-logp.double().sum())
            tokens += int(tok.sum())
    out = inst.evaluate_perplexity("val")
    assert set(out) == {"nll_per_token", "perplexity", "tokens", "captions"}
    assert out["tokens"] == tokens == 2 * L - 1 + 24 and out["captions"] == 7
    assert out["nll_per_token"] == pytest.approx(nll / tokens, rel=1e-5)
    assert out["perplexity"] == pytest.approx(math.exp(nll / tokens), rel=1e-5)
    # a call in train mode evaluates in eval mode all the same, leaves the BatchNorm running statistics alone and restores the mode
    stats = {k: v.clone() for k, v in inst.gen.state_dict().items() if "running_" in k or "num_batches" in k}
    assert stats
    inst.gen.train()
    assert inst.evaluate_perplexity("val")["perplexity"] == pytest.approx(out["perplexity"], rel=1e-5) and inst.gen.training
    assert all(torch.equal(v, inst.gen.state_dict()[k]) for k, v in stats.items())
    inst.gen.eval()
    with torch.no_grad():                                # a uniform predictor: perplexity V
        inst.gen.decoder.linear.weight.zero_()
        inst.gen.decoder.linear.bias.zero_()
    assert inst.evaluate_perplexity("val")["perplexity"] == pytest.approx(float(V), rel=1e-4)
