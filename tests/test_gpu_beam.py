"""Beam-search caption decode on the GPU (gic_decoder_beam_search, Decoder.beam_search, Generator.caption,
GANInstructor.evaluate) against the reference's own greedy run, the library's greedy roll-out and the CPU oracle
(tests/beam_oracle.py)."""
import math

import pytest
import torch

from oracle import cpu_step as O
from tests import beam_oracle as BO
from tests.golden_io import Golden, initial_params
from tests.gpu_util import dec_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _engine(V, E, H, NL, dt):
    from gan_image_captioning_amd import engine
    return engine.DecoderEngine(V, E, H, NL, dt)


def _mask_after_eos(ids, eos=2, pad=0):
    out = ids.clone()
    for b in range(ids.shape[0]):
        hit = (ids[b] == eos).nonzero()
        if len(hit):
            out[b, int(hit[0]) + 1:] = pad
    return out


def test_k1_pinned_by_reference_run(dev):
    g = Golden("pretrain_tiny")
    gp, m = g.group("gp0/"), g.meta
    eng = _engine(m["V"], m["E"], m["H"], m["NL"], 0)
    params = dec_params(gp, dev)
    feats = O.start_features(gp, m["B"]).to(dev)
    assert not eng.beam_fused(m["B"], 1)                 # V = 50: the generic path
    ids, scores, lengths = eng.beam_search(params, feats, m["L"], 1)
    torch.cuda.synchronize()
    ref = g.t("s0/ids")
    assert torch.equal(ids[:, 0].cpu(), _mask_after_eos(ref))
    logp = torch.log_softmax(g.t("s0/logits").double(), dim=-1)
    for b in range(m["B"]):
        n = int(lengths[b, 0])
        want = float(logp[b, torch.arange(n), ref[b, :n]].sum())
        assert float(scores[b, 0]) == pytest.approx(want, rel=1e-4)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("shape", [(8, 10, 64, 32, 512, 1), (64, 20, 10000, 512, 512, 1), (600, 6, 50, 8, 16, 2)],
                         ids=["cfg1", "cfg2", "generic600"])
def test_k1_equals_greedy_rollout(dev, dt, shape):
    B, L, V, E, H, NL = shape
    eng = _engine(V, E, H, NL, dt)
    params = [t.to(dev) for t in BO.random_params(V, E, H, NL, seed=B + V, scale=3.0)]
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(3)).to(dev)
    _, ref, _ = eng.sample_fwd(params, feats, L, 1.0, pretrain=True)
    ids, _, lengths = eng.beam_search(params, feats, L, 1)
    torch.cuda.synchronize()
    assert eng.beam_fused(B, 1) == (shape[0] != 600)
    assert torch.equal(ids[:, 0].cpu(), _mask_after_eos(ref.cpu()))


def _check_vs_oracle(eng, params, feats, L, k, alpha):
    ids, scores, lengths = eng.beam_search(params, feats, L, k, length_penalty=alpha)
    torch.cuda.synchronize()
    rid, rsc, rlen, margins = BO.beam_search([p.cpu() for p in params], feats.cpu(), k, L, length_penalty=alpha)
    ids_c, sc_c, len_c = ids.cpu(), scores.cpu().double(), lengths.cpu().long()
    # every image: the returned order is by score / length**alpha, best first
    norm = sc_c / len_c.double() ** alpha
    assert (norm[:, :-1] >= norm[:, 1:] - 1e-6 * norm.abs()[:, 1:]).all()
    # images whose surviving hypotheses are decided by >= 1e-4 at every step: f32 keeps the same ones, with the same ids, lengths
    # and scores; where the final order is decided by >= 1e-4 too, in the same order (else compared as sets)
    # (at least 3/4 of the batch: the count the oracle gives on the CPU -- cfg1 8 of 8, tiny_scaled 4 of 4, 3 of 4 at k = 8)
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    assert 4 * len(ok) >= 3 * len(margins), f"{len(ok)} of {len(margins)} images with a clear selection to compare: margins {margins}"
    for b in ok:
        if margins[b][1] >= 1e-4:
            assert torch.equal(ids_c[b], rid[b]), b
            assert torch.equal(len_c[b], rlen[b]), b
            torch.testing.assert_close(sc_c[b], rsc[b], rtol=1e-5, atol=1e-6)
        else:
            mine = sorted(zip(ids_c[b].tolist(), len_c[b].tolist()))
            want = sorted(zip(rid[b].tolist(), rlen[b].tolist()))
            assert mine == want, b
            torch.testing.assert_close(sc_c[b].sort().values, rsc[b].sort().values, rtol=1e-5, atol=1e-6)
    return ids, lengths


@pytest.mark.parametrize("alpha", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("k", [2, 3, 5, 8])
@pytest.mark.parametrize("case", ["tiny_scaled", "cfg1"])
def test_beam_matches_oracle(dev, case, k, alpha):
    g = Golden(case)
    gp, m = initial_params(g)[0], g.meta
    eng = _engine(m["V"], m["E"], m["H"], m["NL"], 0)
    params = dec_params(gp, dev)
    params[-1] = params[-1].clone()
    params[-1][2] += 1.5                                  # b_out[<E>] offset: some beams finish early, some never
    feats = torch.randn(m["B"], m["E"], generator=torch.Generator().manual_seed(k)).to(dev) * 0.5
    assert eng.beam_fused(m["B"], k) == (case == "cfg1")
    ids, lengths = _check_vs_oracle(eng, params, feats, 12, k, alpha)
    if case == "tiny_scaled" and alpha == 0.0 and k == 5:
        assert (lengths < 12).any() and (lengths == 12).any(), "the eos offset should give early and unfinished beams"


def test_bf16_cfg2_rescored_and_reproducible(dev):
    B, L, V, E, H, k = 64, 20, 10000, 512, 512, 5
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Decoder
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, gen_num_layers=1, compute_dtype="bf16", max_seq_len=L,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(11)
    dec = Decoder(args).to(dev)
    with torch.no_grad():
        dec.linear.weight.mul_(8.0)
        dec.linear.bias[2] += 2.0
    feats = torch.randn(B, E, device=dev)
    ids, scores, lengths = dec.beam_search(feats, beam_size=k, return_beams=True)
    ids2, scores2, lengths2 = dec.beam_search(feats, beam_size=k, return_beams=True)
    torch.cuda.synchronize()
    assert ids.shape == (B, k, L) and scores.shape == (B, k) and lengths.shape == (B, k)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2) and torch.equal(lengths, lengths2)
    assert dec.engine().beam_fused(B, k)
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    for j in range(k):
        row, n = ids[:, j], lengths[:, j].long()
        pos = torch.arange(L, device=dev)[None]
        assert (row[pos >= n[:, None]] == 0).all()
        fin = row.gather(1, (n - 1)[:, None])[:, 0] == 2
        assert (fin | (n == L)).all()
        caps = row[:, :-1].contiguous()
        pred, _ = dec(feats, caps, n.cpu(), pretrain=True)
        logp = torch.log_softmax(pred.float(), dim=-1)
        tok = row[:, :pred.shape[1]]
        lp = logp.gather(2, tok[..., None])[..., 0]
        lp = torch.where(pos[:, :pred.shape[1]] < n[:, None], lp, torch.zeros_like(lp))
        torch.testing.assert_close(lp.sum(1), scores[:, j], rtol=1e-2, atol=1e-2)


def test_bf16_generic_path_reproducible(dev):
    """The generic path (V % 4 != 0) in bf16 at a shape whose products the library would otherwise split over K with f32 atomics
    (gates: M = 48, N = 1024, K = 512): two searches give the same bits."""
    B, L, V, E, H, k = 16, 12, 1001, 256, 256, 3
    eng = _engine(V, E, H, 1, 1)
    params = [t.to(dev) for t in BO.random_params(V, E, H, 1, seed=9, scale=4.0)]
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(8)).to(dev)
    assert not eng.beam_fused(B, k)
    runs = [eng.beam_search(params, feats, L, k) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def _cfg1_generator(dev, cgan):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Generator
    args = default_args(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=512, gen_num_layers=1, compute_dtype="fp32", image_size=64,
                        conditional_gan=cgan, max_seq_len=10, device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(5)
    return Generator(args).to(dev), args


def test_caption_end_to_end(dev):
    gen, _ = _cfg1_generator(dev, 1)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    ids, scores, lengths = gen.caption(images, beam_size=3)
    with torch.no_grad():
        feats = gen.encoder(images)
    ids2, scores2, lengths2 = gen.decoder.beam_search(feats, beam_size=3)
    torch.cuda.synchronize()
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2) and torch.equal(lengths, lengths2)
    gen0, _ = _cfg1_generator(dev, 0)
    ids0, _, _ = gen0.caption(images, beam_size=2)
    assert ids0.shape == (4, 10)


def test_evaluate_bleu(dev):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64,
                        conditional_gan=1, max_seq_len=8, eval_beam_size=3, adv_eval_batch_size=4, num_workers=0,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    score = inst.evaluate("val", beam_size=args.eval_beam_size)
    assert isinstance(score, float) and 0.0 <= score <= 1.0
    assert seen and seen[0][0] == "BLEU4_val" and seen[0][1] == score


def test_attention_decoder_declines(dev):
    from gan_image_captioning_amd.generator import AttnDecoder
    with pytest.raises(NotImplementedError):
        AttnDecoder.beam_search(None, None)


def test_evaluate_groups_coco_captions_per_image(dev):
    """COCO_data: the captions of one image form one reference set, and each image is loaded and decoded once."""
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import SPECIALS, COCO_data
    from gan_image_captioning_amd.training import GANInstructor

    class FakeCoco(COCO_data):
        def __init__(self):
            self.word_to_index = {w: i for i, w in enumerate(SPECIALS)}
            for w in ("a", "cat", "dog", "sits", "runs"):
                self.word_to_index[w] = len(self.word_to_index)
            self.index_to_word = {i: w for w, i in self.word_to_index.items()}
            self.vocab_size = 64
            self.dataset_percent = 1.0
            self.captions = [{"filepath": "val2014", "filename": f"im{i // 3}.jpg", "tokens": t}
                             for i, t in enumerate([["a", "cat", "sits"], ["a", "cat"], ["cat", "sits"], ["a", "dog", "runs"],
                                                    ["dog", "runs"], ["a", "dog", "zebra"]])]
            self.loads = 0

        def __getitem__(self, index):
            self.loads += 1
            g = torch.Generator().manual_seed(index)
            return torch.randn(3, 64, 64, generator=g), [self.word_to_index.get(t, 3) for t in self.captions[index]["tokens"]]

    args = default_args(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64,
                        conditional_gan=1, max_seq_len=6, adv_eval_batch_size=4, num_workers=0,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    ds = FakeCoco()
    inst = GANInstructor(args, None, ds)
    from gan_image_captioning_amd import utils
    seen = {}
    real = utils.bleu_score

    def spy(c, r):
        seen["c"], seen["r"] = c, r
        return real(c, r)

    utils.bleu_score = spy
    try:
        score = inst.evaluate("val", beam_size=2)
    finally:
        utils.bleu_score = real
    assert 0.0 <= score <= 1.0
    assert ds.loads == 2
    assert len(seen["c"]) == 2
    assert seen["r"][0] == [["a", "cat", "sits"], ["a", "cat"], ["cat", "sits"]]
    assert seen["r"][1] == [["a", "dog", "runs"], ["dog", "runs"], ["a", "dog", "<UNK>"]]
