"""The evaluations on a decode-time ensemble (--eval-ensemble*; GANInstructor.ensemble, generator.Ensemble) end to end on a tiny
synthetic configuration: the EMA member, a checkpoint member, an ensemble of the live model with itself, and the defaults."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64, conditional_gan=1,
                max_seq_len=8, adv_eval_batch_size=4, pre_eval_batch_size=4, num_workers=0, device="cuda", log_file=None, model_dir=None,
                save_dir=None)
    base.update(kw)
    return default_args(**base)


def _instructor(seed=4, **kw):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    torch.manual_seed(seed)
    inst = GANInstructor(_args(**kw), ds, ds)
    with torch.no_grad():
        inst.gen.decoder.linear.weight.mul_(6.0)             # peaked enough that no caption hangs on a rounding
    from gan_image_captioning_amd import engine
    engine.bump_param_epoch()
    if inst.ema is not None:
        inst.ema.reset()                                     # the average starts from the weights as they are now
    inst.writer.add_scalar = lambda tag, v, step: None
    return inst


def _all(inst):
    return {"bleu": inst.evaluate("val", beam_size=3), "metrics": inst.evaluate_metrics("val", beam_size=3),
            "diversity": inst.evaluate_diversity("val", num_samples=3, top_k=10, top_p=0.9),
            "perplexity": inst.evaluate_perplexity("val")}


def _close(a, b, tol=1e-4):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _close(a[k], b[k], tol)
    else:
        assert a == pytest.approx(b, rel=tol, abs=tol), (a, b)


def test_defaults_construct_nothing(dev):
    inst = _instructor()
    assert inst.eval_ensemble is None
    out = _all(inst)
    assert inst._ensemble is None and inst._eval_gen() is inst.gen
    assert out == _all(inst)                                   # and the evaluations repeat themselves


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_ema_member_and_the_live_model_with_itself(dev, mode):
    """Before any optimizer step the average IS the live weights: --eval-ensemble-ema 1 then evaluates the live model ensembled with
    itself, which reports the live model's numbers, through every evaluation that decodes or scores."""
    from gan_image_captioning_amd.generator import Ensemble
    plain = _all(_instructor())
    inst = _instructor(gen_ema_decay=0.9, eval_ensemble_ema=1, eval_ensemble_mode=mode, eval_ensemble_weights=[0.7, 0.3])
    got = _all(inst)
    ens = inst._ensemble
    assert isinstance(ens, Ensemble) and len(ens.members) == 2 and ens.members[0] is inst.gen
    assert ens.members[1].encoder.resnet is inst.gen.encoder.resnet            # the EMA copy sits on the live trunk
    assert ens.mode == mode and ens.weights == [0.7, 0.3]
    for p, q in zip(ens.members[1].decoder.param_list(), inst.gen.decoder.param_list()):
        assert torch.equal(p, q) and p.data_ptr() != q.data_ptr()
    _close(got, plain)
    with inst._live_weights():                                 # checkpoint selection stays on the live generator
        assert inst._eval_gen() is inst.gen
    assert inst.gen.training == ens.members[1].training


def test_checkpoint_member_runs_every_evaluation(dev, tmp_path):
    other = _instructor(seed=9)
    path = str(tmp_path / "pretrained_model.ckpt")
    torch.save(other.gen.state_dict(), path)
    adv = str(tmp_path / "adv_model.ckpt")
    torch.save({"generator": other.gen.state_dict(), "discriminator": other.disc.state_dict()}, adv)
    inst = _instructor(eval_ensemble=[path, adv])
    out = _all(inst)
    ens = inst._ensemble
    assert len(ens.members) == 3 and ens.members[0] is inst.gen and ens.weights is None and ens.mode == "prob"
    for m in ens.members[1:]:                                  # both checkpoint formats hold the other model's weights
        for p, q in zip(m.decoder.param_list(), other.gen.decoder.param_list()):
            assert torch.equal(p, q)
    assert 0.0 <= out["bleu"] <= 1.0 and set(out["metrics"]) == {"bleu1", "bleu2", "bleu3", "bleu4", "rouge_l", "cider_d"}
    assert set(out["diversity"]) == {"bleu4", "mbleu4", "distinct1", "distinct2", "vocab"}
    ppl = out["perplexity"]
    assert ppl["captions"] == 6 and ppl["tokens"] > 0 and math.isfinite(ppl["perplexity"]) and ppl["perplexity"] > 1.0
    # (Jensen: log sum_m w_m p_m >= sum_m w_m log p_m, so the mixture's nll is at most the worst member's)
    with inst._live_weights():
        live = inst.evaluate_perplexity("val")["nll_per_token"]
    assert ppl["nll_per_token"] <= max(live, other.evaluate_perplexity("val")["nll_per_token"]) + 1e-6
    assert out == _all(inst)
