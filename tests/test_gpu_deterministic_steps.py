"""Deterministic mode, whole steps: three optimizer steps run twice from one snapshot of all state (parameter arenas, Adam moments
and step counters, BatchNorm running buffers, the device-noise seed counter, the temperature) give torch.equal sampled ids, losses,
gradients, master weights, Adam moments and running statistics; and the existing parity tests of the rewritten kernel families
still hold with the mode on (the reference tolerances of those tests)."""
import pytest
import torch

from tests import test_gpu_kernels as K
from tests import test_gpu_seqgan as SG
from tests import test_gpu_step as ST
from tests import test_gpu_training as TR
from tests.step_state import _restore, _snapshot, _state
from tests.test_gpu_kernels import E, dev  # noqa: F401  (fixtures of the reused kernel tests)

pytestmark = pytest.mark.gpu


@pytest.fixture
def det():
    from gan_image_captioning_amd import engine
    before = engine.deterministic()
    engine.set_deterministic(True)
    yield
    engine.set_deterministic(before)


def _run(inst, step, n=3):
    rec = []
    for k in range(n):
        out = step(k)
        torch.cuda.synchronize()
        r = {"out." + key: v.detach().clone() for key, v in out.items()}
        r.update({key: v.detach().clone() for key, v in _state(inst).items()})
        rec.append(r)
    return rec


def _twice(inst, step, n=3):
    snap = _snapshot(inst)
    a = _run(inst, step, n)
    _restore(inst, snap)
    b = _run(inst, step, n)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for key in ra:
            assert torch.equal(ra[key], rb[key]), f"step {k}: {key} differs between two runs from one snapshot"
            if ra[key].is_floating_point():
                assert torch.isfinite(ra[key]).all(), f"step {k}: {key} not finite"
    return a


def _bench_instructor(dtype, encoder, cgan, real_as_ids=1, **extra):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import synthetic_batch
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(vocab_size=10000, gen_embed_dim=512, gen_hidden_dim=512, gen_num_layers=1, conditional_gan=cgan,
                        encoder_arch=encoder, compute_dtype=dtype, step_impl="fused", adv_train_batch_size=64, image_size=224,
                        real_as_ids=real_as_ids, deterministic=1, device="cuda", log_file=None, model_dir=None, save_dir=None, **extra)
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    inst.disc.train()
    images, caps, _lengths, L = synthetic_batch(64, 10000, 224, 20, seed=1008, device=args.device, with_images=bool(cgan))
    return inst, images, caps, L


@pytest.mark.parametrize("dtype,encoder,cgan", [("bf16", "resnet50", 1), ("fp32", "resnet18", 1), ("bf16", "resnet50", 0)])
def test_fused_steps_at_bench_shapes_repeat_bit_for_bit(det, dtype, encoder, cgan):
    # B=64, L=20, V=10000, E=H=512, R=64, F=900, device-drawn noise; D backward at gy = 64 (2B*R = 8192 rows)
    inst, images, caps, L = _bench_instructor(dtype, encoder, cgan)

    def step(k):
        out = inst.fused(images, caps, L, True, None, None)
        return {"losses": out["losses"], "ids": out["ids"]}
    _twice(inst, step)


def test_seqgan_steps_repeat_bit_for_bit(det):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import synthetic_batch
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(vocab_size=1000, gen_embed_dim=64, gen_hidden_dim=64, gen_num_layers=1, conditional_gan=0, adv_mode="seqgan",
                        mc_rollouts=4, adv_train_batch_size=16, compute_dtype="bf16", deterministic=1, device="cuda", log_file=None,
                        model_dir=None, save_dir=None)
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    inst.disc.train()
    _, caps, _, L = synthetic_batch(16, 1000, 224, 12, seed=7, device=args.device, with_images=False)
    _twice(inst, lambda k: {"losses": inst.adv_step(None, caps, L, True)})


def test_pretrain_steps_repeat_bit_for_bit(det):
    inst, images, caps, L = _bench_instructor("bf16", "resnet50", 1)
    _twice(inst, lambda k: {"loss": inst.pretrain_step(images, caps, L, True).reshape(-1)})


@pytest.mark.parametrize("impl", ["autograd", "fused"])
@pytest.mark.parametrize("real_as_ids", [0, 1])
def test_tiny_golden_steps_repeat_bit_for_bit(det, impl, real_as_ids):
    from tests.golden_io import Golden, initial_params
    g = Golden("tiny")
    m = g.meta
    inst, args = ST.make_instructor(m, impl, real_as_ids=real_as_ids)
    gp, dp = initial_params(g)
    ST.load_params(inst, gp, dp)
    inst.gen.train()
    inst.disc.train()
    caps = g.t("caps").to(args.device)
    _twice(inst, lambda k: {"losses": inst.adv_step(None, caps, m["L"], True)})


# ---- the existing parity tests, with the mode on
@pytest.mark.parametrize("impl", ["fused", "autograd"])
@pytest.mark.parametrize("name", ["tiny", "tiny_rep2", "cfg1"])
def test_adv_step_matches_reference_in_deterministic_mode(det, name, impl):
    ST.test_adv_step_matches_reference(name, impl)


@pytest.mark.parametrize("name", ["tiny", "tiny_rep2", "cfg1"])
def test_disc_bwd_matches_reference_in_deterministic_mode(det, E, dev, name):  # noqa: F811
    K.test_disc_bwd_f32(E, dev, name)


def test_embedding_bwd_matches_reference_in_deterministic_mode(det, E, dev):  # noqa: F811
    K.test_embedding_fwd_bwd(E, dev)


def test_seqgan_step_matches_oracle_in_deterministic_mode(det):
    SG.test_seqgan_step_f32_matches_oracle((4, 5, 52, 8, 16, 1, 3))


def test_pretrain_step_matches_reference_in_deterministic_mode(det):
    TR.test_pretrain_step_matches_reference()


def test_attention_entry_points_refuse_the_mode(det):
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(decoder="attention", conditional_gan=1, device="cuda", log_file=None, model_dir=None, save_dir=None)
    with pytest.raises(ValueError, match="attention"):
        GANInstructor(args, None, None)
    assert L.load().gic_attn_sample_bwd(None, None, None, None, None, None, None, None, None, 1.0, 0, None, None, None) == L.ERR_UNSUPPORTED
