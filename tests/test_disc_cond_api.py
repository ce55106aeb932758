"""The image-conditioned discriminator (--disc-cond projection) without a GPU: flag validation, state-dict keys, the new entry points'
argument checks, and the self-test of the oracle the GPU tests compare with (tests/disc_cond_oracle.py): its hand-written gradients
against torch.autograd through its own fp64 forward."""
import ctypes as C

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd.args import default_args
from gan_image_captioning_amd.discriminator import Discriminator
from oracle import cpu_step as O
from tests import disc_cond_oracle as DC

TINY = dict(vocab_size=50, disc_embed_dim=4, disc_num_rep=4, disc_filter_sizes=[2, 3], disc_num_filters=[24, 16], device="cpu")
TODAY = ["embeddings.weight", "convs.0.weight", "convs.0.bias", "convs.1.weight", "convs.1.bias", "highway.weight", "highway.bias",
         "feature2out.weight", "feature2out.bias", "out2logits.weight", "out2logits.bias"]


def test_flags_exist_with_their_defaults():
    a = default_args()
    assert (a.disc_cond, a.disc_mismatch_weight, a.eval_match) == ("none", 0.5, 0)


def test_projection_needs_a_conditional_gan():
    with pytest.raises(ValueError, match="conditional-gan 1"):
        Discriminator(default_args(disc_cond="projection", conditional_gan=0, **TINY))


def test_projection_refuses_seqgan_and_names_the_follow_up():
    with pytest.raises(ValueError, match="follow-up"):
        Discriminator(default_args(disc_cond="projection", conditional_gan=1, adv_mode="seqgan", **TINY))


def test_projection_refuses_dense_real_captions_and_bad_weights():
    with pytest.raises(ValueError, match="real-as-ids"):
        Discriminator(default_args(disc_cond="projection", conditional_gan=1, real_as_ids=0, **TINY))
    for w in (-0.1, 1.0):
        with pytest.raises(ValueError, match="disc-mismatch-weight"):
            Discriminator(default_args(disc_cond="projection", conditional_gan=1, disc_mismatch_weight=w, **TINY))


def test_mismatch_needs_two_captions_at_the_step():
    """The check precedes every device call of both step drivers: a batch of one caption has no other image."""
    from gan_image_captioning_amd.fused_step import FusedAdvStep
    from gan_image_captioning_amd.training import GANInstructor

    class Cap:
        shape = (1, 6)
        is_cuda = True

    class Disc:
        cond = "projection"

        def engine(self):
            return None

    class Gen:
        class decoder:
            temperature = 1.0

            @staticmethod
            def engine():
                return None

    args = default_args(disc_cond="projection", conditional_gan=1, **TINY)
    step = FusedAdvStep(Gen(), Disc(), None, None, args)
    with pytest.raises(ValueError, match="at least two captions"):
        step(Cap(), Cap(), 6)
    inst = GANInstructor.__new__(GANInstructor)
    inst.args, inst.disc = args, Disc()
    with pytest.raises(ValueError, match="at least two captions"):
        inst._adv_step_autograd(None, Cap(), 6, True)
    step.mismatch_w = 0.0                      # w = 0: no such requirement (the step goes on to the device, which a CPU tensor refuses)
    with pytest.raises(Exception) as e:
        step(Cap(), Cap(), 6)
    assert "at least two captions" not in str(e.value)


def test_state_dict_keys_off_and_on():
    off = Discriminator(default_args(**TINY))
    assert list(off.state_dict()) == TODAY and len(off.param_list()) == len(TODAY)
    off.load_state_dict({k: torch.zeros_like(v) for k, v in O.make_disc_params(50, torch.Generator().manual_seed(0), 4, 4, (2, 3), (24, 16)).items()})
    on = Discriminator(default_args(disc_cond="projection", conditional_gan=1, **TINY))
    assert list(on.state_dict()) == TODAY + ["img_proj.weight", "img_proj.bias"]
    assert tuple(on.img_proj.weight.shape) == (40, 512) and tuple(on.img_proj.bias.shape) == (40,)
    assert [id(p) for p in on.param_list()[-2:]] == [id(on.img_proj.weight), id(on.img_proj.bias)]
    assert [id(p) for p in on.text_param_list()] == [id(p) for p in on.param_list()[:-2]]
    assert float(on.img_proj.weight.detach().abs().max()) <= 0.05            # init_params' rule (uniform +-0.05), like the other parameters
    r50 = Discriminator(default_args(disc_cond="projection", conditional_gan=1, encoder_arch="resnet50", **TINY))
    assert tuple(r50.img_proj.weight.shape) == (40, 2048)


def test_image_features_required_or_refused():
    x = torch.zeros(2, 6, dtype=torch.int64)
    with pytest.raises(ValueError, match="without --disc-cond projection"):
        Discriminator(default_args(**TINY))(x, image_features=torch.zeros(2, 512))
    with pytest.raises(ValueError, match="needs image_features"):
        Discriminator(default_args(disc_cond="projection", conditional_gan=1, **TINY))(x)


def _dims(B=2, R=4, F=40, Fp=64, dtype=L.F32):
    d = L.DiscDims()
    d.B, d.L, d.V, d.De, d.R, d.nconv = B, 6, 50, 4, R, 2
    d.fsize[0], d.fsize[1], d.nfilt[0], d.nfilt[1] = 2, 3, 24, 16
    d.F, d.Fp, d.dtype, d.drop_p = F, Fp, dtype, 0.2
    return d


def _err():
    return L.load().gic_last_error().decode()


def test_new_entry_points_are_exported_and_the_abi_version_stands():
    for name in ("gic_disc_match_fwd", "gic_disc_bwd_cond", "gic_gan_losses_mismatch"):
        assert name in L.EXPORTED_SYMBOLS
    assert L.load().gic_abi_version() == 5


def test_match_fwd_rejects_null_and_bad_arguments():
    lib = L.load()
    buf = (C.c_float * 1024)()
    ok = C.addressof(buf) + (-C.addressof(buf)) % 16
    st = L.DiscState()
    st.ydrop = ok
    assert lib.gic_disc_match_fwd(None, C.byref(st), ok, 1.0, 0, ok, None) == -1 and "null dims" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims()), None, ok, 1.0, 0, ok, None) == -1 and "null argument" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims()), C.byref(st), None, 1.0, 0, ok, None) == -1 and "null argument" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims()), C.byref(st), ok, 1.0, 0, None, None) == -1 and "null argument" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims()), C.byref(L.DiscState()), ok, 1.0, 0, ok, None) == -1 and "ydrop" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims(B=0)), C.byref(st), ok, 1.0, 0, ok, None) == -1 and "B=0" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims(Fp=60)), C.byref(st), ok, 1.0, 0, ok, None) == -1 and "multiple of 8" in _err()
    assert lib.gic_disc_match_fwd(C.byref(_dims()), C.byref(st), ok, float("nan"), 0, ok, None) == -1 and "NaN" in _err()


def test_bwd_cond_and_the_loss_mix_reject_null_and_bad_arguments():
    lib = L.load()
    buf = (C.c_float * 64)()
    ok = C.addressof(buf)
    d = _dims()
    assert lib.gic_disc_bwd_cond(C.byref(d), None, None, None, None, None, 50, None, 1, None, None, 0, None, 50, ok, 1.0, None, None) == -1
    assert "disc_bwd_cond: null argument" in _err()
    assert lib.gic_disc_bwd_cond(None, None, None, None, None, None, 50, None, 1, None, None, 0, None, 50, ok, 1.0, None, None) == -1
    assert "null dims" in _err()
    assert lib.gic_disc_bwd(C.byref(d), None, None, None, None, None, 50, None, 1, None, None, 0, None, 50, None) == -1
    assert "disc_bwd: null argument" in _err()                      # the plain entry keeps its own name in its messages
    assert lib.gic_gan_losses_mismatch(0.5, 4, None, ok, None, None, None, None, None) == -1 and "null losses" in _err()
    assert lib.gic_gan_losses_mismatch(1.0, 4, ok, ok, None, None, None, None, None) == -1 and "[0, 1)" in _err()
    assert lib.gic_gan_losses_mismatch(0.5, 4, ok, ok, ok, None, None, None, None) == -1 and "all four" in _err()


def test_engine_refuses_a_q_that_is_not_f32_before_the_device_is_touched():
    from gan_image_captioning_amd import engine

    class Q:
        is_cuda, dtype, shape = True, torch.bfloat16, (2, 40)

    eng = engine.DiscEngine(50, 4, 4, [2, 3], [24, 16], L.F32)
    with pytest.raises(ValueError, match="float32"):
        eng._check_cond(Q(), 2)


# ------------------------------------------------------------------------------------------------ oracle self-test (fp64, CPU)
def _setup(B=3, R=4, L_=7, V=20, C_=12, seed=5):
    g = torch.Generator().manual_seed(seed)
    dp = {k: (4.0 * v).double() for k, v in O.make_disc_params(V, g, R, R, (2, 3), (9, 6)).items()}
    F = 15
    dp["img_proj.weight"] = torch.randn(F, C_, generator=g).double() / C_ ** 0.5
    dp["img_proj.bias"] = 0.1 * torch.randn(F, generator=g).double()
    inp = torch.softmax(2 * torch.randn(B, L_, V, generator=g), -1).double()
    pooled = torch.randn(B, C_, generator=g).double()
    mask = torch.empty(B * R, F).bernoulli_(0.8, generator=g).double()
    return g, dp, inp, pooled, mask, B, R, F


def test_oracle_match_gradients_equal_autograd():
    g, dp, inp, pooled, mask, B, R, F = _setup()
    leaf = {k: v.clone().requires_grad_(True) for k, v in dp.items()}
    x = inp.clone().requires_grad_(True)
    base, st = O.disc_forward(leaf, x, mask, R, return_stages=True)
    y = st["highway"] * (mask / (1.0 - O.DROPOUT_P))
    y.retain_grad()
    q = pooled @ leaf["img_proj.weight"].t() + leaf["img_proj.bias"]
    q.retain_grad()
    logits = base + DC.match_term(y, q, R)
    assert torch.allclose(logits, DC.disc_forward(dp, inp, pooled, mask, R), rtol=1e-13, atol=1e-15)
    gl = torch.randn(B * R, generator=g).double()
    (logits * gl).sum().backward()
    d_y, d_q = DC.match_backward(y.detach(), q.detach(), gl, R)
    torch.testing.assert_close(y.grad, d_y, rtol=1e-12, atol=1e-15)      # (this y feeds the match term alone: the head has its own copy)
    torch.testing.assert_close(q.grad, d_q, rtol=1e-12, atol=1e-15)
    d_w, d_b = DC.img_proj_backward(d_q, pooled)
    torch.testing.assert_close(leaf["img_proj.weight"].grad, d_w, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(leaf["img_proj.bias"].grad, d_b, rtol=1e-12, atol=1e-15)
    assert x.grad is not None and float(x.grad.abs().max()) > 0      # G's path: the input gradient flows through d_y


@pytest.mark.parametrize("loss_type", DC.LOSS_TYPES)
def test_oracle_loss_mix_gradients_equal_autograd(loss_type):
    g = torch.Generator().manual_seed(11)
    r, f, wr, go = (torch.randn(12, generator=g).double().requires_grad_(True) for _ in range(4))
    w = 0.3
    g_loss, d_loss = DC.d_loss_mix(r, f, wr, go, loss_type, w)
    g_plain, d_plain = O.get_losses(r, f, go, loss_type)
    assert float(g_loss.detach()) == float(g_plain.detach())                           # g_loss is unchanged
    gr, gf, gw = torch.autograd.grad(d_loss, [r, f, wr], allow_unused=True)
    d_ref, hr, hf, hw = DC.d_loss_mix_grads(r, f, wr, go, loss_type, w)
    torch.testing.assert_close(d_loss.detach(), d_ref, rtol=1e-13, atol=0)
    for got, want in ((gr, hr), (gf, hf), (gw, hw)):
        torch.testing.assert_close(got if got is not None else torch.zeros_like(want), want, rtol=1e-12, atol=1e-16)
    if loss_type == "standard":                                      # GAN-CLS: BCE(real, 1) + (1 - w) BCE(fake, 0) + w BCE(wrong, 0)
        cls = O.bce_logits_mean(r, True) + (1 - w) * O.bce_logits_mean(f, False) + w * O.bce_logits_mean(wr, False)
        torch.testing.assert_close(d_loss, cls, rtol=1e-13, atol=0)
    _, d0 = DC.d_loss_mix(r, f, None, go, loss_type, 0.0)
    assert float(d0.detach()) == float(d_plain.detach())                               # w = 0: d(real, fake), no third pass


def test_oracle_evaluate_match_counts_ties_as_losses():
    g, dp, inp, pooled, mask, B, R, F = _setup()
    caps = torch.randint(0, 20, (B, 7), generator=g)
    out = DC.evaluate_match(dp, [(pooled, caps), (DC.roll(pooled), caps)], R)
    assert 0.0 <= out["pair_acc"] <= 1.0 and out["margin"] != 0.0
    dp0 = dict(dp)
    dp0["img_proj.weight"] = torch.zeros_like(dp["img_proj.weight"])
    assert DC.evaluate_match(dp0, [(pooled, caps)], R) == {"pair_acc": 0.0, "margin": 0.0}
