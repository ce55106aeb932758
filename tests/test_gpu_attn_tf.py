"""Teacher-forced decode with the attention decoder on the GPU (gic_attn_forward_tf / gic_attn_forward_tf_bwd, AttnDecoder.forward,
Generator.forward, --pretrain-mode teacher / --attn-reg) against the float64 oracle (tests/attn_tf_oracle.py).  Tolerances: f32 those of
tests/test_gpu_attention.py (outputs rtol 1e-4, gradients rtol 2e-3); bf16 at cfg4 those of test_attention_decoder_bf16_at_cfg4_shapes."""
import pytest
import torch

from oracle import cpu_step as O
from tests import attn_beam_oracle as AO
from tests import attn_tf_oracle as TF
from tests.gpu_util import close, rel_l2

pytestmark = pytest.mark.gpu

NAMES = ["decoder." + n for n in AO.NAMES]
SMALL = (5, 7, 64, 32, 32, 64, 9, 32)                    # B, T, V, E, H, C, P, A
LENS = [4, 7, 1, 6, 3]                                   # unsorted, with 1 and T
CFG4 = (32, 20, 10000, 512, 512, 2048, 49, 512)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _engine(shape, dt):
    from gan_image_captioning_amd import engine
    return engine.AttnDecoderEngine(*shape[2:], dt)


def _problem(shape, seed, scale=6.0):
    B, T, V, E, H, C, P, A = shape
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=scale)
    g = torch.Generator().manual_seed(seed + 1)
    caps = torch.randint(0, V, (B, T - 1), generator=g)
    return params, feats, fmap, caps, g


def _oracle(params, feats, fmap, caps, lens, T_, pretrain, u, d_pred, d_alphas, dtype=torch.float64):
    """(pred, (h_n, c_n), alphas, grads in NAMES order + d features) of loss = sum(pred * d_pred) + sum(alphas * d_alphas)."""
    leaf = {n: p.to(dtype).clone().requires_grad_(True) for n, p in zip(NAMES, params)}
    f_leaf = feats.to(dtype).clone().requires_grad_(True)
    pred, hc, alphas = TF.forward_tf(leaf, f_leaf, fmap.to(dtype), caps, lens, T_, pretrain, None if u is None else u.to(dtype))
    loss = (pred * d_pred.to(dtype)).sum()
    if d_alphas is not None:
        loss = loss + (alphas * d_alphas.to(dtype)).sum()
    loss.backward()
    return pred.detach(), hc, alphas.detach(), [leaf[n].grad for n in NAMES] + [f_leaf.grad]


@pytest.mark.parametrize("pretrain", [True, False], ids=["logits", "gumbel"])
def test_f32_matches_oracle(dev, pretrain):
    B, T, V = SMALL[:3]
    params, feats, fmap, caps, g = _problem(SMALL, 11)
    Tm = max(LENS)
    u = torch.rand(B, Tm, V, generator=g)
    d_pred = torch.randn(B, Tm, V, generator=g) * (0.1 if pretrain else 1.0)
    d_alphas = torch.randn(B, Tm, SMALL[6], generator=g)
    T_ = 1.0 if pretrain else 1.3
    want, (h_w, c_w), al_w, g_w = _oracle(params, feats, fmap, caps, LENS, T_, pretrain, None if pretrain else u, d_pred, d_alphas)
    eng = _engine(SMALL, 0)
    pd = [p.to(dev) for p in params]
    pred, (h_n, c_n), alphas, saved = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), LENS, T_, pretrain,
                                                     None if pretrain else u.to(dev), want_alphas=True, keep_state=True)
    grads = eng.forward_tf_bwd(pd, saved, pred, d_pred.to(dev), T_, pretrain, d_alphas=d_alphas.to(dev))
    torch.cuda.synchronize()
    close(pred, want, rtol=1e-4, atol_scale=1e-5 if pretrain else 1e-6, what="pred")
    close(alphas, al_w, rtol=1e-4, atol_scale=1e-6, what="alphas")
    close(h_n[0], h_w, rtol=1e-4, atol_scale=1e-6, what="h_n")
    close(c_n[0], c_w, rtol=1e-4, atol_scale=1e-6, what="c_n")
    for n, got, w in zip(NAMES + ["d_features"], grads, g_w):
        close(got, w, rtol=2e-3, atol_scale=1e-4, what=n)


def test_padded_positions(dev):
    B, T, V = SMALL[:3]
    params, feats, fmap, caps, g = _problem(SMALL, 12)
    eng = _engine(SMALL, 0)
    pd = [p.to(dev) for p in params]
    pred, _, alphas, saved = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), LENS, 1.0, True, want_alphas=True,
                                            keep_state=True)
    Tm = max(LENS)
    pad = torch.arange(Tm)[None] >= torch.tensor(LENS)[:, None]                  # [B, Tm]
    assert pad.any()
    assert (alphas.cpu()[pad] == 0).all()
    assert torch.equal(pred.cpu()[pad], params[6].expand(int(pad.sum()), -1))
    # a loss on padded rows alone reaches b_out only
    d_pred = torch.randn(B, Tm, V, generator=g) * pad[..., None]
    d_alphas = torch.randn(B, Tm, SMALL[6], generator=g) * pad[..., None]
    grads = eng.forward_tf_bwd(pd, saved, pred, d_pred.to(dev), 1.0, True, d_alphas=d_alphas.to(dev))
    torch.cuda.synchronize()
    for n, gr in zip(NAMES + ["d_features"], grads):
        if n == "decoder.linear.bias":
            close(gr, d_pred.sum((0, 1)), rtol=1e-5, what=n)
        else:
            assert (gr == 0).all(), n


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_greedy_caps_reproduce_sample_fwd(dev, dt):
    B, T = SMALL[:2]
    params, feats, fmap, _, _ = _problem(SMALL, 13)
    eng = _engine(SMALL, dt)
    pd, f, m = [p.to(dev) for p in params], feats.to(dev), fmap.to(dev)
    out, ids, st = eng.sample_fwd(pd, f, m, T, 1.0, pretrain=True)
    pred, (h_n, c_n), alphas = eng.forward_tf(pd, f, m, ids[:, :-1], [T] * B, 1.0, True, want_alphas=True)
    torch.cuda.synchronize()
    Em, C = SMALL[3], SMALL[5]
    pairs = [(pred.float(), out.float(), "pred"), (alphas, st["alpha"].permute(1, 0, 2), "alphas"),
             (h_n[0], st["xh"][T][:, Em + C:].float(), "h_n"), (c_n[0], st["c"][T], "c_n")]
    for got, want, what in pairs:
        if dt == 0:
            close(got, want, rtol=1e-5, atol_scale=1e-5, what=what)
        else:                                             # bf16: the two paths round z and the hp / vocabulary sums differently
            assert rel_l2(got, want) < 2e-2, what


def test_bf16_at_cfg4_shapes(dev):
    B, T, V = CFG4[:3]
    params, feats, fmap, caps, g = _problem(CFG4, 7, scale=1.0)
    params[5] = params[5] * 20.0
    lens = torch.randint(8, T + 1, (B,), generator=g).tolist()
    lens[0] = T
    Tm = max(lens)
    u = torch.rand(B, Tm, V, generator=g)
    d_pred = torch.randn(B, Tm, V, generator=g) * 1e-3
    d_alphas = torch.randn(B, Tm, CFG4[6], generator=g) * 1e-2
    T_ = 1.7
    eng = _engine(CFG4, 1)
    pd = [p.to(dev) for p in params]
    pred, _, alphas, saved = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), lens, T_, False, u.to(dev), want_alphas=True,
                                            keep_state=True)
    grads = eng.forward_tf_bwd(pd, saved, pred, d_pred.to(dev), T_, False, d_alphas=d_alphas.to(dev))
    logits, _, _ = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), lens, 1.0, True)
    torch.cuda.synchronize()
    want, _, al_w, g_w = _oracle(params, feats, fmap, caps, lens, T_, False, u, d_pred, d_alphas, dtype=torch.float32)
    with torch.no_grad():
        lg_w, _, _ = TF.forward_tf(dict(zip(NAMES, params)), feats, fmap, caps, lens, pretrain=True)
    live = torch.arange(Tm)[None] < torch.tensor(lens)[:, None]
    match = float((logits.float().cpu().argmax(-1) == lg_w.argmax(-1))[live].float().mean())
    assert match >= 0.9, match
    assert rel_l2(pred.float(), want) < 5e-2
    assert rel_l2(alphas, al_w) < 5e-2
    errs = {n: rel_l2(gr, w) for n, gr, w in zip(NAMES + ["d_features"], grads, g_w)}
    print("bf16 teacher-forced rel-L2 gradient errors:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-1, errs


def _run_twice(eng, pd, f, m, caps, lens, backward):
    outs = []
    for _ in range(2):
        pred, (h_n, c_n), alphas, saved = eng.forward_tf(pd, f, m, caps, lens, 1.2, False, None, seed=5, want_alphas=True, keep_state=True)
        res = [pred, h_n, c_n, alphas]
        if backward:
            d = torch.ones_like(pred) * 1e-3
            res += eng.forward_tf_bwd(pd, saved, pred, d, 1.2, False, d_alphas=alphas.detach() * 0.5)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in res])
    return outs


def test_repeated_calls_give_the_same_bits(dev):
    from gan_image_captioning_amd import engine
    shape = (32, 12, 1000, 64, 128, 256, 49, 64)
    params, feats, fmap, caps, g = _problem(shape, 14, scale=1.0)
    lens = torch.randint(1, shape[1] + 1, (shape[0],), generator=g).tolist()
    eng = _engine(shape, 1)
    args = ([p.to(dev) for p in params], feats.to(dev), fmap.to(dev), caps.to(dev), lens)
    a, b = _run_twice(eng, *args, backward=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    engine.set_deterministic(True)
    try:
        a, b = _run_twice(eng, *args, backward=True)
    finally:
        engine.set_deterministic(False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


def _args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=16, gen_hidden_dim=32, conditional_gan=1, encoder_arch="resnet18", attn_dim=24,
                compute_dtype="fp32", image_size=64, device="cuda", log_file=None, model_dir=None, save_dir=None)
    base.update(kw)
    return default_args(**base)


def _batch(B, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = O.make_captions(B, L, V, g)
    lengths = torch.randint(3, L + 1, (B,), generator=g, dtype=torch.int32)
    lengths[0] = L
    for b in range(B):                                    # tasks.collate_fn's layout: <S> body <E> then PAD
        n = int(lengths[b])
        caps[b, n - 1] = 2
        caps[b, n:] = 0
    return images, caps, lengths


def test_generator_forward_with_attention(dev):
    from gan_image_captioning_amd.generator import Generator
    args = _args(decoder="attention")
    gen = Generator(args).to(args.device)
    gen.train()
    images, caps, lengths = _batch(4, 6, 64, 1)
    pred, (h_n, c_n) = gen(images.to(dev), caps[:, :-1].to(dev), lengths, pretrain=True)
    (pred.float() ** 2).sum().backward()
    torch.cuda.synchronize()
    assert pred.shape == (4, 6, 64) and h_n.shape == (1, 4, 32)
    gw = gen.encoder.linear.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().sum() > 0
    assert gen.decoder.attn.w_f.grad.abs().sum() > 0


@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_teacher_pretrain_step_matches_oracle(dev, decoder):
    from gan_image_captioning_amd.training import GANInstructor
    lam = 0.7 if decoder == "attention" else 0.0
    inst = GANInstructor(_args(decoder=decoder, pretrain_mode="teacher", attn_reg=lam), None, None)
    B, L, V = 6, 7, 64
    images, caps, lengths = _batch(B, L, V, 2)
    with torch.no_grad():
        for p in inst.gen.decoder.parameters():
            p.mul_(8.0)
    inst.gen.train()
    dec = inst.gen.decoder
    params = list(dec.parameters())
    with torch.enable_grad():
        feats = inst._features(images.to(dev), B)
        loss = inst._pretrain_step_teacher(feats, caps.to(dev), lengths, train=False)
        grads = torch.autograd.grad(loss, params)
    torch.cuda.synchronize()
    gp = {"decoder." + k: v.detach().cpu().double().requires_grad_(True) for k, v in dec.state_dict().items()}
    names = ["decoder." + k for k, _ in dec.named_parameters()]
    if decoder == "attention":
        f, m = feats[0].detach().cpu().double(), feats[1].detach().cpu().double()
        pred, _, alphas = TF.forward_tf(gp, f, m, caps[:, :-1], lengths.tolist(), pretrain=True)
    else:
        pred, _ = O.decoder_forward_tf(gp, feats.detach().cpu().double(), caps[:, :-1], lengths.tolist(), 1.0, pretrain=True)
    want = torch.nn.functional.cross_entropy(pred.reshape(-1, V), caps.reshape(-1))
    if lam:
        want = want + TF.attn_reg(alphas, lam)
    gw = torch.autograd.grad(want, [gp[n] for n in names])
    assert float(loss) == pytest.approx(float(want), rel=1e-5)
    for n, got, w in zip(names, grads, gw):
        close(got, w, rtol=2e-3, atol_scale=1e-4, what=n)
    if lam:                                               # the penalty's own gradient
        gr = torch.autograd.grad(TF.attn_reg(TF.forward_tf(gp, f, m, caps[:, :-1], lengths.tolist(), pretrain=True)[2], lam),
                                 [gp["decoder.attn.w_h"]])[0]
        with torch.enable_grad():
            _, _, al = dec(feats[0].detach(), feats[1], caps[:, :-1].to(dev), lengths, pretrain=True, return_alphas=True)
            got = torch.autograd.grad(TF.attn_reg(al, lam), [dec.attn.w_h])[0]
        close(got, gr, rtol=2e-3, atol_scale=1e-4, what="attn-reg d w_h")


def test_teacher_steps_lower_the_loss(dev):
    from gan_image_captioning_amd.training import GANInstructor
    inst = GANInstructor(_args(decoder="attention", pretrain_mode="teacher", attn_reg=0.1), None, None)
    images, caps, lengths = _batch(8, 7, 64, 3)
    images, caps = images.to(dev), caps.to(dev)
    inst.gen.train()
    losses = [float(inst.pretrain_step(images, caps, 7, train=True, lengths=lengths)) for _ in range(20)]
    torch.cuda.synchronize()
    assert all(v == v for v in losses) and losses[-1] < 0.9 * losses[0], losses
