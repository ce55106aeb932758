"""SeqGAN policy-gradient training of the attention decoder (--adv-mode seqgan --decoder attention) on the GPU against the plain-torch
definition (tests/attn_seqgan_oracle.py on oracle/cpu_attention.py and oracle/cpu_seqgan.py; no reference counterpart): the
many-rows-per-image roll-out (gic_attn_rollout) id for id in fp32, its prefixes / spread / first sampled tokens in bf16, and the whole
step through the instructor."""
import pytest
import torch

from oracle import cpu_attention as A
from oracle import cpu_step as O
from tests import attn_seqgan_oracle as SO
from tests.gpu_util import close, close_mostly, disc_param_names

pytestmark = pytest.mark.gpu

NAMES = ["decoder.embed.weight", "decoder.lstm.weight_ih_l0", "decoder.lstm.weight_hh_l0", "decoder.lstm.bias_ih_l0", "decoder.lstm.bias_hh_l0",
         "decoder.linear.weight", "decoder.linear.bias", "decoder.attn.w_f", "decoder.attn.b_f", "decoder.attn.w_h", "decoder.attn.w_a"]


def _problem(B, L, V, E, H, C, P, At, N, seed, scale=6.0):
    """tests/test_gpu_attention.py's problem (weights x scale) plus the roll-outs' noise; draws in the order params, feats, fmap, us, u_mc."""
    g = torch.Generator().manual_seed(seed)
    gp = {k: v * scale for k, v in A.make_attn_params(V, E, H, C, At, g).items()}
    feats = torch.randn(B, E, generator=g) * 0.3
    fmap = torch.relu(torch.randn(B, P, C, generator=g))           # post-ReLU trunk activations
    us = [torch.empty(B, V).uniform_(0, 1, generator=g) for _ in range(L)]
    u_mc = torch.empty(L, (L - 1) * N * B, V).uniform_(0, 1, generator=g)
    return gp, feats, fmap, us, u_mc


def _gpu_rollout(eng, params, feats, fmap, Y, N, **kw):
    """Roll-outs of Y as the step forms them: the teacher-forced pass along Y, then gic_attn_rollout from its state."""
    B, L = Y.shape
    saved = eng.forward_tf(params, feats, fmap, Y[:, :-1], [L] * B, 1.0, pretrain=True, keep_state=True)[3]
    return saved, eng.rollout(params, saved, Y, N, **kw)


# (B, L, V, E, H, C, P, A, N), seed: P = 49 is no multiple of any tile; 65 and 68 rows per image pass a 64-row tile (and two 32-row
# tiles) by one and by four; one image; the last: P = 260 positions (five chunks of 64, the 16-row tiles that a long energy row selects, 18
# rows per image), A = 72 and C = 72 (two chunks of the attention width and of the channels each).  The seeds keep the smallest top-2 gap of the perturbed logits >= 1e-3 (asserted below), where
# the f32 and f64 oracles agree on every id.
@pytest.mark.parametrize("shape,seed", [((3, 5, 52, 8, 16, 24, 9, 16, 3), 136), ((5, 4, 64, 16, 32, 40, 49, 24, 2), 237),
                                        ((6, 6, 132, 8, 16, 16, 4, 8, 13), 211), ((4, 5, 64, 16, 32, 40, 49, 24, 17), 254),
                                        ((1, 4, 32, 8, 8, 8, 5, 8, 2), 76), ((2, 4, 32, 8, 8, 72, 260, 72, 9), 467)])
def test_rollout_f32_ids_match_oracle(shape, seed):
    from gan_image_captioning_amd import engine as E
    B, L, V, Em, H, C, P, At, N = shape
    dev = torch.device("cuda:0")
    gp, feats, fmap, us, u_mc = _problem(*shape, seed=seed)
    Y_ref = A.attn_decoder_sample(gp, feats, fmap, L, 1.0, us)[1]
    mc_ref, gap = SO.attn_rollouts(gp, feats, fmap, Y_ref, N, u_mc)
    print(f"rows {mc_ref.shape[0]}, smallest top-2 gap {gap:.2e}")
    assert gap >= 1e-3, gap
    eng = E.AttnDecoderEngine(V, Em, H, C, P, At, 0)
    params = [gp[n].to(dev).contiguous() for n in NAMES]
    _, Y, _ = eng.sample_fwd(params, feats.to(dev), fmap.to(dev), L, 1.0, noise_u=torch.stack(us).to(dev))
    saved, mc = _gpu_rollout(eng, params, feats.to(dev), fmap.to(dev), Y, N, noise_u=u_mc.to(dev))
    mc2 = eng.rollout(params, saved, Y, N, noise_u=u_mc.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(Y.cpu(), Y_ref), "sampled captions differ from the oracle"
    assert torch.equal(mc.cpu(), mc_ref), "roll-outs differ from the oracle"
    assert torch.equal(mc, mc2), "two calls on the same inputs differ"


def test_rollout_bf16_prefixes_spread_and_first_tokens():
    """bf16, 704 rows (44 per image), P = 49.  Device noise: every row starts with its caption's prefix and the completions of the
    length-1 prefixes differ.  Explicit noise: each row's FIRST sampled token (position force_len: a flip there does not cascade)
    against the fp32 oracle on the GPU's own Y -- the match rate must reach the 0.9 that test_attention_decoder_bf16_at_cfg4_shapes
    asks of whole bf16 trajectories of this decoder.  A joining row's first token still uses the context the teacher-forced pass
    left, so the same bar is also asked of ALL sampled tokens (whole trajectories, flips cascading: that test's own terms), which pass
    through the many-rows attention step and its MFMA context product at every later position."""
    from gan_image_captioning_amd import engine as E
    shape = (16, 12, 2000, 64, 128, 256, 49, 64, 4)
    B, L, V, Em, H, C, P, At, N = shape
    dev = torch.device("cuda:0")
    gp, feats, fmap, us, u_mc = _problem(*shape, seed=12, scale=3.0)
    eng = E.AttnDecoderEngine(V, Em, H, C, P, At, 1)
    params = [gp[n].to(dev).contiguous() for n in NAMES]
    _, Y, _ = eng.sample_fwd(params, feats.to(dev), fmap.to(dev), L, 1.0, seed=11)
    saved, mc = _gpu_rollout(eng, params, feats.to(dev), fmap.to(dev), Y, N, seed=12)
    mc_u = eng.rollout(params, saved, Y, N, noise_u=u_mc.to(dev))
    torch.cuda.synchronize()
    Yc = Y.cpu()
    for ids in (mc.cpu().view(L - 1, N, B, L), mc_u.cpu().view(L - 1, N, B, L)):
        for t in range(1, L):
            assert torch.equal(ids[t - 1, :, :, :t], Yc[None, :, :t].expand(N, B, t)), f"prefix of length {t} not kept"
    assert len(torch.unique(mc.cpu()[:N * B], dim=0)) > N * B // 2          # the completions actually differ
    mc_ref, _ = SO.attn_rollouts(gp, feats, fmap, Yc, N, u_mc)
    flen = torch.arange(1, L).repeat_interleave(N * B).view(-1, 1)
    rate = float((mc_u.cpu().gather(1, flen) == mc_ref.gather(1, flen)).float().mean())
    sampled = torch.arange(L)[None, :] >= flen
    whole = float((mc_u.cpu() == mc_ref)[sampled].float().mean())
    print(f"bf16 roll-out: match rate vs the fp32 oracle, first sampled token {rate:.4f}, all sampled tokens {whole:.4f}")
    assert rate >= 0.9, rate
    assert whole >= 0.9, whole


@pytest.mark.parametrize("shape", [(4, 6, 256, 16, 32, 136, 70, 136, 5), (2, 5, 128, 16, 32, 264, 300, 72, 9)])
def test_rollout_bf16_walks_position_width_and_channel_chunks(shape):
    """The bf16 attention step where one chunk is not enough: P = 70 (two position chunks = four K steps of the MFMA, the second mostly
    padding), A = 136 (three width chunks), C = 136 (two channel groups, the second partial), 25 rows per image; and P = 300 with the
    16-row tiles, 36 rows per image, C = 264 (three channel groups).  All sampled tokens against the fp32 oracle on explicit noise and
    the GPU's own Y: the 0.9 of test_attention_decoder_bf16_at_cfg4_shapes; two calls give the same bits."""
    from gan_image_captioning_amd import engine as E
    B, L, V, Em, H, C, P, At, N = shape
    dev = torch.device("cuda:0")
    gp, feats, fmap, us, u_mc = _problem(*shape, seed=sum(shape), scale=3.0)
    eng = E.AttnDecoderEngine(V, Em, H, C, P, At, 1)
    params = [gp[n].to(dev).contiguous() for n in NAMES]
    _, Y, _ = eng.sample_fwd(params, feats.to(dev), fmap.to(dev), L, 1.0, noise_u=torch.stack(us).to(dev))
    saved, mc = _gpu_rollout(eng, params, feats.to(dev), fmap.to(dev), Y, N, noise_u=u_mc.to(dev))
    mc2 = eng.rollout(params, saved, Y, N, noise_u=u_mc.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(mc, mc2), "two calls on the same inputs differ"
    mc_ref, _ = SO.attn_rollouts(gp, feats, fmap, Y.cpu(), N, u_mc)
    flen = torch.arange(1, L).repeat_interleave(N * B).view(-1, 1)
    sampled = torch.arange(L)[None, :] >= flen
    assert torch.equal(mc.cpu()[~sampled], mc_ref[~sampled]), "prefixes not kept"
    whole = float((mc.cpu() == mc_ref)[sampled].float().mean())
    print(f"bf16 roll-out {shape}: match rate of all sampled tokens vs the fp32 oracle {whole:.4f}")
    assert whole >= 0.9, whole


def test_rollout_bf16_through_the_fused_vocabulary_product():
    """The route the benchmark shape takes: at V = 4096 the vocabulary product with Gumbel-max in its epilogue (gemm_gumbelmax, then
    rollout_pick) takes the steps with 513 rows or more -- here steps 5, 6 and 7 (640, 768, 896 of the 896 rows), whose picked tokens
    feed the next step's input -- and the earlier ones go through the plain product.  All sampled tokens against the fp32 oracle on
    explicit noise and the GPU's own Y (the 0.9 of test_attention_decoder_bf16_at_cfg4_shapes), prefixes kept, the same bits twice,
    and device noise gives distinct completions."""
    from gan_image_captioning_amd import engine as E
    shape = (8, 8, 4096, 64, 128, 256, 49, 64, 16)
    B, L, V, Em, H, C, P, At, N = shape
    dev = torch.device("cuda:0")
    gp, feats, fmap, us, u_mc = _problem(*shape, seed=sum(shape), scale=3.0)
    eng = E.AttnDecoderEngine(V, Em, H, C, P, At, 1)
    rows = (L - 1) * N * B
    # the logits scratch holds 512 rows: the later steps can only have run through the fused product
    assert eng.rollout_ws_bytes(B, L, rows) - eng.rollout_ws_bytes(B, L, 512) == (rows - 512) * ((Em + C + H) * 2 + 2 * H * 4 + 4 * H * 4 + At * 4 + L * 8)
    params = [gp[n].to(dev).contiguous() for n in NAMES]
    _, Y, _ = eng.sample_fwd(params, feats.to(dev), fmap.to(dev), L, 1.0, noise_u=torch.stack(us).to(dev))
    saved, mc = _gpu_rollout(eng, params, feats.to(dev), fmap.to(dev), Y, N, noise_u=u_mc.to(dev))
    mc2 = eng.rollout(params, saved, Y, N, noise_u=u_mc.to(dev))
    mc_dev = eng.rollout(params, saved, Y, N, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(mc, mc2), "two calls on the same inputs differ"
    mc_ref, _ = SO.attn_rollouts(gp, feats, fmap, Y.cpu(), N, u_mc)
    flen = torch.arange(1, L).repeat_interleave(N * B).view(-1, 1)
    sampled = torch.arange(L)[None, :] >= flen
    for ids in (mc.cpu(), mc_dev.cpu()):
        assert torch.equal(ids[~sampled], mc_ref[~sampled]), "prefixes not kept"
        assert int(ids.min()) >= 0 and int(ids.max()) < V
    whole = float((mc.cpu() == mc_ref)[sampled].float().mean())
    late = float((mc.cpu() == mc_ref)[:, 5:].float().mean())
    print(f"bf16 roll-out through the fused vocabulary product: match rate vs the fp32 oracle, all sampled tokens {whole:.4f}, steps 5..7 {late:.4f}")
    assert whole >= 0.9, whole
    assert len(torch.unique(mc_dev.cpu()[:N * B], dim=0)) > N * B // 2


def _instructor(dtype, B, V, E, H, At, N, nf=None, **kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    extra = {} if nf is None else {"disc_num_filters": nf}
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, conditional_gan=1, encoder_arch="resnet18", decoder="attention",
                        attn_dim=At, adv_mode="seqgan", mc_rollouts=N, compute_dtype=dtype, adv_train_batch_size=B, image_size=64,
                        device="cuda", log_file=None, model_dir=None, save_dir=None, **extra, **kw)
    return GANInstructor(args, None, None), args


def test_attn_seqgan_step_f32_matches_oracle():
    """The step through the instructor in fp32 parity mode with explicit noise (ResNet-18 trunk at 64x64: a 2x2x512 map) against
    attn_seqgan_step fed the GPU's own trunk features and feature map: Y exact, rewards / logits 1e-4, losses 1e-5, every generator
    gradient (decoder incl. attention, encoder head) 2e-3, D's as the LSTM decoder's step test."""
    from oracle import cpu_encoder as OE
    B, L, V, E, H, At, N, S = 4, 5, 64, 16, 32, 24, 3, 64
    nf = [20, 30, 10]
    C = OE.out_features("resnet18")
    g = torch.Generator().manual_seed(57)
    gp = {k: v * 6 for k, v in A.make_attn_params(V, E, H, C, At, g).items()}
    head = O.make_gen_params(8, E, 8, 1, g, trunk_feat_dim=C)
    gp.update({k: v for k, v in head.items() if k.startswith("encoder.")})
    dp = {k: v * 8 for k, v in O.make_disc_params(V, g, num_filters=nf).items()}       # scaled: an informative reward model
    tp = OE.make_trunk_params("resnet18", g)
    caps = O.make_captions(B, L, V, g)
    images = torch.randn(B, 3, S, S, generator=g)
    us = [torch.empty(B, V).uniform_(0, 1, generator=g) for _ in range(L)]
    u_mc = torch.empty(L, (L - 1) * N * B, V).uniform_(0, 1, generator=g)
    masks = [torch.empty(B * 64, sum(nf)).bernoulli_(0.8, generator=g) for _ in range(2)]
    inst, args = _instructor("fp32", B, V, E, H, At, N, nf)
    dev = args.device
    enc, dec = inst.gen.encoder, inst.gen.decoder
    with torch.no_grad():
        for n, p in zip(NAMES, dec.param_list()):
            p.copy_(gp[n])
        for n, p in zip(disc_param_names(3), inst.disc.param_list()):
            p.copy_(dp[n])
        enc.resnet.load_state_dict({k[len("encoder.resnet."):]: v for k, v in tp.items()}, strict=False)
        for n in ("linear.weight", "linear.bias", "bn.weight", "bn.bias"):
            mod, attr = n.split(".")
            getattr(getattr(enc, mod), attr).copy_(gp["encoder." + n])
    inst.gen.train(); inst.disc.train()
    out = inst.seqgan(images.to(dev), caps.to(dev), L, True, torch.stack(us).to(dev), u_mc.to(dev), [m.to(dev) for m in masks], opt_step=False)
    torch.cuda.synchronize()
    # the oracle is fed what the step's own trunk pass left in the plan's buffers
    trunk_feat = enc.resnet._plan._bufs[(B, S)]["feat"].float().cpu().reshape(B, -1).clone()
    fmap = enc.resnet._plan.last_map(B, S).float().cpu().reshape(B, -1, C).clone()
    ref = SO.attn_seqgan_step(dict(gp), dict(dp), caps, us, u_mc, N, masks, trunk_feat, fmap)
    print(f"rewards std {float(ref['rewards'].std()):.3e}, smallest top-2 gap of the roll-outs {ref['mc_gap']:.2e}")
    assert float(ref["rewards"].std()) > 1e-3                # the rewards actually differ between positions
    assert torch.equal(out["ids"].cpu(), ref["Y"]), "sampled captions differ"
    close(out["rewards"], ref["rewards"], rtol=1e-4, atol_scale=1e-5, what="rewards")
    close(out["logits"], ref["logits"], rtol=1e-4, atol_scale=1e-5, what="logits along Y")
    assert float(out["losses"][0]) == pytest.approx(ref["g_loss"], rel=1e-5)
    assert float(out["losses"][1]) == pytest.approx(ref["d_loss"], rel=1e-5)
    ggot = {n: p.grad for n, p in zip(NAMES, dec.param_list())}
    # (encoder.linear.bias is not compared: BatchNorm1d's mean subtraction cancels it, its gradient is rounding noise)
    ggot.update({"encoder.linear.weight": enc.linear.weight.grad, "encoder.bn.weight": enc.bn.weight.grad, "encoder.bn.bias": enc.bn.bias.grad})
    for n, got in ggot.items():
        close(got, ref["g_grads_raw"][n], rtol=2e-3, atol_scale=1e-4, what=n)
    dgot = {n: p.grad for n, p in zip(disc_param_names(3), inst.disc.param_list())}
    up = set(disc_param_names(3)[:7])
    for n, w in ref["d_grads_raw"].items():
        if n in up:
            close_mostly(dgot[n], w, 2e-3, 1e-4, n, 1e-2, 1.5e-2)                 # may carry a re-routed max-pool near-tie
        else:
            close(dgot[n], w, rtol=2e-3, atol_scale=1e-4, what=n, atol_abs=1e-6)
    # the optimizers move both models
    before = inst.gen_arena.flat.clone(), inst.disc_arena.flat.clone()
    inst.disc_opt.step(); inst.gen_opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before[0], inst.gen_arena.flat) and not torch.equal(before[1], inst.disc_arena.flat)


def test_adv_step_seqgan_attention_bf16_updates_both_models():
    """adv_step with --adv-mode seqgan --decoder attention in bf16 with device noise (the bf16 roll-out test's decoder on the ResNet-18
    trunk at 64x64; 704 roll-out rows): finite losses, generator (attention parameters included) and discriminator updated."""
    B, L, V = 16, 12, 2000
    inst, args = _instructor("bf16", B, V, 64, 128, 64, 4)
    dev = args.device
    g = torch.Generator().manual_seed(1)
    caps = O.make_captions(B, L, V, g).to(dev)
    images = torch.randn(B, 3, 64, 64, generator=g).to(dev)
    inst.gen.train(); inst.disc.train()
    before = inst.gen_arena.flat.clone(), inst.disc_arena.flat.clone()
    attn_before = inst.gen.decoder.attn.w_h.detach().clone()
    losses = inst.adv_step(images, caps, L, train=True)
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    assert not torch.equal(before[0], inst.gen_arena.flat) and not torch.equal(before[1], inst.disc_arena.flat)
    assert not torch.equal(attn_before, inst.gen.decoder.attn.w_h.detach())
