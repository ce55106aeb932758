"""The conditioned discriminator composed: the module API under autograd, one adversarial step through both drivers against the fp64
oracle step (tests/disc_cond_oracle.py), w = 0, the flag-off step against a restatement on the untouched entry points, deterministic
mode with the flag on, and GANInstructor.evaluate_match.  There is no reference counterpart: the oracle is this build's own fp64
PyTorch on the CPU; the step tests pin the trunk's outputs to synthetic features (the trunk is not under test here)."""
import pytest
import torch

from oracle import cpu_step as O
from tests import disc_cond_oracle as DC
from tests import test_gpu_deterministic_steps as DS
from tests.golden_io import Golden
from tests.gpu_util import close, close_mostly, dec_param_names, disc_param_names

pytestmark = pytest.mark.gpu

PROJ = ["img_proj.weight", "img_proj.bias"]
HEAD = ["encoder.linear.weight", "encoder.linear.bias", "encoder.bn.weight", "encoder.bn.bias"]


# ------------------------------------------------------------------------------------------------ module API
def test_module_api_under_autograd_matches_the_oracle():
    """Discriminator(image_features=...) at B=4, L=8, V=50, R=4, filters (2, 3) x (24, 16), C=512, fp32, explicit keep mask: the logits
    and every parameter gradient (img_proj included) and the dense input's, within the tolerances of test_gpu_kernels.py::test_disc_bwd_f32."""
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.discriminator import Discriminator
    B, L, V, R, C = 4, 8, 50, 4, 512
    fs, nf = (2, 3), (24, 16)
    F = sum(nf)
    g = torch.Generator().manual_seed(31)
    dp = {k: 4.0 * v for k, v in O.make_disc_params(V, g, R, R, fs, nf).items()}
    dp["img_proj.weight"] = torch.randn(F, C, generator=g) / C ** 0.5
    dp["img_proj.bias"] = 0.1 * torch.randn(F, generator=g)
    names = disc_param_names(2) + PROJ
    soft = torch.softmax(2 * torch.randn(B, L, V, generator=g), -1)
    pooled = torch.randn(B, C, generator=g)
    mask = torch.empty(B * R, F).bernoulli_(0.8, generator=g)
    gl = torch.randn(B * R, generator=g)
    args = default_args(vocab_size=V, disc_embed_dim=R, disc_num_rep=R, disc_filter_sizes=list(fs), disc_num_filters=list(nf), conditional_gan=1,
                        disc_cond="projection", compute_dtype="fp32", device="cuda")
    disc = Discriminator(args).to(args.device).train()
    with torch.no_grad():
        for n, p in zip(names, disc.param_list()):
            p.copy_(dp[n])
    x = soft.to(args.device).requires_grad_(True)
    logits = disc(x, image_features=pooled.to(args.device), keep_mask=mask.to(args.device))
    (logits * gl.to(args.device)).sum().backward()
    torch.cuda.synchronize()
    leaf = {k: v.double().requires_grad_(True) for k, v in dp.items()}
    xs = soft.double().requires_grad_(True)
    ref = DC.disc_forward(leaf, xs, pooled.double(), mask.double(), R)
    (ref * gl.double()).sum().backward()
    close(logits, ref, rtol=1e-4, atol_scale=1e-5, what="logits")
    # near-ties of the max over time (none expected with Gaussian weights): as test_disc_bwd_f32, a flip loosens the upstream gradients
    emb = (soft.double() @ dp["embeddings.weight"].double().t()).reshape(B, L, R, -1)
    ties = 0
    for k, f in enumerate(fs):
        w, bias = dp[f"convs.{k}.weight"].double(), dp[f"convs.{k}.bias"].double()
        con = torch.relu(torch.einsum("btrej,cje->bctr", emb.unfold(1, f, 1), w[:, 0]) + bias[None, :, None, None])
        top = con.topk(2, dim=2).values
        ties += int(((top[:, :, 0] - top[:, :, 1] <= 1e-6 * top[:, :, 0].abs()) & (top[:, :, 0] > 0)).sum())
    got = dict(zip(names, [p.grad for p in disc.param_list()]))
    upstream = names[:5]
    for n in upstream:
        close_mostly(got[n], leaf[n].grad, 2e-3, 1e-4, n, 1e-2, 1.5e-2 if ties else 1e-5)
    close_mostly(x.grad, xs.grad, 2e-3, 1e-4, "d_inp", 1e-2, 1.5e-2 if ties else 1e-5)
    for n in names[5:]:
        close(got[n], leaf[n].grad, rtol=2e-3, atol_scale=1e-4, what=n)
    assert float(got["img_proj.weight"].abs().max()) > 0
    # the generator's path records no parameter gradients, img_proj's included
    for p in disc.param_list():
        p.grad = None
    with disc.input_grad_only():
        disc(x, image_features=pooled.to(args.device), keep_mask=mask.to(args.device)).sum().backward()
    assert all(p.grad is None for p in disc.param_list())
    # score(): the eval-mode mean logit per caption
    ids = torch.randint(0, V, (B, L), generator=g)
    sc = disc.score(pooled.to(args.device), ids.to(args.device))
    ref_sc = DC.disc_forward({k: v.double() for k, v in dp.items()}, torch.nn.functional.one_hot(ids, V).double(), pooled.double(), None, R)
    close(sc, ref_sc.view(B, R).mean(1), rtol=1e-4, atol_scale=1e-5, what="score")
    assert disc.training


# ------------------------------------------------------------------------------------------------ one adversarial step
def _instructor(m, impl, w, decoder="lstm", loss=None, dtype="fp32", cond="projection", det=0, S=64, seed=None):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    extra = dict(decoder="attention", attn_dim=16) if decoder == "attention" else dict(gen_num_layers=m["NL"])
    args = default_args(vocab_size=m["V"], gen_embed_dim=m["E"], gen_hidden_dim=m["H"], disc_embed_dim=m["De"], disc_num_rep=m["R"],
                        disc_filter_sizes=m["fs"], disc_num_filters=m["nf"], adv_loss_type=loss or m["loss"], clip_norm=m["clip"],
                        gen_lr=m["gen_lr"], disc_lr=m["disc_lr"], compute_dtype=dtype, step_impl=impl, conditional_gan=1, encoder_arch="resnet18",
                        image_size=S, adv_train_batch_size=m["B"], disc_cond=cond, disc_mismatch_weight=w, deterministic=det, device="cuda",
                        log_file=None, model_dir=None, save_dir=None, **extra)
    if seed is not None:
        torch.manual_seed(seed)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    inst.disc.train()
    return inst, args


def _gen_names(inst, attention):
    if attention:
        from tests.test_gpu_attention import NAMES
        return list(NAMES)
    return dec_param_names(inst.args.gen_num_layers)


def _load(inst, gp, dp, gnames):
    from gan_image_captioning_amd import engine
    enc = inst.gen.encoder
    with torch.no_grad():
        for n, p in zip(gnames, inst.gen.decoder.param_list()):
            p.copy_(gp[n])
        for n, p in zip(disc_param_names(len(inst.args.disc_num_filters)) + PROJ, inst.disc.param_list()):
            p.copy_(dp[n])
        for n in HEAD:
            _, mod, attr = n.split(".")
            getattr(getattr(enc, mod), attr).copy_(gp[n])
    engine.bump_param_epoch()


def _weights(inst, gnames):
    enc = inst.gen.encoder
    out = {n: p.detach().cpu().clone() for n, p in zip(gnames, inst.gen.decoder.param_list())}
    out.update({n: p.detach().cpu().clone() for n, p in zip(disc_param_names(len(inst.args.disc_num_filters)) + PROJ, inst.disc.param_list())})
    for n in HEAD:
        _, mod, attr = n.split(".")
        out[n] = getattr(getattr(enc, mod), attr).detach().cpu().clone()
    return out


def _pin_trunk(inst, feat, fmap=None):
    """Both drivers (and the oracle) see the same pooled features / feature map, whatever the trunk computes."""
    enc = inst.gen.encoder
    enc.trunk_features = lambda images, training: feat
    if fmap is not None:
        enc.resnet._plan.last_map = lambda n, s: fmap


def _post_weights_agree(got, want, pre, grads, lr, what):
    """test_adv_step_matches_reference's limits on post-step weights: 5 % of lr wherever the reference gradient is above rounding noise
    (<= 0.1 % of a tensor beyond it, never more than 2.1 lr), and the weights must have moved there."""
    for n in want:
        err = (got[n].double() - want[n].double()).abs()
        live = grads[n].abs() > 1e-6 if n in grads else torch.zeros_like(err, dtype=torch.bool)
        bad = float((err[live] > 0.05 * lr[n]).float().mean()) if bool(live.any()) else 0.0
        assert bad <= 1e-3 and float(err.max()) <= 2.1 * lr[n], (what, n, bad, float(err.max()))
        if bool(live.any()):          # Adam's first update is lr g / (|g| + 1e-8): ~lr wherever the gradient is above rounding noise
            assert float((got[n].double() - pre[n].double()).abs()[live].max()) > 0.5 * lr[n], f"{what}: {n} did not move"


def _one_step(name, loss, decoder):
    g0 = Golden(name)
    m = dict(g0.meta)
    attention = decoder == "attention"
    if attention:                      # one LSTM layer, and the vocabulary padded to the attention kernels' multiple of 4 (main.py pads it too)
        m["NL"], m["V"] = 1, (m["V"] + 3) // 4 * 4
    B, L, V, R, C, S = m["B"], m["L"], m["V"], m["R"], 512, 64
    F = sum(m["nf"])
    w = 0.5
    T = 1.3
    g = torch.Generator().manual_seed(77)
    if attention:
        from oracle import cpu_attention as A
        gp = {k: 6.0 * v for k, v in A.make_attn_params(V, m["E"], m["H"], C, 16, g).items()}
    else:
        gp = {k: 6.0 * v for k, v in O.make_gen_params(V, m["E"], m["H"], m["NL"], g).items()}
    gp.update({k: v for k, v in O.make_gen_params(8, m["E"], 8, 1, g, trunk_feat_dim=C).items() if k.startswith("encoder.")})
    dp = {k: 4.0 * v for k, v in O.make_disc_params(V, g, m["De"], R, m["fs"], m["nf"]).items()}
    dp["img_proj.weight"] = torch.randn(F, C, generator=g) / C ** 0.5
    dp["img_proj.bias"] = 0.1 * torch.randn(F, generator=g)
    caps = O.make_captions(B, L, V, g)
    images = torch.randn(B, 3, S, S, generator=g)
    us = [torch.empty(B, V).uniform_(0, 1, generator=g) for _ in range(L)]
    masks = [torch.empty(B * R, F).bernoulli_(0.8, generator=g) for _ in range(4)]
    res, feat, fmap = {}, None, None
    for impl in ("fused", "autograd"):
        inst, args = _instructor(m, impl, w, decoder, loss)
        dev = args.device
        gnames = _gen_names(inst, attention)
        _load(inst, gp, dp, gnames)
        inst.gen.decoder.temperature = T
        enc = inst.gen.encoder
        with torch.no_grad():
            enc.trunk_features(images.to(dev), True)              # builds this instructor's trunk plan (the attention step reads its map)
        if feat is None:
            # synthetic pooled features and feature map in place of the trunk's outputs: well separated between the images of the batch
            # (the roll must matter), and the same for both drivers and the oracle
            feat = torch.randn(B, C, generator=g).to(dev)
            fmap = torch.randn(B, S // 32, S // 32, C, generator=g).to(dev) if attention else None
        _pin_trunk(inst, feat, fmap)
        with torch.no_grad():
            enc.bn.running_mean.zero_(); enc.bn.running_var.fill_(1.0)
        km = [k.to(dev) for k in masks]
        u = torch.stack(us).to(dev)
        if impl == "fused":
            losses = inst.fused(images.to(dev), caps.to(dev), L, True, u, km)["losses"]
        else:
            losses = inst._adv_step_autograd(images.to(dev), caps.to(dev), L, True, u, km)
        torch.cuda.synchronize()
        res[impl] = (losses.cpu().double(), _weights(inst, gnames))
    # the oracle step, fp64, on the same trunk features
    dd = lambda d: {k: v.double() for k, v in d.items()}
    gp64, dp64 = dd(gp), dd(dp)
    pre = {**gp, **dp}
    sample = None
    if attention:
        fm = fmap.float().cpu().double().view(B, -1, C)
        sample = lambda gl, feats: A.attn_decoder_sample(gl, feats, fm, L, T, [x.double() for x in us])[:2]
    ref = DC.adv_step(gp64, dp64, caps, [x.double() for x in us], [k.double() for k in masks], T, loss, feat.float().cpu().double(), R, w,
                      m["clip"], O.AdamState(m["gen_lr"]), O.AdamState(m["disc_lr"]), sample=sample)
    post = {**gp64, **dp64}
    grads = {**ref["g_grads_raw"], **ref["d_grads_raw"]}
    lr = {n: (m["disc_lr"] if n in dp else m["gen_lr"]) for n in post}
    print(f"[disc cond step] {name} {loss} {decoder}: oracle g_loss {ref['g_loss']:.8f} d_loss {ref['d_loss']:.8f}; "
          + "; ".join(f"{k} {v[0].tolist()}" for k, v in res.items()))
    for impl, (losses, wts) in res.items():
        assert float(losses[0]) == pytest.approx(ref["g_loss"], rel=1e-5), impl
        assert float(losses[1]) == pytest.approx(ref["d_loss"], rel=1e-5), impl
        _post_weights_agree(wts, {n: post[n] for n in wts}, pre, grads, lr, impl + " vs the oracle")
    assert float(res["fused"][0][0]) == pytest.approx(float(res["autograd"][0][0]), rel=1e-5)
    assert float(res["fused"][0][1]) == pytest.approx(float(res["autograd"][0][1]), rel=1e-5)
    _post_weights_agree(res["fused"][1], res["autograd"][1], pre, grads, lr, "fused vs autograd")
    assert float(grads["img_proj.weight"].abs().max()) > 1e-6 and float(ref["d_wrong"].abs().max()) > 0


@pytest.mark.parametrize("name,loss", [("tiny", "standard"), ("tiny_rsgan", "rsgan")])
def test_adv_step_both_drivers_match_the_oracle(name, loss):
    """The shape of tests/golden/tiny.npz's model with --conditional-gan 1, a ResNet-18 trunk at 64x64, explicit noise and four keep
    masks, w = 0.5: g_loss, d_loss (rel 1e-5) and the post-step weights of D (img_proj included) and G."""
    _one_step(name, loss, "lstm")


def test_adv_step_attention_decoder_matches_the_oracle():
    _one_step("tiny", "standard", "attention")


def test_w0_launches_no_third_pass():
    m = Golden("tiny").meta
    B, L, V = m["B"], m["L"], m["V"]
    g = torch.Generator().manual_seed(5)
    images, caps = torch.randn(B, 3, 64, 64, generator=g), O.make_captions(B, L, V, g)
    calls = {}
    for w in (0.0, 0.5):
        inst, args = _instructor(m, "fused", w, seed=3)
        dev = args.device
        den = inst.fused.den
        n = {"fwd": 0, "bwd": 0}
        fwd, bwd = den.fwd, den.bwd
        den.fwd = lambda *a, **k: (n.__setitem__("fwd", n["fwd"] + 1), fwd(*a, **k))[1]
        den.bwd = lambda *a, **k: (n.__setitem__("bwd", n["bwd"] + 1), bwd(*a, **k))[1]
        out = inst.fused(images.to(dev), caps.to(dev), L, True, opt_step=False)
        torch.cuda.synchronize()
        calls[w] = dict(n)
        buf = inst.fused._buf[(B, L)]
        assert ("st_wrong" in buf) == (w > 0)
        lg = out["logits"].cpu().double()
        if w == 0.0:
            want = O.get_losses(lg[0], lg[1], lg[2], m["loss"])[1]
        else:
            want = DC.d_loss_mix(lg[0], lg[1], lg[3], lg[2], m["loss"], w)[1]
        assert float(out["losses"][1]) == pytest.approx(float(want), rel=1e-5)
        assert float(inst.disc.img_proj.weight.grad.abs().max()) > 0
    assert calls[0.0] == {"fwd": 2, "bwd": 2} and calls[0.5] == {"fwd": 3, "bwd": 3}, calls


# ------------------------------------------------------------------------------------------------ the flag off: nothing changes
def _parent_step(inst, caps, L):
    """FusedAdvStep's step for --conditional-gan 0 with the LSTM decoder, restated on the entry points that existed before the flag
    (DiscEngine.fwd / fwd_redrop / bwd without cond, engine.gan_losses), on one stream."""
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.generator import SEEDS
    f = inst.fused
    dec, den = f.dec, f.den
    B = caps.shape[0]
    buf = f._buffers(B, L, caps.device)
    gparams = [p.detach() for p in inst.gen.decoder.param_list()]
    dparams = [p.detach() for p in inst.disc.param_list()]
    g_grads, d_grads = f._grad_lists()
    seeds = [SEEDS.next() for _ in range(4)]
    T = float(inst.gen.decoder.temperature)
    lg = buf["logits"]
    dec.prepare(gparams)
    den.prepare(dparams)
    den.fwd(dparams, None, caps, True, None, seeds[0], state=buf["st_real"], logits=lg[0])
    feats = engine.embedding_fwd(gparams[0], buf["ones"])
    probs, ids, dst = dec.sample_fwd(gparams, feats, L, T, False, None, seeds[3], state=buf["dec_state"], out=buf["probs"], ids=buf["ids"])
    den.fwd(dparams, probs, None, True, None, seeds[1], state=buf["st_fake"], logits=lg[1])
    den.fwd_redrop(dparams, buf["st_fake"], buf["st_gen"], True, None, seeds[2], logits=lg[2])
    losses, lgrads = engine.gan_losses(inst.args.adv_loss_type, lg[0], lg[1], lg[2], want_grads=True)
    den.bwd(dparams, buf["st_gen"], probs, None, True, lgrads["dg_out"], False, True, ws=buf["disc_ws_gen"], d_inp=buf["d_probs"])
    dec.sample_bwd(gparams, dst, probs, ids, buf["d_probs"], T, False, ws=buf["dec_ws"], grads=g_grads + [buf["d_feat"]])
    engine.embedding_bwd(buf["d_feat"], buf["ones"], dec.V, d_weight=g_grads[0], zero_first=False)
    inst.disc_arena.grad.zero_()
    den.bwd(dparams, buf["st_rf"], probs, caps, True, lgrads["dd_real_fake"], True, False, grads=d_grads, accumulate=True, ws=buf["disc_ws"])
    inst.disc_opt.step()
    inst.gen_opt.step()
    return {"losses": losses, "ids": ids}


def test_flag_off_steps_equal_the_untouched_entry_points_bit_for_bit():
    """Three fused steps in deterministic mode with the flag at its default, against three steps from the same snapshot run through the
    entry points the flag does not touch: token ids, losses, weights and Adam moments carry the same bits."""
    from gan_image_captioning_amd import engine
    from tests import test_gpu_step as ST
    g = Golden("cfg1")
    m = g.meta
    before = engine.deterministic()
    engine.set_deterministic(True)
    try:
        inst, args = ST.make_instructor(m, "fused", dtype="bf16")
        assert inst.disc.cond == "none" and not inst.fused.cond and "img_proj.weight" not in inst.disc.state_dict()
        inst.gen.train(); inst.disc.train()
        caps = g.t("caps").to(args.device)
        snap = DS._snapshot(inst)
        a = DS._run(inst, lambda k: {k2: v for k2, v in inst.fused(None, caps, m["L"], True).items() if k2 in ("losses", "ids")})
        DS._restore(inst, snap)
        b = DS._run(inst, lambda k: _parent_step(inst, caps, m["L"]))
    finally:
        engine.set_deterministic(before)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for key in ra:
            assert torch.equal(ra[key], rb[key]), f"step {k}: {key} differs from the untouched entry points"
    assert not torch.equal(a[0]["disc_flat"], a[2]["disc_flat"])


def test_flag_on_steps_repeat_bit_for_bit_in_deterministic_mode():
    """Three conditioned steps (w = 0.5, device-drawn noise and dropout) run twice from one snapshot: ids, losses, gradients, weights and
    Adam moments -- img_proj's are part of D's arena -- bit-identical."""
    from gan_image_captioning_amd import engine
    m = Golden("cfg1").meta
    before = engine.deterministic()
    engine.set_deterministic(True)
    try:
        inst, args = _instructor(m, "fused", 0.5, dtype="bf16", det=1, seed=1008)
        dev = args.device
        g = torch.Generator().manual_seed(9)
        images = torch.randn(m["B"], 3, 64, 64, generator=g).to(dev)
        caps = O.make_captions(m["B"], m["L"], m["V"], g).to(dev)
        arena_ids = {id(p) for p in inst.disc_arena.params}
        assert id(inst.disc.img_proj.weight) in arena_ids and id(inst.disc.img_proj.bias) in arena_ids
        w0 = inst.disc.img_proj.weight.detach().clone()
        DS._twice(inst, lambda k: {k2: v for k2, v in inst.fused(images, caps, m["L"], True).items() if k2 in ("losses", "ids")})
        assert not torch.equal(w0, inst.disc.img_proj.weight.detach())
    finally:
        engine.set_deterministic(before)


# ------------------------------------------------------------------------------------------------ evaluate_match
def test_evaluate_match_equals_the_oracle():
    m = Golden("tiny").meta
    B, L, V, R = 6, m["L"], m["V"], m["R"]
    inst, args = _instructor(dict(m, B=B), "fused", 0.5, seed=21)
    dev = args.device
    g = torch.Generator().manual_seed(13)
    nconv = len(m["nf"])
    with torch.no_grad():
        for i, p in enumerate(inst.disc.text_param_list()):        # embeddings and filters x 20, the rest x 4: captions that D tells apart
            p.mul_(20.0 if i < 1 + 2 * nconv and p.dim() > 1 else 4.0)
        inst.disc.img_proj.weight.copy_(torch.randn(inst.disc.img_proj.weight.shape, generator=g) / 512 ** 0.5)
        inst.disc.img_proj.bias.zero_()
    from gan_image_captioning_amd import engine
    engine.bump_param_epoch()
    batches = [(torch.randn(n, 3, 64, 64, generator=g), O.make_captions(n, L, V, g), None, L) for n in (B, B, 3)]
    inst.adv_eval_loader = batches
    # Synthetic pooled features in place of the trunk's (at its random initialisation the eval-mode trunk maps every image to nearly the
    # same feature).  An image's feature is built so that its projection q is its caption's mean highway output, centred, plus noise,
    # with the direction of the mean over all captions projected out: pooled = pinv(W) q.  The match terms are then no differences of
    # large numbers (the part of y common to all captions is orthogonal to every q) and captions prefer their own image: the margin is a mean
    # of terms of one sign.
    inst.gen.eval()
    names = disc_param_names(nconv) + PROJ
    dp = {n: p.detach().cpu().double() for n, p in zip(names, inst.disc.param_list())}
    pinv = torch.linalg.pinv(dp["img_proj.weight"])                    # [C, F]: W pinv = I
    ys = [O.disc_forward(dp, torch.nn.functional.one_hot(b[1], V).double(), None, R, return_stages=True)[1]["highway"] for b in batches]
    ybar = [y.view(-1, R, y.shape[1]).mean(1) for y in ys]
    mu = torch.cat(ybar).mean(0)
    mu_hat = mu / mu.norm()
    feats = []
    for yb in ybar:
        t = yb - mu
        t = t + float(t.std()) * torch.randn(t.shape, generator=g).double()
        t = t - (t @ mu_hat)[:, None] * mu_hat
        feats.append((t @ pinv.t()).float())
    served = []

    def take_trunk(images, training, stream):
        assert not training
        served.append(images.shape[0])
        return feats[(len(served) - 1) % len(feats)].to(dev)
    inst.gen.encoder.take_trunk = take_trunk
    ref = DC.evaluate_match(dp, [(f.double(), b[1]) for f, b in zip(feats, batches)], R)
    inst.disc.train()
    got = inst.evaluate_match("val")
    assert inst.disc.training                                     # the forward runs in eval mode whatever the module's flag: no dropout
    print(f"[disc cond] evaluate_match {got} oracle {ref}")
    assert served == [B, B, 3] and ref["pair_acc"] > 0.5 and ref["margin"] > 0
    assert got["pair_acc"] == ref["pair_acc"]
    assert got["margin"] == pytest.approx(ref["margin"], rel=1e-5)
    with torch.no_grad():
        inst.disc.img_proj.weight.zero_()
    engine.bump_param_epoch()
    assert inst.evaluate_match("val") == {"pair_acc": 0.0, "margin": 0.0}


# ------------------------------------------------------------------------------------------------ --resume
def test_resume_from_an_unconditioned_checkpoint_keeps_a_fresh_img_proj(tmp_path):
    """A checkpoint saved without img_proj.* loads into a conditioned D: the text path takes the checkpoint's values, img_proj keeps its
    initialisation; any other missing key stays an error."""
    m = Golden("tiny").meta
    inst, args = _instructor(m, "fused", 0.5, seed=4)
    proj0 = {k: v.detach().clone() for k, v in inst.disc.state_dict().items() if k in PROJ}
    gen_sd = {k: v.detach().clone() for k, v in inst.gen.state_dict().items()}
    plain = {k: torch.full_like(v, 0.25) for k, v in inst.disc.state_dict().items() if k not in PROJ}
    path = str(tmp_path / "adv_model.ckpt")
    torch.save({"generator": gen_sd, "discriminator": plain}, path)
    assert inst.load_checkpoint(path) == "adversarial"
    sd = inst.disc.state_dict()
    assert all(torch.equal(sd[k], proj0[k]) for k in PROJ)
    assert all(bool((sd[k] == 0.25).all()) for k in plain)
    del plain["highway.bias"]
    torch.save({"generator": gen_sd, "discriminator": plain}, path)
    with pytest.raises(RuntimeError, match="highway.bias"):
        inst.load_checkpoint(path)
    full = dict(inst.disc.state_dict())
    full["img_proj.bias"] = torch.full_like(full["img_proj.bias"], 0.5)
    torch.save({"generator": gen_sd, "discriminator": full}, path)
    inst.load_checkpoint(path)
    assert bool((inst.disc.img_proj.bias == 0.5).all())
