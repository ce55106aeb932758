"""Scheduled sampling on the GPU (gic_decoder_forward_ss / gic_attn_forward_ss, Decoder / AttnDecoder.forward_scheduled,
--scheduled-sampling-prob) against the float64 oracle (tests/sched_sample_oracle.py) at the cases of tests/sched_sample_cases.py.
The discrete results (inputs, replaced) are exact -- every case has an oracle top-2 gap >= 1e-3 (tests/test_sched_sample_api.py) --
and the tolerances of everything else are those of tests/test_gpu_attn_tf.py: f32 outputs rtol 1e-4, gradients rtol 2e-3
(atol_scale 1e-4); bf16 rel-L2 < 5e-2 and >= 0.9 of the picks as the oracle's from the same prefix."""
import math

import pytest
import torch

from oracle import cpu_step as O
from tests import attn_tf_oracle as TF
from tests import sched_sample_cases as SC
from tests import sched_sample_oracle as SO
from tests.gpu_util import close, rel_l2

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("gic_decoder_forward_ss", "gic_attn_forward_ss")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _engine(pr, dt=0):
    from gan_image_captioning_amd import engine
    d = pr["dims"]
    if pr["kind"] == "lstm":
        return engine.DecoderEngine(d["V"], d["E"], d["H"], d["NL"], dt)
    return engine.AttnDecoderEngine(d["V"], d["E"], d["H"], d["C"], d["P"], d["A"], dt)


def _on(t, dev):
    return None if t is None else t.to(dev)


def _run(eng, pr, dev, p, pick, coin=None, u=None, seed=0, lengths=None, caps=None):
    """One forward through the C entry point: a dict with pd (the parameters on the device), pred, h_n, c_n ([NL, B, H]), alphas,
    saved, inputs, replaced."""
    pd = [t.to(dev) for t in pr["params"]]
    lens = pr["lengths"] if lengths is None else lengths
    caps = (pr["caps"] if caps is None else caps).to(dev)
    if pr["kind"] == "lstm":
        pred, (h_n, c_n), saved, inputs, replaced = eng.forward_scheduled(pd, pr["feats"].to(dev), caps, lens, p, pick, _on(coin, dev),
                                                                           _on(u, dev), seed)
        alphas = None
    else:
        pred, (h_n, c_n), alphas, saved, inputs, replaced = eng.forward_scheduled(pd, pr["feats"].to(dev), pr["fmap"].to(dev), caps, lens, p,
                                                                                   pick, _on(coin, dev), _on(u, dev), seed)
    return dict(pd=pd, pred=pred, h_n=h_n, c_n=c_n, alphas=alphas, saved=saved, inputs=inputs, replaced=replaced)


def _bwd(eng, pr, r, d_pred, d_alphas, dev):
    if pr["kind"] == "lstm":
        return eng.forward_tf_bwd(r["pd"], r["saved"], r["pred"], d_pred.to(dev), 1.0, True)
    return eng.forward_tf_bwd(r["pd"], r["saved"], r["pred"], d_pred.to(dev), 1.0, True, d_alphas=_on(d_alphas, dev))


def _close_outputs(pr, r, want):
    close(r["pred"], want["pred"], rtol=1e-4, atol_scale=1e-5, what="pred")
    w_h, w_c = (want["h_n"], want["c_n"]) if pr["kind"] == "lstm" else (want["h_n"][None], want["c_n"][None])
    close(r["h_n"], w_h, rtol=1e-4, atol_scale=1e-6, what="h_n")
    close(r["c_n"], w_c, rtol=1e-4, atol_scale=1e-6, what="c_n")
    if want["alphas"] is not None:
        close(r["alphas"], want["alphas"], rtol=1e-4, atol_scale=1e-6, what="alphas")


def _close_grads(pr, grads, want):
    for n, got, w in zip(pr["names"] + ["d_features"], grads, want):
        close(got, torch.zeros_like(got, device="cpu") if w is None else w, rtol=2e-3, atol_scale=1e-4, what=n)


# ------------------------------------------------------------------------------------------ 1. every case against the oracle
@pytest.mark.parametrize("pick", SC.PICKS)
@pytest.mark.parametrize("p", SC.PROBS)
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_matches_oracle(dev, name, p, pick):
    pr, want = SC.problem(name), SC.reference(name, p, pick)
    eng = _engine(pr)
    r = _run(eng, pr, dev, p, pick, pr["coin"], pr["u"])
    grads = _bwd(eng, pr, r, want["d_pred"], want["d_alphas"], dev)
    torch.cuda.synchronize()
    assert torch.equal(r["inputs"].cpu(), want["inputs"])
    assert torch.equal(r["replaced"].cpu().bool(), want["replaced"])
    _close_outputs(pr, r, want)
    _close_grads(pr, grads, want["grads"])


# ------------------------------------------------------------------------------------------ 2. coins all >= p
@pytest.mark.parametrize("name", ["L2", "L3", "A1"])
def test_coins_at_or_above_p_replace_nothing(dev, name):
    pr = SC.problem(name)
    V = pr["dims"]["V"]
    caps = pr["caps"].clone()
    caps[0, 0], caps[-1, 1] = V + 5, -3                              # embed_rows_tf's clamp
    coin = torch.full_like(pr["coin"], 0.5)
    coin[:, ::2] = 0.75
    eng = _engine(pr)
    r = _run(eng, pr, dev, 0.5, "sample", coin, pr["u"], caps=caps)
    Tmax = max(pr["lengths"])
    if pr["kind"] == "lstm":
        pred, (h_n, c_n) = eng.forward_tf(r["pd"], pr["feats"].to(dev), caps.to(dev), pr["lengths"], 1.0, True)
    else:
        pred, (h_n, c_n), _ = eng.forward_tf(r["pd"], pr["feats"].to(dev), pr["fmap"].to(dev), caps.to(dev), pr["lengths"], 1.0, True)
    torch.cuda.synchronize()
    want = caps.clone()
    want[:, :Tmax - 1] = caps[:, :Tmax - 1].clamp(0, V - 1)
    assert torch.equal(r["inputs"].cpu(), want)
    assert not r["replaced"].any()
    close(r["pred"], pred, rtol=1e-4, atol_scale=1e-5, what="pred")
    close(r["h_n"], h_n, rtol=1e-4, atol_scale=1e-6, what="h_n")
    close(r["c_n"], c_n, rtol=1e-4, atol_scale=1e-6, what="c_n")


# ------------------------------------------------------------------------------------------ 3. p = 1, argmax, full lengths
@pytest.mark.parametrize("name", ["L2", "L3", "A1", "A2"])
def test_p1_argmax_is_the_pretrain_rollout(dev, name):
    pr = SC.problem(name)
    B, T = pr["dims"]["B"], pr["dims"]["T"]
    eng = _engine(pr)
    r = _run(eng, pr, dev, 1.0, "argmax", pr["coin"], None, lengths=[T] * B)
    maps = () if pr["kind"] == "lstm" else (pr["fmap"].to(dev),)
    out, ids, _ = eng.sample_fwd(r["pd"], pr["feats"].to(dev), *maps, T, 1.0, pretrain=True)
    torch.cuda.synchronize()
    assert torch.equal(r["inputs"], ids[:, :-1])
    assert r["replaced"].all()
    close(r["pred"], out, rtol=1e-4, atol_scale=1e-5, what="logits")


# ------------------------------------------------------------------------------------------ 4. module API
def _module(pr, dev, dtype="fp32"):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder
    d = pr["dims"]
    args = default_args(vocab_size=d["V"], gen_embed_dim=d["E"], gen_hidden_dim=d["H"], gen_num_layers=d["NL"], attn_dim=d["A"] or 512,
                        compute_dtype=dtype, conditional_gan=1, device="cuda")
    dec = Decoder(args) if pr["kind"] == "lstm" else AttnDecoder(args, d["C"], d["P"])
    dec = dec.to(dev)
    with torch.no_grad():
        for q, t in zip(dec.param_list(), pr["params"]):
            q.copy_(t)
    return dec


class _Spy:
    """Counts the calls of the bound library symbols ``names`` (they still run)."""

    def __init__(self, monkeypatch, names):
        from gan_image_captioning_amd import _lib
        self.calls = {n: 0 for n in names}
        lib = _lib.load()
        for n in names:
            monkeypatch.setattr(lib, n, self._wrap(n, getattr(lib, n)))

    def _wrap(self, name, fn):
        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


@pytest.mark.parametrize("name", ["L3", "A2"])
def test_module_forward_scheduled_under_autograd(dev, name, monkeypatch):
    pr, want = SC.problem(name), SC.reference(name, 0.5, "sample")
    dec = _module(pr, dev)
    feats = pr["feats"].to(dev).requires_grad_(True)
    caps, coin, u = pr["caps"].to(dev), pr["coin"].to(dev), pr["u"].to(dev)
    spy = _Spy(monkeypatch, NEW_ENTRIES)
    if pr["kind"] == "lstm":
        pred, (h_n, c_n), (inputs, replaced) = dec.forward_scheduled(feats, caps, pr["lengths"], 0.5, coin_u=coin, noise_u=u,
                                                                     return_inputs=True)
        loss = (pred * want["d_pred"].to(dev)).sum()
    else:
        pred, (h_n, c_n), alphas, (inputs, replaced) = dec.forward_scheduled(feats, pr["fmap"].to(dev), caps, pr["lengths"], 0.5, coin_u=coin,
                                                                             noise_u=u, return_alphas=True, return_inputs=True)
        loss = (pred * want["d_pred"].to(dev)).sum() + (alphas * want["d_alphas"].to(dev)).sum()
    assert sum(spy.calls.values()) == 1
    assert not inputs.requires_grad and not replaced.requires_grad and not h_n.requires_grad
    grads = torch.autograd.grad(loss, dec.param_list() + [feats])
    torch.cuda.synchronize()
    assert torch.equal(inputs.cpu(), want["inputs"]) and torch.equal(replaced.cpu().bool(), want["replaced"])
    close(pred, want["pred"], rtol=1e-4, atol_scale=1e-5, what="pred")
    _close_grads(pr, grads, want["grads"])


@pytest.mark.parametrize("name", ["L3", "A2"])
def test_module_p0_is_forward_and_launches_nothing_new(dev, name, monkeypatch):
    pr = SC.problem(name)
    dec = _module(pr, dev)
    feats, caps = pr["feats"].to(dev).requires_grad_(True), pr["caps"].to(dev)
    maps = () if pr["kind"] == "lstm" else (pr["fmap"].to(dev),)
    spy = _Spy(monkeypatch, NEW_ENTRIES)
    res = dec.forward_scheduled(feats, *maps, caps, pr["lengths"], 0.0, return_inputs=True)
    ref = dec(feats, *maps, caps, pr["lengths"], pretrain=True)
    torch.cuda.synchronize()
    assert spy.calls == {n: 0 for n in NEW_ENTRIES}
    assert torch.equal(res[0], ref[0]) and res[0].requires_grad
    inputs, replaced = res[-1]
    assert torch.equal(inputs, caps) and not replaced.any()


# ------------------------------------------------------------------------------------------ 5. device noise
@pytest.mark.parametrize("name", ["L3", "A2"])
def test_device_noise(dev, name):
    pr = SC.problem(name)
    eng = _engine(pr)
    a = _run(eng, pr, dev, 0.5, "sample", seed=11)
    b = _run(eng, pr, dev, 0.5, "sample", seed=11)
    c = _run(eng, pr, dev, 0.5, "sample", seed=12)
    full = _run(eng, pr, dev, 1.0, "sample", seed=13)
    torch.cuda.synchronize()
    assert torch.equal(a["inputs"], b["inputs"]) and torch.equal(a["pred"], b["pred"]) and torch.equal(a["replaced"], b["replaced"])
    assert not torch.equal(a["inputs"], c["inputs"])
    T, V = pr["dims"]["T"], pr["dims"]["V"]
    live = torch.arange(1, T)[None] < torch.tensor(pr["lengths"])[:, None]
    assert not a["replaced"].cpu().bool()[~live].any()
    assert torch.equal(full["replaced"].cpu().bool(), live)          # p = 1: a coin in [0, 1) is always below it
    assert int(a["inputs"].min()) >= 0 and int(a["inputs"].max()) < V
    gp, feats, fmap = SC.as_f64(pr)
    want = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], 0.0, "sample", pr["coin"], None, inputs=a["inputs"].cpu())
    _close_outputs(pr, a, want)


def test_device_coins_are_binomial_and_do_not_depend_on_the_batch(dev):
    B, T, p = 64, 13, 0.25
    pr = SC.make("lstm", B, T, 64, 16, 32, [T] * B, seed=201)
    eng = _engine(pr)
    r = _run(eng, pr, dev, p, "sample", seed=21)
    few = {k: (v[:8] if torch.is_tensor(v) and v.shape[0] == B else v) for k, v in pr.items()}
    few["u"], few["lengths"] = pr["u"][:, :8], pr["lengths"][:8]
    s = _run(eng, few, dev, p, "sample", seed=21)
    torch.cuda.synchronize()
    n = B * (T - 1)                                                  # 768 positions
    sd = math.sqrt(n * p * (1 - p))                                  # 12
    count = int(r["replaced"].sum())
    print("replaced", count, "of", n)
    assert abs(count - n * p) <= 5 * sd                              # 192 +- 60
    assert torch.equal(s["replaced"], r["replaced"][:8])


# ------------------------------------------------------------------------------------------ 6. deterministic mode
def test_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    pr, want = SC.problem("L3"), SC.reference("L3", 0.5, "sample")
    eng = _engine(pr)
    engine.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            r = _run(eng, pr, dev, 0.5, "sample", pr["coin"], pr["u"])
            grads = _bwd(eng, pr, r, want["d_pred"], None, dev)
            torch.cuda.synchronize()
            runs.append([r["pred"], r["h_n"], r["c_n"], r["inputs"], r["replaced"]] + [g.clone() for g in grads])
        for i, (x, y) in enumerate(zip(*runs)):
            assert torch.equal(x, y), i
        assert torch.equal(runs[0][3].cpu(), want["inputs"])
        at = SC.problem("A1")
        with pytest.raises(NotImplementedError, match="deterministic"):
            _run(_engine(at), at, dev, 0.5, "sample", at["coin"], at["u"])
    finally:
        engine.set_deterministic(False)


# ------------------------------------------------------------------------------------------ 7. bf16
@pytest.mark.parametrize("kind", ["lstm", "attn"])
def test_bf16(dev, kind):
    B, T, V = 16, 12, 2000
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(4, T + 1, (B,), generator=g).tolist()
    lens[0] = T
    extra = dict(C=64, P=49, A=64) if kind == "attn" else {}
    pr = SC.make(kind, B, T, V, 64, 128, lens, seed=301, scale=1.0, **extra)
    w_out = pr["names"].index("decoder.linear.weight")
    pr["params"][w_out] = pr["params"][w_out] * 20.0                 # logits of order 1 (test_gpu_attn_tf.test_bf16_at_cfg4_shapes)
    eng = _engine(pr, 1)
    r = _run(eng, pr, dev, 0.5, "sample", pr["coin"], pr["u"])
    torch.cuda.synchronize()
    gp, feats, fmap = SC.as_f64(pr)
    want = SO.scheduled(gp, feats, fmap, pr["caps"], lens, 0.5, "sample", pr["coin"], pr["u"], inputs=r["inputs"].cpu())
    assert torch.equal(r["replaced"].cpu().bool(), want["replaced"])          # coins are exact in any dtype
    rep = want["replaced"]
    assert int(rep.sum()) >= 40
    match = float((r["inputs"].cpu()[rep] == want["picks"][rep]).float().mean())
    err = rel_l2(r["pred"].float(), want["pred"])
    print(f"bf16 {kind}: picks as the oracle's {match:.3f} over {int(rep.sum())} positions, pred rel-L2 {err:.2e}")
    assert err < 5e-2
    assert match >= 0.9


# ------------------------------------------------------------------------------------------ 8. instructor
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


def _instructor(decoder, p):
    from gan_image_captioning_amd.training import GANInstructor
    lam = 0.7 if decoder == "attention" else 0.0
    inst = GANInstructor(_args(decoder=decoder, pretrain_mode="teacher", attn_reg=lam, scheduled_sampling_prob=p), None, None)
    with torch.no_grad():
        for q in inst.gen.decoder.parameters():
            q.mul_(8.0)
    inst.gen.train()
    return inst, lam


@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_instructor_pretrain_steps_match_oracle(dev, decoder, monkeypatch):
    inst, lam = _instructor(decoder, 0.5)
    B, L, V = 6, 7, 64
    images, caps, lengths = _batch(B, L, V, 2)
    dec = inst.gen.decoder
    params = list(dec.parameters())
    names = ["decoder." + k for k, _ in dec.named_parameters()]
    seen = {}
    inner = dec.forward_scheduled

    def capture(*a, **kw):                                # the decode's own inputs, next to what the trainer asked for
        res = inner(*a, return_inputs=True, **kw)
        seen["feats"], seen["p"], seen["inputs"] = a[:-3], a[-1], res[-1][0]        # (features[, fmap]), caps, lengths, p
        return res[:-1]

    def optimize(opt, loss, model=None, retain_graph=False):        # GANInstructor.optimize, with a look at the gradients before the step
        opt.zero_grad()
        loss.backward()
        seen["grads"] = [q.grad.clone() for q in params]
        opt.step()

    monkeypatch.setattr(dec, "forward_scheduled", capture)
    monkeypatch.setattr(inst, "optimize", optimize)
    for step in range(2):
        gp = {"decoder." + k: v.detach().cpu().double().requires_grad_(True) for k, v in dec.state_dict().items()}
        with torch.enable_grad():
            loss = inst.pretrain_step(images.to(dev), caps.to(dev), L, train=True, lengths=lengths)
        torch.cuda.synchronize()
        assert seen["p"] == 0.5
        inputs = seen["inputs"].cpu()
        assert (inputs != caps[:, :-1]).any()             # this step did mix its own tokens in
        f = seen["feats"][0].detach().cpu().double()
        m = seen["feats"][1].detach().cpu().double() if decoder == "attention" else None
        r = SO.scheduled(gp, f, m, caps[:, :-1], lengths.tolist(), 0.5, "sample", torch.ones(B, L - 1), None, inputs=inputs)
        want = torch.nn.functional.cross_entropy(r["pred"].reshape(-1, V), caps[:, :r["pred"].shape[1]].reshape(-1))
        if lam:
            want = want + TF.attn_reg(r["alphas"], lam)
        gw = torch.autograd.grad(want, [gp[n] for n in names])
        assert float(loss.detach()) == pytest.approx(float(want), rel=1e-5), step
        for n, got, w in zip(names, seen["grads"], gw):
            close(got, w, rtol=2e-3, atol_scale=1e-4, what=f"step {step} {n}")


@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_instructor_p0_and_validation_take_the_teacher_path(dev, decoder, monkeypatch):
    inst, lam = _instructor(decoder, 0.5)
    B, L, V = 6, 7, 64
    images, caps, lengths = _batch(B, L, V, 3)
    dec = inst.gen.decoder
    params = list(dec.parameters())
    spy = _Spy(monkeypatch, NEW_ENTRIES)
    got = {}
    monkeypatch.setattr(inst, "optimize", lambda opt, loss, model=None, retain_graph=False: got.update(
        grads=torch.autograd.grad(loss, params, retain_graph=True)))
    from gan_image_captioning_amd import engine
    with torch.enable_grad():
        feats = inst._features(images.to(dev), B)
    engine.set_deterministic(True)                        # the teacher decode's own backward gives the same bits twice only in this mode
    try:
        _p0_step_is_the_teacher_step(inst, dec, params, decoder, lam, feats, caps, lengths, got, dev)
    finally:
        engine.set_deterministic(False)
    # a validation step ignores p
    inst.ss_prob_now = 0.5
    inst.gen.eval()
    with torch.no_grad():
        v_mixed = inst.pretrain_step(images.to(dev), caps.to(dev), L, train=False, lengths=lengths)
        inst.ss_prob_now = 0.0
        v_plain = inst.pretrain_step(images.to(dev), caps.to(dev), L, train=False, lengths=lengths)
    torch.cuda.synchronize()
    assert torch.equal(v_mixed, v_plain)
    assert spy.calls == {n: 0 for n in NEW_ENTRIES}


def _p0_step_is_the_teacher_step(inst, dec, params, decoder, lam, feats, caps, lengths, got, dev):
    V = 64
    with torch.enable_grad():
        inst.ss_prob_now = 0.0                            # epoch 0 of a ramp
        loss = inst._pretrain_step_teacher(feats, caps.to(dev), lengths, train=True)
        # the step as it was before the flag existed
        c = caps.to(dev)
        if decoder == "attention":
            pred, _, alphas = dec(feats[0], feats[1], c[:, :-1], lengths, pretrain=True, return_alphas=True)
        else:
            pred, _ = dec(feats, c[:, :-1], lengths, pretrain=True)
        from gan_image_captioning_amd.training import _XentFn
        want = _XentFn.apply(pred.reshape(-1, V), c[:, :pred.shape[1]].reshape(-1))
        if lam:
            want = want + lam * ((1.0 - alphas.sum(1)) ** 2).sum(1).mean()
        gw = torch.autograd.grad(want, params)
    assert torch.equal(loss, want)
    for n, a, b in zip([k for k, _ in dec.named_parameters()], got["grads"], gw):
        assert torch.equal(a, b), n
