"""What a train step inherits from the steps and calls before it (tests/step_state.py holds the contract and the tools).

Every test has the same shape: a HISTORY runs on a warm instructor W; W's carried state is snapshot; the PROBE runs on W; a fresh
instructor F is built from the same arguments and seed, the snapshot is transplanted into it, and the same probe runs on F with the
same inputs (explicit noise / keep masks where the entry takes them, else the transplanted seed counter).  W must equal F: outputs and
all carried state after the probe.  F's single step is what the golden and oracle tests pin, so W == F extends them to every later step.

Cases (``CASES``), at the smallest shapes at which their code paths exist; deterministic mode and ``exact=True`` (torch.equal)
unless said otherwise:
  lstm0-*     the tiny golden's model, --conditional-gan 0, drivers fused / autograd, fp32 / bf16
  cgan1-*     resnet18 at image size 32, V=64, E=16, H=32, B=4, L=8, fused driver, bf16 / fp32: trunk running statistics are compared
  cond-bf16   the same with --disc-cond projection, mismatch weight 0.5 (the instructor accepts deterministic mode: exact)
  seqgan-bf16 --adv-mode seqgan, mc_rollouts=2
  scst-bf16   scst.SCSTStep, 3 samples, greedy baseline (the instructor accepts deterministic mode: exact)
  pre-*       pre-training: free-running, --pretrain-mode teacher, teacher with scheduled sampling p=0.5 (coins from the seed counter)
  attn-*      --decoder attention, the fused adversarial step and the teacher pre-training step at B=3, L=5, V=52, E=8, H=16, A=16 and
              a 3x3 map (image size 96; the map's channel count is the trunk's 512, not the kernel test's 24).  This decoder refuses
              deterministic mode: ``exact=False`` -- ids exactly, losses rtol 1e-6, gradient arenas and BatchNorm buffers rtol 1e-5 /
              atol 1e-7 (the numbers of test_checkpoint_roundtrip_reproduces_the_step), post-step weights not compared.  fp32 compute:
              in bf16 one f32 last-bit difference that crosses a bf16 rounding boundary is a 2^-8 relative step, which no tolerance
              derived from f32 reduction lengths covers.  Measured on an MI355X: two correct runs (W against F) differ by at most
              0.12 x these tolerances (attn-teacher after history short; 0.06 x for attn-adv), and are not bit-equal -- so the project's
              numbers hold for the atomically added split-K partials at these shapes and no bound from the reduction length was needed.
              gen_lr = disc_lr = 1e-2, two history steps: the seeded stale weight image moves the losses by 1.9e5 x their tolerance
              (attn-adv; D's gradients 9.1e4 x, G's 5.3e3 x) and G's gradients by 8.3e4 x (attn-teacher; the loss 2.0e3 x), against
              the 10 x that test_harness_flags_seeded_carry_over_faults asks for.
  scale-bf16  the benchmark's model without the encoder (B=64, L=20, V=10000, E=H=512): histories opt and short (B=64, then B=37) only;
              split-K zero fills, deterministic slabs and partials and the 8-wave kernels engage only here.

The trunk look-ahead.  A look-ahead pass folds its batch into the trunk's running statistics when it RUNS, under the step before the
one that consumes it.  A pending look-ahead is therefore carried state that ``full_state`` cannot hold (a snapshot taken with one pending
already counts that batch; a fresh instructor would count it again when it runs the pass itself).  The ``lookahead`` history checks the
two things that can be checked: with the PREDICTED images W must equal a twin that ran the same batches with no look-ahead at all
(same passes, same order), and with OTHER images (mispredicted) W must equal the transplanted F -- the announced batch stays counted
in the running statistics on both sides, the probe's features come from a pass of its own.

The opt-in replayed step graphs (GIC_STEP_GRAPH, GIC_STEP_GRAPH_ATTN) are not covered.
"""
import random

import pytest
import torch

from tests import step_state as S
from tests import test_gpu_deterministic_steps as DS
from tests import test_gpu_step as ST

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=64, gen_embed_dim=16, gen_hidden_dim=32, image_size=32, encoder_arch="resnet18", adv_train_batch_size=4,
             adv_eval_batch_size=4, pre_train_batch_size=4, pre_eval_batch_size=4, num_workers=0)


class Case:
    """One model + one probe entry.  ``kw``: default_args overrides; ``probe``: adv | pre | scst; ``B, L``: the probe's shape."""

    def __init__(self, kw, probe="adv", exact=True, B=4, L=8, tiny=None, bench=False, with_probs=True):
        self.kw, self.probe, self.exact, self.B, self.L = kw, probe, exact, B, L
        self.tiny, self.bench, self.with_probs = tiny, bench, with_probs

    # ---- instructors
    def build(self, dev_dataset=None, **over):
        from gan_image_captioning_amd.args import default_args
        from gan_image_captioning_amd.training import GANInstructor
        torch.manual_seed(1008)
        if self.tiny is not None:
            from tests.golden_io import Golden, initial_params
            g = Golden("tiny")
            inst, _ = ST.make_instructor(g.meta, *self.tiny)
            ST.load_params(inst, *initial_params(g))
        elif self.bench:
            inst = DS._bench_instructor("bf16", "resnet50", 0)[0]
        else:
            kw = dict(SMALL, device="cuda", log_file=None, model_dir=None, save_dir=None, deterministic=int(self.exact))
            kw.update(self.kw)
            kw.update(over)
            inst = GANInstructor(default_args(**kw), None, dev_dataset)
        if self.probe == "scst":
            from gan_image_captioning_amd.cider import CiderD
            from gan_image_captioning_amd.scst import SCSTStep
            rng = random.Random(7)
            V = inst.args.vocab_size
            inst.scst_corpus = [[[rng.randrange(4, V) for _ in range(rng.randrange(1, 7))] for _ in range(rng.randrange(1, 4))] for _ in range(8)]
            scorer = CiderD(inst.scst_corpus, V, inst.args.device)
            inst.scst = SCSTStep(inst, scorer, 3, "greedy", lr=1e-3)
            inst.scst_opt = inst.scst.opt              # an optimizer of its own on G's arena: carried state (step_state._opts finds it here)
            inst._cider["scst"] = scorer
        self.train_mode(inst, True)
        return inst

    @staticmethod
    def train_mode(inst, on):
        inst.gen.train(on)
        inst.disc.train(on)

    # ---- inputs
    def batch(self, inst, B, L, seed, explicit=False):
        from gan_image_captioning_amd.tasks import synthetic_batch
        a = inst.args
        V = a.vocab_size
        images, caps, lengths, _ = synthetic_batch(B, V, a.image_size, L, seed=seed, device=a.device, with_images=bool(a.conditional_gan))
        b = {"images": images, "caps": caps, "L": L, "B": B, "u": None, "masks": None}
        if explicit:
            g = torch.Generator().manual_seed(seed + 1000)
            den = inst.disc.engine()
            n = 3 if self.probe == "scst" else 1
            b["u"] = torch.rand(L, B * n, V, generator=g).to(a.device)
            nm = 4 if inst.fused.mismatch_w > 0.0 else 3
            b["masks"] = [(torch.rand(B * den.R, den.F, generator=g) >= den.drop_p).to(torch.uint8).to(a.device) for _ in range(nm)]
        return b

    # ---- entries
    def run(self, inst, b, kind=None, train=True, next_images=None):
        kind = kind or self.probe
        if not train:
            self.train_mode(inst, False)
        try:
            if kind == "pre":
                with (torch.enable_grad() if train else torch.no_grad()):
                    loss = inst.pretrain_step(b["images"], b["caps"], b["L"], train, next_images=next_images)
                return {"loss": loss.detach().reshape(-1)}
            if kind == "scst":
                from gan_image_captioning_amd.cider import RefBatch
                refs = RefBatch.pack(inst.scst_corpus[:b["B"]]).to(inst.args.device)
                out = inst.scst(b["images"], refs, b["L"], noise_u=b["u"])
                return {k: out[k] for k in ("loss", "ids", "lengths", "rewards", "baselines")}
            a = inst.args
            if getattr(a, "adv_mode", "relgan") == "seqgan":
                out = inst.seqgan(b["images"], b["caps"], b["L"], train, next_images=next_images)
                return {k: out[k] for k in ("losses", "ids", "rewards")}
            if a.step_impl == "fused":
                out = inst.fused(b["images"], b["caps"], b["L"], train, b["u"], b["masks"], next_images=next_images)
                keys = ("losses", "ids", "probs", "logits") if self.with_probs else ("losses", "ids")
                return {k: out[k] for k in keys}
            return {"losses": inst.adv_step(b["images"], b["caps"], b["L"], train, b["u"], b["masks"], next_images=next_images)}
        finally:
            if not train:
                self.train_mode(inst, True)


def _lstm(**kw):
    return dict(conditional_gan=1, compute_dtype="bf16", **kw)


# gen_lr / disc_lr of the attention cases: chosen for the seeded stale-image fault (module docstring)
ATTN = dict(decoder="attention", attn_dim=16, conditional_gan=1, compute_dtype="fp32", vocab_size=52, gen_embed_dim=8, gen_hidden_dim=16,
            image_size=96, adv_train_batch_size=3, gen_lr=1e-2, disc_lr=1e-2)

CASES = {
    "lstm0-fused-fp32": Case({}, tiny=("fused", "fp32"), B=None, L=None),
    "lstm0-fused-bf16": Case({}, tiny=("fused", "bf16"), B=None, L=None),
    "lstm0-autograd-fp32": Case({}, tiny=("autograd", "fp32"), B=None, L=None),
    "lstm0-autograd-bf16": Case({}, tiny=("autograd", "bf16"), B=None, L=None),
    "cgan1-bf16": Case(_lstm()),
    "cgan1-fp32": Case(dict(conditional_gan=1, compute_dtype="fp32")),
    "cond-bf16": Case(_lstm(disc_cond="projection", disc_mismatch_weight=0.5)),
    "seqgan-bf16": Case(_lstm(adv_mode="seqgan", mc_rollouts=2)),
    "scst-bf16": Case(_lstm(), probe="scst"),
    "pre-free": Case(_lstm(), probe="pre"),
    "pre-teacher": Case(_lstm(pretrain_mode="teacher"), probe="pre"),
    "pre-ss": Case(_lstm(pretrain_mode="teacher", scheduled_sampling_prob=0.5), probe="pre"),
    "attn-adv": Case(ATTN, exact=False, B=3, L=5),
    "attn-teacher": Case(dict(ATTN, pretrain_mode="teacher"), probe="pre", exact=False, B=3, L=5),
    "scale-bf16": Case({}, bench=True, B=64, L=20, with_probs=False),
}


def _shape(c):
    if c.tiny is not None:
        from tests.golden_io import Golden
        m = Golden("tiny").meta
        return m["B"], m["L"]
    return c.B, c.L


@pytest.fixture
def mode():
    """Deterministic mode as the case asks for it; put back afterwards (an instructor built with deterministic=1 turns it on for good)."""
    from gan_image_captioning_amd import engine

    before = engine.deterministic()

    def set_for(case):
        engine.set_deterministic(bool(case.exact))
    yield set_for
    engine.set_deterministic(before)


# ------------------------------------------------------------------------------------------------ histories
def h_opt(c, W):
    """Two free-running training steps through the driver's own optimizer: no load_params, no manual bump_param_epoch."""
    B, L = _shape(c)
    for k in range(2):
        c.run(W, c.batch(W, B, L, 11 + k))
    return B, L


def _two_shapes(c, W):
    """((B, L), (B-1, L-1)) [scale: B=37]; where L-1 is shorter than D's widest filter, ((B, L+1), (B-1, L)) instead."""
    B, L = _shape(c)
    Bs = 37 if c.bench else B - 1
    if L - 1 >= max(W.args.disc_filter_sizes):
        return (B, L), (Bs, L - 1)
    return (B, L + 1), (Bs, L)


def h_short(c, W):
    """A step at the full shape, then the last batch of an epoch at the smaller one; the probe at the full shape."""
    big, small = _two_shapes(c, W)
    c.run(W, c.batch(W, *big, 11))
    c.run(W, c.batch(W, *small, 12))
    return big


def h_short_mirror(c, W):
    """The larger shape last, the probe at the smaller one."""
    big, small = _two_shapes(c, W)
    c.run(W, c.batch(W, *small, 12))
    c.run(W, c.batch(W, *big, 11))
    return small


def h_eval(c, W):
    """A training step, a train=False step at another batch size (the eval loaders'), then the probe in training mode.  Under
    --conditional-gan 1 the eval step must leave every running buffer and num_batches_tracked bit-identical."""
    B, L = _shape(c)
    c.run(W, c.batch(W, B, L, 11))
    before = {k: v.clone() for k, v in S.full_state(W).items() if k.startswith(("gen.", "disc."))}
    c.run(W, c.batch(W, B + 2, L, 12), train=False)
    torch.cuda.synchronize()
    if W.cgan:
        for k, v in S.full_state(W).items():
            if k in before:
                assert torch.equal(v, before[k]), f"{k} moved during a validation batch: {S._first_diff(v, before[k])}"
    return B, L


def h_phase(c, W):
    """The other phase first: pre-training steps before an adversarial probe, adversarial steps before a pre-training probe
    (pretrain_opt and gen_opt share one arena)."""
    B, L = _shape(c)
    other = "pre" if c.probe == "adv" else "adv"
    for k in range(2):
        c.run(W, c.batch(W, B, L, 11 + k), kind=other)
    return B, L


def _decodes(c, W, b):
    """Beam search, top-k / nucleus sampling, caption log-likelihood and one evaluation, in eval mode as the trainer runs them."""
    W.gen.eval()
    try:
        W.gen.caption(b["images"] if W.cgan else b["caps"], beam_size=3, max_caption_len=b["L"])
        W.gen.sample_captions(b["images"] if W.cgan else b["caps"], num_samples=2, top_k=5, top_p=0.9, max_caption_len=b["L"], seed=7)
        W.gen.score_captions(b["images"] if W.cgan else b["caps"], b["caps"], [b["L"]] * b["B"])
    finally:
        W.gen.train()
    W.evaluate("val", beam_size=2)


def h_decode(c, W):
    B, L = _shape(c)
    c.run(W, c.batch(W, B, L, 11))
    _decodes(c, W, c.batch(W, B + 1, L, 13))
    c.run(W, c.batch(W, B, L, 12))
    return B, L


HISTORIES = {"opt": h_opt, "short": h_short, "short_mirror": h_short_mirror, "eval": h_eval, "phase": h_phase, "decode": h_decode}

_ADV_PRE = [n for n, c in CASES.items() if n != "scale-bf16"]
PAIRS = ([(n, "opt") for n in CASES] + [(n, "short") for n in CASES] + [(n, "short_mirror") for n in _ADV_PRE]
         + [(n, "eval") for n in _ADV_PRE if CASES[n].probe != "scst"]
         + [(n, "phase") for n in ("lstm0-fused-bf16", "lstm0-autograd-fp32", "cgan1-bf16", "cond-bf16", "pre-teacher", "attn-adv")]
         + [(n, "decode") for n in ("cgan1-bf16", "cgan1-fp32", "pre-teacher", "attn-adv")])


def _dev_dataset(c):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    kw = dict(SMALL, **c.kw)
    return SyntheticCaptionData(5, kw["vocab_size"], image_size=kw["image_size"], caption_len=6)


def _warm_vs_fresh(c, name, history, probe=None, build_kw=None):
    """history on W -> snapshot -> probe on W -> transplant into F -> probe on F -> compare."""
    build_kw = build_kw or {}
    W = c.build(**build_kw)
    B, L = HISTORIES[history](c, W) if isinstance(history, str) else history(c, W)
    torch.cuda.synchronize()
    snap = S.snapshot(W)
    b = c.batch(W, B, L, 21, explicit=True)
    probe = probe or (lambda inst: c.run(inst, b))
    w_rec = S.record(W, probe(W))
    F = S.transplant(snap, c.build(**build_kw))
    f_rec = S.record(F, probe(F))
    what = f"{name} after {history if isinstance(history, str) else history.__name__} (warm / fresh)"
    S.compare(w_rec, f_rec, c.exact, what)
    return W, F, snap, w_rec


@pytest.mark.parametrize("name,history", PAIRS, ids=[f"{n}-{h}" for n, h in PAIRS])
def test_warm_step_equals_fresh_step(mode, name, history):
    c = CASES[name]
    mode(c)
    kw = {"dev_dataset": _dev_dataset(c)} if history == "decode" else {}
    _warm_vs_fresh(c, name, history, build_kw=kw)


# ------------------------------------------------------------------------------------------------ decode after training
@pytest.mark.parametrize("name", ["lstm0-fused-bf16", "cgan1-bf16", "cgan1-fp32", "attn-adv"])
def test_decode_after_training_reads_the_trained_weights(mode, name):
    """Two training steps, then a beam-decode probe and a sampling probe: ids, scores and lengths must equal F's -- a decode that still
    reads the weight image from before the optimizer steps differs.  Eval mode: the trunk runs on its running statistics, no f32
    atomics, so the attention decoder's searches are compared exactly too (its decode kernels add nothing atomically)."""
    c = CASES[name]
    mode(c)

    def probe(inst):
        B, L = _shape(c)
        b = c.batch(inst, B + 1, L, 31)
        src = b["images"] if inst.cgan else b["caps"]
        inst.gen.eval()
        try:
            ids, scores, lengths = inst.gen.caption(src, beam_size=3, max_caption_len=L)[:3]
            s_ids, s_scores, s_len = inst.gen.sample_captions(src, num_samples=2, top_k=5, top_p=0.9, max_caption_len=L, seed=9)
        finally:
            inst.gen.train()
        return {"beam_ids": ids, "beam_scores": scores, "beam_lengths": lengths, "sample_ids": s_ids, "sample_scores": s_scores,
                "sample_lengths": s_len}
    W = c.build()
    h_opt(c, W)
    torch.cuda.synchronize()
    snap = S.snapshot(W)
    w_rec = S.record(W, probe(W))
    F = S.transplant(snap, c.build())
    f_rec = S.record(F, probe(F))
    S.compare(w_rec, f_rec, True, f"{name}: decode after two training steps (warm / fresh)")


# ------------------------------------------------------------------------------------------------ reload
@pytest.mark.parametrize("how", ["state_dict", "checkpoint", "copy", "flat_bump"])
@pytest.mark.parametrize("name", ["lstm0-fused-bf16", "cgan1-bf16"])
def test_reloaded_weights_are_the_weights_the_next_step_reads(mode, tmp_path, name, how):
    """Weights saved at step 0 come back after a training step -- through load_state_dict, load_checkpoint of a file written by _save,
    p.copy_() under no_grad, or a write through arena.flat followed by engine.bump_param_epoch() (the contract of tests/step_state.py) --
    and the probe must equal a fresh instructor holding the same state: no weight image of the trained weights survives."""
    from gan_image_captioning_amd import engine
    c = CASES[name]
    mode(c)

    def history(c, W):
        B, L = _shape(c)
        gen0 = {k: v.detach().clone() for k, v in W.gen.state_dict().items()}
        disc0 = {k: v.detach().clone() for k, v in W.disc.state_dict().items()}
        flat0 = (W.gen_arena.flat.clone(), W.disc_arena.flat.clone())
        params0 = [p.detach().clone() for p in W.gen_arena.params + W.disc_arena.params]
        W.model_dir = str(tmp_path)
        W._save({"generator": W.gen.state_dict(), "discriminator": W.disc.state_dict()}, "adv_model.ckpt")
        c.run(W, c.batch(W, B, L, 11))
        torch.cuda.synchronize()
        assert not torch.equal(W.gen_arena.flat, flat0[0]) and not torch.equal(W.disc_arena.flat, flat0[1])
        if how == "state_dict":
            W.gen.load_state_dict(gen0)
            W.disc.load_state_dict(disc0)
        elif how == "checkpoint":
            assert W.load_checkpoint(str(tmp_path / "adv_model.ckpt")) == "adversarial"
        elif how == "copy":
            with torch.no_grad():
                for p, v in zip(W.gen_arena.params + W.disc_arena.params, params0):
                    p.copy_(v)
        else:
            with torch.no_grad():
                W.gen_arena.flat.copy_(flat0[0])
                W.disc_arena.flat.copy_(flat0[1])
            engine.bump_param_epoch()
        torch.cuda.synchronize()
        assert torch.equal(W.gen_arena.flat, flat0[0]) and torch.equal(W.disc_arena.flat, flat0[1]), "the reload left other weights"
        return B, L
    history.__name__ = "reload:" + how
    _warm_vs_fresh(c, name, history)


# ------------------------------------------------------------------------------------------------ trunk look-ahead
@pytest.mark.parametrize("name", ["cgan1-bf16", "cgan1-fp32", "cond-bf16", "pre-teacher"])
def test_lookahead_history_leaves_nothing_behind(mode, name):
    """History steps pass next_images (module docstring).  Predicted: W (look-ahead consumed by the probe) equals a twin that ran the same
    batches with no look-ahead.  Mispredicted: the probe gets other images than the pending look-ahead's; W equals the transplanted F."""
    c = CASES[name]
    mode(c)
    B, L = _shape(c)

    def batches(inst):
        return [c.batch(inst, B, L, 11 + k) for k in range(3)]
    W, twin = c.build(), c.build()
    bw, bt = batches(W), batches(twin)
    snap0 = S.snapshot(W)
    S.transplant(snap0, twin)
    n0 = snap0.scalars["seed_n"]                   # the seed counter is one per process: the two histories run one after the other
    from gan_image_captioning_amd.generator import SEEDS
    for k in range(2):
        c.run(W, bw[k], next_images=bw[k + 1]["images"])
    assert W.gen.encoder._pre is not None and W.gen.encoder._pre[0] is bw[2]["images"], "the history left no look-ahead pending"
    torch.cuda.synchronize()
    snap = S.snapshot(W)                           # for the mispredicted probe below
    pw = dict(c.batch(W, B, L, 21, explicit=True), images=bw[2]["images"])
    w_rec = S.record(W, c.run(W, pw))
    assert W.gen.encoder._pre is None
    SEEDS.reset(n0)
    for k in range(2):
        c.run(twin, bt[k])
    t_rec = S.record(twin, c.run(twin, dict(pw, images=bt[2]["images"])))
    S.compare(w_rec, t_rec, c.exact, f"{name}: look-ahead consumed (warm with look-ahead / twin without)")
    # mispredicted: W goes back to its first state and runs the same look-ahead history again; the probe then gets other images
    # than the pending look-ahead's
    S._restore(W, snap0)
    for k in range(2):
        c.run(W, bw[k], next_images=bw[k + 1]["images"])
    assert W.gen.encoder._pre is not None
    torch.cuda.synchronize()
    snap2 = S.snapshot(W)
    if c.exact:
        for k in snap[0]:
            assert torch.equal(snap[0][k], snap2[0][k]), f"{name}: {k}: the same look-ahead history twice: {S._first_diff(snap[0][k], snap2[0][k])}"
    other = c.batch(W, B, L, 22, explicit=True)
    w2_rec = S.record(W, c.run(W, other))
    F = S.transplant(snap2, c.build())
    f_rec = S.record(F, c.run(F, other))
    S.compare(w2_rec, f_rec, c.exact, f"{name}: look-ahead mispredicted (warm / fresh)")


# ------------------------------------------------------------------------------------------------ poison
def _poison_case(c, name):
    W = c.build()
    B, L = h_opt(c, W)
    torch.cuda.synchronize()
    snap = S.snapshot(W)
    b = c.batch(W, B, L, 21, explicit=True)
    clean = S.record(W, c.run(W, b))
    S._restore(W, snap)
    written = S.poison(W)
    assert any("dec_engine._shadow" in p for p in written) and len(written) > 4, written
    dirty = S.record(W, c.run(W, b))
    try:
        S.compare(dirty, clean, c.exact, f"{name}: poisoned workspaces / clean (same warm state)")
    except AssertionError as exc:
        def fails(subset):
            S._restore(W, snap)
            S.poison(W, only=subset)
            try:
                S.compare(S.record(W, c.run(W, b)), clean, c.exact)
            except AssertionError:
                return True
            return False
        culprit = S.bisect(written, fails)
        raise AssertionError(f"{exc}\nread before written: {culprit or 'no single buffer reproduces it'}") from None


@pytest.mark.parametrize("name", list(CASES))
def test_poisoned_workspaces_change_nothing(mode, name):
    """After history opt every scratch buffer is overwritten (NaN; valid other values in integer buffers) and every weight image is
    poisoned and invalidated; the probe must give what it gives from the same state unpoisoned: bit-identical under exact=True,
    NaN-free and within the tolerances under exact=False.  A NaN anywhere is a read of a leftover before it was written; the failure
    names the buffer if halving the poisoned list identifies one.  This also asserts that ``workspaces`` places every persistent tensor."""
    c = CASES[name]
    mode(c)
    _poison_case(c, name)


def test_every_persistent_tensor_is_classified(mode):
    """After the calls that leave the most behind -- an eval step (the encoder head's saved forward state), evaluations (scorers), a
    pending look-ahead, SCST -- ``workspaces`` still places every tensor, and the three classes are all populated."""
    c = CASES["scst-bf16"]
    mode(c)
    W = c.build(dev_dataset=_dev_dataset(c))
    B, L = _shape(c)
    c.run(W, c.batch(W, B, L, 11))
    c.run(W, c.batch(W, B, L, 12), kind="adv", train=False)
    c.run(W, c.batch(W, B, L, 15), kind="pre")
    W.evaluate_cider("val", beam_size=2)
    nxt = c.batch(W, B, L, 14)["images"]
    c.run(W, c.batch(W, B, L, 13), kind="adv", next_images=nxt)
    torch.cuda.synchronize()
    entries = S.workspaces(W)
    kinds = {k: [e.path for e in entries if e.kind == k] for k in (S.SCRATCH, S.INVARIANT, S.TABLE)}
    assert all(kinds.values()), kinds
    assert any(p.endswith("['ydrop'][:, F:]") for p in kinds[S.INVARIANT]) and any("_pre[" in p for p in kinds[S.INVARIANT])
    assert any("['table']" in p for p in kinds[S.TABLE])
    held = {t.untyped_storage().data_ptr() for t in S.full_state(W).values()}
    assert not any(e.tensor.untyped_storage().data_ptr() in held for e in entries)


# ------------------------------------------------------------------------------------------------ the checker must be shown to see
def _flags(c, name, fault, history=h_opt):
    """True if compare() raises for W (with ``fault`` applied) against F."""
    W = c.build()
    with fault.get("during_history", _Null)(W):
        B, L = history(c, W)
    torch.cuda.synchronize()
    snap = S.snapshot(W)
    if "after_snapshot" in fault:
        fault["after_snapshot"](W)
    b = c.batch(W, B, L, 21, explicit=True)
    with fault.get("during_probe", _Null)(W):
        w_rec = S.record(W, c.run(W, b))
    F = S.transplant(snap, c.build())
    f_rec = S.record(F, c.run(F, b))
    try:
        S.compare(w_rec, f_rec, c.exact, name)
    except AssertionError:
        return True, S.excess(w_rec, f_rec)
    return False, S.excess(w_rec, f_rec)


class _Null:
    def __init__(self, inst):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _Patched(_Null):
    """Replace ``owner.attr`` by ``value`` for the duration."""
    owner, attr, value = None, "", None

    def __enter__(self):
        self.saved = getattr(self.owner, self.attr)
        setattr(self.owner, self.attr, self.value)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.attr, self.saved)
        return False


def _patch(owner, attr, value):
    return type("_P", (_Patched,), {"owner": owner, "attr": attr, "value": staticmethod(value)})


def test_harness_flags_seeded_carry_over_faults(mode):
    """Each fault is applied to W only, in Python; no kernel changes.
      * engine.bump_param_epoch is a no-op during the history's optimizer steps: the probe reads the weight images of step 0.  Flagged
        in bf16 AND in fp32: fp32 mode keeps images too (the decoder's concatenated [W_ih | W_hh], its transpose and the summed biases;
        the discriminator's padded highway and feature2out weights), only the vocabulary projection and D's embedding are read in place.
        In the exact=False family (attention) the fault moves a compared quantity by at least 10 x its tolerance.
      * ParamArena.zero_grad is a no-op on the autograd driver: gradients accumulate across steps.
      * a real carrier is changed after the snapshot: Adam's exp_avg, and a trunk BatchNorm running_mean."""
    from gan_image_captioning_amd import engine, optim
    stale = {"during_history": _patch(engine, "bump_param_epoch", lambda: None)}
    for name in ("lstm0-fused-bf16", "lstm0-fused-fp32", "cgan1-bf16", "seqgan-bf16", "pre-teacher"):
        c = CASES[name]
        mode(c)
        assert _flags(c, name, stale)[0], f"{name}: a stale weight image was not flagged"
    for name in ("attn-adv", "attn-teacher"):
        c = CASES[name]
        mode(c)
        flagged, ex = _flags(c, name, stale)
        assert flagged and max(ex.values()) >= 10.0, f"{name}: a stale weight image moved the compared quantities by {ex} x their tolerance"

    c = CASES["lstm0-autograd-bf16"]
    mode(c)
    keep = _patch(optim.ParamArena, "zero_grad", lambda self: None)
    assert _flags(c, "lstm0-autograd-bf16", {"during_history": keep, "during_probe": keep})[0], "accumulated gradients were not flagged"

    def bad_moment(W):
        W.gen_opt.exp_avg.add_(1e-3)

    def bad_running_mean(W):
        W.gen.encoder.resnet.get_submodule("1").running_mean.add_(0.25)
    c = CASES["cgan1-bf16"]
    mode(c)
    assert _flags(c, "cgan1-bf16", {"after_snapshot": bad_moment})[0], "a changed Adam moment was not flagged"
    assert _flags(c, "cgan1-bf16", {"after_snapshot": bad_running_mean})[0], "a changed BatchNorm running mean was not flagged"
