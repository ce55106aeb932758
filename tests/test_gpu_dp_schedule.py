"""The data-parallel gradient schedule of every train step, on ONE GPU, against a simulated second rank (tests/dp_sim.py).

Every step type that calls ``GradReducer`` runs with the production reducer attached and a NON-identity collective: the fake
``all_reduce`` averages the span it is handed with the same span of a second rank's gradient, on the stream the reducer put it on.
An optimizer that does not wait for its collective, a collective started before the backward that fills its span has finished, a span
that is never reduced and a span reduced twice all change VALUES, which a one-rank communicator (an identity) cannot show.

Protocol per case (global B = 8 as two shards of 4, L = 6, V = 64, E = 16, H = 32, R = 64; two optimizer steps).  Two instructors with
identical weights: P plain, Q rank 0 of the pair.  Per step:
  1. P runs the step on shard 0, then on shard 1, its optimizer steps skipped by the interceptor: g0, g1 per arena;
  2. Q runs the step on shard 0 with the fake collective supplying g1, real optimizer steps;
  3. P sets each arena's gradient to (g0 + g1) * 0.5 -- the collective's two f32 operations -- and calls its real ``step()``.
Noise is identical between P's shard-0 run and Q's run: explicit where the step takes it, and the seed counter is reset before every call.

Asserted (``Report.faults``):
  a. the ledger tiles every arena exactly once per optimizer step; ``reducer._pending`` is empty after the step;
  b. the optimizer read the average: Q's intercepted gradient equals (in + g1[lo:hi]) * 0.5 span by span, bit for bit, in every mode;
  c. the collective read a complete gradient: its input snapshot equals P's g0 on the span -- bit for bit in deterministic mode;
     for the attention decoder (refused in deterministic mode) within 8 x the run-to-run spread of g0 measured on an MI355X
     (``ATTN_SPREAD``, relative to max|g0| of the arena; a missing backward is off by O(1));
  d. Q's losses and ids equal P's shard-0 values; after each step Q's arenas and both Adam moments equal P's (bit for bit in
     deterministic mode; else ids exactly, losses rtol 1e-5 / atol 1e-7 and the rest rtol 1e-4 / atol 2e-6, the numbers of
     tests/test_gpu_dp.py); ``grad_norm`` is the averaged gradient's;
  e. where the loss is a plain per-row mean with no batch statistics (--conditional-gan 0: fused LSTM, SeqGAN LSTM, free-running
     pre-training) P's step on all 8 rows gives (g0 + g1) / 2 within the tolerances of tests/test_gpu_dp.py.
     (--pretrain-ignore-pad 1: each shard normalises by its own token count; the defined behaviour is the mean of the shard
     gradients, nothing is asserted against the global batch.)
In the attention cases P adopts Q's weights and moments after step 1's comparison, so that step 2's bound (c) again compares two
backward passes from identical weights: the only difference left is the order of the f32 atomic adds, which is what was measured.

Forced timing (fused LSTM, fused attention, both SeqGAN cases): ``slow-collective`` -- the fake enqueues a fixed ~2 ms device-side
delay on its stream before it touches ``flat``; ``slow-producer`` -- every backward entry of the step enqueues the same delay on the
current stream before the real call.  An ordering bug then shows deterministically instead of by luck -- provided the streams
involved really run concurrently: two streams that share a hardware queue run in submission order, and which streams share one
depends on how many the process created before.  Under forced timing the reducer's side stream is therefore chosen by measurement
(``dp_sim.concurrent_stream``) so that it overtakes, and is overtaken by, the main stream and the generator path's stream.

``test_checker_flags_schedule_faults`` seeds schedule faults on Q's reducer object (``seed_fault``) and asserts that each is reported.
"""
import random

import pytest
import torch

from tests import dp_sim as S

pytestmark = pytest.mark.gpu

B, SH, L, V, E, H = 8, 4, 6, 64, 16, 32
BASE = dict(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, compute_dtype="fp32", clip_norm=0.05, adv_train_batch_size=SH,
            adv_eval_batch_size=SH, pre_train_batch_size=SH, pre_eval_batch_size=SH, num_workers=0, device="cuda", log_file=None,
            model_dir=None, save_dir=None)
TRUNK = dict(conditional_gan=1, image_size=32, encoder_arch="resnet18")
ATTN = dict(TRUNK, decoder="attention", attn_dim=32)
TEACHER = dict(TRUNK, pretrain_mode="teacher")

# tolerances of tests/test_gpu_dp.py (two ranks against the single process)
RTOL, ATOL = 1e-4, 2e-6                  # weights, moments, gradients
LOSS_RTOL, LOSS_ATOL = 1e-5, 1e-7        # losses

# Run-to-run spread of g0 in the attention cases (the decoder's split-K products and D's weight gradients add f32 partials atomically):
# the largest element-wise difference between plain runs of P's shard-0 backward from identical weights and noise, relative to max|g0| of
# the arena, measured on an MI355X at these shapes (``measure_spread``: 20 runs on each step's inputs).  Bound (c) allows 8 x that.
ATTN_SPREAD = {"fused-attention": {"gen": 2.47e-7, "disc": 1.40e-6}, "seqgan-attention": {"gen": 2.65e-7, "disc": 1.40e-6}}


class Case:
    def __init__(self, kind, kw, det=True, glob=False, pads=False, baseline="greedy"):
        self.kind, self.kw, self.det, self.glob, self.pads, self.baseline = kind, dict(BASE, **kw), det, glob, pads, baseline


CASES = {
    "fused-lstm-cgan0": Case("fused", dict(conditional_gan=0), glob=True),
    "fused-lstm-cgan1": Case("fused", TRUNK),
    "fused-lstm-bf16": Case("fused", dict(conditional_gan=0, compute_dtype="bf16")),
    "fused-rsgan": Case("fused", dict(conditional_gan=0, adv_loss_type="rsgan")),
    "fused-attention": Case("fused", ATTN, det=False),
    "fused-cond-projection": Case("fused", dict(TRUNK, disc_cond="projection", disc_mismatch_weight=0.5)),
    "fused-real-as-ids0": Case("fused", dict(conditional_gan=0, real_as_ids=0)),
    "seqgan-lstm": Case("seqgan", dict(conditional_gan=0, adv_mode="seqgan", mc_rollouts=2), glob=True),
    "seqgan-attention": Case("seqgan", dict(ATTN, adv_mode="seqgan", mc_rollouts=2), det=False),
    "autograd": Case("autograd", dict(conditional_gan=0, step_impl="autograd")),
    "pretrain-free": Case("pre", dict(conditional_gan=0), glob=True),
    "pretrain-teacher": Case("pre", TEACHER),
    "pretrain-teacher-sched-sampling": Case("pre", dict(TEACHER, scheduled_sampling_prob=0.5)),
    "pretrain-teacher-ignore-pad": Case("pre", dict(TEACHER, pretrain_ignore_pad=1, label_smoothing=0.1), pads=True),
    "scst-greedy": Case("scst", TRUNK, baseline="greedy"),
    "scst-mean": Case("scst", TRUNK, baseline="mean"),
}
TIMED = ["fused-lstm-cgan0", "fused-attention", "seqgan-lstm", "seqgan-attention"]
SCST_SAMPLES = 3


@pytest.fixture
def mode():
    """Deterministic mode as the case asks for it; put back afterwards (an instructor built with deterministic=1 turns it on for good)."""
    from gan_image_captioning_amd import engine
    before = engine.deterministic()
    yield engine.set_deterministic
    engine.set_deterministic(before)


# ------------------------------------------------------------------------------------------------ instructors and inputs
def build(c):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    torch.manual_seed(1008)
    inst = GANInstructor(default_args(deterministic=int(c.det), **c.kw), None, None)
    inst.gen.train()
    inst.disc.train()
    if c.kind == "scst":
        from gan_image_captioning_amd.cider import CiderD
        from gan_image_captioning_amd.scst import SCSTStep
        rng = random.Random(7)
        inst.scst_corpus = [[[rng.randrange(4, V) for _ in range(rng.randrange(1, 7))] for _ in range(rng.randrange(1, 4))] for _ in range(B)]
        inst.scst = SCSTStep(inst, CiderD(inst.scst_corpus, V, inst.args.device), SCST_SAMPLES, c.baseline, lr=1e-3)
    return inst


def optimizers(inst):
    o = {"gen_opt": (S.GEN, inst.gen_opt), "disc_opt": (S.DISC, inst.disc_opt), "pretrain_opt": (S.GEN, inst.pretrain_opt)}
    if hasattr(inst, "scst"):
        o["scst_opt"] = (S.GEN, inst.scst.opt)
    return o


def arenas(inst):
    return {S.GEN: inst.gen_arena, S.DISC: inst.disc_arena}


def param_names(inst):
    names = {id(p): "gen." + n for n, p in inst.gen.named_parameters()}
    names.update({id(p): "disc." + n for n, p in inst.disc.named_parameters()})
    return names


def attach_reducer(inst):
    """The production reducer, forced to run its collectives with one rank, wherever a step reads it."""
    from gan_image_captioning_amd import parallel
    from gan_image_captioning_amd.fused_step import FusedAdvStep
    red = parallel.GradReducer(parallel.DistInfo(0, 0, 1), force=True)
    inst.reducer = red
    inst.fused = FusedAdvStep(inst.gen, inst.disc, inst.gen_arena, inst.disc_arena, inst.args, red).bind_optimizers(inst.gen_opt, inst.disc_opt)
    inst.seqgan.reducer = red
    return red


def shard_inputs(c, inst, k, r):
    """Inputs of step ``k`` for shard ``r`` (4 rows), drawn on the host from a seed of their own."""
    g = torch.Generator().manual_seed(1000 + 10 * k + r)
    a = inst.args
    dev = a.device
    den = inst.disc.engine()
    body = torch.randint(4, V, (SH, L - 2), generator=g)
    caps = torch.cat([torch.ones(SH, 1, dtype=torch.long), body, torch.full((SH, 1), 2, dtype=torch.long)], 1)
    if c.pads:                           # <PAD> tails of different lengths: the two shards hold different token counts
        for row in range(SH):
            n = (row + 2 * r) % 3 + r
            if n:
                caps[row, L - n:] = int(a.padding_idx)
    s = {"caps": caps.to(dev), "images": None, "row0": r * SH}
    if int(a.conditional_gan):
        s["images"] = torch.randn(SH, 3, a.image_size, a.image_size, generator=g).to(dev)
    n = SCST_SAMPLES if c.kind == "scst" else 1
    s["u"] = torch.rand(L, SH * n, V, generator=g).to(dev)
    s["masks"] = [(torch.rand(SH * den.R, den.F, generator=g) >= den.drop_p).to(torch.uint8).to(dev) for _ in range(4)]
    if c.kind == "seqgan":
        s["u_mc"] = torch.rand(L, (L - 1) * inst.seqgan.N * SH, V, generator=g).to(dev)
    return s


def global_inputs(c, s0, s1):
    """The 8-row batch whose shards are ``s0`` and ``s1`` (the (e) cases: no images): rows, noise columns and mask rows concatenated."""
    s = {"caps": torch.cat([s0["caps"], s1["caps"]], 0), "images": None, "row0": 0,
         "u": torch.cat([s0["u"], s1["u"]], 1), "masks": [torch.cat([m0, m1], 0) for m0, m1 in zip(s0["masks"], s1["masks"])]}
    if "u_mc" in s0:                     # rows of the roll-out batch are (prefix length, roll-out, caption): the caption index is innermost
        reps = s0["u_mc"].shape[1] // SH
        s["u_mc"] = torch.cat([s0["u_mc"].view(L, reps, SH, V), s1["u_mc"].view(L, reps, SH, V)], 2).reshape(L, reps * B, V)
    return s


def call(c, inst, s, seed):
    from gan_image_captioning_amd.generator import SEEDS
    torch.manual_seed(1008)
    SEEDS.reset(seed)
    nm = 4 if inst.fused.mismatch_w > 0.0 else 3
    if c.kind == "fused":
        out = inst.fused(s["images"], s["caps"], L, True, s["u"], s["masks"][:nm])
        return {"losses": out["losses"], "ids": out["ids"]}
    if c.kind == "seqgan":
        out = inst.seqgan(s["images"], s["caps"], L, True, s["u"], s["u_mc"], s["masks"][:2])
        return {"losses": out["losses"], "ids": out["ids"], "rewards": out["rewards"]}
    if c.kind == "autograd":
        return {"losses": inst._adv_step_autograd(s["images"], s["caps"], L, True, s["u"], s["masks"][:nm])}
    if c.kind == "pre":
        with torch.enable_grad():
            return {"loss": inst.pretrain_step(s["images"], s["caps"], L, True).detach().reshape(-1)}
    from gan_image_captioning_amd.cider import RefBatch
    n = s["caps"].shape[0]
    refs = RefBatch.pack(inst.scst_corpus[s["row0"]:s["row0"] + n]).to(inst.args.device)
    with torch.enable_grad():
        out = inst.scst(s["images"], refs, L, noise_u=s["u"])
    return {"loss": out["loss"].reshape(-1), "ids": out["ids"], "rewards": out["rewards"]}


def _clone(out):
    return {k: v.detach().clone() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ forced timing, seeded faults
def slow_producers(monkeypatch, inst, delay):
    """Every backward entry of Q's steps enqueues ``delay`` on the current stream before the real call."""
    dec, den = inst.gen.decoder.engine(), inst.disc.engine()
    for owner, names in ((dec, ("sample_bwd", "forward_tf_bwd")), (den, ("bwd", "img_proj_bwd")), (inst.gen.encoder, ("backward_fused",))):
        for n in names:
            real = getattr(owner, n, None)
            if real is None:
                continue

            def slowed(*a, _real=real, **k):
                delay()
                return _real(*a, **k)
            monkeypatch.setattr(owner, n, slowed)


def seed_fault(fault, red, inst, idle=None):
    """One schedule fault on Q's reducer object: value-level races inside the test's own buffers.  ``idle``: the idle stream of
    ``ready_on_idle_stream`` (one that does not queue behind the producer's stream)."""
    real_start = red.start
    gen, disc = inst.gen_arena, inst.disc_arena
    if fault == "wait_all_noop":                     # G's optimizer no longer waits for its collectives
        red.wait_all = lambda: None
    elif fault == "wait_noop":                       # D's Adam no longer waits for D's collective (wait_all comes after it)
        red.wait = lambda done: None
    elif fault == "drop_tail":                       # the span behind the early bucket is silently not reduced
        e1 = inst.fused._early_bucket()[1]
        assert 0 < e1 < gen.numel
        red.start = lambda flat: None if flat.data_ptr() == gen.grad[e1:].data_ptr() else real_start(flat)
    elif fault == "double_disc":                     # D's arena reduced twice
        def twice(flat):
            ev = real_start(flat)
            return real_start(flat) if flat.data_ptr() == disc.grad.data_ptr() else ev
        red.start = twice
    elif fault == "ready_on_idle_stream":            # the ``ready`` event is recorded on a fresh idle stream, not on the producer's
        def misplaced(flat):
            with torch.cuda.stream(idle):
                return real_start(flat)
        red.start = misplaced
    else:
        raise AssertionError(fault)


# ------------------------------------------------------------------------------------------------ the protocol
class Report:
    def __init__(self):
        self.faults = {k: [] for k in "abcde"}
        self.figures = {}

    def add(self, key, step, msgs):
        self.faults[key] += [f"step {step}: {m}" for m in ([msgs] if isinstance(msgs, str) else msgs)]

    def fig(self, key, value):
        self.figures[key] = max(self.figures.get(key, 0.0), float(value))

    def all(self):
        return [f"({k}) {m}" for k, v in self.faults.items() for m in v]


def _mismatch(got, want, exact, rtol=RTOL, atol=ATOL):
    """None if ``got`` equals ``want`` (bit for bit, or within ``rtol`` / ``atol``), else a short description."""
    if got.shape != want.shape:
        return f"shapes {tuple(got.shape)} / {tuple(want.shape)}"
    if exact or not got.is_floating_point():
        if torch.equal(got, want):
            return None
        ne = (got != want)
        i = int(ne.reshape(-1).nonzero()[0])
        return f"{int(ne.sum())} of {got.numel()} elements differ, first at {i}: {got.reshape(-1)[i].item()!r} / {want.reshape(-1)[i].item()!r}"
    bad = (got - want).abs() > atol + rtol * want.abs()
    bad |= ~torch.isfinite(got)
    if not bool(bad.any()):
        return None
    i = int(bad.reshape(-1).nonzero()[0])
    return (f"{int(bad.sum())} of {got.numel()} elements outside rtol {rtol} / atol {atol}, first at {i}: "
            f"{got.reshape(-1)[i].item()!r} / {want.reshape(-1)[i].item()!r}")


def run_case(name, monkeypatch, timing=None, fault=None, steps=2):
    from gan_image_captioning_amd import engine
    c = CASES[name]
    P, Q = build(c), build(c)
    for a in (S.GEN, S.DISC):
        assert torch.equal(arenas(P)[a].flat, arenas(Q)[a].flat), "the two instructors do not start from the same weights"
    red = attach_reducer(Q)
    delay = S.Delay(2.0) if timing is not None or fault in ("wait_all_noop", "wait_noop", "ready_on_idle_stream") else None
    slow_coll = timing == "slow-collective" or fault in ("wait_all_noop", "wait_noop")
    if timing == "slow-producer" or fault == "ready_on_idle_stream":
        slow_producers(monkeypatch, Q, delay)
    fake = S.FakeCollective(arenas(Q), {}, delay=delay if slow_coll else None)
    S.attach(monkeypatch, fake)
    idle = None
    if delay is not None:
        # Forced timing shows an ordering fault only between streams that really run concurrently (dp_sim.concurrent_stream): the
        # reducer's side stream is chosen, by measurement, off the hardware queues of the streams that produce and consume gradients
        dev = torch.device("cuda", torch.cuda.current_device())
        busy = [torch.cuda.current_stream(dev), Q.fused._streams(dev)[1]]
        tried = []
        red._side = S.concurrent_stream(busy, delay, log=tried)
        assert red._side is not None, "no stream runs concurrently with the step's streams: forced timing cannot show anything"
        if fault == "ready_on_idle_stream":
            idle = S.concurrent_stream(busy + [red._side], delay)
            assert idle is not None, "no idle stream off the producer's hardware queue"
    if fault is not None:
        seed_fault(fault, red, Q, idle)
    ic_p = S.OptInterceptor(optimizers(P), None, "skip")
    ic_q = S.OptInterceptor(optimizers(Q), fake.ledger, "call")
    names = param_names(Q)
    rep = Report()
    if delay is not None:
        rep.fig("side_stream_candidates", tried[0])
    exact = c.det
    bounds = None if exact else {a: 8.0 * v for a, v in ATTN_SPREAD[name].items()}

    def grads_of(n_before):
        return {a: ic_p.seen[a][-1] for a in ic_p.seen if len(ic_p.seen[a]) > n_before[a]}

    for k in range(steps):
        s0, s1 = shard_inputs(c, P, k, 0), shard_inputs(c, P, k, 1)
        # 1. P: the two shards' gradients, optimizer steps skipped
        ic_p.mode = "skip"
        shards = []
        for r, s in enumerate((s0, s1)):
            n_before = {a: len(v) for a, v in ic_p.seen.items()}
            out = _clone(call(c, P, s, 100 * (k + 1) + 10 * r))
            torch.cuda.synchronize()
            shards.append((out, grads_of(n_before)))
        (out0, g0), (_, g1) = shards
        assert g0.keys() == g1.keys() and g0, "no optimizer step was intercepted on the plain instructor"
        avg = {a: torch.add(g0[a], g1[a]).mul_(0.5) for a in g0}
        if c.glob:                       # e. the global batch in one process
            n_before = {a: len(v) for a, v in ic_p.seen.items()}
            call(c, P, global_inputs(c, s0, s1), 100 * (k + 1) + 50)
            torch.cuda.synchronize()
            for a, g in grads_of(n_before).items():
                m = _mismatch(g, avg[a], False)
                rep.fig(f"e.{a}.max_abs_diff", (g - avg[a]).abs().max())
                if m:
                    rep.add("e", k, f"{a}: the global-batch gradient is not the mean of the shard gradients: {m}")
        # 2. Q: shard 0 with the collective supplying g1, real optimizer steps
        fake.other = g1
        n_calls = len(ic_q.calls)
        n_win = {a: len(fake.ledger.windows[a]) for a in fake.ledger.windows}
        outq = _clone(call(c, Q, s0, 100 * (k + 1)))
        torch.cuda.synchronize()
        stepped = ic_q.calls[n_calls:]
        if sorted({optimizers(Q)[lbl][0] for lbl in stepped}) != sorted(g0):
            rep.add("a", k, f"optimizer steps {stepped} on Q, gradients of {sorted(g0)} on P")
        if red._pending:
            rep.add("a", k, f"{len(red._pending)} collectives still pending after the step")
        for a, ar in arenas(Q).items():
            wins = fake.ledger.windows[a][n_win[a]:]
            if a not in g0:
                if wins or fake.ledger.open[a]:
                    rep.add("a", k, f"{a}: collectives on an arena that this step does not update")
                continue
            if fake.ledger.open[a]:
                rep.add("a", k, f"{a}: {len(fake.ledger.open[a])} collectives after the arena's optimizer step")
            if len(wins) != 1:
                rep.add("a", k, f"{a}: {len(wins)} optimizer steps on the arena, expected 1")
                continue
            win = wins[0]
            rep.add("a", k, S.tiling_faults([(r["lo"], r["hi"]) for r in win], ar.numel, a, ar, names))
            rep.add("b", k, S.averaging_faults(win, g1[a], ic_q.seen[a][-1], a))
            scale = float(g0[a].abs().max())
            for r in win:                # c. the collective read a complete gradient
                want = g0[a][r["lo"]:r["hi"]]
                if r["in"].shape != want.shape:
                    continue             # a span outside the arena: reported under (a)
                diff = float((r["in"] - want).abs().max()) / max(scale, 1e-30)
                rep.fig(f"c.{a}.rel_diff", diff)
                ok = torch.equal(r["in"], want) if exact else diff <= bounds[a]
                if not ok:
                    rep.add("c", k, f"{a}: the collective on [{r['lo']}, {r['hi']}) did not read the finished gradient: "
                                    f"max |in - g0| = {diff:.3g} x max|g0|" + ("" if exact else f", bound {bounds[a]:.3g}"))
        # 3. P: the averaged gradient through its real optimizer steps
        ic_p.mode = "call"
        for a in g0:
            arenas(P)[a].grad.copy_(avg[a])
        for lbl in stepped:
            optimizers(P)[lbl][1].step()
        torch.cuda.synchronize()
        # d. outcomes
        for key, v in out0.items():
            m = _mismatch(outq[key], v, exact or key == "ids", LOSS_RTOL, LOSS_ATOL)
            if m:
                rep.add("d", k, f"{key} of Q differs from P's shard-0 run: {m}")
        for a in g0:
            m = _mismatch(arenas(Q)[a].flat, arenas(P)[a].flat, exact)
            if m:
                rep.add("d", k, f"{a}: weights after the step: {m}")
        for lbl in stepped:
            a, po = optimizers(P)[lbl]
            qo = optimizers(Q)[lbl][1]
            for what in ("exp_avg", "exp_avg_sq"):
                m = _mismatch(getattr(qo, what), getattr(po, what), exact)
                if m:
                    rep.add("d", k, f"{lbl}.{what}: {m}")
            want = float(avg[a].double().norm())
            for who, o in (("P", po), ("Q", qo)):
                got = float(o.grad_norm)
                if not abs(got - want) <= 1e-5 * want:
                    rep.add("d", k, f"{lbl}.grad_norm of {who} is {got!r}, the averaged gradient's norm is {want!r}")
            if exact and float(qo.grad_norm) != float(po.grad_norm):
                rep.add("d", k, f"{lbl}.grad_norm: {float(qo.grad_norm)!r} / {float(po.grad_norm)!r}")
        if not exact and k + 1 < steps:  # the next step's bound (c) compares backward passes from identical weights (module docstring)
            with torch.no_grad():
                for a in g0:
                    arenas(P)[a].flat.copy_(arenas(Q)[a].flat)
                for lbl in stepped:
                    po, qo = optimizers(P)[lbl][1], optimizers(Q)[lbl][1]
                    po.exp_avg.copy_(qo.exp_avg)
                    po.exp_avg_sq.copy_(qo.exp_avg_sq)
            engine.bump_param_epoch()
    ic_p.restore()
    ic_q.restore()
    return rep


def measure_spread(name, runs=20):
    """Run-to-run spread of P's shard-0 gradient (``ATTN_SPREAD``): {arena: max |g_i - g_0| / max|g_0|} over ``runs`` plain runs per step input."""
    c = CASES[name]
    P = build(c)
    ic = S.OptInterceptor(optimizers(P), None, "skip")
    spread = {}
    for k in range(2):
        s = shard_inputs(c, P, k, 0)
        first = None
        for _ in range(runs):
            n_before = {a: len(v) for a, v in ic.seen.items()}
            call(c, P, s, 100 * (k + 1))
            torch.cuda.synchronize()
            g = {a: ic.seen[a][-1] for a in ic.seen if len(ic.seen[a]) > n_before[a]}
            if first is None:
                first = g
                continue
            for a in g:
                rel = float((g[a] - first[a]).abs().max()) / float(first[a].abs().max())
                spread[a] = max(spread.get(a, 0.0), rel)
        for a in ic.seen:
            ic.seen[a].clear()
    ic.restore()
    return spread


# ------------------------------------------------------------------------------------------------ tests
PARAMS = [(n, None) for n in CASES] + [(n, t) for n in TIMED for t in ("slow-collective", "slow-producer")]


@pytest.mark.parametrize("name,timing", PARAMS, ids=[n if t is None else f"{n}-{t}" for n, t in PARAMS])
def test_schedule_against_a_simulated_second_rank(mode, monkeypatch, name, timing):
    mode(CASES[name].det)
    rep = run_case(name, monkeypatch, timing)
    print(name, timing, {k: f"{v:.3g}" for k, v in rep.figures.items()})
    assert not rep.all(), "\n".join(rep.all())
    if CASES[name].glob:
        assert any(k.startswith("e.") for k in rep.figures), "the global-batch comparison did not run"


def test_checker_flags_schedule_faults(mode, monkeypatch):
    """Each seeded fault (``seed_fault``, on Q's reducer object only) is reported under the assertion that exists for it."""
    mode(True)
    name = "fused-lstm-cgan0"
    trunk = "fused-lstm-cgan1"               # the encoder head lies behind the early bucket: G's arena has an [e1:] span
    with monkeypatch.context() as mp:        # G's optimizer does not wait, under the slow collective: it reads the un-reduced gradient
        rep = run_case(name, mp, fault="wait_all_noop", steps=1)
    assert any(m.startswith("step 0: gen:") and "did not read the average" in m for m in rep.faults["b"]), rep.all()
    assert not any("disc:" in m for m in rep.faults["b"]), rep.all()        # D's Adam is gated by its own wait(ev_dred)
    with monkeypatch.context() as mp:        # (a fifth, the gate of D's Adam: ``wait`` a no-op under the slow collective)
        rep = run_case(name, mp, fault="wait_noop", steps=1)
    assert any(m.startswith("step 0: disc:") and "did not read the average" in m for m in rep.faults["b"]), rep.all()
    assert not any("gen:" in m for m in rep.faults["b"]), rep.all()
    with monkeypatch.context() as mp:        # the [e1:] span of G's arena dropped: the ledger names the gap
        rep = run_case(trunk, mp, fault="drop_tail", steps=1)
    probe = build(CASES[trunk])
    e1, numel = probe.fused._early_bucket()[1], probe.gen_arena.numel
    assert any(f"gen: gap: [{e1}, {numel}) was never reduced" in m for m in rep.faults["a"]), rep.all()
    assert not rep.faults["c"] and not any("disc:" in m for m in rep.faults["a"]), rep.all()
    with monkeypatch.context() as mp:        # D's arena reduced twice: the ledger names the repeat
        rep = run_case(name, mp, fault="double_disc", steps=1)
    assert any(f"disc: repeat: span [0, {probe.disc_arena.numel})" in m for m in rep.faults["a"]), rep.all()
    assert not any("gen:" in m for m in rep.faults["a"]), rep.all()
    with monkeypatch.context() as mp:        # ``ready`` recorded on an idle stream, under the slow producer: the collective reads early
        rep = run_case(name, mp, fault="ready_on_idle_stream", steps=1)
    assert any("did not read the finished gradient" in m for m in rep.faults["c"]), rep.all()
    assert not rep.faults["a"], rep.all()
    with monkeypatch.context() as mp:        # and the unseeded schedule under the same forced timing is clean
        rep = run_case(name, mp, timing="slow-producer", steps=1)
    assert not rep.all(), rep.all()
