"""The optimizer's schedules, weight decay and weight EMA without a GPU: (a) LRSchedule.multiplier against torch's schedulers, (b) a plain
f32 emulation of gic_clip_adamw passes tests/optim_cases.py's checker on every case, the checker flags seeded faults, neutral options
reproduce clip_adam's emulation bit for bit, (c) the decay ranges of the real models' parameter lists, (d) every refusal (Python and
C, which validates before it launches), the new flags' defaults and the default optimizers' route."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch

from tests import aux_cases as A
from tests import optim_cases as OC

CPU_CASES = [c for c in OC.CASES if c.n <= 2 ** 20]          # the grid-cap arenas are checked on the device that produced them


def _sched(sc):
    from gan_image_captioning_amd.optim import LRSchedule
    return LRSchedule(*sc)


def _points(W, T):
    return sorted({s for s in (0, W - 1, W, W + 1, T - 1, T, T + 5) if s >= 0})


# ---------------------------------------------------------------------------------------------------------------- (a) schedules
def _closed_form(make, epoch):
    """torch's closed form of a scheduler at `epoch`, as a multiplier of the base rate 1."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = make(opt)
    sch.last_epoch = epoch
    return sch._get_closed_form_lr()[0]


@pytest.mark.parametrize("W", [0, 1, 5])
@pytest.mark.parametrize("kind", OC.KINDS)
def test_multiplier_is_lambda_lr_of_the_formulas(kind, W):
    """LambdaLR semantics: the optimizer's t-th step runs at base * lambda(t - 1); the package's host mirror is the issue's formula."""
    T, r = W + 7, 0.1
    sc = OC.Sched(kind, W, T, r, 3, 0.5)
    mine = _sched(sc).validate()
    for s in _points(W, T):
        assert mine.multiplier(s) == OC.multiplier(sc, s), (kind, W, s)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.25)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, mine.multiplier)
    for t in range(1, T + 7):
        assert opt.param_groups[0]["lr"] == 0.25 * mine.multiplier(t - 1), (kind, W, t)       # the rate step t uses
        opt.step()
        sch.step()


@pytest.mark.parametrize("W", [0, 1, 5])
def test_linear_and_cosine_against_torch_closed_forms(W):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR
    T, r = W + 7, 0.1
    D = T - W
    lin, cos = _sched(OC.Sched("linear", W, T, r)), _sched(OC.Sched("cosine", W, T, r))
    for s in _points(W, T):
        if s < W:        # warm-up (s + 1) / W: LinearLR from 1 / W to 1 over W - 1 steps
            want = 1.0 if W == 1 else _closed_form(lambda o: LinearLR(o, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1), s)
            assert lin.multiplier(s) == pytest.approx(want, rel=1e-15) and cos.multiplier(s) == lin.multiplier(s)
            continue
        u = s - W
        assert lin.multiplier(s) == pytest.approx(_closed_form(lambda o: LinearLR(o, start_factor=1.0, end_factor=r, total_iters=D), u), rel=1e-14)
        # CosineAnnealingLR's closed form is periodic beyond T_max; the schedule here holds its floor
        want = _closed_form(lambda o: CosineAnnealingLR(o, T_max=D, eta_min=r), min(u, D))
        assert cos.multiplier(s) == pytest.approx(want, rel=1e-14)
    assert lin.multiplier(T + 5) == pytest.approx(r) and cos.multiplier(T + 5) == pytest.approx(r)


@pytest.mark.parametrize("W", [0, 1, 5])
def test_none_is_exactly_one_and_the_warmup_ends_continuously(W):
    none = _sched(OC.Sched("none", W))
    for s in _points(W, W + 7):
        if s >= W:
            assert none.multiplier(s) == 1.0
    assert _sched(OC.Sched()).neutral and (none.neutral == (W == 0))
    for kind in OC.KINDS:
        sc = _sched(OC.Sched(kind, W, W + 7, 0.1, 3, 0.5))
        if W:
            assert sc.multiplier(W - 1) == 1.0                                         # the warm-up ends at the base rate
        if kind == "invsqrt":       # sqrt(W / (W + 1)): one step down its own curve
            assert 1.0 - 1.0 / max(W, 1) <= sc.multiplier(W) <= 1.0 and sc.multiplier(W) == math.sqrt(max(W, 1) / (W + 1))
        else:
            assert sc.multiplier(W) == 1.0, kind
    step = _sched(OC.Sched("step", 2, 0, 0.01, 3, 0.5))
    assert [step.multiplier(s) for s in (2, 4, 5, 7, 8, 30)] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.01]


# ---------------------------------------------------------------------------------------------------------------- (b) emulation
def test_case_table():
    assert len({c.id for c in OC.CASES}) == len(OC.CASES)
    for f in ("decay", "sched", "ema", "all"):
        mine = [c for c in OC.CASES if c.feature == f]
        assert {c.n for c in mine} >= set(OC.NS) | {OC.GRID_CAP_N}, f
    assert {(c.n, c.table) for c in OC.CASES if c.feature == "decay"} >= {(n, t) for n in OC.NS for t in OC.TABLES}
    assert {(c.n, c.table) for c in OC.CASES if c.feature == "all"} >= {(n, t) for n in OC.NS for t in OC.TABLES}
    assert {c.sched.kind for c in OC.CASES} == set(OC.KINDS)
    for sc in OC.SCHEDS:
        ts = {c.t for c in OC.CASES if c.feature == "sched" and c.sched == sc}
        T = sc.total if sc.kind in ("linear", "cosine") else sc.warmup + 7
        assert ts >= {1, max(sc.warmup, 1), sc.warmup + 1, T, T + 3}
        if sc.kind == "step":       # t - 1 = W + S - 1 and W + S: either side of the first decay
            assert ts >= {sc.warmup + sc.step_size, sc.warmup + sc.step_size + 1}
            assert OC.multiplier(sc, sc.warmup + sc.step_size - 1) == 1.0 and OC.multiplier(sc, sc.warmup + sc.step_size) == sc.gamma
    assert {(c.ema[1], c.k) for c in OC.CASES if c.feature == "ema"} >= set(OC.EMA_POINTS)
    assert OC.ema_rate(OC.EMA_D, True, OC.K_STAR) > 1 - OC.EMA_D and OC.ema_rate(OC.EMA_D, True, OC.K_STAR + 1) == pytest.approx(1 - OC.EMA_D, rel=1e-12)
    assert len(OC.table("alt", 12291)) == OC.MAX_RANGES and len(OC.table("alt", 4095)) == 512 // 2
    for n in OC.NS + (OC.GRID_CAP_N,):
        for name in OC.TABLES:
            flat = [x for r in OC.table(name, n) for x in r]
            assert all(x % 4 == 0 for x in flat) and flat == sorted(flat) and len(set(flat)) == len(flat), (name, n)
    seam = 4097 // 4 * 4
    assert OC.table("to_seam", 4097)[-1][1] == seam and OC.table("from_seam", 4097)[0][0] == seam
    assert any(any(o % 4 for o in c.off) for c in OC.CASES) and {c.regime for c in OC.CASES} == {"clip", "noclip", "zero_g", "inf"}


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.id for c in CPU_CASES])
def test_emulation_passes_the_checker(case):
    inp = OC.opt_inputs(case)
    r = OC.opt_check(case, inp, OC.opt_emulate(case, inp))
    assert all(0 <= x <= 1 for x in r.values()), r


FAULT_CASES = {
    "decay_after": OC.OptCase("all", 4097, t=6, table="alt", wd=OC.WD, sched=OC.SCHEDS[3], ema=(OC.EMA_D, True), k=1),
    "decay_outside": OC.OptCase("decay", 4097, table="to_seam", wd=OC.WD),        # the range ends at the seam: the scalar tail decays too
    "lambda_t": OC.OptCase("sched", 4097, t=8, sched=OC.SCHEDS[3]),
    "ema_old_p": OC.OptCase("ema", 4097, ema=(OC.EMA_D, True), k=1),
    "k_plus_1": OC.OptCase("ema", 4097, ema=(OC.EMA_D, True), k=1),
}


@pytest.mark.parametrize("fault", OC.FAULTS)
def test_checker_flags_seeded_faults(fault):
    case = FAULT_CASES[fault]
    inp = OC.opt_inputs(case)
    OC.opt_check(case, inp, OC.opt_emulate(case, inp))
    with pytest.raises(A.Mismatch) as e:
        OC.opt_check(case, inp, OC.opt_emulate(case, inp, fault=fault))
    where = {"decay_after": "params", "decay_outside": "params", "lambda_t": "sched_out[0]", "ema_old_p": "ema", "k_plus_1": "sched_out[1]"}
    assert e.value.what == where[fault]
    if fault == "decay_outside":
        assert e.value.index == OC.table("to_seam", case.n)[-1][1] == 4096        # the first element past the range


@pytest.mark.parametrize("case", [c for c in OC.NEUTRAL_CASES if c.n <= 2 ** 20], ids=lambda c: c.id)
def test_neutral_options_reproduce_clip_adam(case):
    inp = OC.opt_inputs(case)
    mine, theirs = OC.opt_emulate(case, inp), A.adam_emulate(case.adam, inp)
    for k in ("norm", "m", "v", "p"):
        A.same_bits("clip_adamw", case.id, k, mine[k], theirs[k], nan_free=True)
    assert mine["sched"].tolist() == [A.f32(A.ADAM_HYPER["lr"]), 0.0]


# ---------------------------------------------------------------------------------------------------------------- (c) decay ranges
@pytest.mark.parametrize("kw", [dict(), dict(conditional_gan=1), dict(decoder="attention", conditional_gan=1, vocab_size=52),
                                dict(gen_num_layers=2, vocab_size=50), dict(disc_cond="projection", conditional_gan=1)], ids=str)
def test_decay_ranges_of_the_models(kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.discriminator import Discriminator
    from gan_image_captioning_amd.generator import Generator
    from gan_image_captioning_amd.optim import MAX_DECAY_RANGES, slot_ranges
    args = default_args(**dict(dict(vocab_size=51, gen_hidden_dim=24, gen_embed_dim=8, device="cpu", encoder_arch="resnet18"), **kw))
    gen, disc = Generator(args), Discriminator(args)
    g_params = list(gen.decoder.parameters())
    if args.conditional_gan:          # the instructor's gen_arena (training.py)
        g_params += list(gen.encoder.linear.parameters()) + list(gen.encoder.bn.parameters())
    for params in (g_params, list(disc.parameters())):
        ranges = slot_ranges(params)
        flat = [x for r in ranges for x in r]
        assert flat == sorted(flat) and len(set(flat)) == len(flat), "sorted, non-empty and merged (no two ranges touch)"
        assert all(x % 4 == 0 for x in flat) and 0 < len(ranges) <= MAX_DECAY_RANGES
        off = 0
        for p in params:
            end = off + (p.numel() + 3) // 4 * 4
            inside = any(s <= off and end <= e for s, e in ranges)
            outside = all(end <= s or e <= off for s, e in ranges)
            assert inside != outside and inside == (p.ndim >= 2), tuple(p.shape)            # every matrix, no bias, no BatchNorm affine
            off = end
    assert any(p.ndim == 1 for p in g_params) and slot_ranges(g_params, lambda p: False) == []


# ---------------------------------------------------------------------------------------------------------------- (d) refusals, defaults, routes
NEW_FLAGS = {"pretrain_lr_schedule": "none", "adv_lr_schedule": "none", "pretrain_lr_warmup_steps": 0, "adv_lr_warmup_steps": 0,
             "lr_min_ratio": 0.0, "lr_step_size": 0, "lr_step_gamma": 0.1, "gen_weight_decay": 0.0, "disc_weight_decay": 0.0,
             "gen_ema_decay": 0.0, "gen_ema_warmup": 1, "eval_ema": 0, "resume_train_state": ""}


def test_new_flags_default_off():
    from gan_image_captioning_amd.args import build_parser, default_args
    a = default_args()
    for k, v in NEW_FLAGS.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    p = build_parser()
    for kind in OC.KINDS:
        assert p.parse_args(["--pretrain-lr-schedule", kind, "--adv-lr-schedule", kind]).adv_lr_schedule == kind
    with pytest.raises(SystemExit):
        p.parse_args(["--adv-lr-schedule", "exponential"])
    from gan_image_captioning_amd.training import check_optimizer
    oc = check_optimizer(a)
    assert oc["pretrain"].neutral and oc["adv"].neutral and oc["gen_wd"] == oc["disc_wd"] == oc["ema_decay"] == 0.0 and not oc["eval_ema"]


@pytest.mark.parametrize("kw, match", [
    (dict(lr_min_ratio=1.5), "--lr-min-ratio"), (dict(lr_min_ratio=-0.1), "--lr-min-ratio"), (dict(lr_min_ratio=float("nan")), "--lr-min-ratio"),
    (dict(pretrain_lr_schedule="step"), "--lr-step-size"), (dict(adv_lr_schedule="step", lr_step_size=-2), "--lr-step-size"),
    (dict(gen_ema_decay=1.0), "--gen-ema-decay"), (dict(gen_ema_decay=-0.5), "--gen-ema-decay"),
    (dict(gen_weight_decay=-1e-3), "--gen-weight-decay"), (dict(disc_weight_decay=-1.0), "--disc-weight-decay"),
    (dict(eval_ema=1), "--eval-ema"), (dict(adv_lr_warmup_steps=-1), "--adv-lr-warmup-steps"),
], ids=str)
def test_flag_refusals(kw, match):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import check_optimizer
    with pytest.raises(ValueError, match=match):
        check_optimizer(default_args(**kw))


def _fake_arena(n=24):
    return SimpleNamespace(flat=torch.zeros(n), grad=torch.zeros(n), numel=n, decay_ranges=lambda: [(0, 8), (12, 16)])


def test_horizon_and_optimizer_refusals(monkeypatch):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.optim import ArenaEMA, FusedClipAdam, LRSchedule
    from gan_image_captioning_amd.training import build_optimizers, check_optimizer
    monkeypatch.setattr(engine, "require_gpu", lambda *t: None)
    for kind in ("linear", "cosine"):
        for W, T in ((5, 5), (5, 3), (0, 0)):
            with pytest.raises(ValueError, match="horizon"):
                LRSchedule(kind, W, T).validate()
        args = default_args(adv_lr_schedule=kind, adv_lr_warmup_steps=6)
        with pytest.raises(ValueError, match="horizon"):          # 2 epochs of 3 steps against 6 warm-up steps
            build_optimizers(args, check_optimizer(args), _fake_arena(), _fake_arena(), 10, 6)
        build_optimizers(args, check_optimizer(args), _fake_arena(), _fake_arena(), 0, 7)
    with pytest.raises(ValueError, match="step"):
        LRSchedule("step", 0, 0, 0.0, 0).validate()
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        LRSchedule("none", 0, 0, 1.01).validate()
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ArenaEMA(_fake_arena(), 1.0)
    with pytest.raises(ValueError, match="weight decay"):
        FusedClipAdam(_fake_arena(), 1e-3, 5.0, weight_decay=-0.1)
    with pytest.raises(ValueError, match="another arena"):
        FusedClipAdam(_fake_arena(), 1e-3, 5.0, ema=ArenaEMA(_fake_arena(), 0.9))
    with pytest.raises(ValueError, match="at most 256"):
        FusedClipAdam(_fake_arena(), 1e-3, 5.0, weight_decay=0.1, decay_ranges=[(8 * i, 8 * i + 4) for i in range(257)])


def test_default_optimizers_take_the_clip_adam_route(monkeypatch):
    """With every flag at its default the instructor's three optimizers call engine.clip_adam with the arguments they always did;
    any feature moves that optimizer, and only it, to engine.clip_adamw.  The host's step count drives current_lr()."""
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import build_optimizers, check_optimizer
    calls = []
    monkeypatch.setattr(engine, "require_gpu", lambda *t: None)
    monkeypatch.setattr(engine, "clip_adam", lambda *a: calls.append(("clip_adam", a)))
    monkeypatch.setattr(engine, "clip_adamw", lambda *a: calls.append(("clip_adamw", a)))
    args = default_args()
    ga, da = _fake_arena(), _fake_arena()
    pre, gen, disc, ema = build_optimizers(args, check_optimizer(args), ga, da, 10, 10)
    assert ema is None
    for opt, lr, arena in ((pre, args.pretrain_lr, ga), (gen, args.gen_lr, ga), (disc, args.disc_lr, da)):
        opt.step()
        name, a = calls.pop()
        assert name == "clip_adam" and len(a) == 12 and not calls
        assert a[0] is arena.flat and a[1] is arena.grad and a[2] is opt.exp_avg and a[3] is opt.exp_avg_sq
        assert a[4:9] == (lr, 0.9, 0.999, 1e-8, args.clip_norm) and a[9] is opt.step_count and a[10] is opt.grad_norm
        assert opt.current_lr() == lr and opt.steps == 1
        assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "step", "lr"}
    args = default_args(disc_weight_decay=0.01, adv_lr_schedule="invsqrt", adv_lr_warmup_steps=2, gen_ema_decay=0.99)
    pre, gen, disc, ema = build_optimizers(args, check_optimizer(args), ga, da, 10, 10)
    assert ema is not None and ema.arena is ga and pre.ema is ema and gen.ema is ema and disc.ema is None
    for opt, lam in ((pre, [1.0, 1.0, 1.0]), (gen, [0.5, 1.0, math.sqrt(2 / 3)]), (disc, [0.5, 1.0, math.sqrt(2 / 3)])):
        for s in range(3):
            assert opt.current_lr() == opt.lr * lam[s]
            opt.step()
            name, a = calls.pop()
            assert name == "clip_adamw" and len(a) == 13 and a[4] == opt.lr and not calls           # the base rate: the schedule is the kernel's
    o = disc._opts
    assert (o.weight_decay, o.n_ranges, o.schedule, o.warmup_steps, o.ema, o.ema_count) == (0.01, 2, 3, 2, None, None)
    assert [ctypes.cast(o.ranges_host, ctypes.POINTER(ctypes.c_int64))[i] for i in range(4)] == [0, 8, 12, 16]
    assert gen._opts.n_ranges == 0 and gen._opts.ema == ema.shadow.data_ptr() and gen._opts.ema_count == ema.count.data_ptr()
    old = {"exp_avg": torch.ones(24), "exp_avg_sq": torch.ones(24), "step": torch.tensor([7])}       # a state dict from before: loads
    gen.load_state_dict(old)
    assert gen.steps == 7 and gen.current_lr() == gen.lr * math.sqrt(2 / 8)


def _call(lib, opts, n=16):
    """gic_clip_adamw with placeholder operands: every refusal returns before anything is read or launched."""
    fake = ctypes.c_void_p(0x1000)
    return lib.gic_clip_adamw(fake, fake, fake, fake, n, 1e-3, 0.9, 0.999, 1e-8, 5.0, fake, fake, fake, ctypes.byref(opts), None)


def _opts(ranges=(), **kw):
    from gan_image_captioning_amd import _lib
    host = (ctypes.c_int64 * max(len(ranges), 1))(*ranges)
    o = _lib.AdamwOpts()
    o.gamma, o.n_ranges = 0.1, len(ranges) // 2
    if ranges:
        o.ranges_host, o.ranges = ctypes.cast(host, ctypes.c_void_p).value, 0x1000
    for k, v in kw.items():
        setattr(o, k, v)
    o._keep = host
    return o


@pytest.mark.parametrize("opts, text", [
    (dict(ranges=(0, 6)), b"multiple of 4"), (dict(ranges=(2, 8)), b"multiple of 4"),
    (dict(ranges=(8, 12, 0, 4)), b"sorted"), (dict(ranges=(0, 8, 4, 12)), b"sorted"), (dict(ranges=(4, 4)), b"sorted"), (dict(ranges=(-4, 4)), b"sorted"),
    (dict(ranges=tuple(x for i in range(257) for x in (8 * i, 8 * i + 4))), b"at most 256"),
    (dict(weight_decay=-0.5), b"weight_decay"), (dict(min_ratio=1.5), b"min_ratio"), (dict(min_ratio=-0.5), b"min_ratio"),
    (dict(schedule=1, warmup_steps=5, total_steps=5), b"horizon"), (dict(schedule=2, warmup_steps=5, total_steps=2), b"horizon"),
    (dict(schedule=4, step_size=0), b"step_size"), (dict(schedule=9), b"unknown schedule"), (dict(warmup_steps=-1), b"warmup_steps"),
    (dict(ema=0x1000, ema_count=0x1000, ema_decay=1.0), b"ema_decay"), (dict(ema=0x1000), b"come together"),
], ids=str)
def test_c_entry_refuses_before_any_launch(opts, text):
    from gan_image_captioning_amd import _lib
    lib = _lib.load()
    assert _call(lib, _opts(**opts)) == -1
    assert text in lib.gic_last_error()


def test_struct_layout_matches_the_header():
    from gan_image_captioning_amd import _lib
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.AdamwOpts) == 8 + 2 * P + 2 * 4 + 3 * 8 + 2 * 8 + 2 * P + 8 + 2 * 4 + P
    assert _lib.ADAMW_MAX_RANGES == OC.MAX_RANGES and list(_lib.LR_SCHEDULES) == list(OC.KINDS)
