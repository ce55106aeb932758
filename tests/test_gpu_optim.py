"""gic_clip_adamw on the GPU against tests/optim_cases.py: neutral options against gic_clip_adam bit for bit at every clip + Adam case,
each feature alone and all together at every case of the table, the refused range tables, two calls in a row, and a 20-step trajectory
against torch.optim.AdamW + LambdaLR + an explicit EMA in float64.

Every output lives in a tests.gpu_util.Guarded buffer that holds NaN beforehand (the arenas: their inputs) and whose guards must be intact
after the call; misaligned operands are Guarded views with `off`."""
import pytest
import torch

from tests import aux_cases as A
from tests import optim_cases as OC
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

NAN = float("nan")
MAXIMA = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def _report_maxima():
    yield
    for k in sorted(MAXIMA):
        print(f"\n[clip_adamw] err/bound max {MAXIMA[k]:.4f}  {k}", end="")
    print()


def note(ratios):
    A.merge(MAXIMA, ratios)
    assert all(0 <= r <= 1 for r in ratios.values()), ratios


def put(t, dev, off=0):
    g = Guarded(t.shape[0], 1, t.dtype, dev, 0 if t.dtype == torch.int64 else NAN, off)
    g.live.copy_(t)
    return g


def fresh(n, dev):
    return Guarded(n, 1, torch.float32, dev, NAN)


def run(E, dev, case, inp, wd=None, ranges=None):
    """One gic_clip_adamw call on fresh Guarded buffers; returns (out for OC.opt_check, the buffers)."""
    h = A.ADAM_HYPER
    b = {k: put(inp[k], dev, off) for k, off in zip("pgmve", case.off)}
    nparts = E.clip_adam_partials(case.n)
    b["partials"], b["norm"], b["sched"] = fresh(nparts, dev), fresh(1, dev), fresh(2, dev)
    b["step"] = put(torch.tensor([case.t - 1], dtype=torch.int64), dev)
    b["count"] = put(torch.tensor([case.k], dtype=torch.int64), dev)
    wd = case.wd if wd is None else wd
    flat = [x for r in (OC.table(case.table, case.n) if ranges is None else ranges) for x in r] if wd > 0 else []
    if flat:
        b["ranges"] = put(torch.tensor(flat, dtype=torch.int64), dev)
    sc = case.sched
    opts = E.adamw_opts(wd, flat, b["ranges"].live if flat else None, sc.kind, sc.warmup, sc.total, sc.min_ratio, sc.step_size, sc.gamma,
                        b["e"].live if case.ema else None, b["count"].live if case.ema else None, case.ema[0] if case.ema else 0.0,
                        case.ema[1] if case.ema else True, b["sched"].live)
    call = lambda: E.clip_adamw(b["p"].live, b["g"].live, b["m"].live, b["v"].live, h["lr"], h["b1"], h["b2"], h["eps"], h["clip"],     # noqa: E731
                                b["step"].live, b["norm"].live, b["partials"].live, opts)
    call()
    torch.cuda.synchronize()
    return collect(case, b), b, call


def collect(case, b):
    return {"norm": b["norm"].live, "m": b["m"].live, "v": b["v"].live, "p": b["p"].live, "e": b["e"].live if case.ema else None,
            "step": int(b["step"].live[0]), "ema_count": int(b["count"].live[0]) if case.ema else None, "sched": b["sched"].live}


def settle(case, inp, b, dev):
    for name, g in b.items():
        assert g.guards_intact(), f"{case.id}: the guards of {name} changed"
    A.same_bits("clip_adamw", case.id, "the gradients are read only", b["g"].live, inp["g"].to(dev))
    assert not bool(torch.isnan(b["partials"].live).any())
    if not case.ema:        # no EMA: the shadow and its counter are not touched
        A.same_bits("clip_adamw", case.id, "the shadow without an EMA", b["e"].live, inp["e"].to(dev))
        assert int(b["count"].live[0]) == case.k
    if "ranges" in b:
        assert b["ranges"].live.tolist() == [x for r in OC.table(case.table, case.n) for x in r]


# ---------------------------------------------------------------------------------------------------------------- neutral options
@pytest.mark.parametrize("case", OC.NEUTRAL_CASES, ids=[c.id for c in OC.NEUTRAL_CASES])
def test_neutral_options_are_clip_adam_bit_for_bit(E, dev, case):
    inp = OC.opt_inputs(case)
    h = A.ADAM_HYPER
    out, b, _ = run(E, dev, case, inp)
    settle(case, inp, b, dev)
    ref = {k: put(inp[k], dev, off) for k, off in zip("pgmv", case.off)}
    partials, norm = fresh(E.clip_adam_partials(case.n), dev), fresh(1, dev)
    step = put(torch.tensor([case.t - 1], dtype=torch.int64), dev)
    E.clip_adam(ref["p"].live, ref["g"].live, ref["m"].live, ref["v"].live, h["lr"], h["b1"], h["b2"], h["eps"], h["clip"], step.live,
                norm.live, partials.live)
    torch.cuda.synchronize()
    for k in "pmv":
        A.same_bits("clip_adamw", case.id, f"{k} against gic_clip_adam", b[k].live, ref[k].live, nan_free=True)
    A.same_bits("clip_adamw", case.id, "norm_out against gic_clip_adam", b["norm"].live, norm.live, nan_free=True)
    A.same_bits("clip_adamw", case.id, "partials against gic_clip_adam", b["partials"].live, partials.live, nan_free=True)
    assert int(step.live[0]) == out["step"] == case.t
    assert out["sched"].tolist() == [A.f32(h["lr"]), 0.0]


# ---------------------------------------------------------------------------------------------------------------- the features
@pytest.mark.parametrize("case", OC.CASES, ids=[c.id for c in OC.CASES])
def test_clip_adamw(E, dev, case):
    inp = OC.opt_inputs(case)
    out, b, _ = run(E, dev, case, inp)
    settle(case, inp, b, dev)
    note(OC.opt_check(case, inp, out))
    if case.wd > 0:         # outside every range: the bits of the run without decay
        plain, _, _ = run(E, dev, case, inp, wd=0.0)
        outside = ~OC.table_mask(OC.table(case.table, case.n), case.n).to(dev)
        for k in ("p", "m", "v") + (("e",) if case.ema else ()):
            sel = outside if k in "pe" else torch.ones_like(outside)          # the moments do not see the decay at all
            A.same_bits("clip_adamw", case.id, f"{k} outside the ranges against the run without decay", out[k][sel], plain[k][sel], nan_free=True)
        inside = ~outside & (inp["p"].to(dev) != 0)
        if bool(inside.any()) and case.regime != "inf":
            assert bool((out["p"][inside] != plain["p"][inside]).any()), f"{case.id}: nothing decayed inside the ranges"


def test_counters_advance_by_one_per_call(E, dev):
    """Two calls in a row: step_count t - 1 -> t -> t + 1 and ema_count k -> k + 1 -> k + 2, the second update is step t + 1's (the
    schedule one step on, the EMA's warm-up one update on) of the first one's state."""
    first = OC.OptCase("all", 4097, t=7, table="alt", wd=OC.WD, sched=OC.SCHEDS[3], ema=(OC.EMA_D, True), k=0)      # past the warm-up: lambda moves
    second = first._replace(t=8, k=1)
    inp = OC.opt_inputs(first)
    out, b, call = run(E, dev, first, inp)
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    note(OC.opt_check(first, inp, out))
    call()
    torch.cuda.synchronize()
    inp2 = dict(inp, p=out["p"].cpu(), m=out["m"].cpu(), v=out["v"].cpu(), e=out["e"].cpu())
    note(OC.opt_check(second, inp2, collect(second, b)))
    settle(second, inp, b, dev)
    assert float(b["sched"].live[0]) != float(out["sched"][0]) and float(b["sched"].live[1]) != float(out["sched"][1])


# ---------------------------------------------------------------------------------------------------------------- refused tables
@pytest.mark.parametrize("ranges, text", [([(0, 6)], "multiple of 4"), ([(8, 12), (0, 4)], "sorted"),
                                          ([(8 * i, 8 * i + 4) for i in range(257)], "at most 256")], ids=["unaligned", "unsorted", "257"])
def test_refused_tables_launch_nothing(E, dev, ranges, text):
    """An unaligned boundary, an unsorted table and more than 256 ranges: a status and an error text, and every operand as it was."""
    inp = OC.opt_inputs(OC.OptCase("all", 4097, t=5, table="alt", wd=OC.WD, sched=OC.SCHEDS[3], ema=(OC.EMA_D, True), k=2))
    b = {k: put(inp[k], dev) for k in "pgmve"}
    sched, step, count = fresh(2, dev), put(torch.tensor([4], dtype=torch.int64), dev), put(torch.tensor([2], dtype=torch.int64), dev)
    flat = [x for r in ranges for x in r]
    rd = put(torch.tensor(flat, dtype=torch.int64), dev)
    opts = E.adamw_opts(OC.WD, flat, rd.live, "cosine", 5, 12, 0.1, 0, 0.1, b["e"].live, count.live, OC.EMA_D, True, sched.live)
    partials, norm = fresh(2, dev), fresh(1, dev)
    h = A.ADAM_HYPER
    with pytest.raises(ValueError, match=text):
        E.clip_adamw(b["p"].live, b["g"].live, b["m"].live, b["v"].live, h["lr"], h["b1"], h["b2"], h["eps"], h["clip"], step.live,
                     norm.live, partials.live, opts)
    torch.cuda.synchronize()
    for k in "pgmve":
        A.same_bits("clip_adamw", "refused", k, b[k].live, inp[k].to(dev))
    assert int(step.live[0]) == 4 and int(count.live[0]) == 2
    assert bool(torch.isnan(sched.live).all() and torch.isnan(norm.live).all() and torch.isnan(partials.live).all())


# ---------------------------------------------------------------------------------------------------------------- trajectory
def test_trajectory_against_torch_adamw(E, dev):
    """20 steps on a 12291-element arena with schedule, decay and EMA on, against torch.optim.AdamW + LambdaLR + an explicit EMA loop
    in float64 on the CPU, the gradients clipped beforehand the way the kernel clips them.  Tolerances of test_clip_adam_clips
    (rtol 1e-5 = 168 u, atol 1e-7): a step adds at most 3 u |p| (decay, update) and ~12 u |upd| with |upd| <= ~lr, and carries the
    moments' few-u relative error into upd, so 20 steps stay below 20 (3 u |p| + 1e-3 * 20 u) < 60 u |p| + 2.4e-8."""
    from gan_image_captioning_amd.optim import LRSchedule
    n, steps, lr, wd, d, clip = 12291, 20, 1e-3, 0.1, 0.999, 5.0
    sched = LRSchedule("cosine", 4, 16, 0.1).validate()
    ranges = OC.table("alt", n)
    inside = OC.table_mask(ranges, n)
    gen = A.gen_for("trajectory")
    p0 = 0.1 * torch.randn(n, generator=gen)
    pad = torch.arange(n) % 7 == 3
    p0[pad] = 0
    grads = [torch.randn(n, generator=gen) * (0.02 if s % 3 else 0.2) for s in range(steps)]       # norm ~2.2 (no clip) | ~22 (clipped)
    for g in grads:
        g[pad] = 0
    # the reference: float64, two parameter groups
    a, b = torch.nn.Parameter(p0[inside].double()), torch.nn.Parameter(p0[~inside].double())
    opt = torch.optim.AdamW([{"params": [a], "weight_decay": wd}, {"params": [b], "weight_decay": 0.0}], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sched.multiplier)
    ema_ref = p0.double().clone()
    # the kernel
    P, G, M, V, S = (put(x, dev) for x in (p0, grads[0], torch.zeros(n), torch.zeros(n), p0))
    step, count = put(torch.zeros(1, dtype=torch.int64), dev), put(torch.zeros(1, dtype=torch.int64), dev)
    partials, norm, so = fresh(E.clip_adam_partials(n), dev), fresh(1, dev), fresh(2, dev)
    flat = [x for r in ranges for x in r]
    rd = put(torch.tensor(flat, dtype=torch.int64), dev)
    opts = E.adamw_opts(wd, flat, rd.live, sched.kind, sched.warmup, sched.total, sched.min_ratio, 0, 0.1, S.live, count.live, d, True, so.live)
    clipped = 0
    for s in range(steps):
        g64 = grads[s].double()
        coef = min(1.0, clip / (float(g64.norm()) + 1e-6))
        clipped += coef < 1.0
        a.grad, b.grad = (g64 * coef)[inside], (g64 * coef)[~inside]
        opt.step()
        lam.step()
        now = torch.empty(n, dtype=torch.float64)
        now[inside], now[~inside] = a.detach(), b.detach()
        dk = min(d, (1 + s) / (10 + s))
        ema_ref += (now - ema_ref) * (1 - dk)
        G.live.copy_(grads[s])
        E.clip_adamw(P.live, G.live, M.live, V.live, lr, 0.9, 0.999, 1e-8, clip, step.live, norm.live, partials.live, opts)
    torch.cuda.synchronize()
    assert 0 < clipped < steps and int(step.live[0]) == int(count.live[0]) == steps
    for g in (P, G, M, V, S, step, count, partials, norm, so, rd):
        assert g.guards_intact()
    torch.testing.assert_close(P.live.cpu().double(), now, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(S.live.cpu().double(), ema_ref, rtol=1e-5, atol=1e-7)
    assert float(so.live[0]) == pytest.approx(lr * sched.multiplier(steps - 1), rel=2e-7)
    assert bool((P.live[pad.to(dev)] == 0).all() and (S.live[pad.to(dev)] == 0).all())
    assert float((S.live.cpu().double() - now).abs().max()) > 1e-4           # the average lags the weights
