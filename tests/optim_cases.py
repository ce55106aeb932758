"""gic_clip_adamw (csrc/optim.hip): clip + Adam with a device-side learning-rate schedule, decoupled weight decay over arena ranges and
a weight EMA.  The case tables, the references, the per-element bounds, a plain f32 emulation and the checker, behind
tests/test_optim_cases.py (no GPU) and tests/test_gpu_optim.py (every case on the GPU).  Nothing here touches a GPU; the references
run on whichever device their operands live on.  The inputs, the clip + Adam scalars, `check` and `same_bits` are tests/aux_cases.py's.

Rounding model: the one at the top of tests/aux_cases.py (u = 2^-24 per f32 operation on the magnitudes before cancellation, one u for
each scalar that the kernel derives in float64 and rounds to f32).  Every stage's reference is formed from what the kernel stored:

  sched_out[0]  lr_t = lr lambda(t - 1), float64 on the device, rounded to f32 on the store: u lr_t against the host's float64 value,
                plus 2^-44 lr_t for the last places in which the device's cos / pow / sqrt may differ from the host's in float64.
  sched_out[1]  a = (float)(1 - d_k): u a + 2^-44 likewise.
  exp_avg, exp_avg_sq   clip_adam's bounds (aux_cases.adam_check), from the stored norm.
  params        from the stored exp_avg, exp_avg_sq and lr_t' = sched_out[0] (so lr_t = lr_t' (1 + d), |d| <= u):
                  keep = (float)(1 - lr_t wd): |keep - (1 - lr_t' wd)| <= u keep + u lr_t' wd
                  pd = p keep inside a range: one product, u |pd|; together |pd - p (1 - lr_t' wd)| <= |p| u (2 keep + lr_t' wd)
                  upd = step (m / denom), step = (float)(lr_t / (1 - b1^t)): clip_adam's SQRT + 3 + 3 + 1 u |upd|, + 1 for d
                  p_new = pd - upd: u (|pd| + |upd|)
                outside every range pd = p exactly.
  ema           from the stored p_new and a = sched_out[1] (exact: the kernel multiplies by that f32):  e + (p_new - e) a:
                the difference and the product 2 u (|p_new| + |e|) a, the sum u (|e| + (|p_new| + |e|) a).
  exact         both counters, the gradients (read only), arena padding (+0 in p, m, v, e), and -- in the GPU tests -- the elements outside
                every range against a run without decay.

Largest err / bound seen per output on an MI355X (recorded, never asserted against): WORST_OBSERVED below.  Where one last rounding
dominates the bound (the parameter update and the shadow's lerp over millions of elements) a correctly rounded result reaches ~1."""
import math
from typing import NamedTuple, Optional, Tuple

import torch

from tests import aux_cases as A
from tests.aux_cases import AdamCase, SQRT, U, adam_inputs, adam_scalars, check, same_bits  # noqa: F401  (the shared pieces)

F64 = torch.float64
D_ULPS = 2.0 ** -44            # float64 last places of the device's cos / pow / sqrt, relative
MAX_RANGES = 256
KINDS = ("none", "linear", "cosine", "invsqrt", "step")
WD = 0.1
EMA_D = 0.999
K_STAR = 8989                  # the largest k with (1 + k) / (10 + k) < 0.999
assert (1 + K_STAR) / (10 + K_STAR) < EMA_D <= (2 + K_STAR) / (11 + K_STAR)
GRID_CAP_N = 2048 * 2048 + 4096 + 3

# Largest err / bound per output measured on an MI355X by tests/test_gpu_optim.py (recorded, never asserted against).
WORST_OBSERVED = {"sched_lr": 0.797, "sched_a": 0.797, "exp_avg": 0.647, "exp_avg_sq": 0.463, "params": 0.998, "ema": 0.992, "sqnorm_partial": 0.035}


class Sched(NamedTuple):
    """LRSchedule's fields (gan_image_captioning_amd.optim), restated so that this file imports nothing from the package."""
    kind: str = "none"
    warmup: int = 0
    total: int = 0
    min_ratio: float = 0.0
    step_size: int = 0
    gamma: float = 0.1


def multiplier(sc, s):
    """lambda(s) in float64, from the issue's formulas."""
    W, r = sc.warmup, sc.min_ratio
    if s < W:
        return (s + 1) / W
    u = s - W
    if sc.kind == "linear":
        return r + (1.0 - r) * max(0.0, 1.0 - u / (sc.total - W))
    if sc.kind == "cosine":
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * min(1.0, u / (sc.total - W))))
    if sc.kind == "invsqrt":
        return max(r, math.sqrt(max(W, 1) / (s + 1)))
    if sc.kind == "step":
        return max(r, sc.gamma ** (u // sc.step_size))
    return 1.0


def ema_rate(d, warmup, k):
    """a = 1 - d_k in float64."""
    return 1.0 - (min(d, (1.0 + k) / (10.0 + k)) if warmup else d)


# ---------------------------------------------------------------------------------------------------------------- range tables
TABLES = ("empty", "whole", "one", "ends", "to_seam", "from_seam", "alt")


def table(name, n):
    """Sorted, merged half-open ranges with boundaries on multiples of 4.  The seam is 4 (n // 4): where the 16-byte body of an
    aligned call ends and its scalar tail begins."""
    up, seam = A.cdiv(n, 4) * 4, n // 4 * 4
    if name == "empty":
        return []
    if name == "whole":
        return [(0, up)]
    if name == "one":
        q = (n // 4) // 2 * 4
        return [(q, q + 4)]
    if name == "ends":
        last = (n - 1) // 4 * 4
        return [(0, 4)] if last == 0 else [(0, 8)] if last == 4 else [(0, 4), (last, last + 4)]
    if name == "to_seam":
        return [(max(0, seam - 8), seam)] if seam else []
    if name == "from_seam":
        return [(seam, seam + 4)]
    if name == "alt":
        return [(8 * i, 8 * i + 4) for i in range(min(MAX_RANGES, A.cdiv(n, 8)))]
    raise KeyError(name)


def table_mask(ranges, n):
    m = torch.zeros(n, dtype=torch.bool)
    for s, e in ranges:
        m[s:min(e, n)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- cases
class OptCase(NamedTuple):
    feature: str                                       # "neutral" | "decay" | "sched" | "ema" | "all"
    n: int
    t: int = 1                                         # the step this call performs
    table: str = "empty"
    wd: float = 0.0
    sched: Sched = Sched()
    ema: Optional[Tuple[float, bool]] = None           # (decay, warm-up) or None
    k: int = 0                                         # EMA updates before this call
    off: Tuple[int, int, int, int, int] = (0, 0, 0, 0, 0)      # float offsets of p, g, m, v, e off their 16-byte alignment
    regime: str = "clip"

    @property
    def id(self):
        sc = self.sched
        s = f"{sc.kind}W{sc.warmup}T{sc.total}r{sc.min_ratio}S{sc.step_size}"
        e = "noema" if self.ema is None else f"d{self.ema[0]}w{int(self.ema[1])}k{self.k}"
        return f"{self.feature}-n{self.n}-t{self.t}-{self.table}-wd{self.wd}-{s}-{e}-off{''.join(map(str, self.off))}-{self.regime}"

    @property
    def adam(self):
        """The clip + Adam part as an aux_cases.AdamCase (its inputs and its route)."""
        return AdamCase(self.n, self.off[:4], self.regime, self.t)


NS = (1, 3, 4, 5, 4095, 4096, 4097, 12291)
SCHEDS = (Sched("none", 5), Sched("linear", 5, 12, 0.1), Sched("linear", 0, 7), Sched("cosine", 5, 12, 0.1), Sched("cosine", 1, 9),
          Sched("invsqrt", 5, 0, 0.2), Sched("invsqrt", 0), Sched("step", 5, 0, 0.01, 3, 0.5), Sched("step", 0, 0, 0.0, 4, 0.1))


def sched_steps(sc):
    """t in {1, W, W + 1, T, T + 3} (T: the horizon, or W + 7 where the kind has none); for `step`, t on both sides of a boundary."""
    W, T = sc.warmup, sc.total if sc.kind in ("linear", "cosine") else sc.warmup + 7
    ts = {1, max(W, 1), W + 1, T, T + 3}
    if sc.kind == "step":           # s = t - 1 = W + S - 1 | W + S: the last step before the first decay and the first after it
        ts |= {W + sc.step_size, W + sc.step_size + 1, W + 2 * sc.step_size, W + 2 * sc.step_size + 1}
    return sorted(ts)


EMA_POINTS = [(w, k) for w in (True, False) for k in (0, 1, K_STAR, K_STAR + 1)]


def _cases():
    out = []
    # each feature alone
    out += [OptCase("decay", n, table=tb, wd=WD) for n in NS for tb in TABLES]
    i = 0
    for sc in SCHEDS:
        for t in sched_steps(sc):
            out.append(OptCase("sched", NS[i % len(NS)], t=t, sched=sc))
            i += 1
    out += [OptCase("ema", NS[j % len(NS)], ema=(EMA_D, w), k=k) for j, (w, k) in enumerate(EMA_POINTS)]
    out += [OptCase("ema", n, ema=(EMA_D, True), k=3) for n in NS]
    # all together: every n against a rotating table, schedule point and EMA point
    pts = [(sc, t) for sc in SCHEDS[1:] for t in sched_steps(sc)]
    for j, n in enumerate(NS):
        for q in range(len(TABLES)):
            sc, t = pts[(j * len(TABLES) + q) * 5 % len(pts)]
            w, k = EMA_POINTS[(j + q) % len(EMA_POINTS)]
            out.append(OptCase("all", n, t=t, table=TABLES[q], wd=WD, sched=sc, ema=(EMA_D, w), k=k))
    # misaligned operands take the scalar path (the shadow alone, everything, the gradients alone), other regimes
    full = dict(t=6, table="alt", wd=WD, sched=SCHEDS[3], ema=(EMA_D, True), k=1)
    out += [OptCase("all", 12291, off=o, **full) for o in ((0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (2, 2, 2, 2, 2), (3, 3, 3, 3, 3), (0, 1, 0, 0, 0))]
    out += [OptCase("all", 12291, regime=r, **full) for r in ("noclip", "zero_g", "inf")]
    # the grid cap: 2048 blocks stride over the arena more than once
    out += [OptCase("decay", GRID_CAP_N, table="alt", wd=WD), OptCase("sched", GRID_CAP_N, t=8, sched=SCHEDS[3]),
            OptCase("ema", GRID_CAP_N, ema=(EMA_D, True), k=1), OptCase("all", GRID_CAP_N, **dict(full, table="to_seam"))]
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
NEUTRAL_CASES = [OptCase("neutral", c.n, t=c.t, off=c.off + (c.off[0],), regime=c.regime) for c in A.ADAM_CASES]


def opt_inputs(case):
    """aux_cases.adam_inputs plus the shadow arena e (zero on the padding, like the others)."""
    inp = adam_inputs(case.adam)
    gen = A.gen_for("ema" + case.id)
    e = 0.1 * torch.randn(case.n, generator=gen)
    e[inp["pad"]] = 0
    return dict(inp, e=e)


def opt_scalars(case, lr_t, f32_scalars=True):
    """(keep, a) as the kernel forms them from lr_t (float64): double arithmetic, rounded to f32."""
    r = A.f32 if f32_scalars else float
    a = r(ema_rate(case.ema[0], case.ema[1], case.k)) if case.ema else 0.0
    return r(1.0 - lr_t * case.wd), a


# ---------------------------------------------------------------------------------------------------------------- checker
def opt_check(case, inp, out):
    """out: norm, m, v, p, e (None without an EMA), step, ema_count (None without an EMA), sched (the two stored f32 as a tensor)."""
    cid, dev, h = case.id, out["m"].device, A.ADAM_HYPER
    p0, g, m0, v0 = (inp[k].to(dev).double() for k in "pgmv")
    ratios = {}
    assert int(out["step"]) == case.t, f"clip_adamw [{cid}]: step_count {int(out['step'])}, expected {case.t}"
    if case.ema:
        assert int(out["ema_count"]) == case.k + 1, f"clip_adamw [{cid}]: ema_count {int(out['ema_count'])}, expected {case.k + 1}"
    # the schedule's two scalars against the host formulas
    lr_host = h["lr"] * multiplier(case.sched, case.t - 1)
    a_host = ema_rate(case.ema[0], case.ema[1], case.k) if case.ema else 0.0
    sched = out["sched"].double().cpu()
    ratios["sched_lr"] = check("clip_adamw", cid, "sched_out[0]", sched[0].reshape(()), lr_host, (U + D_ULPS) * abs(lr_host))
    ratios["sched_a"] = check("clip_adamw", cid, "sched_out[1]", sched[1].reshape(()), a_host, (U + D_ULPS) * abs(a_host))
    lr_t, a = float(sched[0]), float(sched[1])
    # norm, exp_avg, exp_avg_sq: clip_adam's
    ssq = (g * g).sum()
    chain = 43 + A.cdiv(A.adam_partials(case.n), 256)
    norm_ref = torch.sqrt(ssq)
    ratios["sqnorm_partial"] = check("sqnorm_partial", cid, "norm_out", out["norm"].reshape(()), norm_ref,
                                     (0.5 * (chain + A.C_SUM) + SQRT) * U * norm_ref)
    coef = A.adam_coef(float(out["norm"]))
    omb1, omb2, b2, eps, bc2, _ = adam_scalars(case.t)
    gi = g * coef
    d = (gi - m0) * omb1
    mag_d = (gi.abs() + m0.abs()) * omb1
    ratios["exp_avg"] = check("clip_adamw", cid, "exp_avg", out["m"], m0 + d, U * (m0.abs() + 5 * mag_d))
    mag_v = v0 * b2 + omb2 * gi * gi
    ratios["exp_avg_sq"] = check("clip_adamw", cid, "exp_avg_sq", out["v"], mag_v, 7 * U * mag_v)
    # params from the stored moments and the stored lr_t
    m1, v1 = out["m"].double(), out["v"].double()
    inside = table_mask(table(case.table, case.n) if case.wd > 0 else [], case.n).to(dev)
    keep = 1.0 - lr_t * case.wd
    pd = torch.where(inside, p0 * keep, p0)
    pd_err = torch.where(inside, p0.abs() * (2 * abs(keep) + lr_t * case.wd), torch.zeros_like(p0))
    bc1 = 1.0 - h["b1"] ** case.t
    upd = (lr_t / bc1) * (m1 / (torch.sqrt(v1) / bc2 + eps))
    ratios["params"] = check("clip_adamw", cid, "params", out["p"], pd - upd,
                             U * (pd_err + pd.abs() + (SQRT + 3 + 3 + 1 + 1) * upd.abs()))
    pad = inp["pad"].to(dev)
    outs = {"m": out["m"], "v": out["v"], "p": out["p"]}
    if case.ema:
        e0, p1 = inp["e"].to(dev).double(), out["p"].double()
        mag = (p1.abs() + e0.abs()) * a
        ratios["ema"] = check("clip_adamw", cid, "ema", out["e"], e0 + (p1 - e0) * a, U * (e0.abs() + 3 * mag))
        outs["e"] = out["e"]
    for k, x in outs.items():
        same_bits("clip_adamw", cid, f"arena padding of {k} stays +0", x[pad], torch.zeros_like(x[pad]))
    return ratios


# ---------------------------------------------------------------------------------------------------------------- emulation
FAULTS = ("decay_after", "decay_outside", "lambda_t", "ema_old_p", "k_plus_1")


def opt_emulate(case, inp, fault=None):
    """clip_adamw in plain f32 torch.  fault: "decay_after" (the decay multiplies the updated parameter), "decay_outside" (the 16-byte
    piece after the last range decays too), "lambda_t" (the schedule is read at t instead of t - 1), "ema_old_p" (the shadow follows
    the parameter before the update), "k_plus_1" (the EMA's warm-up reads the counter after its increment)."""
    h = A.ADAM_HYPER
    p, g, m, v, e = (inp[k].clone() for k in "pgmve")
    norm = torch.sqrt((g * g).sum())
    coef = A.adam_coef(float(norm))
    lr_t = h["lr"] * multiplier(case.sched, case.t if fault == "lambda_t" else case.t - 1)
    omb1, omb2, b2, eps, bc2, step = adam_scalars(case.t, h=dict(h, lr=lr_t))
    kcase = case._replace(k=case.k + 1) if fault == "k_plus_1" else case
    keep, a = opt_scalars(kcase, lr_t)
    ranges = table(case.table, case.n) if case.wd > 0 else []
    inside = table_mask(ranges, case.n)
    if fault == "decay_outside":
        s = ranges[-1][1] if ranges else 0
        assert s < case.n
        inside[s:s + 4] = True
    gi = g * coef
    m1 = m + (gi - m) * omb1
    v1 = v * b2 + (omb2 * gi) * gi
    upd = step * (m1 / (torch.sqrt(v1) / bc2 + eps))
    if fault == "decay_after":
        p1 = torch.where(inside, (p - upd) * keep, p - upd)
    else:
        p1 = torch.where(inside, p * keep, p) - upd
    out = {"norm": norm, "m": m1, "v": v1, "p": p1, "step": case.t, "e": None, "ema_count": None,
           "sched": torch.tensor([lr_t, a], dtype=torch.float32)}
    if case.ema:
        src = p if fault == "ema_old_p" else p1
        out["e"], out["ema_count"] = e + (src - e) * a, case.k + 1
    return out
