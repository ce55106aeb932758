"""The small memory-bound kernels around the five pinned families (csrc/optim.hip, csrc/util.hip, csrc/determinism.hip and the
BatchNorm1d pair of csrc/encoder.hip): the case tables, an fp64 reference of every kernel, the per-element bounds, a plain f32 emulation
of every kernel and one checker, behind tests/test_aux_cases.py (no GPU: the references against torch's operators, the emulations
against the bounds, seeded faults, the routing restatements) and tests/test_gpu_aux_kernels.py (which runs every case on the GPU).
Nothing here touches a GPU; the references and the checker are plain torch and run on whichever device their operands live on (the
two multi-million-element Adam arenas and the large cast are checked on the device that produced them).

Rounding model.  u = 2^-24 (half an ulp of f32): every f32 add, subtract, multiply, divide and int->float conversion that is not exact
costs one u relative to its result.  A contracted fma rounds once where the uncontracted form rounds twice, so a count of the
uncontracted operations covers both.  Operations are counted per expression on the MAGNITUDES OF THE OPERANDS BEFORE CANCELLATION
(a - b counts as |a| + |b|), a k-fold count N on a term of magnitude M contributes N u M.  An error already present in an operand is
carried through the expression with the expression's derivative (stated where it is used).  Device math functions: expf 1 ulp and
rsqrtf 2 ulp (the project's allowances, tests/disc_cases.py and tests/test_gpu_trunk_layers.py); the ROCm installation carries no
accuracy table for logf, log1pf, tanhf and sqrtf, so they are taken at 2 ulp.  One ulp of a result x is at most 2^-23 |x| = 2 u |x|,
so a k-ulp function costs 2 k u.  Hyper-parameters that the kernels derive in double precision and round to f32 (Adam's step size and
bias correction) may land on the neighbouring f32 where the device's pow / sqrt differs from the host's in the last place: one u each.
  sum     a sum of n terms in any order: (n_chain + 4) u sum |terms|, where n_chain is the longest chain of roundings the kernel's
          structure allows (per-lane loop + shuffle / LDS fold levels + partials + atomics), stated with each kernel below; errors
          the terms already carry are added term by term.
  bf16    where the output is bf16: + r = 2^-8 |ref| (half a bf16 ulp).
  floor   every non-zero bound carries an underflow floor of 2^-110 (tests/disc_cases.py): results below the smallest normal number
          may be flushed, e.g. sigmoid(-100).
  exact   bit equality: casts, the embedding gather, deterministic-mode scatters against the documented order, zeros that must stay
          zero, paddings and guards.  A NaN must be a NaN where the reference has one (the payload is free) and nowhere else; an
          infinite reference must be met exactly.
Where a stage consumes what another stage stored (Adam from `norm_out` and from the kernel's own new `m`, `v`; BatchNorm1d's `xhat`,
`y`, and its backward from the stored `xhat`, `invstd`, `dgamma`, `dbeta`; the loss mean from the stored row losses) the reference is
formed from the stored values, so errors do not compound.

n_chain per kernel:
  sqnorm_partial + clip_adam's norm   16 squares + 16 adds per lane, 6 shuffle levels, 4 waves; then ceil(parts / 256) adds per
                                      lane, 6 levels and 4 waves over the partials: 43 + ceil(parts / 256).  sqrt halves the
                                      relative error of the sum and adds sqrtf's own.
  gan_losses                          ceil(n / 1024) per lane + 6 + 16 waves
  rollout_rewards                     ceil(count / 256) + 6 + 4
  xent_rows                           ceil(V / 256) + 6 + 4;  mean_kernel ceil(rows / 1024) + 6 + 16
  colsum / colsum_vec                 ceil(rows / (lanes gy)) per lane + lanes (LDS fold; 4 / 8) + gy atomics (+ 1 accumulating),
                                      gy from the launch restated in colsum_plan
  embedding_bwd (atomics)             the id's token count (+ 1 onto the destination)
  bn_stats                            ceil(R / RL) + 1 per lane (the square), RL row lanes, ceil(P / 16) + 16 over the parts
  bn1d                                ceil(B / 16) + 16
The slab fold of the column sums (colsum_fold_kernel) is not reachable through gic_colsum, which passes no scratch; it is pinned by the
discriminator's deterministic cases (tests/test_gpu_disc_stages.py) and stays there.

Largest err / bound seen per kernel on an MI355X (for judging headroom; the bounds are not fitted to these, and no derivation had to
be revisited): WORST_OBSERVED below.  Where the last operation's single rounding dominates the bound (Adam's parameter update over
4 million elements, BatchNorm1d's affine map, a bf16 store) a correctly rounded result reaches ~1."""
import math
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests.disc_cases import SENTINEL, TINY, U, U8

F64 = torch.float64
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
ULP = 2.0                      # one ulp of a result is at most 2 u of its magnitude
EXP, RSQRT = 1 * ULP, 2 * ULP  # the project's allowances
LOG = LOG1P = TANH = SQRT = 2 * ULP          # no ROCm accuracy table on the machine: 2 ulp
C_SUM = 4

# Largest err / bound per kernel measured on an MI355X by tests/test_gpu_aux_kernels.py (recorded, never asserted against).
WORST_OBSERVED = {
    "sqnorm_partial": 0.044, "clip_adam": 0.998, "gan_losses": 0.484, "rollout_rewards": 0.076, "xent_rows": 0.995, "mean": 0.051,
    "cast2d": 0.0, "colsum": 0.092, "colsum_vec": 0.098, "embedding_fwd": 0.0, "embedding_bwd": 0.182, "det_scatter": 0.0,
    "bn_stats": 0.097, "bn1d_fwd": 0.950, "bn1d_bwd": 0.932,
}


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def gen_for(case_id):
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()))


# ---------------------------------------------------------------------------------------------------------------- checker
class Mismatch(AssertionError):
    def __init__(self, kernel, case, what, index, got, ref, bound, bad, total):
        self.kernel, self.case, self.what, self.index = kernel, case, what, index
        super().__init__(f"{kernel} [{case}] {what}: {bad} of {total} elements beyond the bound; first at index {index}: "
                         f"got {got!r}, ref {ref!r}, bound {bound!r}")


def check(kernel, case, what, got, ref, bound):
    """|got - ref| <= bound element by element (NaN and infinities as in the module docstring).  Returns the largest err / bound;
    raises Mismatch naming the kernel, the case, the first failing index, got, ref and the bound."""
    g = got.double().reshape(-1)
    r = torch.as_tensor(ref, dtype=F64, device=g.device).expand(got.shape).reshape(-1)
    b = torch.as_tensor(bound, dtype=F64, device=g.device).expand(got.shape).reshape(-1)
    if g.numel() == 0:
        return 0.0
    nan_r, nan_g, inf_r = torch.isnan(r), torch.isnan(g), torch.isinf(r)
    zero, inf = torch.zeros((), dtype=F64, device=g.device), torch.full((), float("inf"), dtype=F64, device=g.device)
    err = (g - r).abs()
    err = torch.where(nan_r & nan_g, zero, err)
    err = torch.where(nan_r ^ nan_g, inf, err)
    err = torch.where(inf_r, torch.where(g == r, zero, inf), err)
    b = torch.where(nan_r | inf_r, zero, b)
    b = torch.where(b > 0, b + TINY, b)
    bad = ~(err <= b)                                   # (a NaN bound beside a finite reference fails)
    ratio = torch.where(b > 0, err / b, torch.where(err > 0, inf, zero))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise Mismatch(kernel, case, what, i, float(g[i]), float(r[i]), float(b[i]), int(bad.sum()), g.numel())
    return float(ratio.max())


def same_bits(kernel, case, what, got, want, nan_free=False):
    """Bit equality; with nan_free a NaN in `want` only asks for a NaN in `got`."""
    want = want.to(got.dtype)
    view = BITS.get(got.dtype, got.dtype)
    ok = got.contiguous().view(view) == want.contiguous().view(view)
    if nan_free:
        ok = ok | (torch.isnan(got) & torch.isnan(want))
    ok = ok.reshape(-1)
    if not bool(ok.all()):
        i = int(torch.nonzero(~ok)[0])
        raise Mismatch(kernel, case, what + " (bits)", i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]), 0.0,
                       int((~ok).sum()), ok.numel())
    return 0.0


def merge(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)
    return into


# ================================================================================================================ clip + Adam
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, clip=5.0)
K_NORM_ELEMS = 256 * 16


class AdamCase(NamedTuple):
    n: int
    off: Tuple[int, int, int, int] = (0, 0, 0, 0)      # float offsets of p, g, m, v off their 16-byte alignment
    regime: str = "clip"                               # "clip" | "noclip" | "zero_g" | "inf"
    t: int = 1                                         # the step this call performs (step_count holds t - 1 before it)

    @property
    def id(self):
        return f"n{self.n}-off{''.join(map(str, self.off))}-{self.regime}-t{self.t}"


ADAM_CASES = (
    [AdamCase(n) for n in (1, 3, 4, 5, 4095, 4096, 4097, 12291, 2 * 2 ** 20 + 4 + 1, 2048 * 2048 + 4096 + 3)]
    + [AdamCase(12291, off=o) for o in ((1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 0, 0))]
    + [AdamCase(12291, regime=r) for r in ("noclip", "zero_g", "inf")]
    + [AdamCase(4097, regime="noclip", off=(3, 3, 3, 3))]
    + [AdamCase(4097, t=t) for t in (2, 3, 10000)]
)


def adam_partials(n):
    return cdiv(n, K_NORM_ELEMS)


def adam_route(case):
    """The branches of sqnorm_partial_kernel and clip_adam_kernel a case takes, restated from csrc/optim.hip."""
    n, (op, og, om, ov) = case.n, case.off
    g_al = og % 4 == 0
    full = n // K_NORM_ELEMS if g_al else 0
    al = all(o % 4 == 0 for o in case.off)
    n4 = n // 4 if al else 0
    blocks = min(2048, cdiv(n, 256 * 8))
    return {"sq_vec_blocks": full, "sq_scalar_blocks": adam_partials(n) - full, "al": al, "n4": n4, "tail": n - 4 * n4,
            "blocks": blocks, "capped": cdiv(n, 256 * 8) > 2048, "vec_wraps": n4 > blocks * 256, "tail_wraps": n - 4 * n4 > blocks * 256}


def adam_inputs(case):
    """p, g, m, v float32 [n] on the CPU.  Every element with index % 7 == 3, and the n / 8 around the middle, is arena padding: zero
    in all four."""
    gen, n = gen_for("adam" + case.id), case.n
    p, g = 0.1 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.1 * torch.randn(n, generator=gen), (0.1 * torch.randn(n, generator=gen)) ** 2
    i = torch.arange(n)
    pad = (i % 7 == 3) | ((i >= n // 2 - n // 16) & (i < n // 2 - n // 16 + n // 8))
    for x in (p, g, m, v):
        x[pad] = 0
    if case.regime == "zero_g":
        g.zero_()
    else:
        target = {"clip": 3.0, "noclip": 0.5, "inf": 3.0}[case.regime] * ADAM_HYPER["clip"]
        g *= target / float(g.double().norm())
    if case.regime == "inf":
        g[n // 3] = float("inf")
    return {"p": p, "g": g, "m": m, "v": v, "pad": pad}


def adam_scalars(t, f32_scalars=True, h=ADAM_HYPER):
    """omb1, omb2, b2, eps, bc2_sqrt, step_size as clip_adam_kernel forms them: double arithmetic, rounded to f32."""
    r = f32 if f32_scalars else float
    bc1 = 1.0 - h["b1"] ** t
    return (r(1.0 - h["b1"]), r(1.0 - h["b2"]), r(h["b2"]), r(h["eps"]), r(math.sqrt(1.0 - h["b2"] ** t)),
            r(h["lr"] / bc1) if bc1 != 0 else float("inf"))


def adam_coef(norm, f32_scalars=True):
    """clip / (norm + 1e-6) clamped at 1, in f32 from the stored norm as the kernel computes it (norm: a Python float)."""
    if not f32_scalars:
        return min(1.0, ADAM_HYPER["clip"] / (norm + 1e-6))
    with np.errstate(all="ignore"):
        c = np.float32(ADAM_HYPER["clip"]) / (np.float32(norm) + np.float32(1e-6))
    return float(np.float32(1.0) if c > 1 else c)


def adam_check(case, inp, out, f32_scalars=True):
    """out: norm (one f32), m, v, p (the arenas after the call), step (the counter after the call).  References on out's device."""
    cid, dev = case.id, out["m"].device
    p0, g, m0, v0 = (inp[k].to(dev).double() for k in "pgmv")
    ratios = {}
    assert int(out["step"]) == case.t, f"clip_adam [{cid}]: step_count {int(out['step'])}, expected {case.t}"
    # norm: sqrt of the chained sum of squares
    ssq = (g * g).sum()
    chain = 43 + cdiv(adam_partials(case.n), 256)
    norm_ref = torch.sqrt(ssq)
    ratios["sqnorm_partial"] = check("sqnorm_partial", cid, "norm_out", out["norm"].reshape(()), norm_ref,
                                     (0.5 * (chain + C_SUM) + SQRT) * U * norm_ref)
    coef = adam_coef(float(out["norm"]), f32_scalars)
    omb1, omb2, b2, eps, bc2, step = adam_scalars(case.t, f32_scalars)
    gi = g * coef                                                        # 2 u: the division behind coef, the product
    d = (gi - m0) * omb1
    mag_d = (gi.abs() + m0.abs()) * omb1
    r = check("clip_adam", cid, "exp_avg", out["m"], m0 + d, U * (m0.abs() + 5 * mag_d))      # coef, g coef, -, *, + on |m| + |d|
    mag_v = v0 * b2 + omb2 * gi * gi
    r = max(r, check("clip_adam", cid, "exp_avg_sq", out["v"], mag_v, 7 * U * mag_v))         # gi^2 4, two products, then v b2 | +
    m1, v1 = out["m"].double(), out["v"].double()
    upd = step * (m1 / (torch.sqrt(v1) / bc2 + eps))
    # denominator: sqrtf, / bc2, bc2's own last place, + eps; then m / denom, step's last place, the product; the subtraction
    r = max(r, check("clip_adam", cid, "params", out["p"], p0 - upd, U * (p0.abs() + (SQRT + 3 + 3 + 1) * upd.abs())))
    pad = inp["pad"].to(dev)
    for k in "mvp":
        same_bits("clip_adam", cid, f"arena padding of {k} stays +0", out[k][pad], torch.zeros_like(out[k][pad]))
    ratios["clip_adam"] = r
    return ratios


def adam_emulate(case, inp, fault=None):
    """clip_adam in plain f32 torch.  fault: "seam_piece" (the last 16-byte piece before the scalar tail keeps its old values),
    "coef_twice", "t_minus_1"."""
    p, g, m, v = (inp[k].clone() for k in "pgmv")
    norm = torch.sqrt((g * g).sum())
    coef = adam_coef(float(norm))
    omb1, omb2, b2, eps, bc2, step = adam_scalars(case.t - 1 if fault == "t_minus_1" else case.t)
    gi = g * coef
    if fault == "coef_twice":
        gi = gi * coef
    m1 = m + (gi - m) * omb1
    v1 = v * b2 + (omb2 * gi) * gi
    p1 = p - step * (m1 / (torch.sqrt(v1) / bc2 + eps))
    if fault == "seam_piece":
        s = adam_route(case)["n4"] * 4
        assert s >= 4
        m1[s - 4:s], v1[s - 4:s], p1[s - 4:s] = m[s - 4:s], v[s - 4:s], p[s - 4:s]
    return {"norm": norm, "m": m1, "v": v1, "p": p1, "step": case.t}


# ================================================================================================================ gan_losses
LOSS_TYPES = ("standard", "JS", "KL", "hinge", "tv", "rsgan")
LOGIT_POOL = (0.0, 1e-8, -1e-8, 1.0, -1.0, 20.0, -20.0, 50.0, -50.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)
GRAD_NAMES = ("dd_real", "dd_fake", "dg_out", "dg_real", "dg_fake")


class GanCase(NamedTuple):
    type: str
    n: int

    @property
    def id(self):
        return f"{self.type}-n{self.n}"


GAN_CASES = [GanCase(t, n) for t in LOSS_TYPES for n in (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 9001)]


def gan_inputs(case):
    """d_real, d_fake, g_out float32 [n]: every other element from LOGIT_POOL, the rest N(0, 1); element 0 sits on the hinge kinks."""
    gen = gen_for("gan" + case.id)
    pool = torch.tensor(LOGIT_POOL)
    out = []
    for _ in range(3):
        x = torch.randn(case.n, generator=gen)
        pick = pool[torch.randint(0, len(LOGIT_POOL), (case.n,), generator=gen)]
        out.append(torch.where(torch.arange(case.n) % 2 == 0, pick, x))
    out[0][0], out[1][0] = 1.0, -1.0
    return {"d_real": out[0], "d_fake": out[1], "g_out": out[2]}


def _softplus64(z):
    return z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))


def gan_reference(case, inp):
    """fp64: per-element (ld, its bound), (lg, its bound) and the five gradients before the 1 / n with their op counts on their
    magnitudes: {name: (ref, N u-counts times magnitude)}."""
    r, f, g = (inp[k].double() for k in ("d_real", "d_fake", "g_out"))
    sg, sp, z0 = torch.sigmoid, _softplus64, torch.zeros_like(r)
    N_SIG = EXP + 2                                   # expf, 1 + e, 1 / (.)
    N_SP = EXP + LOG1P + 1                            # log1p carries e's error with a factor <= 1; the final add
    t = case.type
    grads = {k: (z0, z0) for k in GRAD_NAMES}
    if t in ("standard", "JS", "KL"):
        ld, ld_b = sp(-r) + sp(f), (N_SP + 1) * (sp(-r) + sp(f))
        grads["dd_real"] = (sg(r) - 1, (N_SIG + 1) * (1 + sg(r)))
        grads["dd_fake"] = (sg(f), N_SIG * sg(f))
        if t == "standard":
            lg, lg_b, grads["dg_out"] = sp(-g), N_SP * sp(-g), (sg(g) - 1, (N_SIG + 1) * (1 + sg(g)))
        elif t == "JS":
            lg, lg_b, grads["dg_out"] = -sp(g), N_SP * sp(g), (-sg(g), N_SIG * sg(g))
        else:
            lg, lg_b, grads["dg_out"] = -g, z0, (z0 - 1, z0)
    elif t == "hinge":
        ld = (1 - r).clamp_min(0) + (1 + f).clamp_min(0)
        ld_b = 3 * ((1 + r.abs()) + (1 + f.abs()))
        grads["dd_real"] = (-(1 - r > 0).double(), z0)
        grads["dd_fake"] = ((1 + f > 0).double(), z0)
        lg, lg_b, grads["dg_out"] = -g, z0, (z0 - 1, z0)
    elif t == "tv":
        tr, tf, tg = torch.tanh(r), torch.tanh(f), torch.tanh(g)
        ld, ld_b = tf - tr, (TANH + 1) * (tf.abs() + tr.abs())
        n_d = 2 * TANH + 2                            # t^2 doubles tanh's error, the product, the subtraction
        grads["dd_real"] = (-(1 - tr * tr), n_d * (1 + tr * tr))
        grads["dd_fake"] = (1 - tf * tf, n_d * (1 + tf * tf))
        lg, lg_b, grads["dg_out"] = -tg, TANH * tg.abs(), (-(1 - tg * tg), n_d * (1 + tg * tg))
    else:                                             # rsgan: z = r - f rounds once; |softplus'| <= 1, |sigmoid'| <= 1 / 4
        z, zm = r - f, r.abs() + f.abs()
        ld, ld_b = sp(-z), zm + N_SP * sp(-z)
        lg, lg_b = sp(z), zm + N_SP * sp(z)
        grads["dd_real"] = (sg(z) - 1, zm / 4 + (N_SIG + 1) * (1 + sg(z)))
        grads["dd_fake"] = (-(sg(z) - 1), grads["dd_real"][1])
        grads["dg_fake"] = (sg(-z) - 1, zm / 4 + (N_SIG + 1) * (1 + sg(-z)))
        grads["dg_real"] = (-(sg(-z) - 1), grads["dg_fake"][1])
    return (ld, ld_b), (lg, lg_b), grads


def gan_check(case, inp, out):
    """out: losses f32 [2] = [g_loss, d_loss]; optionally the five gradients."""
    n, cid = case.n, case.id
    (ld, ld_b), (lg, lg_b), grads = gan_reference(case, inp)
    chain = cdiv(n, 1024) + 6 + 16
    ratio = 0.0
    for idx, name, (l, lb) in ((0, "g_loss", (lg, lg_b)), (1, "d_loss", (ld, ld_b))):
        # the terms' own errors, the chained sum, 1 / n and the product
        bound = U * (lb.sum() + (chain + C_SUM + 2) * l.abs().sum()) / n
        ratio = max(ratio, check("gan_losses", cid, name, out["losses"][idx], l.sum() / n, bound))
    for name in GRAD_NAMES:
        if out.get(name) is not None:
            ref, cnt = grads[name]
            ratio = max(ratio, check("gan_losses", cid, name, out[name], ref / n, U * (cnt + 2 * ref.abs()) / n))
    return {"gan_losses": ratio}


def gan_emulate(case, inp, fault=None, want_grads=True):
    """gan_losses_kernel in plain f32 torch.  fault: "padded_mean" (the means divided by n rounded up to the 4096-element pass)."""
    r, f, g = inp["d_real"], inp["d_fake"], inp["g_out"]
    n = case.n
    sp = lambda z: z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))
    sg = lambda z: 1 / (1 + torch.exp(-z))
    z0 = torch.zeros_like(r)
    G = {k: z0 for k in GRAD_NAMES}
    t = case.type
    if t in ("standard", "JS", "KL"):
        ld = sp(-r) + sp(f)
        G["dd_real"], G["dd_fake"] = sg(r) - 1, sg(f)
        lg, G["dg_out"] = {"standard": (sp(-g), sg(g) - 1), "JS": (-sp(g), -sg(g)), "KL": (-g, z0 - 1)}[t]
    elif t == "hinge":
        ld = (1 - r).clamp_min(0) + (1 + f).clamp_min(0)
        G["dd_real"], G["dd_fake"] = -((1 - r) > 0).float(), ((1 + f) > 0).float()
        lg, G["dg_out"] = -g, z0 - 1
    elif t == "tv":
        tr, tf, tg = torch.tanh(r), torch.tanh(f), torch.tanh(g)
        ld, lg = tf - tr, -tg
        G["dd_real"], G["dd_fake"], G["dg_out"] = -(1 - tr * tr), 1 - tf * tf, -(1 - tg * tg)
    else:
        ld, lg = sp(-(r - f)), sp(-(f - r))
        G["dd_real"] = sg(r - f) - 1
        G["dd_fake"] = -G["dd_real"]
        G["dg_fake"] = sg(f - r) - 1
        G["dg_real"] = -G["dg_fake"]
    inv = torch.tensor(1.0) / torch.tensor(float(n))
    inv_l = torch.tensor(1.0) / torch.tensor(float(cdiv(n, 4096) * 4096)) if fault == "padded_mean" else inv
    out = {"losses": torch.stack([lg.sum() * inv_l, ld.sum() * inv_l])}
    if want_grads:
        out.update({k: v * inv for k, v in G.items()})
    return out


# ================================================================================================================ rollout_rewards
class RolloutCase(NamedTuple):
    B: int
    L: int
    N: int
    R: int

    @property
    def id(self):
        return f"B{self.B}-L{self.L}-N{self.N}-R{self.R}"


ROLLOUT_CASES = [RolloutCase(3, 1, 0, 5), RolloutCase(2, 4, 3, 5), RolloutCase(1, 6, 40, 8), RolloutCase(5, 3, 1, 1), RolloutCase(2, 2, 2, 300)]


def rollout_inputs(case):
    """mc_logits f32 [L - 1, N, B, R] (None for L = 1): D's logits on the roll-outs of prefix length t + 1, roll-out n, caption b,
    representation r; full_logits f32 [B, R] on the complete captions (gicap.h).  N(0, 2) with +-100 sprinkled in."""
    gen = gen_for("rollout" + case.id)

    def draw(*shape):
        x = 2 * torch.randn(*shape, generator=gen)
        k = torch.randint(0, 9, shape, generator=gen)
        return torch.where(k == 0, torch.full_like(x, 100.0), torch.where(k == 1, torch.full_like(x, -100.0), x))
    mc = draw(case.L - 1, case.N, case.B, case.R) if case.L > 1 else None
    return {"mc": mc, "full": draw(case.B, case.R)}


def rollout_check(case, inp, out):
    B, L, N, R = case
    ref, mag, cnt = torch.zeros(B, L, dtype=F64), torch.zeros(B, L, dtype=F64), torch.ones(B, L, dtype=F64)
    for t in range(L):
        s = torch.sigmoid(inp["mc"][t].double()).permute(1, 0, 2).reshape(B, N * R) if t + 1 < L else torch.sigmoid(inp["full"].double())
        ref[:, t], mag[:, t], cnt[:, t] = s.mean(1), s.sum(1), s.shape[1]
    chain = torch.ceil(cnt / 256) + 6 + 4
    bound = U * (EXP + 2 + chain + C_SUM + 1) * mag / cnt            # each sigmoid, the chained sum, the division
    return {"rollout_rewards": check("rollout_rewards", case.id, "rewards", out["rewards"], ref.to(out["rewards"].device), bound.to(out["rewards"].device))}


def rollout_emulate(case, inp, fault=None):
    """fault: "swap_n_r" (the roll-out block read as [t][r][b][n])."""
    B, L, N, R = case
    sg = lambda z: 1 / (1 + torch.exp(-z))
    out = torch.zeros(B, L)
    for t in range(L):
        if t + 1 < L:
            x = inp["mc"][t]
            x = x.reshape(R, B, N).permute(1, 2, 0) if fault == "swap_n_r" else x.permute(1, 0, 2)
            out[:, t] = sg(x.reshape(B, N * R)).sum(1) / float(N * R)
        else:
            out[:, t] = sg(inp["full"]).sum(1) / float(R)
    return {"rewards": out}


# ================================================================================================================ xent
class XentCase(NamedTuple):
    dtype: str
    rows: int
    V: int
    weighted: bool = False
    bad: Optional[int] = None                          # a target outside [0, V) on row 2: -1, or +1 for V

    @property
    def id(self):
        return f"{self.dtype}-{self.rows}x{self.V}" + ("-w" if self.weighted else "") + ({None: "", -1: "-tgt-1", 1: "-tgtV"}[self.bad])


XENT_CASES = ([XentCase(d, r, V, w) for d in ("f32", "bf16") for V in (1, 2, 255, 256, 257, 1000) for r, w in ((1, False), (5, False), (5, True))]
              + [XentCase(d, 5, 257, True, bad) for d in ("f32", "bf16") for bad in (-1, 1)])


def xent_inputs(case):
    """logits [rows, V] in the case's dtype (row 0 of a 5-row case: equal logits; row 1: a spread of 200), targets int64 [rows],
    row_weight f32 [rows] with a zero and a negative entry, or None."""
    gen = gen_for("xent" + case.id)
    x = 3 * torch.randn(case.rows, case.V, generator=gen)
    if case.rows > 1:
        x[0] = 1.25
        x[1] = torch.linspace(-100, 100, case.V) if case.V > 1 else x[1]
    tgt = torch.randint(0, case.V, (case.rows,), generator=gen)
    if case.bad is not None:
        tgt[2] = -1 if case.bad < 0 else case.V
    w = torch.tensor([0.7, 0.0, 1.3, -1.5, 2.0])[:case.rows] if case.weighted else None
    return {"logits": x.to(TD[case.dtype]), "targets": tgt, "w": w}


def xent_reference(case, inp):
    """fp64: (row_loss, its bound, dlogits, its bound); a row with a target outside [0, V) has a NaN loss and unchecked gradients."""
    x, tgt, rows, V = inp["logits"].double(), inp["targets"], case.rows, case.V
    w = inp["w"].double() if inp["w"] is not None else torch.ones(rows, dtype=F64)
    bad = (tgt < 0) | (tgt >= V)
    tc = torch.where(bad, torch.zeros_like(tgt), tgt)
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    s = e.sum(1, keepdim=True)
    chain = cdiv(V, 256) + 6 + 4
    arg = (EXP + (x - mx).abs())                       # expf, and the subtraction's rounding carried through exp (relative)
    rel_s = U * ((e * arg).sum(1, keepdim=True) / s + chain + C_SUM)
    lse, xt = mx + torch.log(s), x.gather(1, tc[:, None])
    loss = (w[:, None] * (lse - xt))[:, 0]
    # logf's own ulps on |log s|, s's relative error, the add, the subtraction, the product with the weight
    loss_b = (w.abs()[:, None] * (rel_s + U * (LOG * torch.log(s).abs() + mx.abs() + torch.log(s).abs() + lse.abs() + xt.abs())))[:, 0] + U * loss.abs()
    loss = torch.where(bad, torch.full_like(loss, float("nan")), loss)
    p = e / s
    oh = torch.zeros_like(p).scatter_(1, tc[:, None], 1.0)
    dl = (p - oh) * w[:, None] / rows
    dl_b = w.abs()[:, None] / rows * (p * (U * (arg + 1) + rel_s) + U * (p + oh) + 2 * U * (p - oh).abs())
    if case.dtype == "bf16":
        dl_b = dl_b + U8 * dl.abs()
    return loss, loss_b, dl, dl_b, bad


def xent_check(case, inp, out):
    """out: loss (the mean, one f32), row_loss f32 [rows] (the stored per-row terms), dlogits [rows, V] in the logits' dtype or None."""
    cid = case.id
    loss, loss_b, dl, dl_b, bad = xent_reference(case, inp)
    r = check("xent_rows", cid, "row_loss", out["row_loss"], loss, loss_b)
    if out.get("dlogits") is not None:
        good = ~bad
        r = max(r, check("xent_rows", cid, "dlogits", out["dlogits"][good], dl[good], dl_b[good]))
    stored = out["row_loss"].double()
    chain = cdiv(case.rows, 1024) + 6 + 16
    rm = check("mean", cid, "loss", out["loss"].reshape(()), stored.sum() / case.rows, U * (chain + C_SUM + 1) * stored.abs().sum() / case.rows)
    return {"xent_rows": r, "mean": rm}


def xent_emulate(case, inp, fault=None):
    x, tgt, rows, V = inp["logits"].float(), inp["targets"], case.rows, case.V
    w = inp["w"] if inp["w"] is not None else torch.ones(rows)
    bad = (tgt < 0) | (tgt >= V)
    tc = torch.where(bad, torch.zeros_like(tgt), tgt)
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    s = e.sum(1, keepdim=True)
    row = (w[:, None] * ((mx + torch.log(s)) - x.gather(1, tc[:, None])))[:, 0]
    row = torch.where(bad, torch.full_like(row, float("nan")), row)
    oh = torch.zeros_like(e).scatter_(1, tc[:, None], 1.0)
    dl = ((e / s - oh) * (w / float(rows))[:, None]).to(TD[case.dtype])
    return {"loss": row.sum() / float(rows), "row_loss": row, "dlogits": dl}


# ================================================================================================================ cast2d
SPECIALS = (0.0, -0.0, 1e-40, -1e-45, 2.0 ** -127, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 2.0 ** -7 + 2.0 ** -8),
            1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38,
            3.3961775292304601e38, float("inf"), float("-inf"), float("nan"), 2.0 ** -126, 2.0 ** -133 + 2.0 ** -134, 65504.0, -1e-30)
# +-0; f32 subnormals; bf16 ties with an even (1 + 2^-8 -> 1) and an odd (1 + 2^-7 + 2^-8 -> 1 + 2^-6) kept mantissa and their neighbours;
# the largest finite f32 (-> inf); the largest bf16 and the midpoint above it (a tie that rounds to inf); +-inf; NaN; the smallest normal;
# a bf16-subnormal tie.


class CastCase(NamedTuple):
    src: str
    dst: str
    rows: int
    cols: int
    lds: int
    ldd: int
    soff: int = 0                                      # elements off the 16-byte alignment
    doff: int = 0
    route: str = "scalar"                              # expected: "vec" (cast2d_f32_bf16_vec_kernel) | "scalar"

    @property
    def id(self):
        return f"{self.src}-{self.dst}-{self.rows}x{self.cols}-ld{self.lds}-{self.ldd}-off{self.soff}{self.doff}"


def cast_route(case):
    """cast2d's choice, restated: (kernel, blocks, whether the capped grid loops, whether a piece pair is odd)."""
    total = case.rows * case.cols
    if (case.src, case.dst) == ("f32", "bf16") and case.cols % 8 == 0 and case.lds % 4 == 0 and case.ldd % 8 == 0 \
            and (case.soff * 4) % 16 == 0 and (case.doff * 2) % 16 == 0:
        pieces = total // 8
        blocks = max(1, min(2048, cdiv(total // 16, 256)))
        S = blocks * 256
        # a thread converts the pieces i and i + S per pass; some thread's second piece is past the end unless 2 S divides the count
        return "vec", blocks, pieces > 2 * S, pieces % (2 * S) != 0
    return "scalar", max(1, min(2048, cdiv(total, 256))), total > 2048 * 256, False


_CAST_SHAPES = ((1, 8), (3, 8), (7, 24), (5, 7), (33, 100))
CAST_BIG = CastCase("f32", "bf16", 1, 2049 * 4096 + 8, 2049 * 4096 + 8, 2049 * 4096 + 8, route="vec")
CAST_BASE = CastCase("f32", "bf16", 7, 24, 24, 24, route="vec")
# each of the four conditions of the 16-byte kernel broken in turn (same 7 rows; the live values of the last three equal CAST_BASE's)
CAST_BROKEN = [CastCase("f32", "bf16", 7, 23, 24, 24), CastCase("f32", "bf16", 7, 24, 26, 24), CastCase("f32", "bf16", 7, 24, 24, 28),
               CastCase("f32", "bf16", 7, 24, 24, 24, soff=1), CastCase("f32", "bf16", 7, 24, 24, 24, doff=1)]
def _cast_cases():
    out = []
    for s, d in (("f32", "f32"), ("f32", "bf16"), ("f32", "bf16v"), ("bf16", "f32"), ("bf16", "bf16")):
        for r, c in _CAST_SHAPES:
            vec = d == "bf16v"                                 # the rows of the 16-byte kernel; the plain f32 -> bf16 rows break a condition
            if vec and c % 8:
                continue
            dd, route = ("bf16", "vec") if vec else (d, "scalar")
            pad = (8, 8) if vec else (3, 5)
            out.append(CastCase(s, dd, r, c, c, c, soff=1 if (s, d) == ("f32", "bf16") and c % 8 == 0 else 0, route=route))
            out.append(CastCase(s, dd, r, c, c + pad[0], c + pad[1], route=route))
    return list(dict.fromkeys(out + [CAST_BASE] + CAST_BROKEN + [CAST_BIG]))


CAST_CASES = _cast_cases()


def cast_values(rows, cols):
    """float32 [rows, cols]: the special values cycled through the first rows, Gaussians of mixed scale after them."""
    gen = gen_for(f"cast{rows}x{cols}")
    n = rows * cols
    x = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-30, 30, (n,), generator=gen).float())
    k = min(n, 4 * len(SPECIALS))
    x[:k] = torch.tensor(SPECIALS, dtype=torch.float32).repeat(4)[:k]
    return x.view(rows, cols)


def cast_inputs(case):
    """src [rows, lds] in the source dtype, its padding columns NaN."""
    src = torch.full((case.rows, case.lds), float("nan"), dtype=TD[case.src])
    src[:, :case.cols] = cast_values(case.rows, case.cols).to(TD[case.src])
    return {"src": src}


def bf16_rne(x):
    """f32 -> bf16 by round-to-nearest-even on the bit pattern, independent of torch's conversion (a NaN keeps its sign and top
    mantissa bits and gets the quiet bit)."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    nan = torch.isnan(x)
    out = torch.where(nan, (b >> 16) | 0x40, rounded) & 0xFFFF
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16).view(torch.bfloat16)


def cast_expected(case, inp):
    live = inp["src"][:, :case.cols]
    if (case.src, case.dst) == ("f32", "bf16"):
        return bf16_rne(live)
    return live.to(TD[case.dst])


def cast_check(case, inp, out):
    """out: dst [rows, ldd] as the call left it; before the call every element held SENTINEL."""
    dst = out["dst"]
    want = cast_expected(case, inp).to(dst.device)
    same_bits("cast2d", case.id, "dst", dst[:, :case.cols], want, nan_free=True)
    if case.ldd > case.cols:
        same_bits("cast2d", case.id, "dst padding untouched", dst[:, case.cols:], torch.full_like(dst[:, case.cols:], SENTINEL))
    return {"cast2d": 0.0}


def cast_emulate(case, inp, fault=None):
    """fault: "skip_odd_piece" (the 16-byte kernel's unpaired last piece stays unwritten)."""
    dst = torch.full((case.rows, case.ldd), SENTINEL, dtype=TD[case.dst])
    dst[:, :case.cols] = inp["src"][:, :case.cols].to(TD[case.dst])
    if fault == "skip_odd_piece":
        kernel, _, _, odd = cast_route(case)
        assert kernel == "vec" and odd
        dst[case.rows - 1, case.cols - 8:case.cols] = SENTINEL
    return {"dst": dst}


# ================================================================================================================ colsum
class ColsumCase(NamedTuple):
    dtype: str
    rows: int
    cols: int
    lda: int
    off: int = 0                                       # elements off the 16-byte alignment
    acc: int = 0
    det: int = 0
    route: str = "vec"

    @property
    def id(self):
        return f"{self.dtype}-{self.rows}x{self.cols}-ld{self.lda}-off{self.off}-acc{self.acc}-det{self.det}"


def colsum_plan(case):
    """colsum's launch, restated from csrc/util.hip with no scratch (gic_colsum passes none): (kernel, row lanes, gx, gy)."""
    vn = 4 if case.dtype == "f32" else 8
    esz = 16 // vn
    vec = case.cols % vn == 0 and case.lda % vn == 0 and (case.off * esz) % 16 == 0
    if vec:
        lanes, gx, gy = 8, cdiv(case.cols // vn, 32), cdiv(case.rows, 64)
        want = 2048 // max(gx, 1)
    else:
        lanes, gx, gy = 4, cdiv(case.cols, 64), cdiv(case.rows, 64)
        want = 1024 // max(gx, 1)
    gy = max(want, 1) if gy > want else gy
    if case.det:
        gy = min(gy, 1 if case.acc else 2)            # no slab: at most two block rows onto a zeroed column, one onto a live one
    return ("vec" if vec else "scalar"), lanes, gx, gy


def _colsum_cases():
    rows = (1, 7, 8, 9, 63, 64, 65, 257, 2100)
    cols = (1, 4, 8, 63, 64, 65, 100, 904)
    out = []
    for i, r in enumerate(rows):
        c = cols[i % len(cols)]
        for d in ("f32", "bf16"):
            vn = 4 if d == "f32" else 8
            out.append(ColsumCase(d, r, c, c, acc=i % 2, det=(i // 2) % 2))
            out.append(ColsumCase(d, r, c, c + 2 * vn, acc=(i + 1) % 2, det=(i // 2 + 1) % 2))
    for d, vn in (("f32", 4), ("bf16", 8)):
        out += [ColsumCase(d, 2100, 904, 904, acc=a, det=t) for a in (0, 1) for t in (0, 1)]
        # the three conditions of the 16-byte kernel broken in turn on 65 x 64 (cols, lda, the pointer), then rows < 8 on each kernel
        out += [ColsumCase(d, 65, 64, 64), ColsumCase(d, 65, 64 - 1, 64), ColsumCase(d, 65, 64, 64 + vn // 2), ColsumCase(d, 65, 64, 64, off=1),
                ColsumCase(d, 7, 64, 64, off=1, acc=1), ColsumCase(d, 7, 64, 64, det=1), ColsumCase(d, 1, 904, 904 + vn, acc=1), ColsumCase(d, 2100, 100, 101, det=1), ColsumCase(d, 257, 904, 904, off=vn // 2, acc=1, det=1)]
    out = list(dict.fromkeys(out))
    return [c._replace(route=colsum_plan(c)[0]) for c in out]


COLSUM_CASES = _colsum_cases()


def colsum_inputs(case):
    """A [rows, lda] in the case's dtype with NaN padding columns, out0 f32 [cols] (what `out` holds before an accumulating call)."""
    gen = gen_for("colsum" + case.id)
    A = torch.full((case.rows, case.lda), float("nan"), dtype=TD[case.dtype])
    A[:, :case.cols] = torch.randn(case.rows, case.cols, generator=gen).to(TD[case.dtype])
    return {"A": A, "out0": torch.randn(case.cols, generator=gen)}


def colsum_check(case, inp, out):
    A = inp["A"][:, :case.cols].double()
    o0 = inp["out0"].double() if case.acc else torch.zeros(case.cols, dtype=F64)
    _, lanes, _, gy = colsum_plan(case)
    chain = cdiv(case.rows, lanes * gy) + lanes + gy + case.acc
    kernel = "colsum_vec" if case.route == "vec" else "colsum"
    return {kernel: check(kernel, case.id, "out", out["out"], A.sum(0) + o0, U * (chain + C_SUM) * (A.abs().sum(0) + o0.abs()))}


def colsum_emulate(case, inp, fault=None):
    """fault: "drop_last_group" (the rows of the last group of 8 are left out)."""
    A = inp["A"][:, :case.cols].float()
    if fault == "drop_last_group":
        A = A[:(case.rows - 1) // 8 * 8]
    s = A.sum(0)
    return {"out": inp["out0"] + s if case.acc else s}


# ================================================================================================================ embedding
K_LONG_RUN, K_SCATTER_MAX_N, K_SCATTER_MAX_V = 64, 8192, 1 << 19
SCATTER_REFUSAL = "deterministic mode: the ordered embedding scatter takes n <= 8192 tokens and V <= 524288 (got n = {n}, V = {V})"


class EmbCase(NamedTuple):
    name: str
    V: int
    E: int
    n: int
    pattern: str                                       # "rand" | "clamp" | "runs" | "corner"
    zero_first: int = 1
    det: int = 0

    @property
    def id(self):
        return f"{self.name}-V{self.V}-E{self.E}-n{self.n}-z{self.zero_first}-det{self.det}"


def _emb_cases():
    out = []
    shapes = [("tiny", 7, 1, 1, "rand"), ("tiny", 7, 63, 2, "clamp"), ("tiny", 7, 64, 3, "clamp"), ("mid", 50, 65, 1000, "clamp"),
              ("runs", 300, 200, 8191, "runs"), ("runs", 300, 64, 8192, "runs"), ("corner", K_SCATTER_MAX_V, 1, 8192, "corner")]
    for i, s in enumerate(shapes):
        for det in (0, 1):
            out.append(EmbCase(*s, zero_first=1, det=det))
            if s[0] != "corner" or det:
                out.append(EmbCase(*s, zero_first=0, det=det))
    out.append(EmbCase("over", 300, 8, 8193, "runs", zero_first=0, det=0))
    return out


EMB_CASES = _emb_cases()
EMB_REFUSED = EmbCase("over", 300, 8, 8193, "runs", zero_first=0, det=1)


def emb_inputs(case):
    """weight f32 [V, E], ids int64 [n] (unclamped), dout f32 [n, E], dw0 f32 [V, E] (what d_weight holds before the call)."""
    gen = gen_for("emb" + case.id)
    V, E, n = case.V, case.E, case.n
    ids = torch.randint(0, V, (n,), generator=gen)
    if case.pattern in ("clamp", "runs") and n >= 2:
        ids[0], ids[n - 1] = -1, V
        if n >= 3:
            ids[1] = 2 ** 40
    if case.pattern == "runs":
        ids = torch.randint(8, V, (n,), generator=gen)
        pos = torch.randperm(n, generator=gen)
        at = 0
        for tok, length in ((1, 63), (2, 64), (3, 65), (4, 1100), (0, 70), (V - 1, 66)):
            ids[pos[at:at + length]] = tok
            at += length
        ids[pos[at]], ids[pos[at + 1]], ids[pos[at + 2]] = -1, V, 2 ** 40           # clamp into the runs of id 0 and V - 1
    if case.pattern == "corner":
        ids[n - 1] = V - 1                             # key (V - 1) << 13 | 8191 = 0xffffffff, the padding sentinel's bit pattern
        ids[5], ids[6] = V - 1, V - 1
    small = V * E <= 1 << 16
    w = torch.randn(V, E, generator=gen)
    dw0 = torch.randn(V, E, generator=gen) if small else torch.arange(V * E, dtype=torch.float32).view(V, E) % 17 - 8
    return {"weight": w, "ids": ids, "dout": torch.randn(n, E, generator=gen), "dw0": dw0}


def emb_clamped(case, inp):
    return inp["ids"].clamp(0, case.V - 1)


def emb_scatter_reference(case, inp):
    """fp64 with numpy's unbuffered add.at (independent of index_add_): (dw, sum of magnitudes, tokens per id)."""
    idc = emb_clamped(case, inp).numpy()
    d = inp["dout"].double().numpy()
    base = inp["dw0"].double().numpy() if not case.zero_first else np.zeros((case.V, case.E))
    ref, mag, cnt = base.copy(), np.abs(base), np.zeros(case.V)
    np.add.at(ref, idc, d)
    np.add.at(mag, idc, np.abs(d))
    np.add.at(cnt, idc, 1.0)
    return torch.from_numpy(ref), torch.from_numpy(mag), torch.from_numpy(cnt)


def emb_det_emulate(case, inp, descending=False):
    """det_scatter_kernel's documented order in f32: tokens sorted by (clamped id, position); a run of up to 64 is summed from zero
    in ascending position; a longer run in 16 fixed sub-ranges of ceil(len / 16), each from zero in ascending position, the 16
    partials then added from zero in wave order; the sum is added onto the destination."""
    idc = emb_clamped(case, inp).numpy()
    order = np.lexsort((np.arange(case.n), idc))
    d = inp["dout"].numpy()
    dw = (np.zeros((case.V, case.E), np.float32) if case.zero_first else inp["dw0"].numpy().copy())
    zero = np.zeros(case.E, np.float32)

    def seq(js):
        s = zero.copy()
        for j in (js[::-1] if descending else js):
            s = s + d[order[j]]
        return s
    i = 0
    while i < case.n:
        end = i + 1
        while end < case.n and idc[order[end]] == idc[order[i]]:
            end += 1
        if end - i <= K_LONG_RUN:
            s = seq(range(i, end))
        else:
            per = (end - i + 15) // 16
            s = zero.copy()
            for w in range(16):
                a = i + w * per
                s = s + seq(range(a, max(a, min(end, a + per))))
        dw[idc[order[i]]] = dw[idc[order[i]]] + s
        i = end
    return torch.from_numpy(dw)


def emb_check_fwd(case, inp, out):
    return {"embedding_fwd": same_bits("embedding_fwd", case.id, "out", out["out"], inp["weight"][emb_clamped(case, inp)].to(out["out"].device))}


def emb_check_bwd(case, inp, out):
    dw = out["dw"]
    if case.det:
        return {"det_scatter": same_bits("det_scatter", case.id, "d_weight", dw.cpu(), emb_det_emulate(case, inp))}
    ref, mag, cnt = emb_scatter_reference(case, inp)
    chain = cnt[:, None] + (0 if case.zero_first else 1)
    return {"embedding_bwd": check("embedding_bwd", case.id, "d_weight", dw.cpu(), ref, U * (chain + C_SUM) * mag * (cnt[:, None] > 0))}


def emb_emulate(case, inp, fault=None):
    """fault: "descending" (deterministic mode's runs summed from the last position down)."""
    if case.det:
        dw = emb_det_emulate(case, inp, descending=fault == "descending")
    else:
        dw = torch.zeros(case.V, case.E) if case.zero_first else inp["dw0"].clone()
        dw.index_add_(0, emb_clamped(case, inp), inp["dout"])
    return {"out": inp["weight"][emb_clamped(case, inp)], "dw": dw}


# ================================================================================================================ bn_stats
K_STATS_MAX_PARTS = 256


class StatsCase(NamedTuple):
    dtype: str
    C: int
    rows: int

    @property
    def id(self):
        return f"{self.dtype}-{self.rows}x{self.C}"


STATS_CASES = [StatsCase(d, C, r) for d in ("f32", "bf16")
               for C, r in ((8, 1), (24, 63), (72, 64), (200, 65), (256, 4099), (2048, 1), (24, 4099), (72, 65), (200, 4099), (2048, 257), (8, 4099))]


def stats_parts(rows, C):
    """determinism.hip's stats_parts, restated: (CG column groups per block, RL row lanes, gx, R rows per part, P parts)."""
    groups = C // 8
    CG = min(groups, 32)
    gx = cdiv(groups, CG)
    P = max(1, min(2048 // gx, K_STATS_MAX_PARTS, cdiv(rows, 64)))
    R = cdiv(rows, P)
    return CG, 256 // CG, gx, R, cdiv(rows, R)


def stats_inputs(case):
    gen = gen_for("stats" + case.id)
    return {"y": (torch.randn(case.rows, case.C, generator=gen) + 0.5).to(TD[case.dtype])}


def stats_check(case, inp, out):
    """out: stats f32 [2 C] = [column sums ; column sums of squares]."""
    y = inp["y"].double()
    CG, RL, gx, R, P = stats_parts(case.rows, case.C)
    chain = cdiv(R, RL) + 1 + RL + cdiv(P, 16) + 16
    ref = torch.cat([y.sum(0), (y * y).sum(0)])
    mag = torch.cat([y.abs().sum(0), (y * y).sum(0)])
    return {"bn_stats": check("bn_stats", case.id, "stats", out["stats"], ref, U * (chain + C_SUM) * mag)}


def stats_emulate(case, inp, fault=None):
    """bn_stats_part / fold in f32 with the kernels' structure.  fault: "red_g" (the fold reads row lane 0's entry red[g] for every
    row lane u instead of red[u CG + g])."""
    y = inp["y"].float()
    CG, RL, gx, R, P = stats_parts(case.rows, case.C)
    tot = torch.zeros(2 * case.C)
    for p in range(P):
        blk = y[p * R:min(case.rows, (p + 1) * R)]
        pad = torch.zeros(cdiv(blk.shape[0], RL) * RL, case.C)
        pad[:blk.shape[0]] = blk
        lanes = torch.cat([pad.view(-1, RL, case.C).sum(0), (pad * pad).view(-1, RL, case.C).sum(0)], 1)        # [RL, 2C]
        tot = tot + (lanes[0] * RL if fault == "red_g" else lanes.sum(0))
    return {"stats": tot}


# ================================================================================================================ bn1d
BN_EPS = 1e-5


class Bn1dCase(NamedTuple):
    B: int
    E: int
    training: int
    momentum: float

    @property
    def id(self):
        return f"B{self.B}-E{self.E}-{'train' if self.training else 'eval'}-m{self.momentum}"


BN1D_CASES = [Bn1dCase(B, E, tr, (0.01, 0.1)[(i + tr) % 2]) for i, (B, E) in enumerate(((1, 1), (2, 15), (15, 16), (16, 17), (17, 300), (100, 256)))
              for tr in (1, 0)]


def bn1d_inputs(case):
    """x [B, E] with column 0 constant (variance 0), gamma, beta, the running statistics before the call, dy."""
    gen = gen_for("bn1d" + case.id)
    B, E = case.B, case.E
    x = 1.5 * torch.randn(B, E, generator=gen) + torch.randn(E, generator=gen)
    x[:, 0] = 0.7251
    return {"x": x, "gamma": 1 + 0.3 * torch.randn(E, generator=gen), "beta": 0.2 * torch.randn(E, generator=gen),
            "rm0": 0.5 * torch.randn(E, generator=gen), "rv0": 0.5 + torch.rand(E, generator=gen), "dy": torch.randn(B, E, generator=gen)}


def bn1d_check_fwd(case, inp, out):
    """out: y, xhat [B, E], invstd, rm, rv [E] after the call."""
    cid, B = case.id, case.B
    x, g, bt, rm0, rv0 = (inp[k].double() for k in ("x", "gamma", "beta", "rm0", "rv0"))
    mom, eps = f32(case.momentum), f32(BN_EPS)
    chain = cdiv(B, 16) + 16
    r = 0.0
    if case.training:
        mean = x.mean(0)
        e_m = U * (chain + C_SUM + 1) * x.abs().sum(0) / B                       # the chained sum and the division
        dev = x - mean
        var = (dev * dev).mean(0)
        # with the kernel's own mean m~ the sum of squares is exactly B (var + (m - m~)^2); each term: the subtraction, its square
        # (2 + 1), then the chained sum and the division
        b_var = e_m ** 2 + U * (chain + C_SUM + 4) * ((dev.abs() + e_m) ** 2).sum(0) / B
        is_ref = (var + eps) ** -0.5
        is_hi = (var + eps - b_var).clamp_min(1e-300) ** -0.5                    # rsqrt is monotone: the error var's bound allows
        r = max(r, check("bn1d_fwd", cid, "invstd", out["invstd"], is_ref, (is_hi - is_ref) + U * (RSQRT + 1) * is_hi))
        is_s = out["invstd"].double()
        r = max(r, check("bn1d_fwd", cid, "xhat", out["xhat"], dev * is_s, is_s * (e_m + 2 * U * (dev.abs() + e_m))))
        unb = B / (B - 1) if B > 1 else 1.0
        r = max(r, check("bn1d_fwd", cid, "running_mean", out["rm"], (1 - mom) * rm0 + mom * mean,
                         mom * e_m + 3 * U * ((1 - mom) * rm0.abs() + mom * mean.abs())))
        r = max(r, check("bn1d_fwd", cid, "running_var", out["rv"], (1 - mom) * rv0 + mom * var * unb,
                         mom * unb * b_var + 5 * U * ((1 - mom) * rv0 + mom * var * unb)))
    else:
        is_ref = (rv0 + eps) ** -0.5
        r = max(r, check("bn1d_fwd", cid, "invstd", out["invstd"], is_ref, U * (RSQRT + 1) * is_ref))
        is_s = out["invstd"].double()
        r = max(r, check("bn1d_fwd", cid, "xhat", out["xhat"], (x - rm0) * is_s, 2 * U * (x.abs() + rm0.abs()) * is_s))
        same_bits("bn1d_fwd", cid, "running_mean unchanged", out["rm"], inp["rm0"])
        same_bits("bn1d_fwd", cid, "running_var unchanged", out["rv"], inp["rv0"])
    xh = out["xhat"].double()
    r = max(r, check("bn1d_fwd", cid, "y", out["y"], xh * g + bt, 2 * U * ((xh * g).abs() + bt.abs())))
    return {"bn1d_fwd": r}


def bn1d_check_bwd(case, inp, saved, out):
    """saved: the stored xhat, invstd the backward read; out: dx [B, E], dgamma, dbeta [E]."""
    cid, B = case.id, case.B
    dy, g = inp["dy"].double(), inp["gamma"].double()
    xh, is_s = saved["xhat"].double(), saved["invstd"].double()
    chain = cdiv(B, 16) + 16
    r = check("bn1d_bwd", cid, "dgamma", out["dgamma"], (dy * xh).sum(0), U * (chain + C_SUM + 1) * (dy * xh).abs().sum(0))
    r = max(r, check("bn1d_bwd", cid, "dbeta", out["dbeta"], dy.sum(0), U * (chain + C_SUM) * dy.abs().sum(0)))
    k = g * is_s
    if case.training:
        sg, sb = out["dgamma"].double(), out["dbeta"].double()
        ref = k * (dy - (sb + xh * sg) / B)
        mag = dy.abs() + (sb.abs() + (xh * sg).abs()) / B                        # k, 1 / B, xh sg, + sb, * 1 / B, d - ., * k
        r = max(r, check("bn1d_bwd", cid, "dx", out["dx"], ref, 7 * U * k.abs() * mag))
    else:
        r = max(r, check("bn1d_bwd", cid, "dx", out["dx"], k * dy, 2 * U * (k * dy).abs()))
    return {"bn1d_bwd": r}


def bn1d_emulate(case, inp, fault=None):
    x, g, bt, rm, rv, dy = (inp[k] for k in ("x", "gamma", "beta", "rm0", "rv0", "dy"))
    B = case.B
    mom, eps = torch.tensor(case.momentum), torch.tensor(BN_EPS)
    if case.training:
        mean = x.sum(0) / float(B)
        var = ((x - mean) ** 2).sum(0) / float(B)
        unb = torch.tensor(float(B)) / torch.tensor(float(B - 1)) if B > 1 else torch.tensor(1.0)
        rm, rv = (1 - mom) * rm + mom * mean, (1 - mom) * rv + mom * var * unb
    else:
        mean, var = rm, rv
    inv = torch.rsqrt(var + eps)
    xh = (x - mean) * inv
    out = {"y": xh * g + bt, "xhat": xh, "invstd": inv, "rm": rm, "rv": rv}
    sg, sb = (dy * xh).sum(0), dy.sum(0)
    k = g * inv
    out.update(dgamma=sg, dbeta=sb, dx=k * (dy - (1 / torch.tensor(float(B))) * (sb + xh * sg)) if case.training else k * dy)
    return out
