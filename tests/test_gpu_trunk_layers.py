"""Every trunk convolution of one eager training pass, element by element, against an fp64 reference formed from the operands the
kernel consumed.

One training-mode pass of ResNetTrunk (parameters from oracle.cpu_encoder.make_trunk_params) leaves every stored tensor and the
operands it was made from on the device.  The walk over TrunkPlan.conv_shapes(N, S) checks each layer on its own: the reference
is computed in float64 (torch on the GPU, never through the library) from the GPU's own stored inputs, packed weights and f32
BatchNorm sums, so kernel error is separated from what 53 stacked BatchNorms do to rounding noise.

Checked per case: the packed weights equal the master weights rounded to the compute type; every stored convolution output element
by element; every layer's BatchNorm sum and sum of squares (replicas folded), including the statistics-only pass whose conv3 output
is never stored; every tensor a BatchNorm pass or a fused launch stores (z1 / z2 of bn_act, every block output, whether bn_act, the
residual-on-load conv1 or conv_b2b formed it); the stem's BatchNorm + ReLU + max-pool (x0); the pooled feature; the running mean
and unbiased running variance of every layer (momentum 0.1).

Rounding model (u = 2^-24, the f32 unit roundoff; r = 2^-8 in bf16 mode, the largest relative error of rounding to bf16; r = u in
fp32 mode):

* Operands normalised on load.  The kernel forms t = y*sc + sh (+ res*rs + rh), sc = gamma * rsqrtf(var + eps), sh = beta - mean*sc
  from the replicas of the producer's f32 sums (csrc/bn_fold.h), in f32, then ReLU and rounding.  The reference forms t in fp64 from
  the same f32 sums and bounds |t_kernel - t| by delta: the fold of nrep replicas and the 1/count scaling (nrep + 3 roundings of the
  sums), the cancellation in var = E[y^2] - mean^2 (propagated exactly through rsqrt over [var - dvar, var + dvar]), 8 roundings of
  sc (rsqrtf is within 2 ulp), 3 of sh and 4 of the affine map, all doubled.  Rounding is monotone, so the kernel's operand lies in
  [lo, hi] = [R(relu(t - delta)), R(relu(t + delta))] (R: round to the stored type); lo == hi away from a rounding boundary.  A
  stored operand is exact.  dA = hi - lo is an operand's allowance.
* Accumulation.  Products of bf16 operands are exact in f32.  The bf16 kernels accumulate on MFMA into f32 registers: one rounding
  per instruction (16 or 32 products), at most 5 inside one instruction's partial dot product, a few when partial accumulators or
  the epilogue combine.  A summation with at most n roundings on any path errs by at most n*u*sum_k |a_k w_k| (Higham's gamma_n), so
  c = (K/8 + 16) * u, four times the MFMA chain (K <= 4608: c <= 3.5e-5).  fp32 mode assumes nothing about the order: c = (K + 16) u.
* Element bound: |got - ref| <= r*|ref| + (1 + r) * E,  E = (1 + 2^-7) * sum_k (c |a_k| + dA_k) |w_k|  -- the fp64 convolution of
  c|a| + dA with |w|.  The first term is the final rounding, E the accumulator's distance from ref.
* Sums.  The epilogues sum the f32 accumulators; on any column the chain of roundings is at most rows / (64 nrep) (atomics per replica
  address, row tiles of >= 64 rows) + 256 (values one lane adds within a tile, lanes, waves, the replica fold) = n_red, so
  |s1 - sum ref| <= sum E + n_red u sum(|ref| + E) and |s2 - sum ref^2| <= sum E (2|ref| + E) + (n_red + 1) u sum (|ref| + E)^2.
  Where the sums are taken from the stored tensor (deterministic mode: gic_bn_stats; fp32 mode: the stored value is the accumulator)
  the reference is the sum of the stored tensor and only the n_red term applies.
* A tensor recomputed in registers and never stored (conv3 inside conv_b2b) enters the block output with |sc3| * E3 added to delta.
* Pooled feature: HW sequential f32 additions, then rounding: |got - ref| <= r|ref| + (1 + r)(HW + 2) u mean|x|.

There is no fraction-of-outliers allowance and no norm check.  A failure names the layer, the buffer, the first failing (image, row,
column, channel), got, ref and the bound.  test_checker_flags_the_failures_this_family_has_had shows that the same check flags a
misplaced 16-byte store, a row tile shifted by one row and one 16-byte operand piece (8 input channels of one tap) missing from the
reference of one output channel.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_encoder as OE

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _relu(t):
    return t.clamp_min(0.0)


def _rounder(mode):
    if mode == "fp32":
        return lambda t: t.float().double()
    return lambda t: t.float().bfloat16().double()


def _conv64(a, w, stride, pad):
    """a NHWC float64, w [Cout, KH, KW, Cin] float64 -> NHWC float64 (torch on the device, a few images at a time)."""
    wt = w.permute(0, 3, 1, 2).contiguous()
    N, H, W, _ = a.shape
    ho, wo = (H + 2 * pad - w.shape[1]) // stride + 1, (W + 2 * pad - w.shape[2]) // stride + 1
    per = max(1, (1 << 25) // max(1, ho * wo * max(w.shape[0], a.shape[3])))
    out = torch.empty(N, ho, wo, w.shape[0], dtype=torch.float64, device=a.device)
    for i in range(0, N, per):
        out[i:i + per] = F.conv2d(a[i:i + per].permute(0, 3, 1, 2).contiguous(), wt, None, stride, pad).permute(0, 2, 3, 1)
    return out


class _Coef:
    """Per-channel (scale, shift) of one BatchNorm in fp64 from the GPU's f32 sums, with bounds on the kernel's f32 values."""

    def __init__(self, b, step):
        C, nrep = step.cout, b["nrep"][step.name]
        st = b["stats"][step.stats_off:step.stats_off + 2 * C * nrep].view(nrep, 2, C).double()
        n = float(b["rows"][step.name])
        self.name, self.nrep, self.n = step.name, nrep, n
        self.s1, self.s2 = st[:, 0].sum(0), st[:, 1].sum(0)
        g, be = step.bn.weight.detach().double(), step.bn.bias.detach().double()
        mean, ex2 = self.s1 / n, self.s2 / n
        var = (ex2 - mean * mean).clamp_min(0)
        dmean = U * (nrep + 3) * st[:, 0].abs().sum(0) / n
        dvar = U * (nrep + 3) * ex2 + 2 * mean.abs() * dmean + dmean * dmean + 3 * U * (ex2 + mean * mean)
        inv = lambda v: torch.rsqrt(v + EPS32)
        self.sc = g * inv(var)
        self.dsc = g.abs() * torch.maximum(inv((var - dvar).clamp_min(0)) - inv(var), inv(var) - inv(var + dvar)) + 8 * U * self.sc.abs()
        self.sh = be - mean * self.sc
        self.dsh = dmean * self.sc.abs() + mean.abs() * self.dsc + dmean * self.dsc + 3 * U * (be.abs() + (mean * self.sc).abs())


def _form(y, cy, rnd, res=None, cr=None, dy=None):
    """relu(bn(y) [+ bn_r(res) | + res]) rounded as stored: (reference, lo, hi).  dy: bound on |y_kernel - y| (a register value)."""
    ya = y.abs() if dy is None else y.abs() + dy
    t = y * cy.sc + cy.sh
    d = ya * cy.dsc + cy.dsh + 4 * U * (ya * cy.sc.abs() + cy.sh.abs())
    if dy is not None:
        d = d + dy * cy.sc.abs()
    if res is not None:
        if cr is None:
            t = t + res
            d = d + 4 * U * res.abs()
        else:
            t = t + (res * cr.sc + cr.sh)
            d = d + res.abs() * cr.dsc + cr.dsh + 4 * U * (res.abs() * cr.sc.abs() + cr.sh.abs())
    d = 2 * d
    return rnd(_relu(t)), rnd(_relu(t - d)), rnd(_relu(t + d))


def _where(idx, shape):
    out = []
    for s in reversed(shape):
        out.append(idx % s)
        idx //= s
    return tuple(reversed(out))


def check_elements(got, ref, bound):
    """-> (number of elements with |got - ref| > bound, largest |got - ref| / bound, first failure (index, got, ref, bound) or None)."""
    err = (got - ref).abs()
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max()) if err.numel() else 0.0
    first = None
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        first = (_where(i, got.shape), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]))
    return nbad, ratio, first


def check_interval(got, z, lo, hi):
    """-> (elements outside [lo, hi], elements off the reference rounding z (inside the interval), first failure or None)."""
    bad = ~((got >= lo) & (got <= hi))
    nbad = int(bad.sum())
    first = None
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        first = (_where(i, got.shape), float(got.reshape(-1)[i]), float(z.reshape(-1)[i]),
                 (float(lo.reshape(-1)[i]), float(hi.reshape(-1)[i])))
    return nbad, int((got != z).sum()), first


class Walk:
    def __init__(self, trunk, N, S, mode):
        self.plan = plan = trunk._plan
        self.N, self.S, self.mode = N, S, mode
        self.b = plan._bufs[plan._bkey(N, S)]
        self.rnd = _rounder(mode)
        self.r = U if mode == "fp32" else 2.0 ** -8
        self.failures, self.table = [], []
        self.stats_from_stored = mode in ("fp32", "det")
        self.act = plan.act

    def fail(self, what):
        self.failures.append(what)

    # ---- a convolution: reference, accumulation bound
    def conv(self, s, A, dA, stride, pad):
        W = s.w.double()
        K = W.shape[1] * W.shape[2] * W.shape[3]
        c = ((K + 16) if self.mode == "fp32" else (K / 8 + 16)) * U
        ref = _conv64(A, W, stride, pad)
        absA = c * A.abs() if dA is None else c * A.abs() + dA
        E = _conv64(absA, W.abs(), stride, pad) * (1 + 2.0 ** -7)
        return ref, E, K

    def weights(self, s):
        m = s.conv.weight.detach().permute(0, 2, 3, 1)
        if s is self.plan.stem:
            want = torch.zeros(64, 7, 8, 4, device=m.device, dtype=self.act)
            want[:, :, :7, :3] = m.to(self.act)
        else:
            want = m.to(self.act)
        if not torch.equal(s.w, want):
            self.fail(f"{s.name}: packed weights differ from the master weights rounded to {self.act} "
                      f"({int((s.w != want).sum())} of {want.numel()})")

    def bound(self, ref, E):
        return self.r * ref.abs() + (1 + self.r) * E + 1e-30

    def elements(self, s, buf, got, ref, E, form, K, unc):
        nbad, ratio, first = check_elements(got.double(), ref, self.bound(ref, E))
        self.table.append((s.name, form, buf, K, ratio, unc))
        if nbad:
            (n, h, w, ch), g, rf, bd = first
            self.fail(f"{s.name} [{form}] {buf}: {nbad} elements out of bound; first at image {n} row {h} col {w} channel {ch}: "
                      f"got {g:.6g} ref {rf:.6g} bound {bd:.3g}")

    def sums(self, s, cy, ref, E, stored):
        nred = cy.n / (64 * cy.nrep) + 256
        if self.stats_from_stored:
            v = stored.double()
            s1r, s2r = v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))
            b1 = nred * U * v.abs().sum((0, 1, 2))
            b2 = (nred + 1) * U * (v * v).sum((0, 1, 2))
        else:
            s1r, s2r = ref.sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))
            m = ref.abs() + E
            b1 = E.sum((0, 1, 2)) + nred * U * m.sum((0, 1, 2))
            b2 = (E * (2 * ref.abs() + E)).sum((0, 1, 2)) + (nred + 1) * U * (m * m).sum((0, 1, 2))
        for what, got, want, bd in (("sum", cy.s1, s1r, b1), ("sum of squares", cy.s2, s2r, b2)):
            err = (got - want).abs()
            bad = ~(err <= bd)
            self.table.append((s.name, "bn sums", what, 0, float((err / bd.clamp_min(1e-300)).max()), 0.0))
            if bad.any():
                ch = int(bad.nonzero()[0])
                self.fail(f"{s.name} BatchNorm {what}: {int(bad.sum())} channels out of bound; first channel {ch}: got {float(got[ch]):.8g} "
                          f"ref {float(want[ch]):.8g} bound {float(bd[ch]):.3g}")
        self.running(s, cy, s1r, s2r, b1, b2)

    def running(self, s, cy, s1r, s2r, b1, b2):
        n = cy.n
        mean, ex2 = s1r / n, s2r / n
        var = ex2 - mean * mean
        dmean = b1 / n
        dvar = b2 / n + 2 * mean.abs() * dmean + dmean * dmean + (cy.nrep + 6) * U * (ex2 + mean * mean)
        unb = n / (n - 1)
        rm_ref, rv_ref = 0.1 * mean, 0.9 + 0.1 * var * unb
        checks = (("running_mean", s.bn.running_mean.double(), rm_ref, 0.1 * dmean + 4 * U * rm_ref.abs() + 1e-30),
                  ("running_var", s.bn.running_var.double(), rv_ref, 0.1 * dvar * unb + 4 * U * (0.9 + (0.1 * var * unb).abs())))
        for what, got, want, bd in checks:
            err = (got - want).abs()
            bad = ~(err <= bd)
            self.table.append((s.name, "running", what, 0, float((err / bd).max()), 0.0))
            if bad.any():
                ch = int(bad.nonzero()[0])
                self.fail(f"{s.name} {what}: {int(bad.sum())} channels out of bound; first channel {ch}: got {float(got[ch]):.8g} "
                          f"ref {float(want[ch]):.8g} bound {float(bd[ch]):.3g}")

    def interval(self, name, buf, got, z, lo, hi):
        nbad, noff, first = check_interval(got.double(), z, lo, hi)
        self.table.append((name, "formed", buf, 0, float(nbad), float(noff) / max(1, z.numel())))
        if nbad:
            (n, h, w, ch), g, rf, (l, hh) = first
            self.fail(f"{name} {buf}: {nbad} elements outside the rounding interval; first at image {n} row {h} col {w} channel {ch}: "
                      f"got {g:.6g} ref {rf:.6g} interval [{l:.6g}, {hh:.6g}]")

    def operand(self, blk, s, prev, xi, x, coef):
        """The A operand the kernel of layer `s` consumed: (A NHWC float64, allowance dA or None, form)."""
        if prev is None or prev[0] in ("res", "b2b"):
            # a plain input, or conv1 of a block whose input was formed on load: the stored block output is the operand (checked
            # against its formation when the previous block closed)
            return x.double(), None, {None: "plain", "res": "block output on load", "b2b": "conv3 + block output + conv1"}[
                None if prev is None else prev[0]]
        if prev[0] == "b2bstats":
            A, lo, hi = _form(prev[2].double(), coef[blk["c2"].name], self.rnd)
            return A, hi - lo, "statistics only"
        if s.fused_in is True:
            A, lo, hi = _form(prev[1].double(), coef[prev[0].name], self.rnd)
            return A, hi - lo, "bn + relu on load"
        z, lo, hi = _form(prev[1].double(), coef[prev[0].name], self.rnd)
        self.interval(prev[0].name, "z (bn_act)", xi, z, lo, hi)
        return xi.double(), None, "plain"

    # ---- the walk
    def run(self):
        plan, b, rnd = self.plan, self.b, self.rnd
        entries = {e[0].name: e for e in plan.conv_shapes(self.N, self.S)}
        coef = {}
        # stem: 7 x 8 window over the zero-bordered NHWC4 image, stride 2
        s = plan.stem
        self.weights(s)
        coef[s.name] = cy = _Coef(b, s)
        ref, E, K = self.conv(s, b["xin"].double(), None, 2, 0)
        self.elements(s, "y0", b["y0"], ref, E, "stem", K, 0.0)
        self.sums(s, cy, ref, E, b["y0"])
        z, lo, hi = _form(b["y0"].double(), cy, rnd)
        mp = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        self.interval("stem", "x0 (bn + relu + max-pool)", b["x0"], mp(z), mp(lo), mp(hi))
        del ref, E, z, lo, hi
        x = b["x0"]
        for blk, e in zip(plan.blocks, b["blocks"]):
            y3reg = None
            for s in (blk["c1"], blk["c2"], blk["c3"], blk["ds"]):
                if s is None:
                    continue
                _, xi, yo, _H, _W, _kw, _macs, prev = entries[s.name]
                self.weights(s)
                coef[s.name] = cy = _Coef(b, s)
                A, dA, form = self.operand(blk, s, prev, xi, x, coef)
                unc = 0.0 if dA is None else float((dA > 0).double().mean())
                ref, E, K = self.conv(s, A, dA, s.stride, s.pad)
                del A, dA
                if form == "statistics only":
                    self.table.append((s.name, form, "(y3 never stored)", K, 0.0, unc))
                    self.sums(s, cy, ref, E, None)
                    y3reg = (ref, E)
                else:
                    self.elements(s, "y", yo, ref, E, form, K, unc)
                    self.sums(s, cy, ref, E, yo)
                    del ref, E
            # the block output, however it was formed
            last = blk["c3"] if blk["c3"] is not None else blk["c2"]
            ds = blk["ds"]
            res, cr = (e["yd"].double(), coef[ds.name]) if ds is not None else (x.double(), None)
            if y3reg is not None:
                z, lo, hi = _form(y3reg[0], coef[last.name], rnd, res, cr, dy=y3reg[1])
                how = "block output (conv_b2b, conv3 in registers)"
            else:
                ylast = e["y3"] if blk["c3"] is not None else e["y2"]
                z, lo, hi = _form(ylast.double(), coef[last.name], rnd, res, cr)
                how = "block output"
            self.interval(last.name, how, e["out"], z, lo, hi)
            del z, lo, hi, res, y3reg
            x = e["out"]
        # pooled feature
        v = x.double()
        HW = v.shape[1] * v.shape[2]
        ref = v.mean((1, 2))
        bound = self.r * ref.abs() + (1 + self.r) * (HW + 2) * U * v.abs().mean((1, 2)) + 1e-30
        nbad, ratio, first = check_elements(b["feat"].double(), ref, bound)
        self.table.append(("avgpool", "pooled", "feat", HW, ratio, 0.0))
        if nbad:
            self.fail(f"pooled feature: {nbad} out of bound; first {first}")
        return self


def _trunk(arch, S, N, dtype, dev, seed, plan_setup=None):
    from gan_image_captioning_amd import encoder_engine
    from gan_image_captioning_amd.trunk import ResNetTrunk
    g = torch.Generator().manual_seed(seed)
    tp = OE.make_trunk_params(arch, g)
    images = torch.randn(N, 3, S, S, generator=g)
    trunk = ResNetTrunk(arch)
    trunk.load_state_dict({k[len("encoder.resnet."):]: v for k, v in tp.items()}, strict=False)
    trunk = trunk.to(dev).train()
    trunk._plan = encoder_engine.TrunkPlan(trunk, dtype)
    trunk._plan.use_graph = False
    if plan_setup is not None:
        plan_setup(trunk._plan)
    trunk(images.to(dev), dtype)
    torch.cuda.synchronize()
    return trunk


def _report(tag, walk):
    worst = {}
    for name, form, buf, K, ratio, unc in walk.table:
        key = (form, buf)
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, name, K, unc)
    print(f"\n[{tag}] largest error / bound per form (formed tensors: elements outside the interval, fraction off the reference rounding)")
    for (form, buf), (ratio, name, K, unc) in sorted(worst.items()):
        print(f"[{tag}]   {form:32s} {buf:44s} {ratio:9.3g}  worst layer {name:16s} K={K:5d}  {unc:.2e}")
    for name, form, buf, K, ratio, unc in walk.table:
        if form not in ("bn sums", "running"):
            print(f"[{tag}] layer {name:18s} {form:30s} {buf:44s} K={K:5d} {ratio:9.3g}")


def _c3s(plan):
    return [blk["c3"] for blk in plan.blocks if blk["c3"] is not None]


CASES = [
    # arch, S, N, mode, why
    ("resnet50", 224, 64, "bf16"),       # the cfg2 bench shape: conv_b2b at 56^2 / 28^2, conv1x1_pix at 14^2 / 7^2, 8 replicas
    ("resnet50", 256, 16, "bf16"),       # the CLI default size: b2b at 64^2 only, pix / panel eligibility at 16^2 / 8^2
    ("resnet18", 256, 8, "bf16"),        # the reference's own trunk at its default size: stride-1 3x3 layers on the patch kernel
    ("resnet50", 200, 3, "bf16"),        # rows not multiples of 128 (7 500 at 50^2): M tails, conv_b2b declines, bn on load engages
    ("resnet50", 200, 3, "bf16-res"),    # ... with the residual-on-load conv1 taking every eligible boundary (M tails in that kernel)
    ("resnet50", 224, 8, "det"),         # deterministic mode: gic_bn_stats statistics, no fused forms
    ("resnet50", 224, 16, "bf16-unfused"),  # the separate-pass plan (GIC_NO_FUSED_BN_IN): bn_act z tensors, plain K = 256 conv3s (panel)
    ("resnet18", 96, 2, "fp32"),         # fp32 parity mode: the bound tightened to f32 rounding
]


@pytest.mark.parametrize("arch,S,N,mode", CASES, ids=[f"{a}-{s}-{n}-{m}" for a, s, n, m in CASES])
def test_every_trunk_layer_element_wise(dev, arch, S, N, mode):
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    dtype = 0 if mode == "fp32" else 1
    setup = None
    if mode == "bf16-res":
        def setup(plan):
            plan.res_min_rows = 0                    # the residual-on-load conv1 on every eligible boundary (tuning switch of the plan)
    elif mode == "bf16-unfused":
        def setup(plan):
            plan.fuse_in = False                     # no BatchNorm on load (and so no conv_b2b): every normalised input is stored
    engine.set_deterministic(mode == "det")
    try:
        trunk = _trunk(arch, S, N, dtype, dev, seed=S * 100 + N, plan_setup=setup)
        plan = trunk._plan
        # the fused forms that must have engaged (a silent fall-back would leave a case vacuous)
        unstored = plan.unstored_convs()
        fused_c3 = [s.name for s in _c3s(plan) if s.fused_in is True]
        fused_any = [s.name for s in plan.steps if s.fused_in is True]
        stride1_c2 = [blk["c2"] for blk in plan.blocks if blk["c2"].stride == 1]
        if mode == "bf16" and (arch, S, N) == ("resnet50", 224, 64):
            assert unstored == {f"4.{i}.conv3" for i in range(3)} | {f"5.{i}.conv3" for i in range(4)}, unstored
            assert all(blk["c3"].fused_in is True for blk in plan.blocks if blk.get("b2b") is not True), fused_c3
            assert all(s.fused_in is True for s in stride1_c2), [s.name for s in stride1_c2 if s.fused_in is not True]
        elif mode == "bf16" and (arch, S, N) == ("resnet50", 256, 16):
            assert unstored == {"4.0.conv3", "4.1.conv3", "4.2.conv3"}, unstored
            assert all(blk["c3"].fused_in is True for blk in plan.blocks if blk.get("b2b") is not True)
            assert all(s.fused_in is True for s in stride1_c2)
        elif mode == "bf16" and arch == "resnet18":
            assert not unstored and all(s.fused_in is True for s in stride1_c2), [s.name for s in stride1_c2 if s.fused_in is not True]
        elif mode in ("bf16", "bf16-res") and S == 200:
            assert not unstored and not any(blk.get("b2b") for blk in plan.blocks)
            assert all(blk["c3"].fused_in is True for blk in plan.blocks), fused_c3
            assert all(s.fused_in is True for s in stride1_c2)
            rows50 = plan._bufs[(N, S)]["rows"]["4.0.conv3"]
            assert rows50 == 7500
            if mode == "bf16-res":
                res_in = {blk["c1"].name for blk in plan.blocks if blk["c1"].fused_in is True}
                assert res_in == {"4.1.conv1", "4.2.conv1", "5.0.conv1", "5.1.conv1", "5.2.conv1", "5.3.conv1"}, res_in
            else:
                # conv_b2b needs rows % 128 == 0: the plan declines it at every boundary, even with the row floor lowered, and so
                # does the library (host-side refusal: nothing is launched)
                plan.res_min_rows = 0
                for blk, nxt in zip(plan.blocks, plan.blocks[1:]):
                    assert not plan._b2b_ok(blk, nxt, plan._bufs[(N, S)]["rows"][blk["c3"].name], True), blk["c3"].name
                b = plan._bufs[(N, S)]
                e0, e1 = b["blocks"][0], b["blocks"][1]
                blk0, c1n = plan.blocks[0], plan.blocks[1]["c1"]
                c2, c3, ds = blk0["c2"], blk0["c3"], blk0["ds"]
                base = b["stats"].data_ptr()
                status = L.load().gic_conv_b2b(
                    e0["y2"].data_ptr(), base + 4 * c2.stats_off, b["nrep"][c2.name], c2.bn.weight.data_ptr(), c2.bn.bias.data_ptr(),
                    c3.w.data_ptr(), base + 4 * c3.stats_off, b["nrep"][c3.name], c3.bn.weight.data_ptr(), c3.bn.bias.data_ptr(),
                    e0["yd"].data_ptr(), base + 4 * ds.stats_off, b["nrep"][ds.name], ds.bn.weight.data_ptr(), ds.bn.bias.data_ptr(),
                    float(rows50), e0["out"].clone().data_ptr(), c1n.w.data_ptr(), e1["y1"].clone().data_ptr(),
                    torch.zeros_like(b["stats"]).data_ptr(), b["nrep"][c1n.name], 1, rows50, c2.cout, c1n.cout, engine.stream_ptr())
                torch.cuda.synchronize()
                assert status == L.ERR_UNSUPPORTED, status
                plan.res_min_rows = 50000
        elif mode in ("det", "fp32"):
            assert not unstored and not fused_any, fused_any
        elif mode == "bf16-unfused":
            assert not unstored and not any(s.fused_in is True for blk in plan.blocks for s in (blk["c2"], blk["c3"])), fused_any
        walk = Walk(trunk, N, S, "fp32" if mode == "fp32" else ("det" if mode == "det" else "bf16")).run()
    finally:
        engine.set_deterministic(False)
    _report(f"{arch}@{S}x{N} {mode}", walk)
    assert not walk.failures, "\n".join(walk.failures[:40])


def test_checker_flags_the_failures_this_family_has_had(dev):
    """The element-wise check above, applied to a perturbed copy of real outputs (or a perturbed reference; no kernel is touched),
    flags each failure this kernel family has had: a 16-byte store landing one piece along the row, a 128-row tile's output shifted
    by one row (a tile seam), and one 16-byte operand piece (8 input channels of one tap) missing from one output channel (a lost
    LDS-DMA piece) -- the last on most of that channel's elements, at the K of a 14 x 14 conv3 (256) and of a 3 x 3 layer (4608).
    ResNet-50 at 224 x 224, 4 images, bf16; the unperturbed outputs pass."""
    trunk = _trunk("resnet50", 224, 4, 1, dev, seed=4)
    plan = trunk._plan
    walk = Walk(trunk, 4, 224, "bf16")
    b = walk.b
    entries = {e[0].name: e for e in plan.conv_shapes(4, 224)}
    blocks = {blk["c1"].name.rsplit(".", 1)[0]: (blk, e) for blk, e in zip(plan.blocks, b["blocks"])}
    report = []
    for layer, tap in (("6.1.conv3", (0, 0)), ("7.1.conv2", (1, 1))):
        blk, e = blocks[layer.rsplit(".", 1)[0]]
        s, xi, yo, _H, _W, _kw, _macs, prev = entries[layer]
        coef = {p.name: _Coef(b, p) for p in (blk["c1"], blk["c2"])}
        A, dA, form = walk.operand(blk, s, prev, xi, None, coef)
        ref, E, K = walk.conv(s, A, dA, s.stride, s.pad)
        got = yo.double()
        bound = walk.bound(ref, E)
        nbad, ratio, _ = check_elements(got, ref, bound)
        assert nbad == 0, (layer, nbad, ratio)
        report.append(f"{layer} [{form}, K={K}]: real output passes (largest error {ratio:.3f} of the bound)")
        C = got.shape[3]
        flat, rflat, bflat = got.reshape(-1, C), ref.reshape(-1, C), bound.reshape(-1, C)
        # (1) a misplaced store: one element replaced by its neighbour 16 bytes (8 bf16 channels) along the row
        m0 = flat.shape[0] // 2
        c = int((flat[m0, :C - 8] - flat[m0, 8:]).abs().argmax())
        bad1 = flat.clone()
        bad1[m0, c] = flat[m0, c + 8]
        n1, _, first1 = check_elements(bad1, rflat, bflat)
        assert n1 == 1 and first1[0] == (m0, c), (layer, n1, first1)
        # (2) a tile seam: the output of one 128-row tile shifted by one row
        t0 = 128 * min(2, flat.shape[0] // 128 - 1)
        bad2 = flat.clone()
        bad2[t0:t0 + 128] = flat[t0 + 1:t0 + 129]
        n2, _, first2 = check_elements(bad2, rflat, bflat)
        assert n2 > 0.5 * 128 * C and first2[0][0] == t0, (layer, n2, first2)
        # (3) a missed LDS-DMA piece: 8 input channels of one tap dropped from the reference of one output channel
        co, c0 = 5, 24
        W2 = s.w.double()[co:co + 1].clone()
        W2[0, tap[0], tap[1], c0:c0 + 8] = 0
        c_acc = (K / 8 + 16) * U
        ref3 = _conv64(A, W2, s.stride, s.pad)
        E3 = _conv64(c_acc * A.abs() + (dA if dA is not None else 0), W2.abs(), s.stride, s.pad) * (1 + 2.0 ** -7)
        n3, _, _ = check_elements(got[..., co:co + 1], ref3, walk.bound(ref3, E3))
        frac = n3 / ref3.numel()
        assert frac > 0.5, (layer, frac)
        report.append(f"{layer}: misplaced store flagged ({n1} element), tile seam flagged ({n2} of {128 * C} elements), "
                      f"dropped operand piece flagged on {frac:.1%} of output channel {co}")
    print("\n" + "\n".join(report))
