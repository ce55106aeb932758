"""The inference-mode trunk, element by element and layer by layer, against fp64 formed from the operands the kernels consumed.

Eval mode runs every convolution through gic_conv2d without a statistics buffer (EPI_PLAIN: tile8<..,0,true,..> and the 4-wave
gemm<..,0,true,..> kernel; none of the specialised convolution kernels, tests/test_trunk_eval_cases.py) and every BatchNorm on the
running statistics (bn_coeffs' run_mean branch under gic_bn_act and gic_bn_relu_maxpool).  Nothing is fused, so every operand is a
stored tensor and every layer is checked on its own with the checker of tests/test_gpu_trunk_layers.py (its rounding model, bounds and
failure messages): `Walk.conv` / `Walk.bound` for the convolutions, `_form` / `check_interval` for what a BatchNorm pass stores.

What differs from the training walk is the coefficient model.  The kernel forms sc = gamma * rsqrtf(var + 1e-5f), sh = beta - mean * sc
in f32 from the running buffers; the reference forms them in fp64 from the same f32 values with dsc = 8 u |sc| (the sum under the root,
rsqrtf within 2 ulp, the product) and dsh = |mean| dsc + 3 u (|beta| + |mean sc|).  There is no statistics fold, so no dmean / dvar term.

Inputs (tests/trunk_eval_cases.py): parameters as Generator.init_params leaves them (negative gammas); the running statistics are the
batch statistics of one training pass over OTHER images, each channel's mean scaled by 1 + U(-0.3, 0.3) and its variance by a log-uniform
factor in [0.25, 4], and in every layer two channels with running_var = 0, two with 1e-6 and one with gamma = 0: a kernel that took the
batch statistics, dropped eps or mixed up the shortcut's pair with the main one is off by far more than any bound here
(test_checker_flags_what_an_eval_kernel_can_get_wrong).

test_every_eval_layer_element_wise        one eager eval pass per walk of EVAL_WALKS: every convolution output, every bn_act output, every
                                          block output (projection shortcuts with their own running pair), the stem's BatchNorm + ReLU +
                                          max-pool, the pooled feature; the state an eval pass must not touch; the route of every layer
test_plain_convolution                    every PLAIN_CONVS case alone, inside NaN guard rows (gic_conv2d's output is dense, ldc = Cout: there
                                          are no pad columns to guard)
test_eval_pass_*                          what an eval pass inherits and leaves: eager against replays, the deterministic mode, running
                                          statistics changed in place under a captured graph, eval after a training pass, the Encoder's API
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_encoder as OE
from tests import trunk_eval_cases as T
from tests.test_gpu_trunk_layers import EPS32, U, Walk, _Coef, _conv64, _form, _report, check_elements, check_interval

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _RunCoef:
    """Per-channel (scale, shift) of one BatchNorm in eval mode, in fp64 from the f32 running buffers, with bounds on the kernel's f32
    values (the interface of test_gpu_trunk_layers._Coef as _form reads it)."""

    def __init__(self, bn, mean=None, var=None, eps=EPS32):
        g, be = bn.weight.detach().double(), bn.bias.detach().double()
        mean = bn.running_mean.double() if mean is None else mean
        var = bn.running_var.double() if var is None else var
        self.sc = g * torch.rsqrt(var + eps)
        self.dsc = 8 * U * self.sc.abs()
        self.sh = be - mean * self.sc
        self.dsh = mean.abs() * self.dsc + 3 * U * (be.abs() + (mean * self.sc).abs())


class EvalWalk(Walk):
    """The walk of test_gpu_trunk_layers over an eval pass: every operand is a stored tensor of the plan's own buffers."""

    def __init__(self, trunk, N, S, mode):
        super().__init__(trunk, N, S, mode)
        self.coef = {s.name: _RunCoef(s.bn) for s in self.plan.steps}
        self.conditions = []             # what the inputs must meet for the walk to mean anything: finite, alive

    def stored(self, name, buf, t, alive=False):
        if not bool(torch.isfinite(t).all()):
            self.conditions.append(f"{name} {buf}: not finite")
        elif alive and float((t != 0).double().mean()) < 0.10:
            self.conditions.append(f"{name} {buf}: {float((t != 0).double().mean()):.1%} non-zero elements")

    def layer(self, s, x, y, buf, form="plain"):
        self.weights(s)
        pad = 0 if s is self.plan.stem else s.pad
        ref, E, K = self.conv(s, x.double(), None, s.stride, pad)
        self.stored(s.name, buf, y)
        self.elements(s, buf, y, ref, E, form, K, 0.0)

    def formed(self, s, y, got, buf, res=None, res_step=None, post=lambda t: t):
        cr = self.coef[res_step.name] if res_step is not None else None
        z, lo, hi = _form(y.double(), self.coef[s.name], self.rnd, None if res is None else res.double(), cr)
        self.stored(s.name, buf, got, alive=True)
        self.interval(s.name, buf, got, post(z), post(lo), post(hi))

    def run(self):
        plan, b = self.plan, self.b
        mp = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        self.layer(plan.stem, b["xin"], b["y0"], "y0", "stem")
        self.formed(plan.stem, b["y0"], b["x0"], "x0 (bn + relu + max-pool)", post=mp)
        x = b["x0"]
        for blk, e in zip(plan.blocks, b["blocks"]):
            c1, c2, c3, ds = blk["c1"], blk["c2"], blk["c3"], blk["ds"]
            self.layer(c1, x, e["y1"], "y1")
            self.formed(c1, e["y1"], e["z1"], "z1 (bn_act)")
            self.layer(c2, e["z1"], e["y2"], "y2")
            last, ylast = c2, e["y2"]
            if c3 is not None:
                self.formed(c2, e["y2"], e["z2"], "z2 (bn_act)")
                self.layer(c3, e["z2"], e["y3"], "y3")
                last, ylast = c3, e["y3"]
            if ds is not None:
                self.layer(ds, x, e["yd"], "yd")
                self.formed(last, ylast, e["out"], "block output (projection shortcut)", res=e["yd"], res_step=ds)
            else:
                self.formed(last, ylast, e["out"], "block output (identity shortcut)", res=x)
            x = e["out"]
        v = x.double()
        HW = v.shape[1] * v.shape[2]
        ref = v.mean((1, 2))
        bound = self.r * ref.abs() + (1 + self.r) * (HW + 2) * U * v.abs().mean((1, 2)) + 1e-30
        self.stored("avgpool", "feat", b["feat"])
        nbad, ratio, first = check_elements(b["feat"].double(), ref, bound)
        self.table.append(("avgpool", "pooled", "feat", HW, ratio, 0.0))
        if nbad:
            self.fail(f"pooled feature: {nbad} out of bound; first {first}")
        return self


def _load(trunk, tp):
    trunk.load_state_dict({k[len("encoder.resnet."):]: v for k, v in tp.items()}, strict=False)


def _install_running(trunk, dtype, train_images, seed):
    """One training pass over `train_images`, then the perturbed running statistics and gammas of trunk_eval_cases.eval_running, made
    from that pass's own batch statistics (the plan's f32 sums), written in place.  Leaves the trunk in eval mode."""
    trunk.train()
    trunk(train_images, dtype)
    torch.cuda.synchronize()
    plan = trunk._plan
    N, S = train_images.shape[0], train_images.shape[2]
    b = plan._bufs[plan._bkey(N, S)]
    batch, gamma = {}, {}
    for s in plan.steps:
        C, nrep, n = s.cout, b["nrep"][s.name], float(b["rows"][s.name])
        st = b["stats"][s.stats_off:s.stats_off + 2 * C * nrep].view(nrep, 2, C).double().sum(0)
        mean = st[0] / n
        batch[OE.bn_name(s.name)] = (mean.float().cpu(), (st[1] / n - mean * mean).clamp_min(0).float().cpu())
        gamma[OE.bn_name(s.name)] = s.bn.weight.detach().cpu()
    table = T.eval_running(batch, gamma, seed)
    with torch.no_grad():
        for s in plan.steps:
            rm, rv, ga = table[OE.bn_name(s.name)]
            s.bn.running_mean.copy_(rm)
            s.bn.running_var.copy_(rv)
            s.bn.weight.copy_(ga)
    plan.sync_counters()
    torch.cuda.synchronize()
    return trunk.eval()


def _eval_trunk(arch, S, N, dtype, dev, use_graph=False):
    """(trunk in eval mode with the walk's parameters and running statistics, the eval images on the device)"""
    from gan_image_captioning_amd import encoder_engine
    from gan_image_captioning_amd.trunk import ResNetTrunk
    tp, train_images, eval_images = T.walk_inputs(arch, S, N)
    trunk = ResNetTrunk(arch)
    _load(trunk, tp)
    trunk = trunk.to(dev)
    trunk._plan = encoder_engine.TrunkPlan(trunk, dtype)
    trunk._plan.use_graph = False
    _install_running(trunk, dtype, train_images.to(dev), seed=S + N)
    trunk._plan.use_graph = use_graph
    return trunk, eval_images.to(dev)


def _twin(trunk, dtype, dev):
    """A fresh trunk and plan (eager) holding a copy of `trunk`'s state."""
    from gan_image_captioning_amd import encoder_engine
    from gan_image_captioning_amd.trunk import ResNetTrunk
    twin = ResNetTrunk(trunk.arch)
    twin.load_state_dict(trunk.state_dict())
    twin = twin.to(dev).eval()
    twin._plan = encoder_engine.TrunkPlan(twin, dtype)
    twin._plan.use_graph = False
    return twin


def _state(plan, b):
    out = {"stats arena": b["stats"].clone()}
    for s in plan.steps:
        out[s.name + " running_mean"] = s.bn.running_mean.clone()
        out[s.name + " running_var"] = s.bn.running_var.clone()
        out[s.name + " num_batches_tracked"] = s.bn.num_batches_tracked.clone()
        out[s.name + " packed weights"] = s.w.clone()
        out[s.name + " gamma"], out[s.name + " beta"] = s.bn.weight.detach().clone(), s.bn.bias.detach().clone()
    return out


def _pass_tensors(b):
    """Every tensor one pass stores, by name."""
    out = {"y0": b["y0"], "x0": b["x0"], "feat": b["feat"]}
    for i, e in enumerate(b["blocks"]):
        out.update({f"block {i} {k}": v for k, v in e.items() if torch.is_tensor(v)})
    return out


def _routes_taken(plan, b, N):
    """layer name -> variant key, from gic_conv2d in route-only mode over the very arguments TrunkPlan._conv passes in eval mode."""
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    e_of = {}
    x = b["x0"]
    for blk, e in zip(plan.blocks, b["blocks"]):
        c1, c2, c3, ds = blk["c1"], blk["c2"], blk["c3"], blk["ds"]
        e_of[c1.name], e_of[c2.name] = (x, e["y1"]), (e["z1"], e["y2"])
        if c3 is not None:
            e_of[c3.name] = (e["z2"], e["y3"])
        if ds is not None:
            e_of[ds.name] = (x, e["yd"])
        x = e["out"]
    e_of[plan.stem.name] = (b["xin"], b["y0"])
    got = {}
    for s in plan.steps:
        xi, yo = e_of[s.name]
        stem = s is plan.stem
        with engine.route_only() as r:
            status = L.load().gic_conv2d(xi.data_ptr(), s.w.data_ptr(), yo.data_ptr(), None, plan._nrep[s.name], plan.dtype, N, xi.shape[1], xi.shape[2],
                                         4 if stem else s.cin, s.cout, s.k, 8 if stem else s.k, s.stride, 0 if stem else s.pad, engine.stream_ptr())
            line = r.last()
        assert status == 0, (s.name, line)
        got[s.name] = T.route_key(line)
    return got


@pytest.mark.parametrize("walk", T.EVAL_WALKS, ids=[w.id for w in T.EVAL_WALKS])
def test_every_eval_layer_element_wise(dev, walk):
    from gan_image_captioning_amd import engine
    arch, S, N, mode = walk.arch, walk.S, walk.N, walk.mode
    dtype = 0 if mode == "fp32" else 1
    engine.set_deterministic(T.MODES[mode][1])
    try:
        trunk, images = _eval_trunk(arch, S, N, dtype, dev)
        plan = trunk._plan
        b = plan._bufs[plan._bkey(N, S)]
        for t in _pass_tensors(b).values():
            t.fill_(float("nan"))                    # nothing of the training pass is left for the eval pass to be credited with
        before = _state(plan, b)
        feat = trunk(images, dtype)
        torch.cuda.synchronize()
        assert feat is b["feat"] and plan._bkey(N, S) == ((N, S, "det") if mode == "det" else (N, S))
        plan.sync_counters()
        after = _state(plan, b)
        changed = [k for k in before if not torch.equal(before[k].view(-1).view(torch.uint8), after[k].view(-1).view(torch.uint8))]
        assert not changed, f"an eval pass changed {changed[:8]}"
        # the recorded route of every layer is the one taken (no case is vacuous), and none is a statistics-epilogue kernel
        want, got = walk.key_of(), _routes_taken(plan, b, N)
        moved = {n: (want[n], got[n]) for n in want if want[n] != got[n]}
        assert not moved and len(got) == len(want), moved
        w = EvalWalk(trunk, N, S, "fp32" if mode == "fp32" else ("det" if mode == "det" else "bf16")).run()
    finally:
        engine.set_deterministic(False)
    _report(f"eval {walk.id}", w)
    assert not w.conditions, "\n".join(w.conditions[:20])
    assert not w.failures, "\n".join(w.failures[:40])
    forms = {(form, buf) for _, form, buf, _, _, _ in w.table}
    assert ("formed", "block output (projection shortcut)") in forms and ("formed", "block output (identity shortcut)") in forms


def test_checker_flags_what_an_eval_kernel_can_get_wrong(dev):
    """The eval check applied to perturbed references (or a perturbed copy of an output; no kernel is touched) flags what an eval-mode
    kernel can get wrong, while the real outputs pass: (1) the batch statistics of the arena used instead of the running ones, (2) eps
    dropped -- seen on every live channel with running_var = 0 or 1e-6, (3) the shortcut normalised with the main branch's running pair,
    (4) a 64-row tile written past row M = 49 (the guard rows of test_plain_convolution).  ResNet-50 at 224 x 224, one image, bf16."""
    arch, S, N = "resnet50", 224, 1
    trunk, images = _eval_trunk(arch, S, N, 1, dev)
    plan = trunk._plan
    trunk(images, 1)
    torch.cuda.synchronize()
    w = EvalWalk(trunk, N, S, "bf16")
    b, rnd = w.b, w.rnd
    report = []

    def flagged(got, z, lo, hi):
        bad = ~((got >= lo) & (got <= hi))
        return bad, float(bad[got != 0].double().mean())

    live0 = live6 = 0
    for bi in (0, 3, 13):                                      # the projection blocks of stages 4, 5 and 7 (56 x 56, 28 x 28, 7 x 7 outputs)
        blk, e = plan.blocks[bi], b["blocks"][bi]
        c1, c3, ds = blk["c1"], blk["c3"], blk["ds"]
        y1, z1, out = e["y1"].double(), e["z1"].double(), e["out"].double()
        # the real outputs pass
        z, lo, hi = _form(y1, w.coef[c1.name], rnd)
        assert check_interval(z1, z, lo, hi)[0] == 0, c1.name
        zo, loo, hio = _form(e["y3"].double(), w.coef[c3.name], rnd, e["yd"].double(), w.coef[ds.name])
        assert check_interval(out, zo, loo, hio)[0] == 0, c3.name
        # (1) batch statistics (the arena still holds the training pass's sums) instead of the running ones
        bad, frac1 = flagged(z1, *_form(y1, _Coef(b, c1), rnd))
        assert frac1 > 0.5, (c1.name, frac1)
        # (2) eps dropped: every live channel whose running variance is 0 or 1e-6 is flagged
        bad, frac2 = flagged(z1, *_form(y1, _RunCoef(c1.bn, eps=0.0), rnd))
        rv = c1.bn.running_var
        for value in (0.0, 1e-6):
            chans = (rv == value).nonzero().flatten().tolist()
            assert len(chans) == 2, (c1.name, value, chans)
            for ch in chans:
                if bool((z1[..., ch] != 0).any()):
                    live0, live6 = live0 + (value == 0.0), live6 + (value != 0.0)
                    assert bool(bad[..., ch].any()), (c1.name, ch, value)
        # (3) the shortcut normalised with the main branch's running pair
        bad, frac3 = flagged(out, *_form(e["y3"].double(), w.coef[c3.name], rnd, e["yd"].double(), w.coef[c3.name]))
        assert frac3 > 0.5, (c3.name, frac3)
        report.append(f"{c1.name} / {c3.name}: real outputs pass; of the non-zero elements, batch statistics flagged {frac1:.1%}, eps dropped "
                      f"{frac2:.1%}, the main pair on the shortcut {frac3:.1%}")
    assert live0 >= 1 and live6 >= 1, (live0, live6)             # (the eps check was not vacuous)
    # (4) a 64-row tile written past row M = 49: the guard rows see it
    case = next(c for c in T.PLAIN_CONVS if c.rows() == 49 and c.dtype == "bf16")
    got, buf, before, G0, M = _launch_plain(case, dev)[:5]
    assert _touched(buf, before, G0, M) == 0
    spill = buf.clone()
    spill[G0 + M:G0 + 64] = buf[G0 + M - 15:G0 + M]              # rows 49 .. 63 of the tile stored as well
    assert _touched(spill, before, G0, M) == 15 * case.cout
    report.append(f"{case.id}: guard rows untouched by the kernel; a tile stored to row 63 flagged on {15 * case.cout} guard elements")
    print("\n" + "\n".join(report))


# ---------------------------------------------------------------------------------------------- isolated plain convolutions
GUARD_FRONT, GUARD_BACK = 8, 136          # rows: behind the output there is room for a whole 128-row tile past the last row


def _launch_plain(case, dev):
    """-> (output [N, Ho, Wo, Cout] as stored, the whole guarded buffer, its image before the launch, guard rows in front, M, x, w)"""
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    act = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    dt = L.BF16 if case.dtype == "bf16" else L.F32
    g = torch.Generator().manual_seed(case.N + case.H + case.cin + case.cout + case.k)
    x = torch.randn(case.N, case.H, case.W, case.cin, generator=g).to(act).to(dev)
    w = (torch.randn(case.cout, case.k, case.kw, case.cin, generator=g) * 0.1).to(act).to(dev)
    M = case.rows()
    buf = torch.full((GUARD_FRONT + M + GUARD_BACK, case.cout), float("nan"), dtype=act, device=dev)
    before = buf.clone()
    out = buf[GUARD_FRONT:GUARD_FRONT + M]
    args = T.conv_args(case, case.N, dt, x.data_ptr(), w.data_ptr(), out.data_ptr(), engine.stream_ptr())
    with engine.route_only() as r:
        status = L.load().gic_conv2d(*args)
        line = r.last()
    assert status == 0 and T.route_key(line) == case.key, line
    L.check(L.load().gic_conv2d(*args), "gic_conv2d " + case.id)
    torch.cuda.synchronize()
    ho, wo = case.out_hw()
    return out.clone().view(case.N, ho, wo, case.cout), buf, before, GUARD_FRONT, M, x, w


def _touched(buf, before, G0, M):
    """Elements of the guard rows whose bits differ from the NaN pattern they were filled with."""
    it = BITS[buf.dtype]
    a, c = buf.view(it), before.view(it)
    return int((a[:G0] != c[:G0]).sum()) + int((a[G0 + M:] != c[G0 + M:]).sum())


@pytest.mark.parametrize("case", T.PLAIN_CONVS, ids=[c.id for c in T.PLAIN_CONVS])
def test_plain_convolution(dev, case):
    """gic_conv2d without statistics against the fp64 convolution of the rounded operands, with the walk's element bound
    r |ref| + (1 + r) E, E = (1 + 2^-7) c conv(|a|, |w|), c = (K / 8 + 16) u in bf16 and (K + 16) u in f32; the rows in front of
    row 0 and behind row M - 1 keep their NaN pattern."""
    got, buf, before, G0, M, x, w = _launch_plain(case, dev)
    K = case.k * case.kw * case.cin
    bf16 = case.dtype == "bf16"
    r = 2.0 ** -8 if bf16 else U
    c = ((K / 8 + 16) if bf16 else (K + 16)) * U
    ref = _conv64(x.double(), w.double(), case.stride, case.pad)
    E = _conv64(c * x.double().abs(), w.double().abs(), case.stride, case.pad) * (1 + 2.0 ** -7)
    assert ref.shape == got.shape
    nbad, ratio, first = check_elements(got.double(), ref, r * ref.abs() + (1 + r) * E + 1e-30)
    print(f"\n[plain conv] {case.id} {case.key} K={K} rows={M}: largest error / bound {ratio:.3g}")
    assert nbad == 0, f"{case.id}: {nbad} of {ref.numel()} elements out of bound; first (image, row, col, channel) {first}"
    touched = _touched(buf, before, G0, M)
    assert touched == 0, f"{case.id}: {touched} elements of the guard rows around the {M} output rows changed"


# ---------------------------------------------------------------------------------------------- what an eval pass inherits and leaves
STATE_CASES = [("resnet50", 224, 1), ("resnet18", 96, 2)]


def _eval_once(trunk, images, dtype):
    N, S = images.shape[0], images.shape[2]
    feat = trunk(images, dtype).clone()
    fmap = trunk._plan.last_map(N, S).clone()
    torch.cuda.synchronize()
    return feat, fmap


@pytest.mark.parametrize("arch,S,N", STATE_CASES, ids=[f"{a}-{s}-{n}" for a, s, n in STATE_CASES])
def test_eval_pass_eager_replays_deterministic_mode_and_running_statistics_in_place(dev, arch, S, N):
    """Eval has no atomics and no split-K (the selection splits bf16 -> f32 products only), so bit equality is the contract: the eager
    first call, the capturing second and the replaying third agree; the deterministic mode switches nothing; and running statistics
    changed in place between two replays are read through their pointers -- the replay equals a fresh plan's eager pass on the new values."""
    from gan_image_captioning_amd import engine
    trunk, images = _eval_trunk(arch, S, N, 1, dev, use_graph=True)
    plan = trunk._plan
    eager = _eval_once(trunk, images, 1)
    assert not plan._graphs
    first = _eval_once(trunk, images, 1)
    assert len(plan._graphs) == 1 and plan.use_graph, "the eval pass was not captured"
    second = _eval_once(trunk, images, 1)
    assert len(plan._graphs) == 1
    for what, other in (("first replay", first), ("second replay", second)):
        assert torch.equal(eager[0], other[0]) and torch.equal(eager[1], other[1]), f"{what} differs from the eager pass"
    assert bool(torch.isfinite(eager[1].float()).all()) and float((eager[1] != 0).float().mean()) >= 0.10
    # deterministic mode: its own buffer set, the same kernels, the same bits
    graph = next(iter(plan._graphs.values()))
    engine.set_deterministic(True)
    try:
        plan.use_graph = False
        det = _eval_once(trunk, images, 1)
        assert (N, S, "det") in plan._bufs
    finally:
        engine.set_deterministic(False)
        plan.use_graph = True
    assert torch.equal(eager[0], det[0]) and torch.equal(eager[1], det[1]), "deterministic mode changed an eval pass"
    # running statistics changed in place under the captured graph
    with torch.no_grad():
        for s in plan.steps:
            s.bn.running_mean.mul_(1.125).add_(0.01)
            s.bn.running_var.mul_(1.5).add_(1e-3)
    replay = _eval_once(trunk, images, 1)
    assert len(plan._graphs) == 1 and next(iter(plan._graphs.values())) is graph, "the pass was captured again"
    assert not torch.equal(replay[1], eager[1])
    fresh = _eval_once(_twin(trunk, 1, dev), images, 1)
    assert torch.equal(replay[0], fresh[0]) and torch.equal(replay[1], fresh[1]), "a replay did not read the running statistics in place"


# ... and 22 images: the smallest batch at 224 x 224 whose training pass leaves a conv3 output unstored (68 992 rows at 56 x 56: a multiple
# of 128 for gic_conv_b2b, and 539 row tiles x 2 for the statistics-only pass of conv1x1_stream, which starts at 1024 tiles)
AFTER_TRAINING = STATE_CASES + [("resnet50", 224, 22)]


@pytest.mark.parametrize("arch,S,N", AFTER_TRAINING, ids=[f"{a}-{s}-{n}" for a, s, n in AFTER_TRAINING])
def test_eval_pass_after_a_training_pass_at_the_same_shape(dev, arch, S, N):
    """A training pass leaves z1 / z2 unwritten where BatchNorm rode on load, conv3's output unwritten where conv_b2b recomputed it, and
    fused_in / b2b set on the plan.  With the running buffers restored, the eval pass that follows at the same (N, S) stores every
    tensor a fresh plan's eval pass stores, bit for bit."""
    trunk, images = _eval_trunk(arch, S, N, 1, dev)
    plan = trunk._plan
    twin = _twin(trunk, 1, dev)
    want_feat, want_map = _eval_once(twin, images, 1)
    want = {k: v.clone() for k, v in _pass_tensors(twin._plan._bufs[(N, S)]).items()}
    saved = {s.name: (s.bn.running_mean.clone(), s.bn.running_var.clone()) for s in plan.steps}
    for s in plan.steps:
        s.fused_in = None                                  # probe again: the training pass below decides the fused forms afresh
    plan.res_min_rows = 0                                  # (tuning switch of the plan) conv_b2b / residual on load wherever the kernels take the shape
    g = torch.Generator().manual_seed(N)
    trunk.train()
    trunk(torch.randn(N, 3, S, S, generator=g).to(dev), 1)
    torch.cuda.synchronize()
    assert any(s.fused_in is True for s in plan.steps), "the training pass fused nothing"
    if (arch, N) == ("resnet50", 22):
        assert plan.unstored_convs() == {"4.0.conv3", "4.1.conv3", "4.2.conv3"}, plan.unstored_convs()
    b = plan._bufs[(N, S)]
    for i, (blk, e) in enumerate(zip(plan.blocks, b["blocks"])):
        # what that pass left unwritten is poisoned: the eval pass has to write it, not inherit it
        for step, buf in ((blk["c2"], "z1"), (blk["c3"], "z2")):
            if step is not None and step.fused_in is True and buf in e:
                e[buf].fill_(float("nan"))
        if blk.get("b2b") is True:
            e["y3"].fill_(float("nan"))
            e["z2"].fill_(float("nan"))
    with torch.no_grad():
        for s in plan.steps:
            s.bn.running_mean.copy_(saved[s.name][0])
            s.bn.running_var.copy_(saved[s.name][1])
    trunk.eval()
    got_feat, got_map = _eval_once(trunk, images, 1)
    got = _pass_tensors(b)
    differ = [k for k in want if not torch.equal(want[k], got[k])]
    assert not differ, f"after a training pass the eval pass stores other bits in {differ[:8]}"
    assert torch.equal(got_feat, want_feat) and torch.equal(got_map, want_map)


@pytest.mark.parametrize("arch,S,N", STATE_CASES, ids=[f"{a}-{s}-{n}" for a, s, n in STATE_CASES])
def test_eval_pass_through_the_encoder(dev, arch, S, N):
    """Encoder.eval().forward_with_map(x): the map is the plan's last block output of an eval pass over x, the head was handed the plan's
    pooled feature, and a look-ahead pass announced for x in training mode is not used.  The head's product splits K over f32 atomics
    (bf16 -> f32), so the features are compared with head_fwd of the same pooled feature within twice the bound of a K-term f32 sum
    taken in any order; the eval-mode head itself is pinned by tests/aux_cases.py."""
    from gan_image_captioning_amd import encoder_engine
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Generator
    args = default_args(vocab_size=32, gen_embed_dim=16, gen_hidden_dim=32, conditional_gan=1, encoder_arch=arch, decoder="attention",
                        attn_dim=24, compute_dtype="bf16", image_size=S, device="cuda", log_file=None, model_dir=None, save_dir=None)
    enc = Generator(args).to(dev).encoder
    tp, train_images, x = T.walk_inputs(arch, S, N)
    _load(enc.resnet, tp)
    _install_running(enc.resnet, 1, train_images.to(dev), seed=S + N)
    a, x = train_images.to(dev), x.to(dev)
    with torch.no_grad():
        enc.train().forward_with_map(a, next_images=x)           # announces x: a training-mode look-ahead pass with its map
        assert enc._pre is not None and enc._pre[0] is x and enc._pre[1] is True and enc._pre[4] is not None
        train_map = enc._pre[4]
        fe, me = enc.eval().forward_with_map(x)
        torch.cuda.synchronize()
    assert enc._pre is None
    plan = enc.resnet._plan
    b = plan._bufs[(N, S)]
    C = b["feat"].shape[1]
    assert torch.equal(me, plan.last_map(N, S).view(N, -1, C)) and not torch.equal(me, train_map.view(N, -1, C))
    assert torch.equal(enc.last_trunk, b["feat"])
    # ... and that pass was an eval pass on the running statistics as they are now (the two training passes above moved them)
    twin = _twin(enc.resnet, 1, dev)
    want_feat, want_map = _eval_once(twin, x, 1)
    assert torch.equal(me, want_map.view(N, -1, C)) and torch.equal(b["feat"], want_feat)
    ref, _ = encoder_engine.head_fwd(1, b["feat"], enc.linear.weight.detach(), enc.linear.bias.detach(), enc.bn.weight.detach(), enc.bn.bias.detach(),
                                     enc.bn.running_mean, enc.bn.running_var, False, enc.bn.momentum, enc.bn.eps)
    torch.cuda.synchronize()
    f64, w64 = b["feat"].double(), enc.linear.weight.detach().bfloat16().double()
    scale = (enc.bn.weight.detach().double() * torch.rsqrt(enc.bn.running_var.double() + enc.bn.eps)).abs()
    bound = 2 * (C + 16) * U * (f64.abs() @ w64.abs().t() + enc.linear.bias.detach().double().abs()) * scale + 1e-30
    nbad, ratio, first = check_elements(fe.detach().double(), ref.double(), bound)
    print(f"\n[encoder eval] {arch}@{S}x{N}: features against head_fwd of the plan's pooled feature, largest difference / bound {ratio:.3g}")
    assert nbad == 0, first
