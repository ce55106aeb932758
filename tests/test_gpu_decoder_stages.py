"""Every kernel of the LSTM caption decoder (csrc/decoder_step.hip, csrc/decoder.hip), step by step and element by element against the
fp64 references and derived bounds of tests/decoder_cases.py.  Every intermediate buffer is caller-owned (DecoderEngine.sample_fwd(
state=, out=, ids=), .sample_bwd(ws=, grads=, phases=7)), read back after the call and checked against a reference formed from the
buffers upstream of it, so a flipped token or a rounding upstream excuses nothing downstream: bf16 is checked as tightly as f32.

Buffers carry sentinel guard rows before and after (their bits must not change); what a kernel has to overwrite holds NaN beforehand,
the input-gradient buffers `dxh` a sentinel that a route must leave wherever it does not write.  Slot L of layer 0's x columns belongs
to no step (the generic route writes the last token's row there, the fused route nothing): not checked.

CALIBRATION (MI355X; recorded, never asserted against; the module prints the measurements again after every run under -s).  The
largest error measured in the exact regimes of tests/decoder_cases.py, in the units of its docstring; its constants are 4 x these:
  tanhf (the cell, both modes)            1.212 u |ref|
  sigmoid on expf (the cell, both modes)  1.878 u |ref|
  __logf in g(u) (bf16 mode)              1.352 of the gumbel bound with K = 1          (logf, f32 mode: 1.352 too)
  __expf (bf16 mode)                      0.622 of u (1 + |x|) exp(x) + u (1 + e)       (expf, f32 mode: 0.615)
Both logarithms are driven by u = 2^-31 (a = u + eps = 5.7e-10, l1 = -21.3, g = -3.058380, device -3.0583792): an error of 6.9 u
against a unit of 5.1 u, which is what two logarithms that are each one ulp off give (an ulp of l1 is 32 u, of g 4 u).  This is why
logf and expf "at 1 ulp" are K_LIBM = 2 in units of u |ref| and not 1: with it the f32 figure is 0.77 of its bound.  part_s cannot be
had without the sum 1 + e; its rounding is in the unit's denominator, so the exp figures are the intrinsic's share at most.

Largest err / bound seen per stage and route (MI355X; f32 mode / bf16 mode; the bounds are NOT tightened to these):
                      fused            generic          fused, det       generic, det
  wcat, wcat_t, wout, bsum, slot0, xrows, h copies, key, ids, dxh keep, d_features: exact on every route
  gates               0.154 / 0.176    0.149 / 0.152
  c                   0.551 / 0.587    0.539 / 0.507
  h                   0.355 / 0.995    0.371 / 0.988
  part_m              0.160 / 0.099
  part_s              0.042 / 0.031
  out                 0.110 / 0.984    0.152 / 0.984
  dlogits             0.264 / 0.994    0.398 / 0.994    0.264 / 0.994    0.398 / 0.994
  dhout               0.272 / 0.106    0.246 / 0.111    0.195 / 0.106    0.246 / 0.111
  d_w_out             0.401 / 0.225    0.002 / 0.000    0.083 / 0.008    0.002 / 0.000
  d_b_out             0.299 / 0.102    0.000 / 0.000    0.065 / 0.001    0.000 / 0.000
  dgates              0.299 / 0.996    0.226 / 0.991    0.204 / 0.979    0.226 / 0.991
  dc                  0.062 / 0.047    0.103 / 0.083    0.028 / 0.035    0.103 / 0.083
  dxh                 0.129 / 0.045    0.103 / 0.044    0.063 / 0.025    0.103 / 0.044
  d_w_ih              0.346 / 0.193    0.002 / 0.001    0.192 / 0.103    0.002 / 0.001
  d_w_hh              0.263 / 0.204    0.003 / 0.000    0.143 / 0.076    0.003 / 0.000
  d_b_ih, d_b_hh      0.238 / 0.024    0.000 / 0.000    0.134 / 0.001    0.000 / 0.000
  d_b_ih == d_b_hh    not checked      not checked      exact            exact
  d_embed             0.116 / 0.109    0.002 / 0.003    0.047 / 0.098    0.002 / 0.004
(bf16 outputs: r dominates the bound, half a bf16 ulp is up to 2^-8 |ref|, so a correctly rounded result reaches ~1: h, out, dlogits,
dgates.  The generic backward runs at B = 516 only, where sums over 1032 rows leave their bound far away.  The fused bf16 `out` of
tails-bf16 reaches 0.884 of its 2 r: 1.77 of the issue's figure, see below.)  The two bias gradients of a layer are one column sum
stored twice by atomics of their own (colsum, three or more block rows): each is held to the sum bound on every route, and they are
bit-equal, and checked for it, in deterministic mode only.
One derivation had to be revisited: the issue's r = 2 * 2^-9 |ref| for the twice-rounded bf16 `out` of the fused route assumes half an
ulp is 2^-9 |ref|; that holds at the top of a binade only, at its bottom it is 2^-8 |ref| (the convention everywhere else here), so
two roundings are 2 * 2^-8 |ref|."""
import math

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests import decoder_cases as D
from tests.decoder_cases import CASES, TD, U
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

DT = {"f32": L.F32, "bf16": L.BF16}
NAN = float("nan")
MAXIMA = {}          # (stage, route, dtype) -> largest err / bound: recorded, never asserted against
CAL = {}             # (intrinsic, dtype) -> largest measured error in its unit


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(CAL):
        print(f"\n[decoder stages] calibration {key[0]:<10} {key[1]:<5} largest error {CAL[key]:.3f} (constant: 4 x)", end="")
    routes = ("fused", "generic", "fused det", "generic det")
    print("\n[decoder stages] largest err/bound, f32 / bf16:  " + "   ".join(routes), end="")
    for stage in D.ORDER:
        cell = lambda r, d: f"{MAXIMA[(stage, r, d)]:.3f}" if (stage, r, d) in MAXIMA else "-"
        if any(k[0] == stage for k in MAXIMA):
            print(f"\n[decoder stages]   {stage:<18}" + "   ".join(f"{cell(r, 'f32')} / {cell(r, 'bf16')}" for r in routes), end="")
    print()


class gpu_call:
    """A GPU fault (not a wrong result) ends the module's run: nothing more is launched on a device that has faulted."""

    def __enter__(self):
        return self

    def __exit__(self, kind, exc, tb):
        if exc is not None and isinstance(exc, RuntimeError) and ("HIP error" in str(exc) or "illegal memory access" in str(exc)):
            pytest.exit(f"GPU fault: {exc}", returncode=3)
        return False


def gbuf(shape, dtype, dev, fill):
    """A Guarded buffer of `shape` (guard rows of the last dimension's length)."""
    g = Guarded(math.prod(shape[:-1]), shape[-1], dtype, dev, fill)
    g.view = g.live.view(shape)
    return g


def alloc_state(case, dev, ids_only=False):
    c, td, f32 = case, TD[case.dtype], torch.float32
    g = {"xh": [gbuf((c.L + 1, c.B, c.ldx(l)), td, dev, NAN) for l in range(c.NL)],
         "gates": [gbuf((c.L, c.B, 4 * c.H), f32, dev, NAN) for _ in range(c.NL)],
         "c": [gbuf((c.L + 1, c.B, c.H), f32, dev, NAN) for _ in range(c.NL)],
         "hout": None if ids_only else gbuf((c.B, c.L, c.H), td, dev, NAN),
         "logits": gbuf((c.B, c.V), f32, dev, NAN), "gpre": gbuf((c.B, 4 * c.H), f32, dev, NAN),
         "part": gbuf((1, 2 * c.L * c.B * c.nblk + 2 * c.L * c.B + 4), f32, dev, NAN) if c.part else None,
         "out": gbuf((c.B, c.L, c.V), td, dev, NAN), "ids": gbuf((c.B, c.L), torch.int64, dev, -7)}
    return g


def each(g):
    for name, v in g.items():
        for i, b in enumerate(v if isinstance(v, list) else [v]):
            if b is not None:
                yield f"{name}[{i}]" if isinstance(v, list) else name, b


def assert_guards(case, *groups):
    for g in groups:
        for name, b in each(g):
            assert b.guards_intact(), f"{case.id}: the guard rows of {name} changed"


def views(g):
    return {k: ([b.view for b in v] if isinstance(v, list) else (None if v is None else v.view)) for k, v in g.items()}


def forward(eng, case, params, X, g, dev, ids_only=False):
    v = views(g)
    st = {k: v[k] for k in ("xh", "gates", "c", "hout", "logits", "gpre")}
    st["part"] = v["part"].view(-1) if v["part"] is not None else None
    to = lambda t: None if t is None else t.to(dev)
    with gpu_call():
        eng.sample_fwd(params, X["features"].to(dev), case.L, X["T"], case.pretrain, noise_u=X["u"].to(dev), state=st, out=v["out"], ids=v["ids"],
                       states=(to(X["h0"]), to(X["c0"])) if X["h0"] is not None else None, force_ids=to(X["force_ids"]),
                       force_len=to(X["force_len"]), ids_only=ids_only)
        torch.cuda.synchronize()
    return st


def state_cpu(case, g):
    """The state read back in new_state's layout (`part` split into its planes and the decoded keys)."""
    v = views(g)
    st = {k: [t.cpu() for t in v[k]] for k in ("xh", "gates", "c")}
    st.update(hout=v["hout"].cpu() if v["hout"] is not None else None, out=v["out"].cpu(), ids=v["ids"].cpu(), part_m=None, part_s=None, key=None)
    if D.select(case)["fwd"] == "fused":
        st["part_m"], st["part_s"], st["key"], st["key_val"] = D.split_part(case, v["part"].view(-1).cpu())
    return st


def shadow_cpu(eng):
    sh = eng._shadow
    return {"wcat": [t.cpu() for t in sh["wcat"]], "wcat_t": [t.cpu() for t in sh["wcat_t"]], "bsum": [t.cpu() for t in sh["bsum"]],
            "wout": sh["wout"].cpu() if sh["wout"] is not None else None}


def alloc_bwd(case, P, dev):
    c, td, f32 = case, TD[case.dtype], torch.float32
    ws = {"dlogits": gbuf((c.B, c.L, c.V), td, dev, NAN), "dhout": gbuf((c.B, c.L, c.H), f32, dev, NAN),
          "dgates": [gbuf((c.L, c.B, 4 * c.H), td, dev, NAN) for _ in range(c.NL)],
          "dxh": [gbuf((c.L + 1, c.B, c.ldx(l)), f32, dev, D.DXH_FILL) for l in range(c.NL)],
          "dc": [gbuf((c.B, c.H), f32, dev, NAN) for _ in range(c.NL)]}
    grads = {"grads": [gbuf(tuple(p.shape) if p.dim() > 1 else (1, p.shape[0]), f32, dev, NAN) for p in P] + [gbuf((c.B, c.E), f32, dev, NAN)]}
    return ws, grads


def backward(E, eng, case, params, P, X, g, dev, det=False):
    ws, gr = alloc_bwd(case, P, dev)
    v = views(g)
    st = {k: v[k] for k in ("xh", "gates", "c", "hout", "logits", "gpre")}
    st["part"] = v["part"].view(-1) if v["part"] is not None else None
    grads = [b.view.view(p.shape) for b, p in zip(gr["grads"], P)] + [gr["grads"][-1].view]
    E.set_deterministic(det)
    try:
        with gpu_call():
            eng.sample_bwd(params, st, v["out"], v["ids"], X["d_out"].to(dev), X["T"], case.pretrain, ws=views(ws), grads=grads, phases=7)
            torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)
    assert_guards(case, ws, gr, g)
    w = views(ws)
    return {k: ([t.cpu() for t in w[k]] if isinstance(w[k], list) else w[k].cpu()) for k in w}, [t.cpu() for t in grads]


def note(case, rep, tag=""):
    s = D.select(case)
    for stage, ratio in rep.ratio.items():
        route = s["fwd"] if D.ORDER.index(stage) <= D.ORDER.index("out") else s["bwd"]
        key = (stage, route + (tag if tag == " det" else ""), case.dtype)
        MAXIMA[key] = max(MAXIMA.get(key, 0.0), ratio)
    print(f"[decoder stages] {case.id}{tag}: " + "  ".join(f"{s} {r:.3f}" for s, r in rep.ratio.items() if r > 0))
    assert not rep.failed, f"{case.id}{tag}: {rep.failed}"


def make_engine(E, case):
    return E.DecoderEngine(case.V, case.E, case.H, case.NL, DT[case.dtype])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_stage(E, dev, case):
    """Forward and backward (phases = 7) of one case, every stage; the ids-only roll-out gives the same ids and leaves the buffers it
    does not own alone; the cases marked det run the backward once more in deterministic mode."""
    P, X = D.data(case)
    eng = make_engine(E, case)
    params = [p.to(dev) for p in P]
    g = alloc_state(case, dev)
    forward(eng, case, params, X, g, dev)
    assert_guards(case, g)
    img = shadow_cpu(eng)
    rep = D.Report()
    D.check_images(case, P, img, rep)
    if img["wout"] is None:
        img["wout"] = P[-2]
    st = state_cpu(case, g)
    near = []
    D.run_forward(case, P, img, X, st, rep, near=near)
    fused = D.select(case)["fwd"] == "fused"
    if fused:      # the key's value is the largest tile maximum, bit for bit
        assert torch.equal(st["key_val"].view(torch.int32), st["part_m"].max(2).values.view(torch.int32)), "rowkey value != max part_m"
    w, grads = backward(E, eng, case, params, P, X, g, dev)
    D.run_backward(case, P, img, X, st, w, grads, rep)
    assert set(rep.ratio) >= {"gates", "c", "h", "h copies", "ids", "out", "dhout", "dgates", "dc", "dxh", "dxh keep", "d_w_ih", "d_w_hh", "d_b_ih",
                              "d_features", "d_embed"} | ({"part_m", "part_s", "key"} if fused else set()) | (set() if case.pretrain else {"dlogits"})
    note(case, rep)
    # the ids-only roll-out: the same tokens; gates are not its to write
    g2 = alloc_state(case, dev, ids_only=True)
    forward(eng, case, params, X, g2, dev, ids_only=True)
    assert_guards(case, g2)
    ids2 = g2["ids"].view.cpu()
    same = ids2 == st["ids"]
    if near[0][0] == 0:
        assert same.all(), f"{case.id}: the ids-only roll-out chose other tokens"
    else:          # rows without a clear margin may resolve differently (and every later token of such a caption with them)
        assert int((~same.all(1)).sum()) <= near[0][0]
        print(f"[decoder stages] {case.id}: {near[0][0]} of {near[0][1]} rows without a clear margin: the ids-only tokens are compared by count")
    # gates and out are never an ids-only roll-out's to write; nor is the other route's scratch (hout is not passed: whoever passes it owns it)
    theirs = g2["gates"] + [g2["out"]] + ([g2["logits"], g2["gpre"]] if fused else [g2["part"]] if g2["part"] is not None else [])
    for b in theirs:
        assert bool(torch.isnan(b.view).all()), f"{case.id}: the ids-only roll-out wrote gates / out / the other route's scratch"
    if case.det:
        wd, gd = backward(E, eng, case, params, P, X, g, dev, det=True)
        repd = D.Report()
        D.run_backward(case, P, img, X, st, wd, gd, repd, det=True)
        assert {"d_embed", "d_b_ih == d_b_hh"} <= set(repd.ratio)
        note(case, repd, tag=" det")


@pytest.mark.parametrize("part", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_first_maximal_index_wins_a_tie(E, dev, dtype, part):
    """pretrain mode, w_out = 0, integer biases: y is the bias exactly; equal maxima either side of a quad, two lane groups, two 16-entry
    sub-tiles, two 64-entry tiles (the rowkey atomicMax) and into / inside the partial last tile: the first index, bit-exact logits."""
    case = D.TIES[(dtype, part)]
    eng = make_engine(E, case)
    for pair in D.TIE_PAIRS:
        gen = torch.Generator().manual_seed(D.SEED)
        P, X = D.tie_params(case, gen, pair), D.make_inputs(case, gen)
        g = alloc_state(case, dev)
        forward(eng, case, [p.to(dev) for p in P], X, g, dev)
        assert_guards(case, g)
        img = shadow_cpu(eng)
        if img["wout"] is None:
            img["wout"] = P[-2]
        st = state_cpu(case, g)
        rep = D.Report()
        D.run_forward(case, P, img, X, st, rep, exact=True)
        assert (st["ids"] == pair[0]).all(), (pair, st["ids"])
        note(case, rep, tag=f" {pair}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_calibrate_the_cell_intrinsics(E, dev, dtype):
    """tanhf and the sigmoid on expf in the exact regime (exact_cell): step 0's pre-activation is exact, the saved gates carry the
    intrinsic's error alone.  Recorded in units of u |ref|."""
    case = D.CAL_CELL[dtype]
    P, X = D.exact_cell(case, torch.Generator().manual_seed(D.SEED))
    eng = make_engine(E, case)
    g = alloc_state(case, dev)
    forward(eng, case, [p.to(dev) for p in P], X, g, dev)
    assert_guards(case, g)
    st, img, H = state_cpu(case, g), D.images(case, P), case.H
    a = st["xh"][0][0].double()
    assert torch.equal(a, torch.cat([X["features"], X["h0"][0]], 1).double())
    pre = a @ img["wcat"][0].double().t() + img["bsum"][0].double()
    assert torch.equal(pre.float().double(), pre) and float(pre.abs().max()) > 4
    ref = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])], 1)
    rel = (st["gates"][0][0].double() - ref).abs() / (U * ref.abs()).clamp_min(1e-300)
    rel = torch.where(ref == 0, torch.zeros_like(rel), rel)
    CAL[("tanhf", dtype)] = float(rel[:, 2 * H:3 * H].max())
    CAL[("sigmoid", dtype)] = float(torch.cat([rel[:, :2 * H], rel[:, 3 * H:]], 1).max())
    print(f"[decoder stages] calibration {dtype}: tanhf {CAL[('tanhf', dtype)]:.3f} u |ref|, sigmoid {CAL[('sigmoid', dtype)]:.3f} u |ref|")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_calibrate_the_gumbel_intrinsics(E, dev, dtype):
    """logf / __logf and expf / __expf in the exact regime (exact_gumbel): part_m is the device's g(u) itself, part_s = 1 + exp(x) with x
    known exactly.  Recorded in units of the gumbel bound with K = 1 (the roundings of a = u + eps and of a2 are in that unit) and of
    u (1 + |x|) exp(x) + u (1 + e), the second term being the rounding of the sum 1 + e that part_s cannot be had without."""
    case = D.CAL_GUMBEL[dtype]
    P, X, ia, ib, k = D.exact_gumbel(case, torch.Generator().manual_seed(D.SEED))
    eng = make_engine(E, case)
    g = alloc_state(case, dev)
    forward(eng, case, [p.to(dev) for p in P], X, g, dev)
    assert_guards(case, g)
    st = state_cpu(case, g)
    ua = X["u"][:, :, ia]
    gref, unit = D.gumbel(ua, 1.0)
    m = st["part_m"]
    rl = (m.double() - gref).abs() / unit
    CAL[("log", dtype)] = float(rl.max())
    x = ((m - k) - m).double()                                # both differences in f32, as the kernel forms them
    e = torch.exp(x)
    re = (st["part_s"].double() - (1 + e)).abs() / (U * (1 + x.abs()) * e + U * (1 + e))
    CAL[("exp", dtype)] = float(re.max())
    i, j = int(rl.argmax()), int(re.argmax())
    print(f"[decoder stages] calibration {dtype}: log driven by u = {float(ua.reshape(-1)[i])!r} (g = {float(gref.reshape(-1)[i]):.6f}, device "
          f"{float(m.reshape(-1)[i])!r}, unit {float(unit.reshape(-1)[i]) / U:.3f} u); exp by x = {float(x.reshape(-1)[j])!r}")
    print(f"[decoder stages] calibration {dtype}: log {CAL[('log', dtype)]:.3f}, exp {CAL[('exp', dtype)]:.3f}")
