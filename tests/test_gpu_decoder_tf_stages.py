"""The LSTM decoder's teacher-forced path (csrc/teacher_forced.hip: gic_decoder_forward_tf / _ss / _tf_bwd and their dropout forms) on the
GPU, stage by stage and element by element against the fp64 references and derived bounds of tests/decoder_tf_cases.py.  Every buffer
is caller-owned (DecoderEngine.forward_tf / forward_scheduled(state=, buffers=), forward_tf_bwd(ws=, grads=)), wrapped in
tests.gpu_util.Guarded (sentinel guard rows before and after whose bits must not change), holds NaN beforehand where a kernel has to
overwrite it (-7 in the integer buffers, DXH_FILL in `dxh`), is read back after the call and handed to the checker.  No (row, step),
pick or element is excluded from any check.  The backward must leave every byte of the forward's state as it was.

MEASURED (MI355X; recorded, never asserted against; the module prints the table again after every run under -s).
No constant had to be calibrated: every bound is a rule of tests/decoder_cases.py with its constants as they stand.
Largest err / bound seen per stage (f32 mode / bf16 mode; the bounds are NOT tightened to these).  The forward stages are one column
(the forward has one route per case); the backward stages are listed by the BPTT route, plain and in deterministic mode:
                      forward          fused            generic          fused, det       generic, det
  slot0, xrows, pad gates, pad state, h copies, hout, hdrop, replaced, pick, inputs, ss tail, h_n, c_n, untouched: exact everywhere
  gates               0.125 / 0.094
  c                   0.520 / 0.541
  h                   0.411 / 0.995
  logits              0.105 / 0.059
  y                   0.576 / 0.576
  out                 0.105 / 0.994
  dlogits                              0.141 / 0.992    0.135 / 0.984    0.097 / 0.970    0.135 / 0.984
  dhout                                0.078 / 0.037    0.069 / 0.038    0.059 / 0.024    0.069 / 0.019
  d_w_out                              0.296 / 0.147    0.187 / 0.055    0.090 / 0.043    0.150 / 0.055
  d_b_out                              0.155 / 0.014    0.062 / 0.000    0.047 / 0.000    0.055 / 0.000
  dgates                               0.261 / 0.992    0.166 / 0.981    0.177 / 0.970    0.105 / 0.967
  dc                                   0.187 / 0.235    0.024 / 0.022    0.020 / 0.012    0.017 / 0.015
  dxh                                  0.058 / 0.026    0.052 / 0.016    0.025 / 0.007    0.045 / 0.009
  d_w_ih                               0.270 / 0.146    0.157 / 0.065    0.084 / 0.063    0.150 / 0.058
  d_w_hh                               0.213 / 0.131    0.162 / 0.076    0.088 / 0.038    0.153 / 0.059
  d_b_ih, d_b_hh                       0.155 / 0.044    0.097 / 0.000    0.053 / 0.001    0.084 / 0.000
  d_b_ih == d_b_hh                     not checked      not checked      exact            exact
  dxh keep, d_features                 exact            exact            exact            exact
  d_embed                              0.081 / 0.083    0.065 / 0.060    0.029 / 0.021    0.000 / 0.000
(bf16 outputs: r dominates the bound and a correctly rounded result reaches ~1: h, out, dlogits, dgates.  `y` is f32 in both modes -- the
epilogue calls logf in both -- hence the same figure twice: the Gumbel value of a uniform close to 1.  `out` in bf16 stays below one r: the
epilogue rounds once.  The whole module, 102 runs, takes about 5 s.)  Every stage held in every case and mode: no kernel of the path had
to be changed and no derivation revisited."""
import math

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests import decoder_tf_cases as F
from tests.decoder_tf_cases import ORDER, RUNS, TD
from tests.gemm_cases import route_key
from tests.test_gpu_decoder_stages import assert_guards, gbuf, gpu_call, views

pytestmark = pytest.mark.gpu

DT = {"f32": L.F32, "bf16": L.BF16}
NAN = float("nan")
MAXIMA = {}          # (stage, column, dtype) -> largest err / bound: recorded, never asserted against
COLUMNS = ("forward", "fused", "generic", "fused det", "generic det")


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
    print("\n[decoder tf stages] largest err/bound, f32 / bf16:  " + "   ".join(COLUMNS), end="")
    for stage in ORDER:
        cell = lambda r, d: f"{MAXIMA[(stage, r, d)]:.3f}" if (stage, r, d) in MAXIMA else "-"
        if any(k[0] == stage for k in MAXIMA):
            print(f"\n[decoder tf stages]   {stage:<18}" + "   ".join(f"{cell(r, 'f32')} / {cell(r, 'bf16')}" for r in COLUMNS), end="")
    print()


def ibuf(shape, dtype, dev):
    """An integer buffer of -7; guarded unless it has no element (a caption length of 0)."""
    if math.prod(shape) == 0:
        class Bare:
            view = torch.empty(shape, dtype=dtype, device=dev)
            guards_intact = staticmethod(lambda: True)
        return Bare
    return gbuf(shape, dtype, dev, -7)


def alloc_forward(case, mode, dev):
    c, td, f32 = case, TD[case.dtype], torch.float32
    rows = c.B * c.Tmax
    ws_floats = (rows * c.V + 3) // 4 * 4                 # gic_decoder_forward_ss_ws_bytes: the f32 logits, whole 16 bytes
    return {"xh": [gbuf((c.T + 1, c.B, c.ldx(l)), td, dev, NAN) for l in range(c.NL)],
            "gates": [gbuf((c.T, c.B, 4 * c.H), f32, dev, NAN) for _ in range(c.NL)],
            "c": [gbuf((c.T + 1, c.B, c.H), f32, dev, NAN) for _ in range(c.NL)],
            "hout": gbuf((c.B * c.T, c.H), td, dev, NAN), "logits": gbuf((c.B, c.V), f32, dev, NAN), "gpre": gbuf((c.B, 4 * c.H), f32, dev, NAN),
            "ws": gbuf((1, ws_floats), f32, dev, NAN), "ids_ws": gbuf((1, rows), torch.int64, dev, -7),
            "out": gbuf((c.B, c.Tmax, c.V), td, dev, NAN), "h_n": gbuf((c.NL, c.B, c.H), f32, dev, NAN), "c_n": gbuf((c.NL, c.B, c.H), f32, dev, NAN),
            "hdrop": gbuf((c.B, c.Tmax, c.H), td, dev, NAN) if mode.drop else None,
            "inputs": ibuf((c.B, c.Lc), torch.int64, dev) if mode.ss else None, "replaced": ibuf((c.B, c.Lc), torch.int32, dev) if mode.ss else None}


def forward(eng, case, mode, params, X, g, dev, own=True):
    """The mode's forward call over the buffers of `g` (own False: over the engine's own allocations); what it returns."""
    c, v = case, views(g)
    st = bufs = None
    if own:
        st = {k: v[k] for k in ("xh", "gates", "c", "logits", "gpre")}
        st.update(hout=v["hout"].view(-1), part=None)
        bufs = {k: v[k] for k in ("out", "h_n", "c_n", "hdrop", "inputs", "replaced")}
        bufs["ws"] = v["ws"].view(-1) if mode.ss else (v["ws"].view(-1)[:c.B * c.Tmax * c.V].view(c.B * c.Tmax, c.V), v["ids_ws"].view(-1))
    drop = dict(dropout=mode.drop, dropout_seed=F.DROP_SEED, keep_u=None if mode.philox or not mode.drop else X["keep_u"].to(dev))
    feats, caps, lens = X["features"].to(dev), X["caps"].to(dev), [int(n) for n in X["lengths"]]
    with gpu_call():
        if mode.ss:
            res = eng.forward_scheduled(params, feats, caps, lens, mode.ss[0], mode.ss[1], coin_u=X["coin_u"].to(dev), noise_u=X["ss_noise"].to(dev),
                                        state=st, buffers=bufs, **drop)
        else:
            res = eng.forward_tf(params, feats, caps, lens, X["T"], mode.pretrain, noise_u=None if mode.philox else X["u"].to(dev),
                                 seed=F.PHILOX_SEED, keep_state=True, state=st, buffers=bufs, **drop)
        torch.cuda.synchronize()
    return res


def state_cpu(case, mode, g):
    """The buffers read back in decoder_tf_cases.new_state's layout."""
    c, v = case, views(g)
    st = {k: [t.cpu() for t in v[k]] for k in ("xh", "gates", "c")}
    st.update(hout=v["hout"].view(-1).cpu(), logits_ws=v["ws"].view(-1)[:c.B * c.Tmax * c.V].view(c.B * c.Tmax, c.V).cpu(),
              out=v["out"].cpu(), h_n=v["h_n"].cpu(), c_n=v["c_n"].cpu())
    for k in ("hdrop", "inputs", "replaced"):
        st[k] = v[k].cpu() if v[k] is not None else None
    return st


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def alloc_backward(case, P, dev):
    c, td, f32 = case, TD[case.dtype], torch.float32
    ws = {"dlogits": gbuf((c.B, c.Tmax, c.V), td, dev, NAN), "dhout": gbuf((c.B, c.Tmax, c.H), f32, dev, NAN),
          "dgates": [gbuf((c.Tmax, c.B, 4 * c.H), td, dev, NAN) for _ in range(c.NL)],
          "dxh": [gbuf((c.Tmax + 1, c.B, c.ldx(l)), f32, dev, F.DXH_FILL) for l in range(c.NL)],
          "dc": [gbuf((c.B, c.H), f32, dev, NAN) for _ in range(c.NL)]}
    grads = {"grads": [gbuf(tuple(p.shape) if p.dim() > 1 else (1, p.shape[0]), f32, dev, NAN) for p in P] + [gbuf((c.B, c.E), f32, dev, NAN)]}
    return ws, grads


def shadow_cpu(eng, P):
    sh = eng._shadow
    return {"wcat": [t.cpu() for t in sh["wcat"]], "wcat_t": [t.cpu() for t in sh["wcat_t"]], "bsum": [t.cpu() for t in sh["bsum"]],
            "wout": sh["wout"].cpu() if sh["wout"] is not None else P[-2]}


def note(case, mode, rep):
    bwd = F.select(case)["bwd"] + (" det" if mode.det else "")
    for stage, ratio in rep.ratio.items():
        key = (stage, "forward" if stage in F.FORWARD else bwd, case.dtype)
        MAXIMA[key] = max(MAXIMA.get(key, 0.0), ratio)
    print(f"[decoder tf stages] {case.id} {mode.id}: " + "  ".join(f"{s} {r:.3f}" for s, r in rep.ratio.items() if r > 0))
    assert not rep.failed, f"{case.id} {mode.id}: {rep.failed}"


@pytest.mark.parametrize("run", RUNS, ids=[F.run_id(r) for r in RUNS])
def test_every_stage(E, dev, run):
    """Forward and backward of one case in one mode, every stage."""
    case, mode = run
    c = case
    P, X = F.data(case, mode)
    eng = E.DecoderEngine(c.V, c.E, c.H, c.NL, DT[c.dtype])
    params = [p.to(dev) for p in P]
    pretrain = mode.pretrain or mode.ss is not None
    if mode.ss == (0.5, "sample") and c.name == "tf-splitk":
        # the gate product must not split K under scheduled sampling: the selection of the last GEMM of the call (the fused logits are no
        # GEMM), read in route-only mode over throw-away buffers
        with E.route_only() as r:
            forward(eng, case, mode, params, X, {}, dev, own=False)
            line = r.last()
        torch.cuda.synchronize()
        assert route_key(line)[1] == "nosplit" and " grid=16x1 " in line and " splits=1 " in line, line
    g = alloc_forward(case, mode, dev)
    pred, _, saved = forward(eng, case, mode, params, X, g, dev)[:3]
    assert_guards(case, g)
    assert pred.data_ptr() == g["out"].view.data_ptr() and bool((g["ids_ws"].view == -7).all())
    img = shadow_cpu(eng, P)
    st = state_cpu(case, mode, g)
    rep = F.Report()
    F.run_forward(case, mode, P, img, X, st, rep)
    if mode.drop and not mode.ss:      # the recurrence, h_n and c_n are those of the undropped call, bit for bit
        plain = mode._replace(drop=0.0)
        g0 = alloc_forward(case, plain, dev)
        forward(eng, case, plain, params, X, g0, dev)
        st0 = state_cpu(case, plain, g0)
        for k in ("xh", "gates", "c"):
            assert all(same_bytes(a, b) for a, b in zip(st[k], st0[k])), f"{case.id} {mode.id}: dropout moved {k}"
        assert same_bytes(st["h_n"], st0["h_n"]) and same_bytes(st["c_n"], st0["c_n"]) and same_bytes(st["hout"], st0["hout"])
    ws, gr = alloc_backward(case, P, dev)
    grads = [b.view.view(p.shape) for b, p in zip(gr["grads"], P)] + [gr["grads"][-1].view]
    E.set_deterministic(mode.det)
    try:
        with gpu_call():
            eng.forward_tf_bwd(params, saved, pred, X["d_pred"].to(dev), X["T"], pretrain, ws=views(ws), grads=grads)
            torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)
    assert_guards(case, ws, gr, g)
    w = views(ws)
    w = {k: ([t.cpu() for t in w[k]] if isinstance(w[k], list) else w[k].cpu()) for k in w}
    F.run_backward(case, mode, P, img, X, st, w, [t.cpu() for t in grads], rep)
    after = state_cpu(case, mode, g)
    for k, a in after.items():
        for x, y in zip(a if isinstance(a, list) else [a], st[k] if isinstance(a, list) else [st[k]]):
            assert x is None or same_bytes(x, y), f"{case.id} {mode.id}: the backward wrote into {k}"
    want = {"slot0", "xrows", "gates", "c", "h", "pad gates", "pad state", "hout", "out", "h_n", "c_n", "untouched", "dhout", "d_w_out", "d_b_out",
            "dgates", "dc", "dxh", "dxh keep", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "d_features", "d_embed", "logits" if pretrain else "y"}
    want |= (set() if pretrain else {"dlogits"}) | ({"hdrop"} if mode.drop else set()) | ({"d_b_ih == d_b_hh"} if mode.det else set())
    want |= {"replaced", "pick", "inputs"} if mode.ss and c.Tmax > 1 else set()
    assert want <= set(rep.ratio), want - set(rep.ratio)
    note(case, mode, rep)
