"""Every discriminator kernel (csrc/disc.hip) and both highway epilogues (csrc/gemm.hip), stage by stage and element by element against
the fp64 references and derived bounds of tests/disc_cases.py.  Every intermediate buffer is caller-owned (DiscEngine.fwd(state=),
.bwd(ws=)), read back after the call and checked against a reference formed from the buffers upstream of it.

Buffers carry sentinel guard rows before and after (their bits must not change); what a kernel has to overwrite holds NaN beforehand,
`ydrop` zeros (its pad columns are the allocation's).  The pad columns of `hpre` and `keep` are never read as values and a kernel may
leave them unwritten (gemm_kernel's epilogue skips n >= N, tile8's skips whole 8-column patches beyond N): they are not checked.

Largest err / bound seen per stage and kernel (MI355X; f32 mode / bf16 mode; the module prints the table again after every run under
-s; the bounds are NOT tightened to these, and no stage's derivation had to be revisited):
  emb (soft product)   0.072 / 0.025
  pooled               mfma 0.312 / 0.996   scalar<8> 0.116 / 0.989   scalar<32> 0.094 / 0.982   bf16-product - / 0.988
  hpre                 0.065 / 0.033        (highway routes: gemm f32 <= 0.021, gemm bf16 <= 0.008, tile8 <= 0.010)
  ydrop                0.388 / 0.996        (highway routes: gemm f32 <= 0.431, gemm bf16 <= 0.996, tile8 <= 0.996)
  feat, logits         0.064 / 0.029, 0.050 / 0.053
  dydrop, dh, dpooled  0.044 / 0.014, 0.439 / 0.996, 0.097 / 0.034
  demb                 small (1 row) 0.032 / 0.989   small (4 rows) 0.033 / 0.992   general 0.036 / 0.986
  conv_w               lds 0.218 / 0.248   <8> 0.270 / 0.189   <32> 0.016 / 0.014    (deterministic: 0.221 / 0.234, 0.270 / 0.189, 0.013 / 0.012)
  conv_b               lds 0.170 / 0.174   <8> 0.142 / 0.182   <32> 0.005 / 0.005    (deterministic: 0.142 / 0.140, 0.188 / 0.191, 0.007 / 0.007)
  o2l_w, o2l_b         0.233 / 0.252, 0.081 / 0.081
  f2o_w, f2o_b         0.290 / 0.154, 0.212 / 0.112
  hw_w, hw_b           0.389 / 0.172, 0.171 / 0.132
  emb_w, d_inp         0.120 / 0.098, 0.341 / 0.996
  argmax, keep, dfeat, every pad column, the weight images, and emb / pooled / argmax of the integer regime: exact.
(bf16 outputs: r dominates the bound, half a bf16 ulp is up to 2^-8 |ref|, so a correctly rounded result reaches ~1.)"""
import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests import disc_cases as D
from tests.disc_cases import CASES, HIGHWAY, TD
from tests.gpu_util import U8_SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DT = {"f32": L.F32, "bf16": L.BF16}
EXACT_SEED, ROUND_SEED = 101, 202
MAXIMA = {}          # (stage, kernel) -> largest err / bound: recorded, never asserted against


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
    for key in sorted(MAXIMA):
        print(f"\n[disc stages] err/bound max {MAXIMA[key]:.4f}  {key[0]:<12} {key[1]}", end="")
    print()


def make_engine(E, case, monkeypatch):
    monkeypatch.setenv("GIC_DISC_FP_ALIGN", str(case.fp_align))
    eng = E.DiscEngine(case.V, case.De, case.R, list(case.fs), list(case.nf), DT[case.dtype], dropout=D.DROP_P)
    assert (eng.F, eng.Fp, eng.s) == (case.F, case.Fp, case.s)
    return eng


def alloc_state(case, dev, hpre_off=0):
    td, MR, Fp, nan = TD[case.dtype], case.MR, case.Fp, float("nan")
    g = {"emb": Guarded(case.B * case.L, case.De, torch.float32, dev, nan), "pooled": Guarded(MR, Fp, td, dev, nan),
         "ydrop": Guarded(MR, Fp, td, dev, 0.0), "feat": Guarded(MR, D.OUT, torch.float32, dev, nan), "logits": Guarded(MR, 1, torch.float32, dev, nan)}
    if not case.forward_only:
        g.update(argmax=Guarded(MR, Fp, torch.uint8, dev, U8_SENTINEL), hpre=Guarded(MR, Fp, torch.float32, dev, nan, off=hpre_off),
                 keep=Guarded(MR, Fp, torch.uint8, dev, U8_SENTINEL))
    return g


def alloc_ws(case, dev, dh_off=0):
    td, MR, Fp, nan = TD[case.dtype], case.MR, case.Fp, float("nan")
    return {"dfeat": Guarded(MR, D.OUT_PAD, td, dev, nan), "dh": Guarded(MR, Fp, td, dev, nan, off=dh_off), "dydrop": Guarded(MR, Fp, torch.float32, dev, nan),
            "dpooled": Guarded(MR, Fp, torch.float32, dev, nan), "demb": Guarded(case.B * case.L, case.De, td, dev, nan)}


def live(g):
    return {k: v.live for k, v in g.items()}


def cpu(g):
    """The buffers read back (a forward-only state has no argmax / hpre / keep: None, as DiscEngine.alloc_state has them)."""
    out = {k: v.live.cpu() for k, v in g.items()}
    if "pooled" in out:
        for k in ("argmax", "hpre", "keep"):
            out.setdefault(k, None)
    return out


def assert_guards(case, *groups):
    for g in groups:
        for name, buf in g.items():
            assert buf.guards_intact(), f"{case.id}: the guard rows of {name} changed"


def forward(eng, case, params, X, g, dev, seed=0, device_dropout=False):
    st = live(g)
    state = {k: st.get(k) for k in ("emb", "pooled", "argmax", "hpre", "keep", "ydrop", "feat")}
    mask = X["mask"].to(dev) if X["mask"] is not None else None
    assert X["train"] is False or mask is not None or device_dropout
    eng.fwd(params, X["soft"].to(dev) if X["soft"] is not None else None, X["ids"].to(dev) if X["ids"] is not None else None,
            X["train"], mask, seed=seed, state=state, logits=st["logits"], forward_only=case.forward_only)
    torch.cuda.synchronize()
    return state


def shadow_cpu(eng):
    return {k: (v.cpu() if v is not None else None) for k, v in eng._shadow.items()}


def note(case, rep, kernels):
    """Record the report's ratios under the kernel that served each stage, print them, and fail on any flagged stage."""
    for stage, ratio in rep.ratio.items():
        base = stage.split(".")[0]
        key = (base, f"{kernels[base]} {case.dtype}" if kernels.get(base) else case.dtype)
        MAXIMA[key] = max(MAXIMA.get(key, 0.0), ratio)
    print(f"[disc stages] {case.id}: " + "  ".join(f"{s} {r:.3f}" for s, r in rep.ratio.items() if r > 0))
    assert not rep.failed, f"{case.id}: {rep.failed}"


def kernels_of(case, highway=None):
    fwd = "bf16-product" if case.fwd == "bf16" else case.fwd
    k = {"pooled": fwd, "argmax": fwd, "demb": case.bwd_x, "conv_w": case.bwd_w, "conv_b": case.bwd_w}
    if highway:
        k.update(hpre=highway, ydrop=highway)
    return k


@pytest.mark.parametrize("case", [c for c in CASES if c.exact], ids=[c.id for c in CASES if c.exact])
def test_forward_convolution_is_exact_on_integers(E, dev, case, monkeypatch):
    """Integer weights and biases: every pre-activation is an integer exact in f32 under any summation order and in bf16, ties and zero
    maxima are frequent (counted in tests/test_disc_cases.py).  emb, pooled and argmax bit for bit, first index on ties, 0 at maximum 0."""
    gen = torch.Generator().manual_seed(EXACT_SEED)
    P = D.make_params(case, "exact", gen)
    X = D.make_inputs(case, gen, train=False)
    eng = make_engine(E, case, monkeypatch)
    g = alloc_state(case, dev)
    forward(eng, case, [p.to(dev) for p in P], X, g, dev)
    assert_guards(case, g)
    rep = D.Report()
    D.run_forward(case, P, D.images(case, P), X, cpu(g), rep, exact=True)
    assert {"emb", "pooled"} <= set(rep.ratio) and (case.forward_only or "argmax" in rep.ratio)
    note(case, rep, kernels_of(case))


def backward(E, eng, case, params, P, X, g, dev, want_param, want_inp, accumulate, gen, det=False, dh_off=0, mixed=None):
    """One gic_disc_bwd over the state `g`; returns (ws, grads on the CPU, G0, d_inp on the CPU)."""
    w = alloc_ws(case, dev, dh_off)
    G0 = grads = None
    if want_param:
        G0 = [torch.randn(p.shape, generator=gen) if accumulate else torch.full(p.shape, float("nan")) for p in P]
        grads = [t.to(dev) for t in G0]
        G0 = G0 if accumulate else None
    d_inp = Guarded(case.B * case.L, case.V, TD[case.dtype], dev, float("nan")) if want_inp else None
    st = live(g)
    ids, soft = (X["ids"], X["soft"]) if mixed is None else mixed
    E.set_deterministic(det)
    try:
        eng.bwd(params, st, soft.to(dev) if soft is not None else None, ids.to(dev) if ids is not None else None, X["train"],
                X["d_logits"].to(dev), want_param, want_inp, grads=grads, accumulate=accumulate, ws=live(w),
                d_inp=d_inp.live.view(case.B, case.L, case.V) if want_inp else None)
        torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)
    assert_guards(case, w, g, {"d_inp": d_inp} if want_inp else {})
    return w, ([t.cpu() for t in grads] if want_param else None), G0, (d_inp.live.cpu() if want_inp else None)


def run_pass(E, dev, case, monkeypatch, soft, train, accumulate, want_inp, det=False, dh_off=0, seed=ROUND_SEED):
    gen = torch.Generator().manual_seed(seed)
    P = D.make_params(case, "rounding", gen)
    X = D.make_inputs(case, gen, soft=soft, train=train)
    eng = make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    g = alloc_state(case, dev)
    forward(eng, case, params, X, g, dev)
    assert_guards(case, g)
    img = shadow_cpu(eng)
    if img["emb"] is None:
        img["emb"] = P[0]
    rep = D.Report()
    D.check_images(case, P, {k: v for k, v in img.items() if not (k == "emb" and case.dtype == "f32")}, rep)
    st = cpu(g)
    D.run_forward(case, P, img, X, st, rep)
    if case.forward_only:
        assert st.get("hpre") is None and st.get("keep") is None and st.get("argmax") is None
        note(case, rep, kernels_of(case))
        return
    w, grads, G0, d_inp = backward(E, eng, case, params, P, X, g, dev, True, want_inp, accumulate, gen, dh_off=dh_off)
    D.run_backward(case, P, img, X, st, cpu(w), grads, G0, d_inp, rep)
    note(case, rep, kernels_of(case))
    if want_inp:            # the generator's path: the input gradient alone, no parameter gradients
        w2, _, _, d_inp2 = backward(E, eng, case, params, P, X, g, dev, False, True, False, gen, dh_off=dh_off)
        rep2 = D.Report()
        D.run_backward(case, P, img, X, st, cpu(w2), None, None, d_inp2, rep2)
        note(case, rep2, kernels_of(case))
    if det and case.det:
        runs = []
        for _ in range(2):
            gen_d = torch.Generator().manual_seed(seed + 1)
            wd, gd, G0d, _ = backward(E, eng, case, params, P, X, g, dev, True, False, accumulate, gen_d, det=True)
            runs.append(gd)
            repd = D.Report()
            D.run_backward(case, P, img, X, st, cpu(wd), gd, G0d, None, repd, det=True)
            note(case, repd, {k: v + " det" for k, v in kernels_of(case).items() if v})
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{case.id}: two deterministic runs differ"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_stage_ids_input_train_mode(E, dev, case, monkeypatch):
    """Token ids, train mode with an explicit keep mask (forward only: eval), parameter gradients overwritten; then again in
    deterministic mode (cases marked det), twice, bit-identical."""
    run_pass(E, dev, case, monkeypatch, soft=False, train=not case.forward_only, accumulate=False, want_inp=False, det=True)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_stage_soft_input_eval_mode(E, dev, case, monkeypatch):
    """A soft input, eval mode, parameter gradients accumulated onto a Gaussian G0, the input gradient with and without them; the
    deterministic mode accumulates too."""
    run_pass(E, dev, case, monkeypatch, soft=True, train=False, accumulate=True, want_inp=not case.forward_only, det=True, seed=ROUND_SEED + 7)


@pytest.mark.parametrize("name", ["r24-L11-f32", "r24-L11-bf16"])
def test_scalar_highway_backward(E, dev, name, monkeypatch):
    """`dh` two elements off its alignment: disc_bwd_t takes the element-wise disc_highway_bwd_kernel (and the products that read `dh`
    their scalar loads)."""
    case = {c.id: c for c in CASES}[name]
    run_pass(E, dev, case._replace(name="dh-off2-" + case.name), monkeypatch, soft=False, train=True, accumulate=False, want_inp=False, dh_off=2)


@pytest.mark.parametrize("det", [False, True], ids=["", "det"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mixed_batch_backward(E, dev, dtype, det, monkeypatch):
    """The train step's one backward over the real (ids) and fake (soft) passes: the state holds the ids pass in its first half of the
    rows; embeddings.weight's gradient is the scatter of the first half plus the product of the second."""
    half = {c.id: c for c in CASES}["r24-L11-" + dtype]
    case = half._replace(name="mixed-" + half.name, B=2 * half.B)
    gen = torch.Generator().manual_seed(ROUND_SEED + 13)
    P = D.make_params(case, "rounding", gen)
    Xi, Xs = D.make_inputs(half, gen, soft=False), D.make_inputs(half, gen, soft=True)
    eng = make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    g = alloc_state(case, dev)
    st = {k: v for k, v in live(g).items()}
    a, b = eng.split_state(st)
    for X, part in ((Xi, a), (Xs, b)):
        eng.fwd(params, X["soft"].to(dev) if X["soft"] is not None else None, X["ids"].to(dev) if X["ids"] is not None else None, True,
                X["mask"].to(dev), state={k: part[k] for k in ("emb", "pooled", "argmax", "hpre", "keep", "ydrop", "feat")}, logits=part["logits"])
    torch.cuda.synchronize()
    assert_guards(case, g)
    img = shadow_cpu(eng)
    if img["emb"] is None:
        img["emb"] = P[0]
    X = {"train": True, "ids": None, "soft": None, "mask": torch.cat([Xi["mask"], Xs["mask"]]), "d_logits": torch.cat([Xi["d_logits"], Xs["d_logits"]])}
    for acc in (False, True):
        w, grads, G0, _ = backward(E, eng, case, params, P, X, g, dev, True, False, acc, gen, det=det, mixed=(Xi["ids"], Xs["soft"]))
        rep = D.Report()
        D.run_backward(case, P, img, X, cpu(g), cpu(w), grads, G0, None, rep, det=det, mixed=(Xi["ids"], Xs["soft"]))
        assert "emb_w" in rep.ratio
        note(case, rep, kernels_of(case))


@pytest.mark.parametrize("h", HIGHWAY, ids=[h.id for h in HIGHWAY])
def test_highway_forward_on_every_route(E, dev, h, monkeypatch):
    """Each highway route of the scan on its smallest shape, three ways: an explicit mask, device-drawn dropout, eval mode.  The route is
    asserted with the real pointers.  Device-drawn: the fused epilogue's keep and ydrop are bit-equal to disc_highway_redrop_kernel's
    for the same seed, differ for another, and the kept fraction lies within 4 standard errors of 1 - p."""
    case = h.case()
    gen = torch.Generator().manual_seed(ROUND_SEED + 21)
    P = D.make_params(case, "rounding", gen)
    eng = make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    eng.prepare(params)
    img = shadow_cpu(eng)
    if img["emb"] is None:
        img["emb"] = P[0]
    F = case.F
    kern = h.route.split(" grid")[0]
    first = True
    for way in ("mask", "philox", "eval"):
        X = D.make_inputs(case, gen, train=way != "eval", mask=way == "mask")
        g = alloc_state(case, dev, hpre_off=h.off // 4)
        with E.route_only() as r:
            forward(eng, case, params, X, g, dev, seed=11, device_dropout=True)
            line = r.last()
        assert line.split(" lds=")[0] == h.route, line
        forward(eng, case, params, X, g, dev, seed=11, device_dropout=True)
        assert_guards(case, g)
        st = cpu(g)
        rep = D.Report()
        D.run_forward(case, P, img, X, st, rep, stages=None if first else {"ydrop", "feat"})
        first = False
        assert {"hpre", "ydrop", "feat"} <= set(rep.ratio)
        note(case, rep, kernels_of(case, highway=kern))
        if way == "philox":
            keep = st["keep"][:, :F]
            p_keep, n = 1.0 - D.DROP_P, keep.numel()
            assert set(keep.unique().tolist()) <= {0, 1}
            assert abs(float(keep.float().mean()) - p_keep) <= 4 * (p_keep * (1 - p_keep) / n) ** 0.5, float(keep.float().mean())
            for seed, same in ((11, True), (12, False)):
                g2 = alloc_state(case, dev)
                dst = {k: live(g2)[k] for k in ("keep", "ydrop", "feat")}
                eng.fwd_redrop(params, live(g), dst, True, None, seed=seed, logits=live(g2)["logits"])
                torch.cuda.synchronize()
                assert_guards(case, g2)
                k2, y2 = g2["keep"].live[:, :F].cpu(), g2["ydrop"].live.cpu()
                assert float(y2[:, F:].float().abs().max()) == 0.0
                eq = torch.equal(k2, keep) and torch.equal(y2.view(D.BITS[y2.dtype]), st["ydrop"].view(D.BITS[y2.dtype]))
                assert eq == same, f"{h.id}: redrop with seed {seed} {'differs from' if same else 'equals'} the fused epilogue's draw"
