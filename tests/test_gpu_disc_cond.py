"""The conditioned discriminator's kernels (csrc/disc_cond.hip) and gic_disc_bwd_cond, element by element, by the method of
tests/disc_cases.py: every stage against an fp64 reference formed from the buffers the kernels wrote upstream of it, bounds derived per
element (tests/disc_cond_oracle.py: u = 2^-24; logits (F + OUT + 4) u (sum |feat w| + |b| + s sum |y q|); dydrop (OUT_PAD + 5) u
(|dfeat| |W| + s |g q|); d_q (R + 4) u s sum_r |g y|; q and d img_proj: disc_cases.sum_bound over C and over B), pad columns exactly zero,
no element excluded.  The stages of gic_disc_bwd_cond downstream of dydrop are walked by disc_cases.run_backward on the buffers it wrote.

Shapes (B, R, F, Fp): (3,24,91,128) pad columns and F % 8 != 0; (3,24,88,88) no pad; (2,72,64,64) R > 64; (1,5,40,64) one caption, R below
a wave's rows; (70,40,91,128) 2800 rows; (2,4,1030,1088) F > 1024 -- the cases of the same names in disc_cases.CASES."""
import pytest
import torch

from tests import disc_cases as D
from tests import disc_cond_oracle as DC
from tests import test_gpu_disc_stages as S

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in D.CASES if not c.forward_only}
NAMES = ("r24-L11", "fp8", "r72-L9", "det-cap5", "r40-b70", "f1030")
SHAPES = {"r24-L11": (3, 24, 91, 128), "fp8": (3, 24, 88, 88), "r72-L9": (2, 72, 64, 64), "det-cap5": (1, 5, 40, 64),
          "r40-b70": (70, 40, 91, 128), "f1030": (2, 4, 1030, 1088)}
IDS = [f"{n}-{dt}" for n in NAMES for dt in ("f32", "bf16")]
SEED = 606


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


def note(case, rep):
    print(f"[disc cond] {case.id}: " + "  ".join(f"{s} {r:.3f}" for s, r in rep.ratio.items() if r > 0))
    assert not rep.failed, f"{case.id}: {rep.failed}"


def images_of(eng, P):
    img = S.shadow_cpu(eng)
    if img["emb"] is None:
        img["emb"] = P[0]
    return img


def forward_cond(E, eng, case, params, P, X, q, dev, rep):
    """The plain forward into a guarded state (walked by disc_cases), then the match term three ways: added onto those logits, alone, and
    through fwd(cond=), a forward of its own.  Returns the state and logits of that last forward (what the backward then differentiates)."""
    g = S.alloc_state(case, dev)
    state = S.forward(eng, case, params, X, g, dev)
    img = images_of(eng, P)
    st = S.cpu(g)
    D.run_forward(case, P, img, X, st, rep)
    qd = q.to(dev)
    eng.match_logits(state, qd, logits=g["logits"].live, accumulate=True)
    alone = S.Guarded(case.MR, 1, torch.float32, dev, float("nan"))
    eng.match_logits(state, qd, logits=alone.live)
    torch.cuda.synchronize()
    S.assert_guards(case, g, {"alone": alone})
    st2 = S.cpu(g)
    for k in ("ydrop", "feat"):
        assert torch.equal(st[k].view(D.BITS.get(st[k].dtype, st[k].dtype)), st2[k].view(D.BITS.get(st[k].dtype, st[k].dtype))), f"the match kernel changed {k}"
    DC.check_match_forward(case, P, st2, q, st2["logits"], rep)
    DC.check_match_only(case, st2, q, alone.live.cpu(), rep)
    # fwd(cond=): a forward of its own (the head's split-K sums are not reproducible bit for bit), checked against the state it wrote
    again = S.Guarded(case.MR, 1, torch.float32, dev, float("nan"))
    mask = X["mask"].to(dev) if X["mask"] is not None else None
    eng.fwd(params, X["soft"].to(dev) if X["soft"] is not None else None, X["ids"].to(dev) if X["ids"] is not None else None, X["train"], mask,
            state=state, logits=again.live, forward_only=case.forward_only, cond=qd)
    torch.cuda.synchronize()
    S.assert_guards(case, g, {"again": again})
    rep3 = D.Report()
    DC.check_match_forward(case, P, S.cpu(g), q, again.live.cpu(), rep3)
    rep.ratio["fwd(cond=) logits"] = rep3.ratio["match logits"]
    if rep3.failed:
        rep.failed["fwd(cond=) logits"] = rep3.failed["match logits"]
    assert {"match logits", "match term"} <= set(rep.ratio)
    st2 = S.cpu(g)
    st2["logits"] = again.live.cpu()
    return g, st2, img


def backward_cond(E, eng, case, params, P, X, g, q, dev, gen, accumulate=False, det=False, mixed=None, cond=True):
    w = S.alloc_ws(case, dev)
    G0 = [torch.randn(p.shape, generator=gen) if accumulate else torch.full(p.shape, float("nan")) for p in P]
    grads = [t.to(dev) for t in G0]
    d_q = S.Guarded(case.B, case.F, torch.float32, dev, float("nan"))
    ids, soft = (X["ids"], X["soft"]) if mixed is None else mixed
    E.set_deterministic(det)
    try:
        eng.bwd(params, S.live(g), soft.to(dev) if soft is not None else None, ids.to(dev) if ids is not None else None, X["train"],
                X["d_logits"].to(dev), True, False, grads=grads, accumulate=accumulate, ws=S.live(w),
                cond=q.to(dev) if cond else None, d_q=d_q.live if cond else None, cond_entry=True)
        torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)
    S.assert_guards(case, w, g, {"d_q": d_q})
    return S.cpu(w), [t.cpu() for t in grads], (G0 if accumulate else None), d_q.live.cpu()


def walk_backward(case, P, img, X, st, ws, grads, G0, q, d_q, rep, det=False, mixed=None):
    """disc_cases' walker over everything downstream of dydrop (its own `dydrop` stage knows no match term: replaced by ours)."""
    D.run_backward(case, P, img, X, st, ws, grads, G0, None, rep, det=det, mixed=mixed)
    rep.failed.pop("dydrop", None)
    rep.ratio.pop("dydrop", None)
    DC.check_match_backward(case, img, st, ws, q, X["d_logits"], d_q, rep, det=det)
    assert "d_q" in rep.ratio and (det or {"cond dydrop", "dh", "dpooled"} <= set(rep.ratio))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_case(E, dev, case, monkeypatch, soft, train, accumulate):
    assert (case.B, case.R, case.F, case.Fp) == SHAPES[case.name]
    gen = torch.Generator().manual_seed(SEED)
    P = D.make_params(case, "rounding", gen)
    X = D.make_inputs(case, gen, soft=soft, train=train)
    q = torch.randn(case.B, case.F, generator=gen)
    eng = S.make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    rep = D.Report()
    g, st, img = forward_cond(E, eng, case, params, P, X, q, dev, rep)
    ws, grads, G0, d_q = backward_cond(E, eng, case, params, P, X, g, q, dev, gen, accumulate)
    walk_backward(case, P, img, X, st, ws, grads, G0, q, d_q, rep)
    note(case, rep)
    # the same call again: dydrop and d_q carry the same bits in the default mode (no atomics, a fixed order)
    gen2 = torch.Generator().manual_seed(SEED + 1)
    ws2, _, _, d_q2 = backward_cond(E, eng, case, params, P, X, g, q, dev, gen2, accumulate)
    assert same_bits(ws["dydrop"], ws2["dydrop"]) and same_bits(d_q, d_q2), f"{case.id}: dydrop / d_q differ between two runs"
    return eng, params, P, X, g, st, img, q, d_q, gen


@pytest.mark.parametrize("cid", IDS)
def test_every_stage_ids_input_train_mode(E, dev, cid, monkeypatch):
    """Token ids, train mode with an explicit keep mask, gradients overwritten.  Then deterministic mode: the backward with q twice
    (every gradient and d_q bit-identical, d_q also to the default mode's), and gic_disc_bwd_cond(q = NULL) against gic_disc_bwd."""
    case = BY_ID[cid]
    eng, params, P, X, g, st, img, q, d_q, gen = run_case(E, dev, case, monkeypatch, soft=False, train=True, accumulate=False)
    runs = []
    for _ in range(2):
        wsd, gd, _, dqd = backward_cond(E, eng, case, params, P, X, g, q, dev, gen, det=True)
        repd = D.Report()
        walk_backward(case, P, img, X, st, wsd, gd, None, q, dqd, repd, det=True)
        note(case, repd)
        runs.append((gd, dqd))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert same_bits(a, b), f"{cid}: two deterministic runs differ"
    assert same_bits(runs[0][1], runs[1][1]) and same_bits(runs[0][1], d_q), f"{cid}: d_q is not the same in and out of deterministic mode"
    # q = NULL through the conditioned entry: exactly gic_disc_bwd (state, logits gradient and workspace contents included)
    _, g_null, _, _ = backward_cond(E, eng, case, params, P, X, g, q, dev, gen, det=True, cond=False)
    w = S.alloc_ws(case, dev)
    grads = [torch.full(p.shape, float("nan"), device=dev) for p in P]
    E.set_deterministic(True)
    try:
        eng.bwd(params, S.live(g), None, X["ids"].to(dev), True, X["d_logits"].to(dev), True, False, grads=grads, ws=S.live(w))
        torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)
    for a, b in zip(g_null, grads):
        assert same_bits(a, b.cpu()), f"{cid}: gic_disc_bwd_cond(q = NULL) differs from gic_disc_bwd"


@pytest.mark.parametrize("cid", IDS)
def test_every_stage_soft_input_eval_mode(E, dev, cid, monkeypatch):
    """A soft input, eval mode, parameter gradients accumulated onto a Gaussian G0."""
    run_case(E, dev, BY_ID[cid], monkeypatch, soft=True, train=False, accumulate=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_match_term_on_a_forward_only_state(E, dev, dtype, monkeypatch):
    case = {c.id: c for c in D.CASES if c.forward_only}["fo-r24-L11-" + dtype]
    gen = torch.Generator().manual_seed(SEED + 3)
    P = D.make_params(case, "rounding", gen)
    X = D.make_inputs(case, gen, train=False)
    q = torch.randn(case.B, case.F, generator=gen)
    eng = S.make_engine(E, case, monkeypatch)
    rep = D.Report()
    _, st, _ = forward_cond(E, eng, case, [p.to(dev) for p in P], P, X, q, dev, rep)
    assert st["hpre"] is None and st["keep"] is None and st["argmax"] is None
    note(case, rep)


@pytest.mark.parametrize("det", [False, True], ids=["", "det"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mixed_batch_backward_with_q_twice(E, dev, dtype, det, monkeypatch):
    """The step's one backward over the real (ids) | fake (soft) halves of one state, with q = [q; q]."""
    half = BY_ID["r24-L11-" + dtype]
    case = half._replace(name="mixed-" + half.name, B=2 * half.B)
    gen = torch.Generator().manual_seed(SEED + 13)
    P = D.make_params(case, "rounding", gen)
    Xi, Xs = D.make_inputs(half, gen, soft=False), D.make_inputs(half, gen, soft=True)
    qh = torch.randn(half.B, half.F, generator=gen)
    q = torch.cat([qh, qh])
    eng = S.make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    g = S.alloc_state(case, dev)
    a, b = eng.split_state(dict(S.live(g)))
    for X, part in ((Xi, a), (Xs, b)):
        eng.fwd(params, X["soft"].to(dev) if X["soft"] is not None else None, X["ids"].to(dev) if X["ids"] is not None else None, True,
                X["mask"].to(dev), state={k: part[k] for k in ("emb", "pooled", "argmax", "hpre", "keep", "ydrop", "feat")}, logits=part["logits"],
                cond=qh.to(dev))
    torch.cuda.synchronize()
    S.assert_guards(case, g)
    img = images_of(eng, P)
    st = S.cpu(g)
    X = {"train": True, "ids": None, "soft": None, "mask": torch.cat([Xi["mask"], Xs["mask"]]), "d_logits": torch.cat([Xi["d_logits"], Xs["d_logits"]])}
    rep = D.Report()
    DC.check_match_forward(case, P, st, q, st["logits"], rep)
    mixed = (Xi["ids"], Xs["soft"])
    for acc in (False, True):
        ws, grads, G0, d_q = backward_cond(E, eng, case, params, P, X, g, q, dev, gen, acc, det=det, mixed=mixed)
        walk_backward(case, P, img, X, st, ws, grads, G0, q, d_q, rep, det=det, mixed=mixed)
    assert "emb_w" in rep.ratio
    note(case, rep)


@pytest.mark.parametrize("shape", [(3, 91, 512), (70, 91, 512), (2, 1030, 2048), (1, 40, 512)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_image_projection_and_its_gradients(E, dev, dtype, shape, monkeypatch):
    """q = pooled W^T + b on the compute-dtype image of W (sum_bound over C); d W = d_q^T pooled, d b = colsum(d_q) (sum_bound over B),
    overwritten and accumulated."""
    B, F, C = shape
    monkeypatch.setenv("GIC_DISC_FP_ALIGN", "64")
    td = D.TD[dtype]
    eng = E.DiscEngine(50, 4, 4, [1], [F], S.DT[dtype])
    gen = torch.Generator().manual_seed(SEED + 29)
    W, b = torch.randn(F, C, generator=gen) / C ** 0.5, 0.1 * torch.randn(F, generator=gen)
    pooled = torch.randn(B, C, generator=gen).to(td)
    d_q = torch.randn(B, F, generator=gen)
    q, kept = eng.img_proj_fwd(W.to(dev), b.to(dev), pooled.to(dev))
    rep = D.Report()
    pd, Wd = pooled.double(), W.to(td).double()
    rep.check("q", q.cpu(), pd @ Wd.t() + b.double(), D.sum_bound(C, pd.abs() @ Wd.abs().t() + b.double().abs(), None))
    rep.bits("pooled kept", kept.cpu(), pooled)
    for acc in (False, True):
        G0w, G0b = torch.randn(F, C, generator=gen), torch.randn(F, generator=gen)
        gw, gb = G0w.to(dev), G0b.to(dev)
        eng.img_proj_bwd(d_q.to(dev), kept, gw, gb, accumulate=acc)
        torch.cuda.synchronize()
        c0w, c0b = (G0w.double(), G0b.double()) if acc else (torch.zeros(F, C, dtype=torch.float64), torch.zeros(F, dtype=torch.float64))
        dd = d_q.double()
        rep.check("d img_proj.weight", gw.cpu(), dd.t() @ pd + c0w, D.sum_bound(B, dd.abs().t() @ pd.abs() + c0w.abs(), None))
        rep.check("d img_proj.bias", gb.cpu(), dd.sum(0) + c0b, D.sum_bound(B, dd.abs().sum(0) + c0b.abs(), None))
    case = D.Case(f"proj-{B}x{F}x{C}", B, 1, 4, 4, (1,), (F,), dtype, "mfma", None, None)
    note(case, rep)
