"""The loss, optimizer and helper kernels (csrc/optim.hip, csrc/util.hip, csrc/determinism.hip, BatchNorm1d of csrc/encoder.hip) on the
GPU, element by element against the fp64 references and derived bounds of tests/aux_cases.py, every case of its tables, through the
existing entry points: engine.clip_adam / gan_losses / xent / rollout_rewards / embedding_fwd / embedding_bwd, and gic_cast2d,
gic_colsum, gic_bn_stats, gic_bn1d_fwd / bwd through _lib.

Every output lives in a tests.gpu_util.Guarded buffer whose sentinel guards must be intact after the call; the engine wrappers that
allocate their own outputs get them from `guarded_allocs`, which hands the engine module guarded buffers for the duration of the call.
Outputs hold NaN (casts: the sentinel) beforehand, input padding columns hold NaN, misaligned operands are Guarded views with `off`.
The largest err / bound per kernel is printed after the module under -s (recorded in tests/aux_cases.py, never asserted against)."""
import contextlib
import ctypes as C
import re

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests import aux_cases as A
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

DT = {"f32": L.F32, "bf16": L.BF16}
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
        print(f"\n[aux kernels] err/bound max {MAXIMA[k]:.4f}  {k}", end="")
    print()


def note(ratios):
    A.merge(MAXIMA, ratios)
    assert all(0 <= r <= 1 for r in ratios.values()), ratios


def put(t, dev, off=0, fill=NAN):
    """A Guarded buffer holding t (1-D or [rows, ld])."""
    rows, ld = (t.shape[0], 1) if t.dim() == 1 else t.shape
    g = Guarded(rows, ld, t.dtype, dev, 0 if t.dtype == torch.int64 else fill, off)
    g.live.copy_(t.reshape(g.live.shape))
    return g


def fresh(rows, ld, dtype, dev, fill=NAN, off=0):
    return Guarded(rows, ld, dtype, dev, fill, off)


def intact(case, **bufs):
    for name, g in bufs.items():
        assert g.guards_intact(), f"{case.id}: the guards of {name} changed"


class _GuardedTorch:
    """`torch` as the engine module sees it while guarded_allocs is open: empty / empty_like come from Guarded buffers."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, device=None, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= int(s)
        g = Guarded(n, 1, dtype, device, NAN)
        self.bufs.append(g)
        return g.live.view(*shape)

    def empty_like(self, t):
        return self.empty(*t.shape, device=t.device, dtype=t.dtype)


@contextlib.contextmanager
def guarded_allocs(E):
    proxy = E.torch = _GuardedTorch()
    try:
        yield proxy
        torch.cuda.synchronize()
        for i, g in enumerate(proxy.bufs):
            assert g.guards_intact(), f"the guards of the call's output buffer {i} changed"
    finally:
        E.torch = torch


@contextlib.contextmanager
def deterministic(E, on):
    was = E.deterministic()
    E.set_deterministic(bool(on))
    try:
        yield
    finally:
        E.set_deterministic(was)


# ---------------------------------------------------------------------------------------------------------------- clip + Adam
@pytest.mark.parametrize("case", A.ADAM_CASES, ids=[c.id for c in A.ADAM_CASES])
def test_clip_adam(E, dev, case):
    inp = A.adam_inputs(case)
    h = A.ADAM_HYPER
    b = {k: put(inp[k], dev, off) for k, off in zip("pgmv", case.off)}
    nparts = E.clip_adam_partials(case.n)
    assert nparts == A.adam_partials(case.n)
    partials, norm = fresh(nparts, 1, torch.float32, dev), fresh(1, 1, torch.float32, dev)
    step = put(torch.tensor([case.t - 1], dtype=torch.int64), dev)
    assert partials.live.numel() == nparts
    E.clip_adam(b["p"].live, b["g"].live, b["m"].live, b["v"].live, h["lr"], h["b1"], h["b2"], h["eps"], h["clip"], step.live, norm.live, partials.live)
    torch.cuda.synchronize()
    intact(case, partials=partials, norm=norm, step=step, **b)
    A.same_bits("clip_adam", case.id, "the gradients are read only", b["g"].live, inp["g"].to(dev))
    assert not bool(torch.isnan(partials.live).any())
    note(A.adam_check(case, inp, {"norm": norm.live, "m": b["m"].live, "v": b["v"].live, "p": b["p"].live, "step": int(step.live[0])}))


def test_clip_adam_counts_one_step_per_call(E, dev):
    """Two calls in a row: the counter goes t - 1 -> t -> t + 1 and the second update is step t + 1's of the first one's state."""
    first, second = A.AdamCase(4097, t=2), A.AdamCase(4097, t=3)
    inp = A.adam_inputs(first)
    h = A.ADAM_HYPER
    b = {k: put(inp[k], dev) for k in "pgmv"}
    partials, norm = fresh(2, 1, torch.float32, dev), fresh(1, 1, torch.float32, dev)
    step = put(torch.tensor([1], dtype=torch.int64), dev)
    args = (b["p"].live, b["g"].live, b["m"].live, b["v"].live, h["lr"], h["b1"], h["b2"], h["eps"], h["clip"], step.live, norm.live, partials.live)
    E.clip_adam(*args)
    out = {"norm": norm.live.clone(), "m": b["m"].live.clone(), "v": b["v"].live.clone(), "p": b["p"].live.clone(), "step": int(step.live[0])}
    note(A.adam_check(first, inp, out))
    E.clip_adam(*args)
    torch.cuda.synchronize()
    inp2 = dict(inp, p=out["p"].cpu(), m=out["m"].cpu(), v=out["v"].cpu())
    note(A.adam_check(second, inp2, {"norm": norm.live, "m": b["m"].live, "v": b["v"].live, "p": b["p"].live, "step": int(step.live[0])}))
    intact(first, partials=partials, norm=norm, step=step, **b)


# ---------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("case", A.GAN_CASES, ids=[c.id for c in A.GAN_CASES])
def test_gan_losses(E, dev, case):
    inp = A.gan_inputs(case)
    x = [inp[k].to(dev) for k in ("d_real", "d_fake", "g_out")]
    with guarded_allocs(E):
        losses, g = E.gan_losses(case.type, *x, want_grads=True)
    with guarded_allocs(E):
        bare, none = E.gan_losses(case.type, *x, want_grads=False)
    assert none is None
    A.same_bits("gan_losses", case.id, "losses without the gradient pointers", bare.cpu(), losses.cpu())
    out = {"losses": losses.cpu()}
    out.update({k: g[k].cpu() for k in A.GRAD_NAMES})
    note(A.gan_check(case, inp, out))


@pytest.mark.parametrize("case", A.ROLLOUT_CASES, ids=[c.id for c in A.ROLLOUT_CASES])
def test_rollout_rewards(E, dev, case):
    inp = A.rollout_inputs(case)
    with guarded_allocs(E):
        r = E.rollout_rewards(inp["mc"].to(dev) if inp["mc"] is not None else None, inp["full"].to(dev), case.B, case.L, case.N, case.R)
    note(A.rollout_check(case, inp, {"rewards": r.cpu()}))


@pytest.mark.parametrize("case", A.XENT_CASES, ids=[c.id for c in A.XENT_CASES])
def test_xent(E, dev, case):
    inp = A.xent_inputs(case)
    with guarded_allocs(E) as alloc:
        loss, dl = E.xent(inp["logits"].to(dev), inp["targets"].to(dev), True, inp["w"].to(dev) if inp["w"] is not None else None)
    buf = alloc.bufs[0].live.cpu()                        # [mean, the rows' terms]
    assert buf.numel() == 1 + case.rows and loss.data_ptr() == alloc.bufs[0].live.data_ptr()
    note(A.xent_check(case, inp, {"loss": buf[0], "row_loss": buf[1:], "dlogits": dl.cpu()}))
    with guarded_allocs(E) as alloc:
        E.xent(inp["logits"].to(dev), inp["targets"].to(dev), False, inp["w"].to(dev) if inp["w"] is not None else None)
    A.same_bits("xent_rows", case.id, "losses without the gradient pointer", alloc.bufs[0].live.cpu(), buf, nan_free=True)


# ---------------------------------------------------------------------------------------------------------------- cast2d
def run_cast(case, dev):
    inp = A.cast_inputs(case)
    src = put(inp["src"], dev, case.soff)
    dst = fresh(case.rows, case.ldd, A.TD[case.dst], dev, A.SENTINEL, case.doff)
    L.check(L.load().gic_cast2d(src.live.data_ptr(), DT[case.src], case.lds, dst.live.data_ptr(), DT[case.dst], case.ldd, case.rows, case.cols,
                                torch.cuda.current_stream().cuda_stream), "gic_cast2d")
    torch.cuda.synchronize()
    intact(case, src=src, dst=dst)
    assert src.live.data_ptr() % 16 == (case.soff * src.live.element_size()) % 16 and dst.live.data_ptr() % 16 == (case.doff * dst.live.element_size()) % 16
    return inp, dst.live.view(case.rows, case.ldd)


@pytest.mark.parametrize("case", A.CAST_CASES, ids=[c.id for c in A.CAST_CASES])
def test_cast2d(dev, case):
    inp, dst = run_cast(case, dev)
    note(A.cast_check(case, inp, {"dst": dst}))


def test_cast2d_scalar_kernel_gives_the_vector_kernels_bits(dev):
    _, base = run_cast(A.CAST_BASE, dev)
    for case in A.CAST_BROKEN:
        if case.cols == A.CAST_BASE.cols:
            _, dst = run_cast(case, dev)
            A.same_bits("cast2d", case.id, "against the 16-byte kernel", dst[:, :case.cols], base[:, :case.cols], nan_free=True)


# ---------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("case", A.COLSUM_CASES, ids=[c.id for c in A.COLSUM_CASES])
def test_colsum(E, dev, case):
    inp = A.colsum_inputs(case)
    a = put(inp["A"], dev, case.off)
    out = put(inp["out0"], dev) if case.acc else fresh(case.cols, 1, torch.float32, dev)
    with deterministic(E, case.det):
        L.check(L.load().gic_colsum(a.live.data_ptr(), DT[case.dtype], case.lda, case.rows, case.cols, out.live.data_ptr(), case.acc,
                                    torch.cuda.current_stream().cuda_stream), "gic_colsum")
        torch.cuda.synchronize()
    intact(case, A=a, out=out)
    note(A.colsum_check(case, inp, {"out": out.live.cpu()}))


# ---------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("case", A.EMB_CASES, ids=[c.id for c in A.EMB_CASES])
def test_embedding(E, dev, case):
    inp = A.emb_inputs(case)
    ids = inp["ids"].to(dev)
    with guarded_allocs(E):
        emb = E.embedding_fwd(inp["weight"].to(dev), ids)
    note(A.emb_check_fwd(case, inp, {"out": emb.cpu()}))
    dw = put(inp["dw0"], dev)
    with deterministic(E, case.det):
        E.embedding_bwd(inp["dout"].to(dev), ids, case.V, d_weight=dw.live.view(case.V, case.E), zero_first=bool(case.zero_first))
        torch.cuda.synchronize()
    intact(case, d_weight=dw)
    note(A.emb_check_bwd(case, inp, {"dw": dw.live.view(case.V, case.E)}))


def test_ordered_scatter_refuses_more_than_8192_tokens(E, dev):
    case = A.EMB_REFUSED
    inp = A.emb_inputs(case)
    dw = put(inp["dw0"], dev)
    with deterministic(E, True):
        with pytest.raises(NotImplementedError, match=re.escape(A.SCATTER_REFUSAL.format(n=case.n, V=case.V))):
            E.embedding_bwd(inp["dout"].to(dev), inp["ids"].to(dev), case.V, d_weight=dw.live.view(case.V, case.E), zero_first=False)
        torch.cuda.synchronize()
    intact(case, d_weight=dw)
    A.same_bits("det_scatter", case.id, "d_weight after the refused call", dw.live.cpu().view(case.V, case.E), inp["dw0"])


# ---------------------------------------------------------------------------------------------------------------- bn_stats
@pytest.mark.parametrize("case", A.STATS_CASES, ids=[c.id for c in A.STATS_CASES])
def test_bn_stats(dev, case):
    inp = A.stats_inputs(case)
    n = C.c_int64(0)
    L.check(L.load().gic_bn_stats_slab_floats(case.rows, case.C, C.byref(n)), "gic_bn_stats_slab_floats")
    assert n.value == A.stats_parts(case.rows, case.C)[4] * 2 * case.C
    y = put(inp["y"], dev)
    slab, stats = fresh(n.value, 1, torch.float32, dev), fresh(2 * case.C, 1, torch.float32, dev)
    L.check(L.load().gic_bn_stats(y.live.data_ptr(), DT[case.dtype], case.rows, case.C, slab.live.data_ptr(), stats.live.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "gic_bn_stats")
    torch.cuda.synchronize()
    intact(case, y=y, slab=slab, stats=stats)
    assert not bool(torch.isnan(slab.live).any()), "a slab entry was left unwritten"
    note(A.stats_check(case, inp, {"stats": stats.live.cpu()}))


def test_bn_stats_refuses_channels_off_the_8_column_groups(dev):
    y, slab, stats = fresh(4, 12, torch.float32, dev, 1.0), fresh(64, 1, torch.float32, dev), fresh(24, 1, torch.float32, dev)
    with pytest.raises(ValueError, match=re.escape("bn_stats: C = 12 is not a multiple of 8")):
        L.check(L.load().gic_bn_stats(y.live.data_ptr(), L.F32, 4, 12, slab.live.data_ptr(), stats.live.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "gic_bn_stats")
    torch.cuda.synchronize()
    assert bool(torch.isnan(stats.live).all()) and bool(torch.isnan(slab.live).all()) and slab.guards_intact() and stats.guards_intact()


# ---------------------------------------------------------------------------------------------------------------- bn1d
@pytest.mark.parametrize("case", A.BN1D_CASES, ids=[c.id for c in A.BN1D_CASES])
def test_bn1d(dev, case):
    inp = A.bn1d_inputs(case)
    B, E_ = case.B, case.E
    f = torch.float32
    x, gamma, beta, dy = (put(inp[k], dev) for k in ("x", "gamma", "beta", "dy"))
    rm, rv = put(inp["rm0"], dev), put(inp["rv0"], dev)
    y, xhat, invstd = fresh(B, E_, f, dev), fresh(B, E_, f, dev), fresh(E_, 1, f, dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda g: g.live.data_ptr()
    L.check(L.load().gic_bn1d_fwd(p(x), p(gamma), p(beta), p(rm), p(rv), case.training, case.momentum, A.BN_EPS, p(y), p(xhat), p(invstd), B, E_, s),
            "gic_bn1d_fwd")
    dx, dgamma, dbeta = fresh(B, E_, f, dev), fresh(E_, 1, f, dev), fresh(E_, 1, f, dev)
    L.check(L.load().gic_bn1d_bwd(p(dy), p(xhat), p(invstd), p(gamma), case.training, p(dx), p(dgamma), p(dbeta), B, E_, s), "gic_bn1d_bwd")
    torch.cuda.synchronize()
    intact(case, x=x, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv, y=y, xhat=xhat, invstd=invstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    mat = lambda g: g.live.cpu().reshape(B, E_)
    saved = {"y": mat(y), "xhat": mat(xhat), "invstd": invstd.live.cpu(), "rm": rm.live.cpu(), "rv": rv.live.cpu()}
    note(A.bn1d_check_fwd(case, inp, saved))
    note(A.bn1d_check_bwd(case, inp, saved, {"dx": mat(dx), "dgamma": dgamma.live.cpu(), "dbeta": dbeta.live.cpu()}))
