"""gic_xent_seq on the GPU against the float64 CPU oracle (tests/xent_seq_oracle.py): every case calls the C entry point on buffers with
guard words behind them and a NaN-prefilled gradient, so the buffer edges are checked everywhere.  The rows kernel has one variant for
every V (no threshold): a row is split by its address into scalars up to the 16-byte boundary, whole vectors and a scalar rest, so the
shapes and base offsets below cover rows that are aligned, misaligned, shorter than a vector and spread over several passes.

Tolerances (outputs are f32 whatever the input dtype): row_nll / cap_nll rtol = atol = 1e-4; loss rel 1e-5; counts exact; gradient
|err| <= r |ref| + 1e-6 max|w| / count with r = 1e-4 (f32) or 2^-8 (bf16: one output rounding is 2^-9 relative, taken with a factor 2)."""
import math

import pytest
import torch

from tests import xent_seq_oracle as XO

pytestmark = pytest.mark.gpu

GUARD = 8
F_GUARD, I_GUARD = 12345.0, -77
DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(2, 3, 50), (3, 5, 1001), (2, 2, 4), (2, 2, 1), (4, 7, 10000)]
PAD = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(n, dtype, dev, fill, guard, off=0):
    buf = torch.full((off + n + GUARD,), fill, dtype=dtype, device=dev)
    buf[off + n:] = guard
    return buf


def _run(dev, x, t, group, lengths=None, ignore=-100, eps=0.0, w=None, grad=True, xoff=0, doff=0):
    """One gic_xent_seq call on ``x`` [rows, V] (a CPU tensor of the kernel's dtype; ``xoff`` / ``doff`` = element offsets of the logits /
    gradient rows inside their allocations).  Returns the outputs on the CPU after checking every guard word."""
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.engine import ptr, stream_ptr
    rows, V = x.shape
    caps = rows // group
    xbuf = torch.zeros(xoff + rows * V, dtype=x.dtype, device=dev)
    xbuf[xoff:] = x.reshape(-1).to(dev)
    xd = xbuf[xoff:]
    td = t.to(dev)
    ld = None if lengths is None else lengths.to(dev).to(torch.int32)
    wd = None if w is None else w.to(dev).float()
    loss = _guarded(2, torch.float32, dev, float("nan"), F_GUARD)
    row_nll = _guarded(rows, torch.float32, dev, float("nan"), F_GUARD)
    row_ws = _guarded(rows, torch.float32, dev, float("nan"), F_GUARD)
    cap_nll = _guarded(caps, torch.float32, dev, float("nan"), F_GUARD)
    cap_tokens = _guarded(caps, torch.int32, dev, -1, I_GUARD)
    dl = _guarded(rows * V, x.dtype, dev, float("nan"), F_GUARD, off=doff) if grad else None
    dt = L.F32 if x.dtype == torch.float32 else L.BF16
    L.check(L.load().gic_xent_seq(ptr(xd), dt, rows, V, ptr(td), group, ptr(ld), int(ignore), float(eps), ptr(wd), ptr(loss), ptr(row_nll),
                                  ptr(row_ws), ptr(cap_nll), ptr(cap_tokens), None if dl is None else ptr(dl[doff:]), stream_ptr()),
            "gic_xent_seq")
    torch.cuda.synchronize()
    for name, buf, n, g in (("loss", loss, 2, F_GUARD), ("row_nll", row_nll, rows, F_GUARD), ("row_ws", row_ws, rows, F_GUARD),
                            ("cap_nll", cap_nll, caps, F_GUARD), ("cap_tokens", cap_tokens, caps, I_GUARD)):
        assert bool((buf[n:] == g).all()), f"guard words behind {name} were written"
    out = {"loss": loss[0].cpu(), "count": loss[1].cpu(), "row_nll": row_nll[:rows].cpu(), "cap_nll": cap_nll[:caps].cpu(),
           "cap_tokens": cap_tokens[:caps].cpu(), "d_logits": None}
    if grad:
        assert bool((dl[doff + rows * V:].float() == torch.tensor(F_GUARD, dtype=x.dtype).float()).all()), "guard words behind d_logits were written"
        assert bool(torch.isnan(dl[:doff]).all()), "words in front of d_logits were written"
        out["d_logits"] = dl[doff:doff + rows * V].view(rows, V).cpu()
    return out


def _check(out, ref, dtype, w=None, grad=True):
    assert out["cap_tokens"].tolist() == ref["cap_tokens"].tolist()
    assert float(out["count"]) == ref["count"]
    assert torch.allclose(out["row_nll"].double(), ref["row_nll"], rtol=1e-4, atol=1e-4), (out["row_nll"].double() - ref["row_nll"]).abs().max()
    assert torch.allclose(out["cap_nll"].double(), ref["cap_nll"], rtol=1e-4, atol=1e-4), (out["cap_nll"].double() - ref["cap_nll"]).abs().max()
    assert float(out["loss"]) == pytest.approx(float(ref["loss"]), rel=1e-5)
    if not grad:
        return
    got, want = out["d_logits"].double(), ref["d_logits"]
    assert not torch.isnan(got).any()
    m = ref["cap_tokens"].sum() > 0
    wmax = 1.0 if w is None else float(w.abs().max())
    r = 1e-4 if dtype == torch.float32 else 2.0 ** -8
    bound = r * want.abs() + (1e-6 * wmax / ref["count"] if m else 0.0)
    err = (got - want).abs()
    assert bool((err <= bound).all()), (float(err.max()), float((err - bound).max()))
    zero_rows = (want == 0).all(1)
    assert bool((out["d_logits"][zero_rows] == 0).all())                  # exact zeros over the NaN prefill in every uncounted row


def _problem(B, Lc, V, dtype, seed, scale=2.0, pads=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * Lc, V, generator=g) * scale).to(dtype)
    t = torch.randint(0, V, (B * Lc,), generator=g)
    if pads and V > 1:
        t[torch.rand(B * Lc, generator=g) < 0.3] = PAD
        t[0] = PAD
        t[1] = max(V - 1, 1) if V > 1 else 0
    return x, t


def _lengths(B, Lc):
    return torch.tensor(([7, 4, 1, 0] if (B, Lc) == (4, 7) else [Lc - 1, 0] + [Lc] * (B - 2))[:B], dtype=torch.int32)


# ---------------------------------------------------------------- shapes and base offsets
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(dev, shape, dtype):
    B, Lc, V = shape
    x, t = _problem(B, Lc, V, dtype, seed=V + B, pads=False)
    for eps in (0.0, 0.1):
        out = _run(dev, x, t, Lc, eps=eps)
        _check(out, XO.xent_seq(x, t, Lc, smoothing=eps), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("offs", [(1, 1), (3, 2), (0, 5), (4, 0)], ids=lambda o: f"x{o[0]}d{o[1]}")
@pytest.mark.parametrize("shape", [(2, 3, 50), (3, 5, 1001), (2, 3, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_rows_that_start_off_the_16_byte_boundary(dev, shape, offs, dtype):
    """The logits and the gradient start ``offs`` elements into their allocations: heads and tails of every length, and a gradient row
    aligned differently from its logits row (scalar stores)."""
    B, Lc, V = shape
    x, t = _problem(B, Lc, V, dtype, seed=11 + V)
    lengths = _lengths(B, Lc)
    out = _run(dev, x, t, Lc, lengths=lengths, ignore=PAD, eps=0.1, xoff=offs[0], doff=offs[1])
    _check(out, XO.xent_seq(x, t, Lc, lengths=lengths, ignore_index=PAD, smoothing=0.1), dtype)


# ---------------------------------------------------------------- masks and options
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mode", ["lengths", "ignore", "both", "neither", "weights"])
@pytest.mark.parametrize("shape", [(4, 7, 10000), (2, 3, 50)], ids=lambda s: "x".join(map(str, s)))
def test_masks_and_options(dev, shape, mode, eps, dtype):
    B, Lc, V = shape
    x, t = _problem(B, Lc, V, dtype, seed=3 * V + Lc)
    lengths = _lengths(B, Lc) if mode in ("lengths", "both", "weights") else None
    ignore = PAD if mode in ("ignore", "both", "weights") else -100
    w = torch.randn(B * Lc, generator=torch.Generator().manual_seed(9)) if mode == "weights" else None
    if w is not None:
        assert bool((w < 0).any())
    out = _run(dev, x, t, Lc, lengths=lengths, ignore=ignore, eps=eps, w=w)
    ref = XO.xent_seq(x, t, Lc, lengths=lengths, ignore_index=ignore, smoothing=eps, row_weight=w)
    if lengths is not None:
        assert 0 in ref["cap_tokens"].tolist()                            # a caption with nothing counted
    _check(out, ref, dtype, w=w)


def test_weights_without_a_mask_and_group_of_all_rows(dev):
    x, t = _problem(3, 5, 1001, torch.float32, seed=2)
    w = torch.randn(15, generator=torch.Generator().manual_seed(4))
    _check(_run(dev, x, t, 15, eps=0.1, w=w), XO.xent_seq(x, t, 15, smoothing=0.1, row_weight=w), torch.float32, w=w)
    lengths = torch.tensor([9], dtype=torch.int32)                        # lengths with group == rows
    _check(_run(dev, x, t, 15, lengths=lengths), XO.xent_seq(x, t, 15, lengths=lengths), torch.float32)
    _check(_run(dev, x, t, 1, grad=False), XO.xent_seq(x, t, 1), torch.float32, grad=False)


# ---------------------------------------------------------------- large logits
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_logits_so_spread_that_exp_underflows(dev, eps, dtype):
    B, Lc, V = 3, 5, 1001
    g = torch.Generator().manual_seed(21)
    x = ((torch.rand(B * Lc, V, generator=g) * 2 - 1) * 80.0).to(dtype)
    t = torch.randint(0, V, (B * Lc,), generator=g)
    assert float(torch.exp(x.float().min() - x.float().max())) == 0.0     # exp underflows in f32
    _check(_run(dev, x, t, Lc, eps=eps), XO.xent_seq(x, t, Lc, smoothing=eps), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_constant_1e4_added_to_every_logit_of_a_row(dev, eps, dtype):
    """nll = (max - x_t) + log sum exp(x - max): with lse formed as one f32 number the offset would cost three digits."""
    B, Lc, V = 3, 5, 1001
    x, t = _problem(B, Lc, V, torch.float32, seed=31)
    x[::2] += 1e4
    x = x.to(dtype)
    _check(_run(dev, x, t, Lc, ignore=PAD, eps=eps), XO.xent_seq(x, t, Lc, ignore_index=PAD, smoothing=eps), dtype)


# ---------------------------------------------------------------- empty batch, bad target
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_empty_batch_gives_zero_loss_and_zero_gradient(dev, dtype):
    x, _ = _problem(2, 3, 50, dtype, seed=1)
    t = torch.full((6,), PAD, dtype=torch.int64)
    for kw in (dict(ignore=PAD), dict(lengths=torch.zeros(2, dtype=torch.int32))):
        out = _run(dev, x, t, 3, eps=0.1, **kw)
        assert float(out["loss"]) == 0.0 and float(out["count"]) == 0.0
        assert bool((out["d_logits"] == 0).all()) and bool((out["row_nll"] == 0).all()) and bool((out["cap_nll"] == 0).all())
        assert out["cap_tokens"].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_counted_target_outside_the_vocabulary_poisons_the_loss(dev, dtype):
    B, Lc, V = 2, 3, 50
    x, t = _problem(B, Lc, V, dtype, seed=8, pads=False)
    t[4] = V
    out = _run(dev, x, t, Lc)
    ref = XO.xent_seq(x, t, Lc)
    assert math.isnan(float(out["loss"])) and float(out["count"]) == 6.0
    assert math.isnan(float(out["row_nll"][4])) and math.isnan(float(out["cap_nll"][1]))
    ok = torch.arange(6) != 4
    assert torch.allclose(out["row_nll"][ok].double(), ref["row_nll"][ok], rtol=1e-4, atol=1e-4)
    assert float(out["cap_nll"][0]) == pytest.approx(float(ref["cap_nll"][0]), rel=1e-4)
    # the same target is fine when it is not counted
    t2 = t.clone()
    out = _run(dev, x, t2, Lc, ignore=V)
    _check(out, XO.xent_seq(x, t2, Lc, ignore_index=V), dtype)
    t2[4] = -5
    _check(_run(dev, x, t2, Lc, lengths=torch.tensor([3, 1], dtype=torch.int32)),
           XO.xent_seq(x, t2, Lc, lengths=torch.tensor([3, 1], dtype=torch.int32)), dtype)


# ---------------------------------------------------------------- the old kernel, reproducibility, the engine wrapper
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(4, 7, 10000), (2, 3, 50)], ids=lambda s: "x".join(map(str, s)))
def test_same_job_as_gic_xent(dev, shape, dtype):
    from gan_image_captioning_amd import engine
    B, Lc, V = shape
    x, t = _problem(B, Lc, V, dtype, seed=5 + V)
    old_loss, old_dl = engine.xent(x.to(dev), t.to(dev))
    new = engine.xent_seq(x.to(dev), t.to(dev), Lc)
    assert float(new["loss"]) == pytest.approx(float(old_loss[0]), rel=1e-6)
    assert float(new["count"]) == B * Lc
    r = 1e-4 if dtype == torch.float32 else 2.0 ** -8
    got, want = new["d_logits"].double().cpu(), old_dl.double().cpu()
    assert bool(((got - want).abs() <= r * want.abs() + 1e-6 / (B * Lc)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_two_calls_and_both_determinism_modes_give_the_same_bits(dev, dtype):
    from gan_image_captioning_amd import engine
    B, Lc, V = 4, 7, 10000
    x, t = _problem(B, Lc, V, dtype, seed=77)
    xd, td = x.to(dev), t.to(dev)
    lengths = _lengths(B, Lc).to(dev)
    w = torch.randn(B * Lc, generator=torch.Generator().manual_seed(9)).to(dev)
    call = lambda: engine.xent_seq(xd, td, Lc, lengths=lengths, ignore_index=PAD, smoothing=0.1, row_weight=w)      # noqa: E731
    was = engine.deterministic()
    try:
        engine.set_deterministic(False)
        a, b = call(), call()
        engine.set_deterministic(True)
        c = call()
    finally:
        engine.set_deterministic(was)
    for k in ("loss", "count", "row_nll", "cap_nll", "cap_tokens", "d_logits"):
        for other in (b, c):
            assert torch.equal(a[k], other[k]), k


def test_engine_wrapper_returns_the_entry_points_outputs(dev):
    from gan_image_captioning_amd import engine
    B, Lc, V = 3, 5, 1001
    x, t = _problem(B, Lc, V, torch.float32, seed=13)
    lengths = _lengths(B, Lc)
    raw = _run(dev, x, t, Lc, lengths=lengths, ignore=PAD, eps=0.1)
    out = engine.xent_seq(x.to(dev), t.to(dev), Lc, lengths=lengths.to(dev), ignore_index=PAD, smoothing=0.1)
    for k in ("loss", "count", "row_nll", "cap_nll", "cap_tokens", "d_logits"):
        assert torch.equal(out[k].cpu(), raw[k]), k
    assert out["loss"].shape == () and out["cap_tokens"].dtype == torch.int32
    assert engine.xent_seq(x.to(dev), t.to(dev), Lc, want_grad=False)["d_logits"] is None
    with pytest.raises(ValueError, match="group"):
        engine.xent_seq(x.to(dev), t.to(dev), 4)
    with pytest.raises(ValueError, match="smoothing"):
        engine.xent_seq(x.to(dev), t.to(dev), Lc, smoothing=1.0)
    with pytest.raises(ValueError, match="lengths"):
        engine.xent_seq(x.to(dev), t.to(dev), Lc, lengths=lengths[:2].to(dev))
