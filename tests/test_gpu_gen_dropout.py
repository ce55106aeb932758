"""Output dropout of the caption decoder on the GPU (csrc/gen_dropout.hip, the gic_*_drop entry points of csrc/teacher_forced.hip,
Decoder / AttnDecoder .forward / .forward_scheduled with ``dropout``, --gen-dropout) against tests/gen_dropout_oracle.py.

Shapes: B = 3, captions of 6 columns (T = 7) with lengths [6, 3, 1], so Tmax = 6 < T; V in {37, 64}.  LSTM decoder with (E, H, NL) in
{(32, 64, 1): the fused step kernels and the 16-byte dropout form in both dtypes; (24, 36, 2): the generic products, the 16-byte form
in f32 and the scalar one in bf16; (24, 30, 1): H % 4 != 0, which check_decoder_dims accepts -- the scalar form in both dtypes}.
Attention decoder with P = 9, A = 16 and H in {64, 40}: check_attn_dims refuses every H that is not a multiple of 8 (asserted for
the H = 36 of the LSTM cases in tests/test_gen_dropout_api.py), so its decode reaches the 16-byte form only and the scalar form is
covered by the LSTM decoder and by gic_hidden_dropout.  The tensor-level call has no step argument; that the per-step launches of the scheduled-sampling decode draw what the
all-rows launch draws is asserted inside the decode (every hdrop is compared with the host map, which knows no steps).

Tolerances are those of the plain teacher-forced tests for the same quantities: f32 outputs rtol 1e-4, gradients rtol 2e-3 with an
absolute floor of 1e-4 of the largest entry (tests/test_gpu_attn_tf.py, tests/test_gpu_kernels.py); bf16 relative L2 -- LSTM decoder
logits / h_n / c_n 2e-2 and gradients 6e-2 (test_gpu_kernels.py, the teacher-forced golden tests), attention decoder pred / alphas 5e-2 and
gradients 1e-1 (test_gpu_attn_tf.py::test_bf16_at_cfg4_shapes).  Two training steps of the attention decoder run outside the deterministic
mode (its scheduled-sampling entry is refused there): their spread is held to the 1e-3 relative L2 that tests/test_gpu_attention.py allows
a pass through the trunk's f32-atomic BatchNorm sums, while the mask itself, a function of the seed alone, must agree exactly."""
import numpy as np
import pytest
import torch

from oracle import cpu_step as O
from tests import attn_beam_oracle as AO
from tests import gen_dropout_oracle as GD
from tests.gpu_util import Guarded, close, dec_param_names, dec_params, rel_l2

pytestmark = pytest.mark.gpu

B, LC, LENS = 3, 6, [6, 3, 1]
TMAX = max(LENS)
LSTM_SHAPES = [(64, 32, 64, 1), (37, 24, 36, 2), (37, 24, 30, 1)]          # V, E, H, NL
ATTN_SHAPES = [(64, 32, 64), (64, 32, 40)]                                  # V, E, H; C = 16, P = 9, A = 16
ATTN_C, ATTN_P, ATTN_A = 16, 9, 16
ATTN_NAMES = ["decoder." + n for n in AO.NAMES]
PS = [0.5, 0.1]
SEED = 0x5EED_0000_1234_ABCD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _keep(seed, shape, p):
    n = int(np.prod(shape[:-1]))
    return torch.from_numpy(GD.dropout_keep(seed, n, 1, shape[-1], p).reshape(shape))


def _u(seed, shape):
    n = int(np.prod(shape[:-1]))
    return torch.from_numpy(GD.dropout_u(seed, n, 1, shape[-1]).reshape(shape))


def _bits_equal(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    g, w = got.contiguous().view(it), want.contiguous().view(it)
    zero = (got == 0) & (want == 0)                                 # a dropped -x and a kept -0 * s are both zero
    assert bool(((g == w) | zero).all()), f"{what}: {int(((g != w) & ~zero).sum())} of {g.numel()} elements differ"


# ================================================================================================ 1. the stage, bit-exact
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("rows,H", [(18, 64), (18, 36), (18, 30), (5, 7), (3, 2)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_hidden_dropout_matches_the_host_map(dev, dt, rows, H, off, p):
    from gan_image_captioning_amd import engine
    g = torch.Generator().manual_seed(rows * 1000 + H)
    x = (torch.randn(rows, H, generator=g) * 3).to(dt)
    x[0, 0] = -0.0
    src, dst = Guarded(rows, H, dt, dev, 0.0, off), Guarded(rows, H, dt, dev, 7.0, off)
    src.live.copy_(x)
    assert src.live.data_ptr() % 16 == (off * x.element_size()) % 16 and src.live.is_contiguous()
    y = engine.hidden_dropout(src.live, p, seed=SEED, out=dst.live)
    torch.cuda.synchronize()
    assert y is dst.live and dst.guards_intact() and src.guards_intact()
    want = GD.apply(x, _keep(SEED, (rows, H), p), p)
    _bits_equal(y, want, "device draw")
    _bits_equal(src.live, x, "the input is left alone")
    # the same uniforms given: the same bits, from an aligned and from a misaligned keep_u
    u = _u(SEED, (rows, H))
    for uoff in (0, 1):
        ub = Guarded(rows, H, torch.float32, dev, 0.0, uoff)
        ub.live.copy_(u)
        dst.live.fill_(7.0)
        engine.hidden_dropout(src.live, p, seed=SEED + 1, keep_u=ub.live, out=dst.live)
        torch.cuda.synchronize()
        assert dst.guards_intact()
        _bits_equal(dst.live, want, f"keep_u (offset {uoff})")
    # default output, and a leading shape [B, T, H] is the [rows, H] view
    if off == 0 and rows == 18:
        y3 = engine.hidden_dropout(src.live.view(3, 6, H), p, seed=SEED)
        torch.cuda.synchronize()
        _bits_equal(y3.view(rows, H), want, "[B, T, H]")


def test_hidden_dropout_more_items_than_the_grid(dev):
    """4100 x 512 f32: 524 800 16-byte pieces against 2048 x 256 threads -- the grid-stride loop takes a second turn."""
    from gan_image_captioning_amd import engine
    rows, H, p = 4100, 512, 0.5
    x = torch.randn(rows, H, generator=torch.Generator().manual_seed(1))
    y = engine.hidden_dropout(x.to(dev), p, seed=SEED)
    torch.cuda.synchronize()
    _bits_equal(y, GD.apply(x, _keep(SEED, (rows, H), p), p), "large")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("H", [64, 36, 30, 7])
def test_hidden_dropout_bwd_matches_the_host_formula(dev, H, off, p):
    from gan_image_captioning_amd import engine
    g = torch.Generator().manual_seed(H)
    d = torch.randn(B, TMAX, H, generator=g)
    buf = Guarded(B * TMAX, H, torch.float32, dev, 0.0, off)
    buf.live.copy_(d.view(B * TMAX, H))
    view = buf.live.view(B, TMAX, H)
    want = GD.apply_bwd(d, _keep(SEED, (B, TMAX, H), p), LENS, p)
    assert (want[1, 3:] == 0).all() and (want[2, 1:] == 0).all() and (want[0] != 0).any()
    got = engine.hidden_dropout_bwd(view, LENS, p, seed=SEED)
    torch.cuda.synchronize()
    assert got is view and buf.guards_intact()
    _bits_equal(got, want, "device draw")
    buf.live.copy_(d.view(B * TMAX, H))
    engine.hidden_dropout_bwd(view, torch.tensor(LENS), p, seed=3, keep_u=_u(SEED, (B, TMAX, H)).to(dev))
    torch.cuda.synchronize()
    assert buf.guards_intact()
    _bits_equal(view, want, "keep_u")


# ================================================================================================ problems
def _lstm_problem(shape, seed=5):
    V, E, H, NL = shape
    g = torch.Generator().manual_seed(seed)
    gp = {k: v * 4 for k, v in O.make_gen_params(V, E, H, NL, g).items()}
    feats = torch.randn(B, E, generator=g) * 0.5
    caps = torch.randint(0, V, (B, LC), generator=g)
    return gp, feats, caps


def _attn_problem(shape, seed=6):
    V, E, H = shape
    params, feats, fmap = AO.random_problem(B, V, E, H, ATTN_C, ATTN_P, ATTN_A, seed=seed)
    caps = torch.randint(0, V, (B, LC), generator=torch.Generator().manual_seed(seed + 1))
    return params, feats, fmap, caps


def _lstm_engine(shape, dt):
    from gan_image_captioning_amd import engine
    return engine.DecoderEngine(*shape, dt)


def _attn_engine(shape, dt):
    from gan_image_captioning_amd import engine
    return engine.AttnDecoderEngine(*shape, ATTN_C, ATTN_P, ATTN_A, dt)


def _saved_hout(saved, H):
    return saved["st"]["hout"].reshape(-1)[:B * TMAX * H].view(B, TMAX, H)


def _check_hdrop(saved, H, keep, p, what):
    """hdrop = apply(hout) bit for bit, zero past every length, and really dropped."""
    d = saved["drop"]
    hout, hdrop = _saved_hout(saved, H).cpu(), d["hdrop"].cpu()
    _bits_equal(hdrop, GD.apply(hout, keep, p), what)
    live = torch.arange(TMAX)[None] < torch.tensor(LENS)[:, None]
    assert (hdrop[~live] == 0).all() and (hout[~live] == 0).all(), what
    assert ((hdrop[live] == 0) != (hout[live] == 0)).any() and (hdrop[live] != 0).any(), what
    return hout, hdrop


# ================================================================================================ 2. inside the decode, bit-exact
@pytest.mark.parametrize("given", [False, True], ids=["draw", "keep_u"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=lambda s: "V%d-E%d-H%d-NL%d" % s)
def test_lstm_decode_writes_the_dropped_rows(dev, shape, dt, p, given):
    V, E, H, NL = shape
    gp, feats, caps = _lstm_problem(shape)
    eng, params = _lstm_engine(shape, dt), dec_params(gp, dev)
    u = torch.rand(B, TMAX, H, generator=torch.Generator().manual_seed(8))
    keep = GD.keep_of(u, p) if given else _keep(SEED, (B, TMAX, H), p)
    kw = dict(dropout=p, dropout_seed=SEED, keep_u=u.to(dev) if given else None)
    pred, (h_n, c_n), saved = eng.forward_tf(params, feats.to(dev), caps.to(dev), LENS, 1.0, pretrain=True, keep_state=True, **kw)
    torch.cuda.synchronize()
    assert set(saved["drop"]) == {"p", "seed", "keep_u", "hdrop"} and saved["drop"]["hdrop"].dtype == eng.act
    _, hd_tf = _check_hdrop(saved, H, keep, p, "forward_tf")
    # scheduled sampling: the same map, drawn step by step; coins at 1 replace nothing, coins at 0 replace every live position
    for coin in (1.0, 0.0):
        out = eng.forward_scheduled(params, feats.to(dev), caps.to(dev), LENS, 0.5, "sample", torch.full((B, LC), coin, device=dev), None, 3, **kw)
        torch.cuda.synchronize()
        hout_ss, hd_ss = _check_hdrop(out[2], H, keep, p, f"forward_scheduled coin {coin}")
        assert bool(out[4].any()) == (coin == 0.0)
        if coin == 1.0:                                            # the teacher's inputs: the rows the all-rows launch saw
            close(hout_ss.float(), _saved_hout(saved, H).float(), rtol=1e-5 if dt == 0 else 2e-2, what="hout of the two decodes")
            assert torch.equal(hd_ss == 0, hd_tf == 0)


@pytest.mark.parametrize("given", [False, True], ids=["draw", "keep_u"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "V%d-E%d-H%d" % s)
def test_attn_decode_writes_the_dropped_rows(dev, shape, dt, p, given):
    V, E, H = shape
    params, feats, fmap, caps = _attn_problem(shape)
    eng, pd = _attn_engine(shape, dt), [q.to(dev) for q in params]
    u = torch.rand(B, TMAX, H, generator=torch.Generator().manual_seed(9))
    keep = GD.keep_of(u, p) if given else _keep(SEED, (B, TMAX, H), p)
    kw = dict(dropout=p, dropout_seed=SEED, keep_u=u.to(dev) if given else None)
    pred, _, alphas, saved = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), LENS, 1.0, pretrain=True, want_alphas=True,
                                            keep_state=True, **kw)
    torch.cuda.synchronize()
    _, hd_tf = _check_hdrop(saved, H, keep, p, "forward_tf")
    for coin in (1.0, 0.0):
        out = eng.forward_scheduled(pd, feats.to(dev), fmap.to(dev), caps.to(dev), LENS, 0.5, "sample", torch.full((B, LC), coin, device=dev),
                                    None, 3, **kw)
        torch.cuda.synchronize()
        _, hd_ss = _check_hdrop(out[3], H, keep, p, f"forward_scheduled coin {coin}")
        assert bool(out[5].any()) == (coin == 0.0)
        if coin == 1.0:
            assert torch.equal(hd_ss == 0, hd_tf == 0)


# ================================================================================================ 3. against the float64 oracle
def _lstm_oracle(gp, feats, caps, keep, p, d_pred):
    names = dec_param_names(O.num_lstm_layers(gp))
    leaf = {n: gp[n].double().clone().requires_grad_(True) for n in names}
    f = feats.double().clone().requires_grad_(True)
    pred, (h_n, c_n) = GD.lstm_forward_tf(leaf, f, caps, LENS, keep, p)
    (pred * d_pred.double()).sum().backward()
    return pred.detach(), h_n.detach(), c_n.detach(), [leaf[n].grad for n in names] + [f.grad], names + ["d_features"]


def _attn_oracle(params, feats, fmap, caps, keep, p, d_pred, d_alphas):
    leaf = {n: q.double().clone().requires_grad_(True) for n, q in zip(ATTN_NAMES, params)}
    f = feats.double().clone().requires_grad_(True)
    pred, (h_n, c_n), alphas = GD.attn_forward_tf(leaf, f, fmap.double(), caps, LENS, keep, p)
    loss = (pred * d_pred.double()).sum()
    if d_alphas is not None:
        loss = loss + (alphas * d_alphas.double()).sum()
    loss.backward()
    return pred.detach(), h_n.detach(), c_n.detach(), alphas.detach(), [leaf[n].grad for n in ATTN_NAMES] + [f.grad], ATTN_NAMES + ["d_features"]


def _compare(dt, outs, grads, out_bar, grad_bar):
    """outs / grads: (name, got, want) triples.  f32: the element-wise tolerances of the plain tests; bf16: their relative-L2 bars."""
    for n, got, want in outs:
        print(f"{n}: rel-L2 {rel_l2(got.float(), want):.2e}")
        if dt == 0:
            close(got, want, rtol=1e-4, atol_scale=1e-5, what=n)
        else:
            assert rel_l2(got.float(), want) < out_bar, (n, rel_l2(got.float(), want))
    for n, got, want in grads:
        print(f"{n}: rel-L2 {rel_l2(got, want):.2e}")
        if dt == 0:
            close(got, want, rtol=2e-3, atol_scale=1e-4, what=n)
        else:
            assert rel_l2(got, want) < grad_bar, (n, rel_l2(got, want))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=lambda s: "V%d-E%d-H%d-NL%d" % s)
def test_lstm_decode_matches_oracle(dev, shape, dt, p):
    V, E, H, NL = shape
    gp, feats, caps = _lstm_problem(shape)
    g = torch.Generator().manual_seed(21)
    u = torch.rand(B, TMAX, H, generator=g)
    d_pred = torch.randn(B, TMAX, V, generator=g) * 0.1
    keep = GD.keep_of(u, p)
    want, h_w, c_w, g_w, names = _lstm_oracle(gp, feats, caps, keep, p, d_pred)
    eng, params = _lstm_engine(shape, dt), dec_params(gp, dev)
    pred, (h_n, c_n), saved = eng.forward_tf(params, feats.to(dev), caps.to(dev), LENS, 1.0, pretrain=True, keep_state=True, dropout=p,
                                             keep_u=u.to(dev))
    grads = eng.forward_tf_bwd(params, saved, pred, d_pred.to(dev), 1.0, True)
    torch.cuda.synchronize()
    _compare(dt, [("pred", pred, want), ("h_n", h_n, h_w), ("c_n", c_n, c_w)], list(zip(names, grads, g_w)), 2e-2, 6e-2)
    # the backward's own keywords stand in for what saved carries: the same mask by another route gives the same gradients
    again = eng.forward_tf_bwd(params, saved, pred, d_pred.to(dev), 1.0, True, dropout=p, dropout_seed=99, keep_u=u.to(dev))
    torch.cuda.synchronize()
    for n, a, b in zip(names, again, grads):              # (two runs of the f32 backward: its atomic sums may reorder)
        close(a, b, rtol=1e-4, atol_scale=1e-5, what=n)


# every (shape, dtype, p) with a loss on pred; the loss on the alphas is carried by one shape and one p per dtype
ATTN_ORACLE_CASES = [(s, dt, p, False) for s in ATTN_SHAPES for dt in (0, 1) for p in PS] + [(ATTN_SHAPES[0], dt, 0.5, True) for dt in (0, 1)]


@pytest.mark.parametrize("shape,dt,p,with_alphas", ATTN_ORACLE_CASES,
                         ids=["H%d-%s-p%s-%s" % (c[0][2], ("f32", "bf16")[c[1]], c[2], ("pred", "pred+alphas")[c[3]]) for c in ATTN_ORACLE_CASES])
def test_attn_decode_matches_oracle(dev, shape, dt, p, with_alphas):
    V, E, H = shape
    params, feats, fmap, caps = _attn_problem(shape)
    g = torch.Generator().manual_seed(22)
    u = torch.rand(B, TMAX, H, generator=g)
    d_pred = torch.randn(B, TMAX, V, generator=g) * 0.1
    d_alphas = torch.randn(B, TMAX, ATTN_P, generator=g) if with_alphas else None
    keep = GD.keep_of(u, p)
    want, h_w, c_w, al_w, g_w, names = _attn_oracle(params, feats, fmap, caps, keep, p, d_pred, d_alphas)
    eng, pd = _attn_engine(shape, dt), [q.to(dev) for q in params]
    pred, (h_n, c_n), alphas, saved = eng.forward_tf(pd, feats.to(dev), fmap.to(dev), caps.to(dev), LENS, 1.0, pretrain=True,
                                                     want_alphas=True, keep_state=True, dropout=p, keep_u=u.to(dev))
    grads = eng.forward_tf_bwd(pd, saved, pred, d_pred.to(dev), 1.0, True, d_alphas=None if d_alphas is None else d_alphas.to(dev))
    torch.cuda.synchronize()
    _compare(dt, [("pred", pred, want), ("alphas", alphas, al_w), ("h_n", h_n[0], h_w), ("c_n", c_n[0], c_w)],
             list(zip(names, grads, g_w)), 5e-2, 1e-1)


def _lstm_module(gp, shape, dt, dev):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Decoder
    V, E, H, NL = shape
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, gen_num_layers=NL, temperature=1,
                        compute_dtype="fp32" if dt == 0 else "bf16", device="cuda")
    dec = Decoder(args).to(dev)
    with torch.no_grad():
        for n, q in zip(dec_param_names(NL), dec.param_list()):
            q.copy_(gp[n])
    dec.temperature = 1.0
    return dec


def _attn_module(params, shape, dt, dev):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import AttnDecoder
    V, E, H = shape
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, attn_dim=ATTN_A, temperature=1, conditional_gan=1,
                        compute_dtype="fp32" if dt == 0 else "bf16", device="cuda")
    dec = AttnDecoder(args, ATTN_C, ATTN_P).to(dev)
    with torch.no_grad():
        for q, w in zip(dec.param_list(), params):
            q.copy_(w)
    dec.temperature = 1.0
    return dec


def test_module_forward_with_dropout_under_autograd(dev):
    """Decoder.forward(..., dropout=p) through autograd: the oracle's gradients, on the parameters themselves."""
    shape, p = LSTM_SHAPES[1], 0.5
    V, E, H, NL = shape
    gp, feats, caps = _lstm_problem(shape)
    g = torch.Generator().manual_seed(23)
    u = torch.rand(B, TMAX, H, generator=g)
    d_pred = torch.randn(B, TMAX, V, generator=g) * 0.1
    want, h_w, c_w, g_w, names = _lstm_oracle(gp, feats, caps, GD.keep_of(u, p), p, d_pred)
    dec = _lstm_module(gp, shape, 0, dev)
    f = feats.to(dev).requires_grad_(True)
    pred, (h_n, c_n) = dec(f, caps.to(dev), LENS, pretrain=True, dropout=p, keep_u=u.to(dev))
    assert pred.requires_grad and not h_n.requires_grad
    (pred * d_pred.to(dev)).sum().backward()
    torch.cuda.synchronize()
    _compare(0, [("pred", pred, want), ("h_n", h_n, h_w), ("c_n", c_n, c_w)],
             list(zip(names, [q.grad for q in dec.param_list()] + [f.grad], g_w)), None, None)
    # the device-drawn mask of a given seed is the host map's
    with torch.no_grad():
        again, _ = dec(feats.to(dev), caps.to(dev), LENS, pretrain=True, dropout=p, dropout_seed=SEED)
    ref, _, _, _, _ = _lstm_oracle(gp, feats, caps, _keep(SEED, (B, TMAX, H), p), p, d_pred)
    torch.cuda.synchronize()
    close(again, ref, rtol=1e-4, atol_scale=1e-5, what="no-grad forward drops too")


# ================================================================================================ 4. what must not change
def _seed_count():
    from gan_image_captioning_amd.generator import SEEDS
    return SEEDS._n


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_dropout_zero_is_the_call_without_it(dev, kind):
    from gan_image_captioning_amd.generator import SEEDS
    if kind == "lstm":
        shape = LSTM_SHAPES[0]
        gp, feats, caps = _lstm_problem(shape)
        dec, maps = _lstm_module(gp, shape, 0, dev), ()
    else:
        shape = ATTN_SHAPES[0]
        params, feats, fmap, caps = _attn_problem(shape)
        dec, maps = _attn_module(params, shape, 0, dev), (fmap.to(dev),)
    dec.temperature = 1.3
    f, c = feats.to(dev), caps.to(dev)
    zero = dict(dropout=0.0, dropout_seed=None, keep_u=None)
    calls = [lambda kw: dec(f, *maps, c, LENS, pretrain=False, **kw),                       # draws its Gumbel noise from SEEDS
             lambda kw: dec(f, *maps, c, LENS, pretrain=True, **kw),
             lambda kw: dec.forward_scheduled(f, *maps, c, LENS, 0.5, return_inputs=True, **kw),
             lambda kw: dec.forward_scheduled(f, *maps, c, LENS, 0.0, **kw)]
    for i, call in enumerate(calls):
        for grad in (False, True):
            outs, counts = [], []
            for kw in ({}, zero):
                SEEDS.reset(40)
                with (torch.enable_grad() if grad else torch.no_grad()):
                    res = call(kw)
                torch.cuda.synchronize()
                flat = [res[0], *res[1]] + ([*res[2]] if len(res) > 2 and isinstance(res[2], tuple) else [])
                outs.append([t.detach().clone() for t in flat])
                counts.append(_seed_count())
            assert counts[0] == counts[1], (i, grad, counts)
            for a, b in zip(*outs):
                assert torch.equal(a, b), (i, grad)
    # ... and a drawn mask takes exactly one more seed, after the call's own
    SEEDS.reset(40)
    with torch.no_grad():
        dec(f, *maps, c, LENS, pretrain=False)
        n_plain = _seed_count()
        SEEDS.reset(40)
        dec(f, *maps, c, LENS, pretrain=False, dropout=0.5)
        assert _seed_count() == n_plain + 1
        SEEDS.reset(40)
        dec(f, *maps, c, LENS, pretrain=False, dropout=0.5, dropout_seed=7)
        assert _seed_count() == n_plain
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_recurrence_is_undropped_and_seeds_decide_the_mask(dev, kind, dt):
    if kind == "lstm":
        shape = LSTM_SHAPES[0]
        gp, feats, caps = _lstm_problem(shape)
        eng, pd, maps = _lstm_engine(shape, dt), dec_params(gp, dev), ()
    else:
        shape = ATTN_SHAPES[0]
        params, feats, fmap, caps = _attn_problem(shape)
        eng, pd, maps = _attn_engine(shape, dt), [q.to(dev) for q in params], (fmap.to(dev),)
    f, c = feats.to(dev), caps.to(dev)

    def run(**kw):
        res = eng.forward_tf(pd, f, *maps, c, LENS, 1.0, pretrain=True, keep_state=True, **kw)
        torch.cuda.synchronize()
        return res[0], res[1], res[-1]
    plain, (h0, c0), s0 = run()
    again, _, _ = run(dropout=0.0, dropout_seed=5, keep_u=None)
    assert torch.equal(plain, again) and "drop" not in s0
    a, (ha, ca), sa = run(dropout=0.5, dropout_seed=5)
    b, (hb, cb), sb = run(dropout=0.5, dropout_seed=5)
    d, (hd, cd), sd = run(dropout=0.5, dropout_seed=6)
    assert torch.equal(ha, h0) and torch.equal(ca, c0) and torch.equal(hd, h0) and torch.equal(cd, c0)      # the recurrence is undropped
    assert torch.equal(a, b) and torch.equal(sa["drop"]["hdrop"], sb["drop"]["hdrop"])
    assert not torch.equal(sa["drop"]["hdrop"], sd["drop"]["hdrop"]) and not torch.equal(a, d) and not torch.equal(a, plain)


# ================================================================================================ 5. the training path
def _args(**kw):
    from gan_image_captioning_amd.args import default_args
    base = dict(vocab_size=64, gen_embed_dim=16, gen_hidden_dim=32, conditional_gan=1, encoder_arch="resnet18", attn_dim=24,
                compute_dtype="fp32", image_size=64, device="cuda", log_file=None, model_dir=None, save_dir=None)
    base.update(kw)
    return default_args(**base)


def _batch(Bt, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(Bt, 3, 64, 64, generator=g)
    caps = O.make_captions(Bt, L, V, g)
    lengths = torch.randint(3, L + 1, (Bt,), generator=g, dtype=torch.int32)
    lengths[0] = L
    for b in range(Bt):                                    # tasks.collate_fn's layout: <S> body <E> then PAD
        n = int(lengths[b])
        caps[b, n - 1] = 2
        caps[b, n:] = 0
    return images, caps, lengths


class _HdropSpy:
    """Every gic_decoder_dropout the engine builds, in call order: the forward's first."""

    def __init__(self, monkeypatch):
        from gan_image_captioning_amd import engine
        self.seen = []
        inner = engine._drop_struct

        def spy(d):
            self.seen.append(d)
            return inner(d)
        monkeypatch.setattr(engine, "_drop_struct", spy)


@pytest.mark.parametrize("ss", [0.0, 0.5], ids=["teacher", "scheduled"])
@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_training_steps_with_gen_dropout(dev, decoder, ss, monkeypatch):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.generator import SEEDS
    from gan_image_captioning_amd.training import GANInstructor
    from tests.step_state import _restore, _snapshot, _state, transplant
    det = decoder == "lstm"                    # the attention decoder's scheduled-sampling entry is refused in the deterministic mode
    was = engine.deterministic()
    engine.set_deterministic(det)
    try:
        torch.manual_seed(11)
        kw = dict(decoder=decoder, pretrain_mode="teacher", scheduled_sampling_prob=ss, deterministic=int(det))
        inst = GANInstructor(_args(gen_dropout=0.5, **kw), None, None)
        assert inst.gen_dropout == 0.5
        with torch.no_grad():
            for q in inst.gen.decoder.parameters():
                q.mul_(8.0)
        inst.gen.train()
        Bt, L, V = 6, 7, 64
        images, caps, lengths = _batch(Bt, L, V, 4)
        images, caps = images.to(dev), caps.to(dev)
        spy = _HdropSpy(monkeypatch)
        snap = _snapshot(inst)

        def two_steps(rank=0):
            _restore(inst, snap)
            SEEDS.rank = rank
            spy.seen.clear()
            losses = []
            try:
                for _ in range(2):
                    with torch.enable_grad():
                        losses.append(inst.pretrain_step(images, caps, L, train=True, lengths=lengths).detach().clone())
                torch.cuda.synchronize()
            finally:
                SEEDS.rank = 0
            assert len(spy.seen) == 4 and all(d["p"] == 0.5 and d["keep_u"] is None for d in spy.seen)      # forward + backward, twice
            assert spy.seen[0]["seed"] == spy.seen[1]["seed"] != spy.seen[2]["seed"]
            return losses, [spy.seen[0]["hdrop"].clone(), spy.seen[2]["hdrop"].clone()], {k: v.detach().clone() for k, v in _state(inst).items()}
        la, ha, sa = two_steps()
        lb, hb, sb = two_steps()
        assert all(torch.isfinite(v).all() for v in la)
        if det:
            assert all(torch.equal(x, y) for x, y in zip(la, lb)) and all(torch.equal(x, y) for x, y in zip(ha, hb))
            for k in sa:
                assert torch.equal(sa[k], sb[k]), k
        else:
            assert torch.equal(ha[0] == 0, hb[0] == 0)             # the mask is the seed's, whatever the sums before it did
            for x, y in zip(la + ha[:1], lb + hb[:1]):
                assert rel_l2(x.float(), y.float()) < 1e-3
        frac = float((ha[0][:, 0] == 0).float().mean())            # step 0 is live in every caption: about half of it is dropped
        assert 0.25 < frac < 0.75, frac
        # another data-parallel rank draws another mask
        lr, hr, _ = two_steps(rank=1)
        assert not torch.equal(hr[0] == 0, ha[0] == 0)
        # a validation step never drops: the bits of an instructor built without the flag, from the same weights
        _restore(inst, snap)
        torch.manual_seed(11)                                      # the trunk's frozen weights are drawn at construction: the same ones
        plain = GANInstructor(_args(gen_dropout=0.0, **kw), None, None)
        transplant(inst, plain)
        vals = []
        for who in (inst, plain):
            who.gen.eval()
            spy.seen.clear()
            SEEDS.reset(70)
            with torch.no_grad():
                vals.append(who.pretrain_step(images, caps, L, train=False, lengths=lengths).detach().clone())
            torch.cuda.synchronize()
            assert spy.seen == []
        assert torch.equal(vals[0], vals[1]) and torch.isfinite(vals[0]).all()
    finally:
        engine.set_deterministic(was)
        SEEDS.rank = 0
