"""Output dropout of the caption decoder without a GPU: the eight C ABI symbols and gic_decoder_dropout's layout, the argument checks
of the gic_*_drop entry points and of the two tensor-level calls (status codes and texts, after everything the plain entry checks),
--gen-dropout and its check, the new keywords of the module and engine surface, and the host map of tests/gen_dropout_oracle.py."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import gen_dropout_oracle as GD
from tests import philox_ref as PR

SYMBOLS = ("gic_decoder_forward_tf_drop", "gic_decoder_forward_ss_drop", "gic_decoder_forward_tf_drop_bwd", "gic_attn_forward_tf_drop",
           "gic_attn_forward_ss_drop", "gic_attn_forward_tf_drop_bwd", "gic_hidden_dropout", "gic_hidden_dropout_bwd")
PLAIN = {"gic_decoder_forward_tf_drop": "gic_decoder_forward_tf", "gic_decoder_forward_ss_drop": "gic_decoder_forward_ss",
         "gic_decoder_forward_tf_drop_bwd": "gic_decoder_forward_tf_bwd", "gic_attn_forward_tf_drop": "gic_attn_forward_tf",
         "gic_attn_forward_ss_drop": "gic_attn_forward_ss", "gic_attn_forward_tf_drop_bwd": "gic_attn_forward_tf_bwd"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2
PTR = 256                                                          # a non-null, 16-byte aligned stand-in: no check dereferences it


def _lib():
    from gan_image_captioning_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_agree_across_header_lib_and_so():
    L_, lib = _lib()
    with open(os.path.join(ROOT, "include", "gicap.h")) as f:
        header = f.read()
    assert "typedef struct gic_decoder_dropout" in header
    nargs = {}
    for s in SYMBOLS + tuple(PLAIN.values()):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % s, header)
        assert m, s
        nargs[s] = len(m.group(1).split(","))
        assert s in L_._SIGNATURES and s in L_.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
        assert len(L_._SIGNATURES[s][1]) == nargs[s], s
    for drop, plain in PLAIN.items():                              # the plain entry's arguments, and drop in front of stream
        assert nargs[drop] == nargs[plain] + 1
        sig, base = L_._SIGNATURES[drop][1], L_._SIGNATURES[plain][1]
        assert sig[:-2] == base[:-1] and sig[-1] == base[-1] and sig[-2] == ctypes.POINTER(L_.DecoderDropout)
    assert lib.gic_abi_version() == 5 and L_.ABI_VERSION == 5
    assert re.search(r"#define\s+GIC_ABI_VERSION\s+5\b", header)


def test_dropout_struct_layout():
    L_, _ = _lib()
    o = L_.DecoderDropout
    assert [f[0] for f in o._fields_] == ["p", "seed", "keep_u", "hdrop"]
    assert (o.p.offset, o.seed.offset, o.keep_u.offset, o.hdrop.offset) == (0, 8, 16, 24) and ctypes.sizeof(o) == 32


def _drop(L_, p=0.5, hdrop=PTR, keep_u=None):
    o = L_.DecoderDropout()
    o.p, o.seed, o.keep_u, o.hdrop = p, 7, keep_u, hdrop
    return o


def _lstm_structs(L_, dims):
    d = L_.DecoderDims(*dims)
    p, s, st = L_.DecoderParams(), L_.DecoderShadow(), L_.DecoderState()
    p.embed = p.w_out = p.b_out = PTR
    s.wout = PTR
    st.hout = st.gpre = st.logits = PTR
    for l in range(dims[5]):
        st.xh[l] = st.c[l] = st.gates[l] = PTR
        s.wcat[l] = s.bsum[l] = s.wcat_t[l] = PTR
    return d, p, s, st


def _attn_structs(L_, dims):
    d = L_.AttnDims(*dims)
    p, s, st = L_.AttnParams(), L_.AttnShadow(), L_.AttnState()
    for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
        setattr(p, n, PTR)
    for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
        setattr(s, n, PTR)
    for n in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
        setattr(st, n, PTR)
    return d, p, s, st


LSTM_DIMS, ATTN_DIMS = (2, 4, 50, 8, 8, 1, 0), (2, 4, 64, 8, 8, 8, 4, 8, 0)


def _ss_opts(L_):
    o = L_.SchedSampleOpts()
    o.prob, o.pick, o.coin_u, o.noise_u, o.seed, o.inputs, o.replaced = 0.5, 0, None, None, 0, PTR, None
    return o


def _call(entry, drop, Tmax=3, out=PTR):
    """One gic_*_drop entry point on stand-in pointers that pass every check of its plain counterpart: (status, text)."""
    L_, lib = _lib()
    dref = None if drop is None else ctypes.byref(drop)
    ref = ctypes.byref
    if entry.startswith("gic_decoder"):
        d, p, s, st = _lstm_structs(L_, LSTM_DIMS)
        head = (ref(d), ref(p), ref(s), ref(st))
        if entry == "gic_decoder_forward_tf_drop":
            rc = lib.gic_decoder_forward_tf_drop(*head, PTR, PTR, PTR, Tmax, None, 0, 1.0, 1, PTR, PTR, out, PTR, PTR, dref, None)
        elif entry == "gic_decoder_forward_ss_drop":
            o = _ss_opts(L_)
            rc = lib.gic_decoder_forward_ss_drop(*head, PTR, PTR, PTR, Tmax, ref(o), PTR, out, PTR, PTR, dref, None)
        else:
            ws, g = L_.DecoderBwdWs(), L_.DecoderGrads()
            ws.dlogits = ws.dhout = PTR
            g.embed = g.w_out = g.b_out = g.features = PTR
            for l in range(LSTM_DIMS[5]):
                ws.dgates[l] = ws.dxh[l] = ws.dc[l] = PTR
                g.w_ih[l] = g.w_hh[l] = g.b_ih[l] = g.b_hh[l] = PTR
            rc = lib.gic_decoder_forward_tf_drop_bwd(*head, ref(ws), out, PTR, PTR, Tmax, PTR, 1.0, 1, ref(g), dref, None)
    else:
        d, p, s, st = _attn_structs(L_, ATTN_DIMS)
        head = (ref(d), ref(p), ref(s), ref(st))
        if entry == "gic_attn_forward_tf_drop":
            rc = lib.gic_attn_forward_tf_drop(*head, PTR, PTR, PTR, PTR, Tmax, None, 0, 1.0, 1, PTR, out, None, PTR, PTR, dref, None)
        elif entry == "gic_attn_forward_ss_drop":
            o = _ss_opts(L_)
            rc = lib.gic_attn_forward_ss_drop(*head, PTR, PTR, PTR, PTR, Tmax, ref(o), PTR, out, None, PTR, PTR, dref, None)
        else:
            ws, g = L_.AttnBwdWs(), L_.AttnGrads()
            for n, _ in ws._fields_:
                setattr(ws, n, PTR)
            for n, _ in g._fields_:
                setattr(g, n, PTR)
            rc = lib.gic_attn_forward_tf_drop_bwd(*head, ref(ws), PTR, out, PTR, PTR, Tmax, PTR, None, 1.0, 1, ref(g), dref, None)
    return rc, lib.gic_last_error().decode()


ENTRIES = tuple(PLAIN)
DROP_ERRORS = [
    ("null", None, "null dropout"),
    ("p0", dict(p=0.0), "p must be in (0, 1)"),
    ("p1", dict(p=1.0), "p must be in (0, 1)"),
    ("p_neg", dict(p=-0.25), "p must be in (0, 1)"),
    ("p_nan", dict(p=math.nan), "p must be in (0, 1)"),
    ("hdrop_null", dict(hdrop=None), "hdrop is null"),
    ("hdrop_align", dict(hdrop=PTR + 8), "hdrop must be 16-byte aligned"),
]


@pytest.mark.parametrize("case,kw,msg", DROP_ERRORS, ids=[c[0] for c in DROP_ERRORS])
@pytest.mark.parametrize("entry", ENTRIES)
def test_drop_entries_refuse_bad_dropout_arguments(entry, case, kw, msg):
    """Every one of them passes the plain entry's checks first (the stand-ins are complete), then fails on the dropout struct."""
    L_, _ = _lib()
    rc, err = _call(entry, None if kw is None else _drop(L_, **kw))
    assert rc == INVALID_ARG and msg in err and entry[4:] in err, (rc, err)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_plain_checks_come_first(entry):
    """A call that is wrong twice reports the plain entry's error: Tmax out of range and a NULL out, each with a bad dropout struct."""
    L_, _ = _lib()
    rc, err = _call(entry, _drop(L_, p=2.0), Tmax=0)
    assert rc == INVALID_ARG and "Tmax" in err and entry[4:] in err, (rc, err)
    rc, err = _call(entry, None, out=None)
    assert rc == INVALID_ARG and "null argument" in err and entry[4:] in err, (rc, err)


def test_attn_ss_drop_is_refused_in_the_deterministic_mode_with_the_plain_text():
    L_, lib = _lib()
    was = lib.gic_get_deterministic()
    lib.gic_set_deterministic(1)
    try:
        rc, err = _call("gic_attn_forward_ss_drop", _drop(L_))
        d, p, s, st = _attn_structs(L_, ATTN_DIMS)
        o = _ss_opts(L_)
        rc0 = lib.gic_attn_forward_ss(ctypes.byref(d), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), PTR, PTR, PTR, PTR, 3,
                                      ctypes.byref(o), PTR, PTR, None, PTR, PTR, None)
        err0 = lib.gic_last_error().decode()
        rc_tf, err_tf = _call("gic_attn_forward_tf_drop", None)      # the teacher-forced forms stay available: this one fails on its own check
    finally:
        lib.gic_set_deterministic(was)
    assert rc == rc0 == UNSUPPORTED and err == err0 and "deterministic" in err
    assert rc_tf == INVALID_ARG and "null dropout" in err_tf


def test_tensor_level_calls_check_their_arguments():
    _, lib = _lib()
    f = lib.gic_hidden_dropout
    for args, msg in (((None, 0, 4, 8, 0.5, 0, None, PTR, None), "null argument"),
                      ((PTR, 0, 4, 8, 0.5, 0, None, None, None), "null argument"),
                      ((PTR, 7, 4, 8, 0.5, 0, None, PTR, None), "dtype"),
                      ((PTR, 0, 0, 8, 0.5, 0, None, PTR, None), "bad dims"),
                      ((PTR, 1, 4, 0, 0.5, 0, None, PTR, None), "bad dims"),
                      ((PTR, 0, 4, 8, 0.0, 0, None, PTR, None), "p must be in (0, 1)"),
                      ((PTR, 0, 4, 8, 1.0, 0, None, PTR, None), "p must be in (0, 1)"),
                      ((PTR, 0, 4, 8, math.nan, 0, None, PTR, None), "p must be in (0, 1)")):
        assert f(*args) == INVALID_ARG
        err = lib.gic_last_error().decode()
        assert msg in err and err.startswith("hidden_dropout:"), err
    b = lib.gic_hidden_dropout_bwd
    for args, msg in (((None, PTR, 2, 3, 8, 0.5, 0, None, None), "null argument"),
                      ((PTR, None, 2, 3, 8, 0.5, 0, None, None), "null argument"),
                      ((PTR, PTR, 0, 3, 8, 0.5, 0, None, None), "bad dims"),
                      ((PTR, PTR, 2, 0, 8, 0.5, 0, None, None), "bad dims"),
                      ((PTR, PTR, 2, 3, 0, 0.5, 0, None, None), "bad dims"),
                      ((PTR, PTR, 2, 3, 8, math.nan, 0, None, None), "p must be in (0, 1)"),
                      ((PTR, PTR, 2, 3, 8, 1.5, 0, None, None), "p must be in (0, 1)")):
        assert b(*args) == INVALID_ARG
        err = lib.gic_last_error().decode()
        assert msg in err and err.startswith("hidden_dropout_bwd:"), err


def test_attention_dims_refuse_a_width_that_is_no_multiple_of_8():
    """Why tests/test_gpu_gen_dropout.py has no attention case at H = 36: check_attn_dims wants H % 8 == 0, before any dropout check."""
    L_, lib = _lib()
    d, p, s, st = _attn_structs(L_, (2, 4, 64, 8, 36, 8, 4, 8, 0))
    rc = lib.gic_attn_forward_tf_drop(ctypes.byref(d), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), PTR, PTR, PTR, PTR, 3, None, 0,
                                      1.0, 1, PTR, PTR, None, PTR, PTR, None, None)
    assert rc == INVALID_ARG and "multiples of 8" in lib.gic_last_error().decode()
    d = L_.DecoderDims(2, 4, 50, 8, 30, 1, 0)                     # the LSTM decoder takes any H: the scalar form is reachable through it
    out = (ctypes.c_uint64 * (3 * L_.MAX_LAYERS + 4))()
    assert lib.gic_decoder_state_bytes(ctypes.byref(d), out) == 0


# ------------------------------------------------------------------------------------------ the flag and its check
def test_flag_default_and_parse():
    from gan_image_captioning_amd.args import default_args
    assert default_args().gen_dropout == 0.0
    assert default_args(gen_dropout=0.3, pretrain_mode="teacher").gen_dropout == 0.3
    from gan_image_captioning_amd.args import build_parser
    parser = build_parser()
    assert parser.parse_args([]).gen_dropout == 0.0
    assert parser.parse_args(["--gen-dropout", "0.25"]).gen_dropout == 0.25
    act = {a.option_strings[0]: a for a in parser._actions if a.option_strings}["--gen-dropout"]
    assert act.type is float and "vocabulary projection" in act.help and "training batches only" in act.help


@pytest.mark.parametrize("kw,msg", [
    (dict(gen_dropout=-0.1, pretrain_mode="teacher"), "--gen-dropout"),
    (dict(gen_dropout=1.0, pretrain_mode="teacher"), "--gen-dropout"),
    (dict(gen_dropout=math.nan, pretrain_mode="teacher"), "--gen-dropout"),
    (dict(gen_dropout=0.3, pretrain_mode="sample"), "--pretrain-mode teacher"),
    (dict(gen_dropout=0.3, pretrain_mode="sample", decoder="attention"), "--pretrain-mode teacher"),
])
def test_check_gen_dropout_refuses(kw, msg):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor, check_gen_dropout
    with pytest.raises(ValueError, match=msg):
        check_gen_dropout(default_args(device="cpu", **kw))
    with pytest.raises(ValueError, match=msg):                     # the instructor runs it before anything touches the device
        GANInstructor(default_args(device="cpu", **kw), None, None)


def test_check_gen_dropout_accepts():
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import check_gen_dropout
    assert check_gen_dropout(default_args()) == 0.0
    assert check_gen_dropout(default_args(pretrain_mode="sample", gen_dropout=0.0)) == 0.0
    assert check_gen_dropout(default_args(pretrain_mode="teacher", gen_dropout=0.5)) == 0.5


# ------------------------------------------------------------------------------------------ keywords
def test_new_keywords_and_their_defaults():
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder
    for fn in (Decoder.forward, Decoder.forward_scheduled, AttnDecoder.forward, AttnDecoder.forward_scheduled):
        ps = inspect.signature(fn).parameters
        assert list(ps)[-3:] == ["dropout", "dropout_seed", "keep_u"], fn
        assert (ps["dropout"].default, ps["dropout_seed"].default, ps["keep_u"].default) == (0.0, None, None), fn
    for cls in (engine.DecoderEngine, engine.AttnDecoderEngine):
        for name in ("forward_tf", "forward_scheduled", "forward_tf_bwd"):
            ps = inspect.signature(getattr(cls, name)).parameters
            assert list(ps)[-3:] == ["dropout", "dropout_seed", "keep_u"], (cls, name)
            assert (ps["dropout"].default, ps["dropout_seed"].default, ps["keep_u"].default) == (0.0, 0, None), (cls, name)
    assert callable(engine.hidden_dropout) and callable(engine.hidden_dropout_bwd)


def test_module_methods_check_dropout_before_the_gpu():
    from gan_image_captioning_amd.generator import SEEDS, Decoder, _drop_args
    caps = torch.zeros(2, 3, dtype=torch.long)
    for bad in (-0.1, 1.0, math.nan):
        with pytest.raises(ValueError, match="dropout"):
            Decoder.forward_scheduled(None, torch.zeros(2, 8), caps, [4, 4], 0.5, dropout=bad)
    SEEDS.reset()
    assert _drop_args(0.0, None, None) == (0.0, 0, None)           # nothing drawn: no seed is taken
    a = SEEDS.next()
    SEEDS.reset()
    assert _drop_args(0.5, None, None) == (0.5, a, None)           # a drawn mask takes the next seed ...
    SEEDS.reset()
    u = torch.zeros(1)
    assert _drop_args(0.5, None, u) == (0.5, 0, u) and _drop_args(0.5, 11, None) == (0.5, 11, None)      # ... a given one does not
    assert SEEDS.next() == a


# ------------------------------------------------------------------------------------------ the host map
@pytest.mark.parametrize("shape", [(3, 6, 64), (3, 6, 36), (2, 5, 7), (1, 1, 1)])
def test_triples_and_counter_forms_agree(shape):
    seed = 0x1234_5678_9ABC_DEF1
    stream, ctr, lane = GD.dropout_triples(*shape)
    assert (stream == np.uint64(0x6764726F << 32)).all()
    flat = np.arange(np.prod(shape), dtype=np.uint64).reshape(shape)
    assert np.array_equal(ctr, flat >> np.uint64(2)) and np.array_equal(lane, (flat & np.uint64(3)).astype(np.int64))
    u = GD.dropout_u(seed, *shape)
    assert u.dtype == np.float32 and u.shape == shape
    assert np.array_equal(PR.from_triples(seed, (stream, ctr, lane)), u)
    for p in (0.5, 0.1):
        assert np.array_equal(GD.dropout_keep(seed, *shape, p), u >= np.float32(p))


def test_stream_tag_is_its_own():
    tags = {PR.STREAM_TF, PR.STREAM_DISC, PR.STREAM_SS_COIN, PR.STREAM_SS_NOISE, GD.STREAM_GEN_DROP}
    assert len(tags) == 5 and GD.STREAM_GEN_DROP >> 32 == int.from_bytes(b"gdro", "big")
    assert (GD.STREAM_GEN_DROP & 0xFFFFFFFF) == 0 and GD.STREAM_GEN_DROP > (1 << 32)      # above every roll-out step index


def test_keep_fraction():
    p, n = 0.25, 64 * 1024
    keep = GD.dropout_keep(99, 64, 1, 1024, p)
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(float(keep.mean()) - (1 - p)) < 4 * sigma


def test_apply_is_the_f32_product():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 8, generator=g)
    keep = torch.rand(2, 3, 8, generator=g) >= 0.1
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    want = np.where(keep.numpy(), x.numpy() * s, np.float32(0))
    assert want.dtype == np.float32 and np.array_equal(GD.apply(x, keep, 0.1).numpy(), want)
    yb = GD.apply(x.bfloat16(), keep, 0.1)
    assert yb.dtype == torch.bfloat16
    assert torch.equal(yb, torch.where(keep, torch.from_numpy(x.bfloat16().float().numpy() * s).bfloat16(), torch.zeros((), dtype=torch.bfloat16)))
    d = torch.randn(2, 3, 8, generator=g)
    got = GD.apply_bwd(d, keep, [3, 1], 0.1)
    assert (got[1, 1:] == 0).all() and torch.equal(got[0], torch.from_numpy(np.where(keep[0].numpy(), d[0].numpy() * s, np.float32(0))))


def test_oracles_with_everything_kept_are_the_plain_oracles():
    from oracle import cpu_step as O
    from tests import attn_beam_oracle as AO
    from tests import attn_tf_oracle as TF
    g = torch.Generator().manual_seed(5)
    B, Lc, V, E, H = 3, 5, 37, 8, 12
    lens = [6, 3, 1]
    caps = torch.randint(0, V, (B, Lc), generator=g)
    gp = {k: v.double() * 4 for k, v in O.make_gen_params(V, E, H, 2, g).items()}
    feats = torch.randn(B, E, generator=g).double()
    keep = torch.ones(B, 6, H, dtype=torch.bool)
    pred, (h, c) = GD.lstm_forward_tf(gp, feats, caps, lens, keep, 0.0)
    want, (hw, cw) = O.decoder_forward_tf(gp, feats, caps, lens, 1.0, pretrain=True)
    assert torch.equal(pred, want) and torch.equal(h, hw) and torch.equal(c, cw)
    # a dropped decode keeps the recurrence and scales what it keeps
    keep = torch.rand(B, 6, H, generator=g) >= 0.5
    pred2, (h2, c2) = GD.lstm_forward_tf(gp, feats, caps, lens, keep, 0.5)
    assert torch.equal(h2, hw) and torch.equal(c2, cw) and not torch.equal(pred2, want)
    params, f, fmap = AO.random_problem(B, 64, 8, 16, 8, 4, 8, seed=2)
    ap = {"decoder." + n: t.double() for n, t in zip(AO.NAMES, params)}
    caps = torch.randint(0, 64, (B, Lc), generator=g)
    keep = torch.ones(B, 6, 16, dtype=torch.bool)
    got = GD.attn_forward_tf(ap, f.double(), fmap.double(), caps, lens, keep, 0.0)
    want = TF.forward_tf(ap, f.double(), fmap.double(), caps, lens, pretrain=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1][0], want[1][0]) and torch.equal(got[2], want[2])
