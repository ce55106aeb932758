"""Teacher-forced decode with the attention decoder without a GPU: the float64 oracle (tests/attn_tf_oracle.py) pinned to the greedy
roll-out of oracle/cpu_attention.py and to itself at shorter lengths, the new C ABI symbols, the argument checks of
gic_attn_forward_tf / gic_attn_forward_tf_bwd and the host-only size query, AttnDecoder.forward without a map and the trainer flags."""
import ctypes
import os
import re

import pytest
import torch

from oracle import cpu_attention as CA
from tests import attn_beam_oracle as AO
from tests import attn_tf_oracle as TF

SYMBOLS = ("gic_attn_forward_tf_ws_bytes", "gic_attn_forward_tf", "gic_attn_forward_tf_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(B=5, T=7, V=12, E=8, H=16, C=8, P=9, A=8, seed=3):
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed)
    return AO.as_dict(params), feats.double(), fmap.double()


def test_oracle_with_greedy_caps_is_the_pretrain_rollout():
    gp, feats, fmap = _problem()
    B, T = feats.shape[0], 7
    logits, ids, alphas = CA.attn_decoder_sample(gp, feats, fmap, T, 1.0, pretrain=True)
    pred, (h_n, c_n), al = TF.forward_tf(gp, feats, fmap, ids[:, :-1], [T] * B, pretrain=True)
    torch.testing.assert_close(pred, logits, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(al, alphas, rtol=1e-12, atol=1e-12)


def test_oracle_short_caption_equals_its_own_decode():
    gp, feats, fmap = _problem(seed=4)
    B, T = feats.shape[0], 7
    g = torch.Generator().manual_seed(5)
    caps = torch.randint(0, 12, (B, T - 1), generator=g)
    lengths = [3, 7, 1, 5, 6]
    u = torch.rand(B, T, 12, generator=g, dtype=torch.float64)
    for pretrain in (True, False):
        pred, (h_n, c_n), al = TF.forward_tf(gp, feats, fmap, caps, lengths, 1.3, pretrain, u)
        for b, n in enumerate(lengths):
            p1, (h1, c1), a1 = TF.forward_tf(gp, feats[b:b + 1], fmap[b:b + 1], caps[b:b + 1, :n - 1], [n], 1.3, pretrain, u[b:b + 1, :n])
            torch.testing.assert_close(pred[b, :n], p1[0], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(al[b, :n], a1[0], rtol=1e-12, atol=1e-12)
            assert (al[b, n:] == 0).all()
            # h_n / c_n: the state at the caption's own last step
            torch.testing.assert_close(h_n[b], h1[0], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(c_n[b], c1[0], rtol=1e-12, atol=1e-12)
            if pretrain:
                torch.testing.assert_close(pred[b, n:], gp["decoder.linear.bias"].expand(T - n, -1), rtol=0, atol=0)


def test_oracle_hn_is_the_last_step_state():
    gp, feats, fmap = _problem(seed=6)
    B, T = feats.shape[0], 7
    caps = torch.randint(0, 12, (B, T - 1), generator=torch.Generator().manual_seed(1))
    lengths = [2, 4, 7, 1, 3]
    _, (h_n, c_n), _ = TF.forward_tf(gp, feats, fmap, caps, lengths, pretrain=True)
    for b, n in enumerate(lengths):          # the full-length decode's state after step n - 1 (the first n steps do not see the length)
        _, (h, c), _ = TF.forward_tf(gp, feats, fmap, caps, [n] * B, pretrain=True)
        torch.testing.assert_close(h_n[b], h[b], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(c_n[b], c[b], rtol=1e-12, atol=1e-12)


def _lib():
    from gan_image_captioning_amd import _lib
    return _lib, _lib.load()


def test_symbols_agree_across_header_lib_and_so():
    L_, lib = _lib()
    with open(os.path.join(ROOT, "include", "gicap.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in L_._SIGNATURES, s
        assert hasattr(lib, s), s
    nargs = {s: len(re.search(r"\bint\s+%s\s*\(([^;]*)\);" % s, header).group(1).split(",")) for s in SYMBOLS}
    for s in SYMBOLS:
        assert len(L_._SIGNATURES[s][1]) == nargs[s], s


def test_ws_bytes_is_host_only():
    from gan_image_captioning_amd import engine
    L_, lib = _lib()
    d = L_.AttnDims(32, 20, 10000, 512, 512, 2048, 49, 512, 1)
    out = ctypes.c_uint64(0)
    assert lib.gic_attn_forward_tf_ws_bytes(ctypes.byref(d), 20, ctypes.byref(out)) == 0
    assert out.value == 32 * 20 * 10000 * 4
    eng = engine.AttnDecoderEngine(10000, 512, 512, 2048, 49, 512, 1)
    assert eng.tf_ws_bytes(32, 20, 13) == 32 * 13 * 10000 * 4
    d = L_.AttnDims(4, 3, 4, 8, 8, 8, 1000, 8, 0)               # the energies outgrow the logits
    assert lib.gic_attn_forward_tf_ws_bytes(ctypes.byref(d), 1, ctypes.byref(out)) == 0
    assert out.value == 4 * 1000 * 4
    for tm in (0, 4):
        assert lib.gic_attn_forward_tf_ws_bytes(ctypes.byref(d), tm, ctypes.byref(out)) != 0
        assert "Tmax" in lib.gic_last_error().decode()
    assert lib.gic_attn_forward_tf_ws_bytes(ctypes.byref(d), 1, None) != 0
    assert lib.gic_attn_forward_tf_ws_bytes(None, 1, ctypes.byref(out)) != 0


def _fwd(lib, L_, dims, Tmax=3, caps=256, fmap=256, lengths=256, out=256, null_params=False, null_state=False):
    p, s, st = L_.AttnParams(), L_.AttnShadow(), L_.AttnState()
    if not null_params:
        for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
            setattr(p, n, 256)
        for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
            setattr(s, n, 256)
    if not null_state:
        for n in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
            setattr(st, n, 256)
    rc = lib.gic_attn_forward_tf(ctypes.byref(dims), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), 256, fmap, caps, lengths, Tmax,
                                 None, 0, 1.0, 1, 256, out, None, 256, 256, None)
    return rc, lib.gic_last_error().decode()


def _bwd(lib, L_, dims, Tmax=3, caps=256, pred=256, null_ws=False, null_grads=False):
    p, s, st, w, g = L_.AttnParams(), L_.AttnShadow(), L_.AttnState(), L_.AttnBwdWs(), L_.AttnGrads()
    for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
        setattr(p, n, 256)
        if not null_grads:
            setattr(g, n, 256)
    g.features = None if null_grads else 256
    for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
        setattr(s, n, 256)
    for n in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
        setattr(st, n, 256)
    if not null_ws:
        for n in ("dlogits", "dhout", "dgates", "dc", "dz", "dalpha", "dh_extra", "dhproj", "dfproj", "dfproj_act", "dwa_rows", "dx"):
            setattr(w, n, 256)
    rc = lib.gic_attn_forward_tf_bwd(ctypes.byref(dims), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), ctypes.byref(w), 256, pred, caps,
                                     256, Tmax, 256, None, 1.0, 1, ctypes.byref(g), None)
    return rc, lib.gic_last_error().decode()


@pytest.mark.parametrize("case,kw,msg", [
    ("Tmax0", dict(Tmax=0), "Tmax"),
    ("Tmax_gt_L", dict(Tmax=5), "Tmax"),
    ("caps", dict(caps=None), "caps is null"),
    ("fmap", dict(fmap=None), "null argument"),
    ("lengths", dict(lengths=None), "null argument"),
    ("out", dict(out=None), "null argument"),
    ("weights", dict(null_params=True), "null weights"),
    ("state", dict(null_state=True), "null state buffer"),
    ("V4", dict(dims=(2, 4, 62, 8, 8, 8, 4, 8, 0)), "multiple of 4"),
    ("C8", dict(dims=(2, 4, 64, 8, 8, 12, 4, 8, 0)), "multiples of 8"),
    ("P", dict(dims=(2, 4, 64, 8, 8, 8, 1025, 8, 0)), "positions"),
    ("B0", dict(dims=(0, 4, 64, 8, 8, 8, 4, 8, 0)), "bad dims"),
    ("dtype", dict(dims=(2, 4, 64, 8, 8, 8, 4, 8, 7)), "dtype"),
])
def test_forward_refuses_bad_arguments(case, kw, msg):
    L_, lib = _lib()
    dims = L_.AttnDims(*kw.pop("dims", (2, 4, 64, 8, 8, 8, 4, 8, 0)))
    rc, err = _fwd(lib, L_, dims, **kw)
    assert rc != 0 and msg in err, (rc, err)


@pytest.mark.parametrize("case,kw,msg", [
    ("Tmax0", dict(Tmax=0), "Tmax"),
    ("Tmax_gt_L", dict(Tmax=5), "Tmax"),
    ("caps", dict(caps=None), "caps is null"),
    ("pred", dict(pred=None), "null argument"),
    ("ws", dict(null_ws=True), "null workspace buffer"),
    ("grads", dict(null_grads=True), "null gradient buffer"),
    ("A", dict(dims=(2, 4, 64, 8, 8, 8, 4, 2056, 0)), "attention width"),
])
def test_backward_refuses_bad_arguments(case, kw, msg):
    L_, lib = _lib()
    dims = L_.AttnDims(*kw.pop("dims", (2, 4, 64, 8, 8, 8, 4, 8, 0)))
    rc, err = _bwd(lib, L_, dims, **kw)
    assert rc != 0 and msg in err, (rc, err)


def test_null_dims_and_structs():
    L_, lib = _lib()
    assert lib.gic_attn_forward_tf(None, None, None, None, 256, 256, 256, 256, 1, None, 0, 1.0, 1, 256, 256, None, 256, 256, None) != 0
    d = L_.AttnDims(2, 4, 64, 8, 8, 8, 4, 8, 0)
    assert lib.gic_attn_forward_tf(ctypes.byref(d), None, None, None, 256, 256, 256, 256, 1, None, 0, 1.0, 1, 256, 256, None, 256, 256,
                                   None) != 0
    assert "null argument" in lib.gic_last_error().decode()
    assert lib.gic_attn_forward_tf_bwd(ctypes.byref(d), None, None, None, None, 256, 256, 256, 256, 1, 256, None, 1.0, 1, None, None) != 0
    assert "null argument" in lib.gic_last_error().decode()


def test_forward_without_a_map_raises_before_the_gpu():
    from gan_image_captioning_amd.generator import AttnDecoder
    with pytest.raises(ValueError, match="feature map"):
        AttnDecoder.forward(None, torch.zeros(2, 8), None, torch.zeros(2, 3, dtype=torch.long), [4, 4])


def test_flag_defaults():
    from gan_image_captioning_amd.args import default_args
    args = default_args()
    assert args.pretrain_mode == "sample" and args.attn_reg == 0.0


@pytest.mark.parametrize("kw", [dict(decoder="lstm", pretrain_mode="teacher"), dict(decoder="lstm", pretrain_mode="sample"),
                                dict(decoder="attention", pretrain_mode="sample")])
def test_attn_reg_outside_attention_teacher_is_refused(kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(attn_reg=0.5, device="cpu", **kw)
    with pytest.raises(ValueError, match="--attn-reg"):
        GANInstructor(args, None, None)


def test_unknown_pretrain_mode_is_refused():
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    with pytest.raises(ValueError, match="--pretrain-mode"):
        GANInstructor(default_args(pretrain_mode="free", device="cpu"), None, None)
