"""Scheduled sampling without a GPU: the C ABI symbols and the argument checks of gic_decoder_forward_ss / gic_attn_forward_ss, their
host-only workspace queries, the trainer flags and the ramp, the float64 oracle (tests/sched_sample_oracle.py) pinned to the teacher-
forced and the free-running oracles, and the top-2 gap condition of every case of tests/sched_sample_cases.py."""
import ctypes
import math
import os
import re

import pytest
import torch

from oracle import cpu_attention as CA
from oracle import cpu_step as O
from tests import attn_tf_oracle as TF
from tests import sched_sample_cases as SC
from tests import sched_sample_oracle as SO

SYMBOLS = ("gic_decoder_forward_ss_ws_bytes", "gic_decoder_forward_ss", "gic_attn_forward_ss_ws_bytes", "gic_attn_forward_ss")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2


def _lib():
    from gan_image_captioning_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_agree_across_header_lib_and_so():
    L_, lib = _lib()
    with open(os.path.join(ROOT, "include", "gicap.h")) as f:
        header = f.read()
    assert "typedef struct gic_sched_sample_opts" in header
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % s, header)
        assert m, s
        assert s in L_._SIGNATURES and s in L_.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
        assert len(L_._SIGNATURES[s][1]) == len(m.group(1).split(",")), s
    assert lib.gic_abi_version() == 5 and L_.ABI_VERSION == 5
    assert re.search(r"#define\s+GIC_ABI_VERSION\s+5\b", header)


def test_opts_struct_layout():
    L_, _ = _lib()
    o = L_.SchedSampleOpts
    assert [f[0] for f in o._fields_] == ["prob", "pick", "coin_u", "noise_u", "seed", "inputs", "replaced"]
    assert (o.prob.offset, o.pick.offset, o.coin_u.offset, o.noise_u.offset, o.seed.offset, o.inputs.offset, o.replaced.offset) == \
        (0, 4, 8, 16, 24, 32, 40) and ctypes.sizeof(o) == 48


def test_ws_bytes_are_host_only_and_monotone():
    L_, lib = _lib()
    out = ctypes.c_uint64(0)
    d = L_.DecoderDims(32, 20, 10000, 512, 512, 1, 1)
    a = L_.AttnDims(32, 20, 10000, 512, 512, 2048, 49, 512, 1)
    for fn, dims, name in ((lib.gic_decoder_forward_ss_ws_bytes, d, "decoder_forward_ss_ws_bytes"),
                           (lib.gic_attn_forward_ss_ws_bytes, a, "attn_forward_ss_ws_bytes")):
        sizes = []
        for tm in range(1, 21):
            assert fn(ctypes.byref(dims), tm, ctypes.byref(out)) == 0
            assert out.value >= 32 * tm * 10000 * 4 and out.value % 16 == 0
            sizes.append(out.value)
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        for tm in (0, 21):
            assert fn(ctypes.byref(dims), tm, ctypes.byref(out)) == INVALID_ARG
            err = lib.gic_last_error().decode()
            assert "Tmax" in err and name in err
        assert fn(ctypes.byref(dims), 1, None) == INVALID_ARG
        assert name in lib.gic_last_error().decode()
        assert fn(None, 1, ctypes.byref(out)) == INVALID_ARG
    odd = L_.DecoderDims(3, 6, 50, 12, 20, 1, 0)                   # any V: the size is rounded up to whole 16-byte chunks
    assert lib.gic_decoder_forward_ss_ws_bytes(ctypes.byref(odd), 5, ctypes.byref(out)) == 0
    assert out.value == (3 * 5 * 50 * 4 + 15) // 16 * 16
    assert lib.gic_attn_forward_ss_ws_bytes(ctypes.byref(a), 13, ctypes.byref(out)) == 0
    assert out.value == (32 * 13 * 10000 + 32 * 49) * 4          # the logits of every step and the energies of one


def _opts(L_, prob=0.5, pick=0, inputs=256):
    o = L_.SchedSampleOpts()
    o.prob, o.pick, o.coin_u, o.noise_u, o.seed, o.inputs, o.replaced = prob, pick, None, None, 0, inputs, None
    return o


def _lstm(lib, L_, dims=(2, 4, 50, 8, 8, 1, 0), Tmax=3, features=256, caps=256, lengths=256, opts="default", ws=256, out=256, h_n=256,
          null_params=False, null_state=False, null_layer=False, **okw):
    d = L_.DecoderDims(*dims)
    p, s, st = L_.DecoderParams(), L_.DecoderShadow(), L_.DecoderState()
    if not null_params:
        p.embed = p.w_out = p.b_out = 256
        s.wout = 256
    if not null_state:
        st.hout = st.gpre = st.logits = 256
    for l in range(max(0, min(dims[5], L_.MAX_LAYERS))):
        if not null_layer:
            st.xh[l] = st.c[l] = st.gates[l] = 256
            s.wcat[l] = s.bsum[l] = 256
    o = _opts(L_, **okw) if opts == "default" else opts
    rc = lib.gic_decoder_forward_ss(ctypes.byref(d), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), features, caps, lengths, Tmax,
                                    None if o is None else ctypes.byref(o), ws, out, h_n, 256, None)
    return rc, lib.gic_last_error().decode()


def _attn(lib, L_, dims=(2, 4, 64, 8, 8, 8, 4, 8, 0), Tmax=3, features=256, fmap=256, caps=256, lengths=256, opts="default", ws=256,
          out=256, null_params=False, null_state=False, **okw):
    d = L_.AttnDims(*dims)
    p, s, st = L_.AttnParams(), L_.AttnShadow(), L_.AttnState()
    if not null_params:
        for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
            setattr(p, n, 256)
        for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
            setattr(s, n, 256)
    if not null_state:
        for n in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
            setattr(st, n, 256)
    o = _opts(L_, **okw) if opts == "default" else opts
    rc = lib.gic_attn_forward_ss(ctypes.byref(d), ctypes.byref(p), ctypes.byref(s), ctypes.byref(st), features, fmap, caps, lengths, Tmax,
                                 None if o is None else ctypes.byref(o), ws, out, None, 256, 256, None)
    return rc, lib.gic_last_error().decode()


COMMON_ERRORS = [
    ("Tmax0", dict(Tmax=0), "Tmax"),
    ("Tmax_gt_L", dict(Tmax=5), "Tmax"),
    ("features", dict(features=None), "null argument"),
    ("caps", dict(caps=None), "caps is null"),
    ("lengths", dict(lengths=None), "null argument"),
    ("opts", dict(opts=None), "null argument"),
    ("ws", dict(ws=None), "null argument"),
    ("ws_align", dict(ws=260), "16-byte aligned"),
    ("out", dict(out=None), "null argument"),
    ("inputs", dict(inputs=None), "inputs is null"),
    ("prob_neg", dict(prob=-0.01), "prob must be in [0, 1]"),
    ("prob_gt1", dict(prob=1.5), "prob must be in [0, 1]"),
    ("prob_nan", dict(prob=math.nan), "prob must be in [0, 1]"),
    ("pick_neg", dict(pick=-1), "pick must be 0"),
    ("pick_2", dict(pick=2), "pick must be 0"),
]


@pytest.mark.parametrize("case,kw,msg", COMMON_ERRORS + [
    ("h_n", dict(h_n=None), "null argument"),
    ("params", dict(null_params=True), "null buffer"),
    ("state", dict(null_state=True), "null buffer"),
    ("layer", dict(null_layer=True), "null layer 0 buffer"),
    ("NL0", dict(dims=(2, 4, 50, 8, 8, 0, 0)), "gen_num_layers"),
    ("NL_big", dict(dims=(2, 4, 50, 8, 8, 99, 0)), "gen_num_layers"),
    ("B0", dict(dims=(0, 4, 50, 8, 8, 1, 0)), "bad dims"),
    ("dtype", dict(dims=(2, 4, 50, 8, 8, 1, 7)), "dtype"),
])
def test_lstm_entry_refuses_bad_arguments(case, kw, msg):
    L_, lib = _lib()
    rc, err = _lstm(lib, L_, **kw)
    assert rc == INVALID_ARG and msg in err, (rc, err)
    if "dims" not in kw:
        assert "decoder_forward_ss" in err, err


@pytest.mark.parametrize("case,kw,msg", COMMON_ERRORS + [
    ("fmap", dict(fmap=None), "null argument"),
    ("weights", dict(null_params=True), "null weights"),
    ("state", dict(null_state=True), "null state buffer"),
    ("V4", dict(dims=(2, 4, 62, 8, 8, 8, 4, 8, 0)), "multiple of 4"),
    ("C8", dict(dims=(2, 4, 64, 8, 8, 12, 4, 8, 0)), "multiples of 8"),
    ("P", dict(dims=(2, 4, 64, 8, 8, 8, 1025, 8, 0)), "positions"),
    ("A", dict(dims=(2, 4, 64, 8, 8, 8, 4, 2056, 0)), "attention width"),
    ("B0", dict(dims=(0, 4, 64, 8, 8, 8, 4, 8, 0)), "bad dims"),
])
def test_attn_entry_refuses_bad_arguments(case, kw, msg):
    L_, lib = _lib()
    rc, err = _attn(lib, L_, **kw)
    assert rc == INVALID_ARG and msg in err, (rc, err)
    if "dims" not in kw:
        assert "attn_forward_ss" in err, err


def test_attn_entry_is_refused_in_the_deterministic_mode():
    L_, lib = _lib()
    was = lib.gic_get_deterministic()
    lib.gic_set_deterministic(1)
    try:
        rc, err = _attn(lib, L_)
    finally:
        lib.gic_set_deterministic(was)
    assert rc == UNSUPPORTED and "attn_forward_ss" in err and "deterministic" in err


# ------------------------------------------------------------------------------------------ flags, checks and the ramp
def test_flag_defaults():
    from gan_image_captioning_amd.args import default_args
    args = default_args()
    assert args.scheduled_sampling_prob == 0.0 and args.scheduled_sampling_ramp_epochs == 0
    assert args.scheduled_sampling_pick == "sample"
    args = default_args(scheduled_sampling_prob=0.25, scheduled_sampling_ramp_epochs=4, scheduled_sampling_pick="argmax")
    assert (args.scheduled_sampling_prob, args.scheduled_sampling_ramp_epochs, args.scheduled_sampling_pick) == (0.25, 4, "argmax")


@pytest.mark.parametrize("kw,msg", [
    (dict(scheduled_sampling_prob=0.5, pretrain_mode="sample"), "--pretrain-mode teacher"),
    (dict(scheduled_sampling_prob=0.5, pretrain_mode="sample", decoder="attention"), "--pretrain-mode teacher"),
    (dict(scheduled_sampling_prob=1.5, pretrain_mode="teacher"), "--scheduled-sampling-prob"),
    (dict(scheduled_sampling_prob=-0.1, pretrain_mode="teacher"), "--scheduled-sampling-prob"),
    (dict(scheduled_sampling_prob=math.nan, pretrain_mode="teacher"), "--scheduled-sampling-prob"),
    (dict(scheduled_sampling_prob=0.5, pretrain_mode="teacher", scheduled_sampling_pick="beam"), "--scheduled-sampling-pick"),
])
def test_instructor_refuses_bad_flags_before_the_device(kw, msg):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    with pytest.raises(ValueError, match=msg):
        GANInstructor(default_args(device="cpu", **kw), None, None)


def test_check_modes_keeps_its_two_tuple():
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import check_modes, check_scheduled_sampling
    args = default_args(pretrain_mode="teacher", scheduled_sampling_prob=0.5)
    assert check_modes(args) == ("teacher", 0.0)
    assert check_scheduled_sampling(args) == (0.5, 0, "sample")


def test_ramp_on_hand_worked_epochs():
    from gan_image_captioning_amd.training import scheduled_sampling_prob as ramp
    assert [ramp(0.25, 0, e) for e in (0, 1, 7)] == [0.25, 0.25, 0.25]
    assert [ramp(0.5, 4, e) for e in range(7)] == [0.0, 0.125, 0.25, 0.375, 0.5, 0.5, 0.5]
    assert [ramp(1.0, 1, e) for e in range(3)] == [0.0, 1.0, 1.0]
    assert ramp(0.3, 3, 2) == pytest.approx(0.2)


def test_module_methods_check_their_arguments_before_the_gpu():
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder
    caps = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="sample_prob"):
        Decoder.forward_scheduled(None, torch.zeros(2, 8), caps, [4, 4], 1.5)
    with pytest.raises(ValueError, match="pick"):
        Decoder.forward_scheduled(None, torch.zeros(2, 8), caps, [4, 4], 0.5, pick="beam")
    with pytest.raises(ValueError, match="feature map"):
        AttnDecoder.forward_scheduled(None, torch.zeros(2, 8), None, caps, [4, 4], 0.5)


# ------------------------------------------------------------------------------------------ oracle self-tests
@pytest.mark.parametrize("name", ["L2", "L3", "A2"])
def test_oracle_p0_is_the_teacher_forced_oracle(name):
    pr = SC.problem(name)
    gp, feats, fmap = SC.as_f64(pr)
    r = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], 0.0, "sample", pr["coin"], pr["u"])
    if fmap is None:
        pred, (h_n, c_n) = O.decoder_forward_tf(gp, feats, pr["caps"], pr["lengths"], 1.0, pretrain=True)
    else:
        pred, (h_n, c_n), alphas = TF.forward_tf(gp, feats, fmap, pr["caps"], pr["lengths"], pretrain=True)
        assert torch.equal(r["alphas"], alphas)
    assert torch.equal(r["pred"], pred) and torch.equal(r["h_n"], h_n) and torch.equal(r["c_n"], c_n)
    assert torch.equal(r["inputs"], pr["caps"]) and not r["replaced"].any() and r["min_gap"] == float("inf")


@pytest.mark.parametrize("name", ["L3", "A1"])
def test_oracle_p1_argmax_is_the_free_running_oracle(name):
    pr = SC.problem(name)
    gp, feats, fmap = SC.as_f64(pr)
    B, T = pr["dims"]["B"], pr["dims"]["T"]
    r = SO.scheduled(gp, feats, fmap, pr["caps"], [T] * B, 1.0, "argmax", pr["coin"], pr["u"])
    if fmap is None:
        logits, ids = O.decoder_sample(gp, feats, T, 1.0, pretrain=True)
    else:
        logits, ids, _ = CA.attn_decoder_sample(gp, feats, fmap, T, 1.0, pretrain=True)
    assert torch.equal(r["inputs"], ids[:, :-1]) and r["replaced"].all()
    torch.testing.assert_close(r["pred"], logits, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["L2", "L3", "A2"])
def test_oracle_never_replaces_past_a_length(name):
    pr = SC.problem(name)
    gp, feats, fmap = SC.as_f64(pr)
    r = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], 1.0, "sample", pr["coin"], pr["u"])
    T = pr["dims"]["T"]
    t = torch.arange(1, T)[None]                                   # position t-1 feeds step t
    live = t < torch.tensor(pr["lengths"])[:, None]
    assert torch.equal(r["replaced"], live)                        # p = 1: every live position, no other
    assert torch.equal(r["inputs"][~live], pr["caps"][~live])


def test_oracle_follows_given_inputs():
    pr = SC.problem("L2")
    gp, feats, fmap = SC.as_f64(pr)
    own = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], 0.5, "sample", pr["coin"], pr["u"])
    again = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], 0.5, "sample", pr["coin"], pr["u"], inputs=own["inputs"])
    assert torch.equal(again["pred"], own["pred"]) and torch.equal(again["picks"], own["picks"])


# ------------------------------------------------------------------------------------------ the cases' gap condition
@pytest.mark.parametrize("pick", SC.PICKS)
@pytest.mark.parametrize("p", SC.PROBS)
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_every_case_has_its_top2_gap(name, p, pick):
    r = SC.reference(name, p, pick)
    print(f"{name} p={p} {pick}: replaced {int(r['replaced'].sum())} of {r['replaced'].numel()}, min top-2 gap {r['min_gap']:.3e}")
    assert r["min_gap"] >= SC.MIN_GAP
    if name != "L4" and p == 1.0:
        assert r["replaced"].any()
    if name == "L4":
        assert r["inputs"].numel() == 0
