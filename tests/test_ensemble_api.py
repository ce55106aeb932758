"""Ensemble decoding without a GPU: the C ABI (symbols, struct layout, the workspace queries, every refusal as a status and a text on
fake pointers, before any launch), the float64 oracle (tests/ensemble_oracle.py) against the single-model oracles, the Python
surface's refusals, the flags and the instructor's member order."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import ensemble_cases as EC
from tests import ensemble_oracle as EO
from tests import sample_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gic_ensemble_mix", "gic_decoder_ensemble_beam_ws_bytes", "gic_attn_ensemble_beam_ws_bytes", "gic_decoder_ensemble_sample_ws_bytes",
       "gic_attn_ensemble_sample_ws_bytes", "gic_decoder_ensemble_beam_search", "gic_attn_ensemble_beam_search",
       "gic_decoder_ensemble_sample_captions", "gic_attn_ensemble_sample_captions")


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- the C ABI
def test_symbols_declared_bound_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.gic_abi_version() == 5 and "#define GIC_ABI_VERSION 5" in hdr           # additive: the version stays
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, name


def test_struct_and_constants_match_header():
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    assert int(re.search(r"#define GIC_MAX_ENSEMBLE (\d+)", hdr).group(1)) == L.MAX_ENSEMBLE == 4
    assert {k: int(re.search(r"#define GIC_ENSEMBLE_%s (\d+)" % k.upper(), hdr).group(1)) for k in L.ENSEMBLE_MODES} == L.ENSEMBLE_MODES
    body = re.search(r"typedef struct gic_ensemble_opts \{(.*?)\} gic_ensemble_opts;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*([a-z_0-9]+)\s+([a-zA-Z_]+)(?:\[(\w+)\])?;", re.sub(r"/\*.*?\*/", "", body), re.M)
    assert fields == [("int32_t", "M", ""), ("int32_t", "mode", ""), ("float", "weights", "GIC_MAX_ENSEMBLE")]
    assert [f[0] for f in L.EnsembleOpts._fields_] == ["M", "mode", "weights"]
    assert [getattr(L.EnsembleOpts, f).offset for f in ("M", "mode", "weights")] == [0, 4, 8] and C.sizeof(L.EnsembleOpts) == 24


LSTM_DIMS = (4, 6, 50, 8, 16, 2, 0)          # B, L, V, E, H, NL, dtype: the generic path
LSTM_FUSED = (8, 12, 64, 32, 64, 1, 0)       # the fused path
ATTN_DIMS = (2, 4, 64, 8, 8, 8, 9, 8, 0)     # B, L, V, E, H, C, P, A, dtype


def _members(L, lstm, M, null=None):
    """M fake (non-null, aligned) members: arrays of pointers to params / shadow structs, and the structs they point to."""
    keep = []
    for m in range(M):
        if lstm:
            p, s = L.DecoderParams(), L.DecoderShadow()
            p.embed, p.w_out, p.b_out, s.wout = 256, 256, 256, 256
            for l in range(L.MAX_LAYERS):
                s.wcat[l], s.bsum[l] = 256, 256
        else:
            p, s = L.AttnParams(), L.AttnShadow()
            for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
                setattr(p, n, 256)
            for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
                setattr(s, n, 256)
        keep.append((p, s))
    parr = (C.c_void_p * M)(*[None if m == null else C.addressof(p) for m, (p, _) in enumerate(keep)])
    sarr = (C.c_void_p * M)(*[C.addressof(s) for _, s in keep])
    ptrs = (C.c_void_p * M)(*[256] * M)
    return parr, sarr, ptrs, keep


def _call(L, lib, which, head, M=2, mode=0, weights=(1.0, 1.0, 1.0, 1.0), eM=None, dims=None, ws=256, cws=256, beam=4, groups=2, cons=None,
          null=None, eopts=True, opts=True, arrays=True, h0=None):
    """One ensemble call on fake pointers: every status comes back before any launch."""
    lstm = which == "lstm"
    d = (L.DecoderDims if lstm else L.AttnDims)(*(dims or (LSTM_DIMS if lstm else ATTN_DIMS)))
    parr, sarr, ptrs, keep = _members(L, lstm, max(1, min(M, 4)), null)
    e = L.EnsembleOpts()
    e.M, e.mode = M if eM is None else eM, mode
    for i, w in enumerate(weights):
        e.weights[i] = w
    ep = C.byref(e) if eopts else None
    cp = None if cons is None else C.byref(cons)
    maps = () if lstm else (ptrs,)
    pa = parr if arrays else None
    if head == "beam":
        o = L.DiverseBeamOpts()
        o.beam.beam, o.beam.eos_id, o.beam.pad_id, o.groups, o.diversity, o.beam.h0 = beam, 2, 0, groups, 0.5, h0
        fn = lib.gic_decoder_ensemble_beam_search if lstm else lib.gic_attn_ensemble_beam_search
        rc = fn(C.byref(d), M, pa, sarr, ep, C.byref(o) if opts else None, cp, ws, cws, ptrs, *maps, 256, 256, 256, None)
    else:
        o = L.SampleOpts()
        o.num_samples, o.top_k, o.top_p, o.temperature, o.eos_id, o.pad_id, o.h0 = beam, 0, 1.0, 1.0, 2, 0, h0
        fn = lib.gic_decoder_ensemble_sample_captions if lstm else lib.gic_attn_ensemble_sample_captions
        rc = fn(C.byref(d), M, pa, sarr, ep, C.byref(o) if opts else None, cp, ws, cws, ptrs, *maps, None, 0, 256, 256, 256, None)
    return rc, lib.gic_last_error().decode()


BOTH = pytest.mark.parametrize("which,head", [("lstm", "beam"), ("lstm", "sample"), ("attn", "beam"), ("attn", "sample")])


@BOTH
@pytest.mark.parametrize("case,kw,msg", [
    ("M_zero", dict(M=0), "M must be 1..4"),
    ("M_five", dict(M=5), "M must be 1..4"),
    ("M_differs", dict(M=2, eM=3), "differs from the ensemble options"),
    ("mode", dict(mode=2), "mode must be"),
    ("weight_zero", dict(weights=(1.0, 0.0)), "weights[1]"),
    ("weight_negative", dict(weights=(-1.0, 1.0)), "weights[0]"),
    ("weight_nan", dict(weights=(1.0, float("nan"))), "weights[1]"),
    ("weight_inf", dict(weights=(float("inf"), 1.0)), "weights[0]"),
    ("null_eopts", dict(eopts=False), "null ensemble options"),
    ("null_opts", dict(opts=False), "null options"),
    ("null_arrays", dict(arrays=False), "null member array"),
    ("null_member", dict(M=3, null=1), "null member 1"),
    ("states", dict(h0=256), "no initial states"),
    ("ws_unaligned", dict(ws=260), "256-byte aligned"),
    ("ws_null", dict(ws=None), "null argument"),
])
def test_refusals_are_statuses_with_their_own_texts(which, head, case, kw, msg):
    L, lib = _lib()
    rc, err = _call(L, lib, which, head, **kw)
    assert rc == -1 and msg in err, (rc, err)
    assert "ensemble" in err, err                    # the new entry points speak for themselves


@BOTH
def test_mismatched_dims_and_constraints(which, head):
    L, lib = _lib()
    bad = (4, 6, 1, 8, 16, 2, 0) if which == "lstm" else (2, 4, 63, 8, 8, 8, 9, 8, 0)      # V = 1; V % 4 != 0
    rc, err = _call(L, lib, which, head, dims=bad)
    assert rc == -1, err
    rc, err = _call(L, lib, which, head, beam=9)
    assert rc == -1 and "1..8" in err, err
    c = L.DecodeConstraints()
    c.no_repeat_ngram = 99
    rc, err = _call(L, lib, which, head, cons=c)
    assert rc == -1 and "no_repeat_ngram" in err, err
    c.no_repeat_ngram = 2
    rc, err = _call(L, lib, which, head, cons=c, cws=None)
    assert rc == -1 and "constraint workspace" in err, err


def test_python_members_of_different_dims_are_refused():
    from gan_image_captioning_amd import engine
    a, b = engine.DecoderEngine(50, 8, 16, 2, 0), engine.DecoderEngine(50, 8, 32, 2, 0)
    with pytest.raises(ValueError, match="member 1 differs"):
        a._ensemble_members([(a, []), (b, [])], [None, None], None)
    with pytest.raises(ValueError, match="1..4 members"):
        a._ensemble_members([(a, [])] * 5, [None] * 5, None)
    with pytest.raises(ValueError, match="first member"):
        a._ensemble_members([(b, [])], [None], None)


def _host_bytes(dims, M, k, beam, attn):
    """The workspace restated on the host: decode.hip's header comment, every region rounded up to 256 bytes."""
    r = lambda n: (n + 255) & ~255                                # noqa: E731
    if attn:
        B, L, V, E, H, Cc, P, A, dt = dims
        NL, fused = 1, True
    else:
        B, L, V, E, H, NL, dt = dims
        Cc = P = A = 0
        from gan_image_captioning_amd import engine
        fused = B * k <= engine.DecoderEngine(V, E, H, NL, dt).fused_rollout_rows()
    R, asz, nblk = B * k, 4 if dt == 0 else 2, -(-V // 64)
    rec = sum(r(2 * R * ((E + Cc if l == 0 else H) + H) * asz) + r(2 * R * H * 4) for l in range(NL))
    rec += 0 if fused else r(R * 4 * H * 4)
    rec += (r(B * P * A * asz) + r(R * A * 4) + r(R * P * 4)) if attn else 0
    shared = r(R * V * 4)                                          # the mixed logits: always
    if beam:
        shared += 2 * r(R * nblk * 4) + 2 * r(R * nblk * k * 4)
    shared += 5 * r(R * 4) + r(L * R * 4) * (2 if beam else 1) + 2 * r(B * 4) + r(4)
    return rec * M + shared + r(M * R * V * 4)


@pytest.mark.parametrize("which,dims", [("lstm", LSTM_DIMS), ("lstm", LSTM_FUSED), ("attn", ATTN_DIMS), ("lstm", (64, 20, 10000, 512, 512, 1, 1))])
def test_ws_bytes_against_the_host_layout(which, dims):
    L, lib = _lib()
    lstm = which == "lstm"
    d = (L.DecoderDims if lstm else L.AttnDims)(*dims)
    out = C.c_uint64(0)
    for head in ("beam", "sample"):
        fn = getattr(lib, f"gic_{'decoder' if lstm else 'attn'}_ensemble_{head}_ws_bytes")
        sizes = []
        for M in (1, 2, 3, 4):
            assert fn(C.byref(d), M, 5, C.byref(out)) == 0, lib.gic_last_error()
            assert out.value == _host_bytes(dims, M, 5, head == "beam", not lstm), (head, M)
            sizes.append(out.value)
        assert all(b > a for a, b in zip(sizes, sizes[1:]))          # every member adds its regions
        for M in (0, 5):
            assert fn(C.byref(d), M, 5, C.byref(out)) == -1 and "M must be 1..4" in lib.gic_last_error().decode()
        assert fn(C.byref(d), 2, 9, C.byref(out)) == -1
        assert fn(C.byref(d), 2, 5, None) == -1 and "null out" in lib.gic_last_error().decode()


def test_ensemble_mix_argument_statuses():
    L, lib = _lib()
    w = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    for args, msg in (((256, 0, 4, 8, w, 0, 256, None), "M must be 1..4"), ((256, 5, 4, 8, w, 0, 256, None), "M must be 1..4"),
                      ((256, 2, 0, 8, w, 0, 256, None), "rows"), ((256, 2, (1 << 24) + 1, 8, w, 0, 256, None), "rows"),
                      ((256, 2, 4, 1, w, 0, 256, None), "V >= 2"), ((None, 2, 4, 8, w, 0, 256, None), "null argument"),
                      ((256, 2, 4, 8, None, 0, 256, None), "null argument"), ((256, 2, 4, 8, w, 0, None, None), "null argument"),
                      ((256, 2, 4, 8, w, 3, 256, None), "mode must be"), ((258, 2, 4, 8, w, 0, 256, None), "4-byte aligned"),
                      ((256, 2, 4, 8, (C.c_float * 4)(1.0, 0.0), 0, 256, None), "weights[1]")):
        assert lib.gic_ensemble_mix(*args) == -1
        assert msg in lib.gic_last_error().decode(), (msg, lib.gic_last_error())


def test_engine_ensemble_opts():
    from gan_image_captioning_amd import engine
    o = engine.ensemble_opts(3, (0.6, 0.3, 0.1), "logprob")
    assert (o.M, o.mode) == (3, 1) and [round(v, 6) for v in list(o.weights)[:3]] == [0.6, 0.3, 0.1]
    assert list(engine.ensemble_opts(2).weights)[:2] == [1.0, 1.0] and engine.ensemble_opts(2).mode == 0
    for bad, msg in (((2, (1.0,), "prob"), "2 members"), ((2, (1.0, 0.0), "prob"), "> 0"), ((2, None, "mean"), "mode"),
                     ((5, None, "prob"), "1..4"), ((0, None, "prob"), "1..4"), ((2, (1.0, float("nan")), "prob"), "> 0")):
        with pytest.raises(ValueError, match=msg):
            engine.ensemble_opts(*bad)


# ---------------------------------------------------------------- the oracle against the single-model oracles
def _lstm_members(M, V=50, E=8, H=16, NL=2, B=3):
    members = [BO.random_params(V, E, H, NL, seed=100 + 7 * m + V, scale=3.0) for m in range(M)]
    feats = [torch.randn(B, E, generator=torch.Generator().manual_seed(11 + m)) * 0.5 for m in range(M)]
    return members, feats


@pytest.mark.parametrize("k", [1, 3, 5])
def test_oracle_one_member_is_beam_search(k):
    members, feats = _lstm_members(1)
    for alpha in (0.0, 0.7):
        want = BO.beam_search(members[0], feats[0], k, 9, length_penalty=alpha)
        for mode in EO.MODES:
            got = EO.beam_search(members, feats, k, 9, mode=mode, length_penalty=alpha)
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
            # one member's z is its log-softmax: the same candidates and order, scores to the last rounding of a logsumexp
            torch.testing.assert_close(got[1], want[1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", EO.MODES)
def test_oracle_two_identical_members_equal_one(mode):
    members, feats = _lstm_members(1)
    one = EO.beam_search(members, feats, 3, 9, mode=mode)
    two = EO.beam_search(members * 2, feats * 2, 3, 9, weights=(0.3, 0.7), mode=mode)
    assert torch.equal(one[0], two[0]) and torch.equal(one[2], two[2])
    torch.testing.assert_close(one[1], two[1], rtol=0, atol=1e-12)


def test_oracle_one_member_is_the_other_oracles():
    members, feats = _lstm_members(1)
    u = torch.rand(7, 3 * 2, 50, generator=torch.Generator().manual_seed(3))
    want = SO.decode(members[0], feats[0], 2, 7, u, 5, 0.9, 0.7)
    got = EO.sample(members, feats, 2, 7, u, top_k=5, top_p=0.9, temperature=0.7)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    torch.testing.assert_close(got[1], want[1], rtol=0, atol=1e-12)
    want = CO.beam_search(members[0], feats[0], 4, 8, groups=2, diversity=0.5, no_repeat_ngram=2, min_length=4, suppress_tokens=(1, 3))
    got = EO.beam_search(members, feats, 4, 8, groups=2, diversity=0.5, no_repeat_ngram=2, min_length=4, suppress_tokens=(1, 3))
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    params, feats_a, fmap = AO.random_problem(2, 64, 8, 8, 8, 9, 8, seed=5)
    want = AO.beam_search(params, feats_a, fmap, 3, 5)
    got = EO.attn_beam_search([params], [feats_a], [fmap], 3, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


def test_oracle_mix_is_the_case_reference_and_members_matter():
    x, w = EC.make_inputs(EC.BY_ID["prob-M3-uneven"])
    for mode in EO.MODES:
        assert torch.allclose(EO.mix(x.double(), EO.normalise(w, 3), mode), EC.reference(x, w, mode), rtol=0, atol=1e-12)
    members, feats = _lstm_members(2)
    both = EO.beam_search(members, feats, 3, 9)
    alone = EO.beam_search(members[:1], feats[:1], 3, 9)
    assert not torch.equal(both[0], alone[0])                     # the second member changes the captions
    lean = EO.beam_search(members, feats, 3, 9, weights=(1 - 1e-6, 1e-6))
    assert torch.equal(lean[0], alone[0])
    swapped = EO.beam_search(members[::-1], feats[::-1], 3, 9, weights=(0.3, 0.7))
    straight = EO.beam_search(members, feats, 3, 9, weights=(0.7, 0.3))
    assert torch.equal(swapped[0], straight[0])
    torch.testing.assert_close(swapped[1], straight[1], rtol=0, atol=1e-12)
    ll = EO.sequence_logprob(members, feats, both[0][:, 0], both[2][:, 0])
    torch.testing.assert_close(ll, both[1][:, 0], rtol=0, atol=1e-10)


# ---------------------------------------------------------------- flags and the instructor
def _parse(*argv):
    from gan_image_captioning_amd.args import build_parser, check_eval_ensemble
    return check_eval_ensemble(build_parser().parse_args(list(argv)))


def test_flags_default_to_no_ensemble():
    from gan_image_captioning_amd.args import check_eval_ensemble, default_args
    assert _parse() is None
    assert check_eval_ensemble(default_args()) is None


def test_flag_parsing():
    got = _parse("--eval-ensemble", "a.ckpt, b_ema.ckpt", "--eval-ensemble-ema", "1", "--gen-ema-decay", "0.99", "--eval-ensemble-weights",
                 "0.5,0.3,0.1,0.1", "--eval-ensemble-mode", "logprob")
    assert got == {"paths": ["a.ckpt", "b_ema.ckpt"], "with_ema": True, "weights": [0.5, 0.3, 0.1, 0.1], "mode": "logprob"}
    assert _parse("--eval-ensemble", "a.ckpt") == {"paths": ["a.ckpt"], "with_ema": False, "weights": None, "mode": "prob"}


@pytest.mark.parametrize("argv,msg", [
    (("--eval-ensemble", "a.ckpt", "--eval-ema", "1", "--gen-ema-decay", "0.9"), "use one of the two"),
    (("--eval-ensemble-ema", "1", "--eval-ema", "1", "--gen-ema-decay", "0.9"), "use one of the two"),
    (("--eval-ensemble-ema", "1"), "--gen-ema-decay > 0"),
    (("--eval-ensemble", "a,b,c,d"), "at most 4"),
    (("--eval-ensemble", "a,b,c", "--eval-ensemble-ema", "1", "--gen-ema-decay", "0.9"), "at most 4"),
    (("--eval-ensemble", "a.ckpt", "--eval-ensemble-weights", "0.5,0.3,0.2"), "3 values for 2 members"),
    (("--eval-ensemble", "a.ckpt", "--eval-ensemble-weights", "0.5,0"), "> 0"),
    (("--eval-ensemble-weights", "0.5,0.5"), "need an ensemble"),
    (("--eval-ensemble-mode", "logprob"), "need an ensemble"),
])
def test_refused_flag_combinations(argv, msg):
    with pytest.raises(ValueError, match=msg):
        _parse(*argv)


def test_instructor_refuses_at_construction_before_the_device():
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    with pytest.raises(ValueError, match="use one of the two"):
        GANInstructor(default_args(device="cpu", eval_ensemble=["a.ckpt"], eval_ema=1, gen_ema_decay=0.9), None, None)
    with pytest.raises(ValueError, match="--gen-ema-decay > 0"):
        GANInstructor(default_args(device="cpu", eval_ensemble_ema=1), None, None)


class _Gen:
    """What GANInstructor.ensemble reads of a generator."""


def test_instructor_member_order(monkeypatch, tmp_path):
    """live, the checkpoints in the order given (both checkpoint formats), the EMA last: built on stand-ins, no device."""
    from gan_image_captioning_amd import training as T

    made, loaded = [], []

    class Member:
        def __init__(self, tag):
            self.tag = tag

        def load_state_dict(self, sd):
            loaded.append((self.tag, sd["tag"]))

    class Ens:
        def __init__(self, members, weights, mode):
            self.members, self.weights, self.mode = list(members), weights, mode

    inst = T.GANInstructor.__new__(T.GANInstructor)
    inst.args = type("A", (), {"device": "cpu"})()
    inst.gen = Member("live")
    inst.gen.state_dict = lambda: {"tag": "ema-weights"}

    class Ema:
        def swapped(self):
            import contextlib
            return contextlib.nullcontext()

    inst.ema = Ema()

    def copy(self, share_trunk=False):
        made.append(share_trunk)
        return Member(f"copy{len(made)}")

    monkeypatch.setattr(T.GANInstructor, "_member_copy", copy)
    monkeypatch.setattr(T, "Ensemble", Ens)
    monkeypatch.setattr(T.engine, "bump_param_epoch", lambda: None)
    a, b = str(tmp_path / "pretrained_model.ckpt"), str(tmp_path / "adv_model.ckpt")
    torch.save({"tag": "a"}, a)
    torch.save({"generator": {"tag": "b"}, "discriminator": {}}, b)
    ens = inst.ensemble(paths=(a, b), with_ema=True, weights=(0.4, 0.3, 0.2, 0.1), mode="logprob")
    assert [m.tag for m in ens.members] == ["live", "copy1", "copy2", "copy3"]
    assert loaded == [("copy1", "a"), ("copy2", "b"), ("copy3", "ema-weights")]
    assert made == [False, False, True]                                   # only the EMA copy sits on the live trunk
    assert ens.weights == (0.4, 0.3, 0.2, 0.1) and ens.mode == "logprob"
    inst.ema = None
    with pytest.raises(ValueError, match="gen-ema-decay"):
        inst.ensemble(with_ema=True)
    assert [m.tag for m in inst.ensemble().members] == ["live"]


def test_eval_gen_is_the_live_generator_by_default():
    from gan_image_captioning_amd import training as T
    inst = T.GANInstructor.__new__(T.GANInstructor)
    inst.gen = object()
    assert inst.eval_ensemble is None and inst._eval_gen() is inst.gen and inst._ensemble is None       # nothing constructed
    inst.eval_ensemble = {"paths": [], "with_ema": True, "weights": None, "mode": "prob"}
    with inst._live_weights():
        assert inst._eval_gen() is inst.gen                               # checkpoint selection never sees the ensemble
