"""Caption sampling and diversity metrics without a GPU: the CPU oracle (tests/sample_oracle.py) against brute force, the C ABI
(symbols, host-only workspace queries, argument statuses before any launch), utils.distinct_n / mbleu4 on hand-worked cases and the
--eval-* sampling flags."""
import ctypes as C
import itertools
import json
import math
import os
import re

import pytest
import torch

from tests import sample_oracle as SO

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NEW = ("gic_sample_logits", "gic_decoder_sample_ws_bytes", "gic_decoder_sample_captions", "gic_attn_sample_ws_bytes",
       "gic_attn_sample_captions")


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- oracle against brute force
def _rows(V, count, seed):
    g = torch.Generator().manual_seed(seed)
    for i in range(count):
        l = torch.randn(V, generator=g) * (0.5 + i % 4)
        if i % 3 == 0:                                      # coarse values: many ties
            l = torch.round(l * 2) / 2
        yield l


@pytest.mark.parametrize("V", [2, 5, 9, 16])
def test_kept_set_matches_full_sort(V):
    for i, l in enumerate(_rows(V, 40, V)):
        for top_k, top_p, tau in itertools.product([0, 1, 2, V - 1, V], [1.0, 0.3, 0.75, 0.95], [0.5, 1.0, 2.0]):
            keep, _ = SO.truncate(l, top_k, top_p, tau)
            assert set(torch.nonzero(keep)[:, 0].tolist()) == SO.kept_brute_force(l, top_k, top_p, tau), (i, top_k, top_p, tau)


def test_ties_at_the_top_k_boundary_are_kept():
    l = torch.tensor([3.0, 1.0, 2.0, 2.0, 2.0, 0.0])
    keep, _ = SO.truncate(l, top_k=2)
    assert keep.tolist() == [True, False, True, True, True, False]
    keep, _ = SO.truncate(l, top_k=1)
    assert keep.tolist() == [True, False, False, False, False, False]


def test_ties_at_the_top_p_boundary_are_kept():
    # masses: the top value alone carries e^2 / (e^2 + 3 e + 1 + 1); asking for a little more keeps all three ties of the 1.0s
    l = torch.tensor([2.0, 1.0, 1.0, 1.0, 0.0, 0.0])
    w = torch.exp(l.double())
    top = float(w[0] / w.sum())
    keep, _ = SO.truncate(l, top_p=top + 1e-3)
    assert keep.tolist() == [True, True, True, True, False, False]
    assert SO.kept_brute_force(l, top_p=top + 1e-3) == {0, 1, 2, 3}


def test_top_p_just_above_and_below_a_cumulative_mass():
    l = torch.tensor([1.5, 0.7, -0.2, -1.0, 0.3])
    q = torch.softmax(l.double(), 0)
    srt = torch.sort(q, descending=True).values
    for j in range(1, 5):
        mass = float(srt[:j].sum())
        below, m_below = SO.truncate(l, top_p=mass - 1e-6)
        above, m_above = SO.truncate(l, top_p=mass + 1e-6)
        assert int(below.sum()) == j and int(above.sum()) == j + 1
        assert m_below == pytest.approx(1e-6, abs=1e-9) and m_above == pytest.approx(1e-6, abs=1e-9)


def test_top_k_1_is_argmax_whatever_the_noise():
    g = torch.Generator().manual_seed(5)
    for l in _rows(30, 20, 7):
        u = torch.rand(30, generator=g)
        tok, lp, kept, dm, _ = SO.draw(l, u, top_k=1)
        if kept == 1:
            assert tok == int(torch.argmax(l)) and dm == math.inf
        assert lp == pytest.approx(float(l.double()[tok] - torch.logsumexp(l.double(), 0)))


def test_draw_is_the_gumbel_argmax_over_the_kept_set():
    g = torch.Generator().manual_seed(2)
    l = torch.randn(12, generator=g)
    for _ in range(30):
        u = torch.rand(12, generator=g)
        keep, _ = SO.truncate(l, 4, 0.8, 0.7)
        y = l.double() / 0.7 + SO.gumbel(u)
        best = max((v for v in range(12) if keep[v]), key=lambda v: (float(y[v]), -v))
        assert SO.draw(l, u, 4, 0.8, 0.7)[0] == best


def test_draw_frequencies_follow_the_truncated_distribution():
    g = torch.Generator().manual_seed(9)
    l = torch.tensor([2.0, 1.0, 0.5, 0.0, -1.0])
    keep, _ = SO.truncate(l, top_k=4, top_p=0.9, temperature=0.8)
    p = torch.where(keep, torch.softmax(l.double() / 0.8, 0), torch.zeros(5, dtype=torch.float64))
    p = p / p.sum()
    N = 4000
    counts = torch.zeros(5)
    for _ in range(N):
        counts[SO.draw(l, torch.rand(5, generator=g), 4, 0.9, 0.8)[0]] += 1
    sd = torch.sqrt(N * p * (1 - p))
    assert ((counts - N * p).abs() <= 5 * sd + 1e-9).all(), (counts, N * p)


def test_oracle_decode_finishes_rows_and_pads():
    from tests.beam_oracle import random_params
    V, E, H, B, n, L = 9, 4, 8, 2, 3, 6
    params = random_params(V, E, H, 1, seed=3, scale=3.0)
    params[-1] = params[-1].clone()
    params[-1][2] += 1.5
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(1))
    u = torch.rand(L, B * n, V, generator=torch.Generator().manual_seed(2))
    ids, scores, lengths, margin = SO.decode(params, feats, n, L, u)
    for b in range(B):
        for j in range(n):
            k = int(lengths[b, j])
            assert 1 <= k <= L and (ids[b, j, k:] == 0).all()
            assert k == L or int(ids[b, j, k - 1]) == 2
            assert (ids[b, j, :k - 1] != 2).all()
            assert float(scores[b, j]) < 0


# ---------------------------------------------------------------- the C ABI
def test_symbols_declared_bound_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "gic_sample_opts" in hdr
    assert lib.gic_abi_version() == 5


@pytest.mark.parametrize("shape", [(64, 20, 10000, 512, 512, 1, 1), (4, 6, 50, 8, 16, 2, 0), (600, 6, 52, 8, 16, 1, 0)])
def test_decoder_ws_bytes_match_the_engine(shape):
    from gan_image_captioning_amd import engine
    L, lib = _lib()
    B, Lc, V, E, H, NL, dt = shape
    eng = engine.DecoderEngine(V, E, H, NL, dt)
    sizes = []
    for n in range(1, 9):
        out = C.c_uint64(0)
        assert lib.gic_decoder_sample_ws_bytes(C.byref(L.DecoderDims(B, Lc, V, E, H, NL, dt)), n, C.byref(out)) == 0
        assert eng.sample_ws_bytes(B, Lc, n) == out.value and out.value % 256 == 0
        R = B * n
        assert out.value >= R * V * 4 + Lc * R * 4 + sum(2 * R * ((E if l == 0 else H) + H) * (4 if dt == 0 else 2) for l in range(NL))
        sizes.append(out.value)
    assert sizes == sorted(sizes) and len(set(sizes)) == 8


def test_attn_ws_bytes_match_the_engine():
    from gan_image_captioning_amd import engine
    L, lib = _lib()
    eng = engine.AttnDecoderEngine(10000, 512, 512, 2048, 49, 512, 1)
    for n in (1, 5, 8):
        out = C.c_uint64(0)
        assert lib.gic_attn_sample_ws_bytes(C.byref(L.AttnDims(32, 20, 10000, 512, 512, 2048, 49, 512, 1)), n, C.byref(out)) == 0
        assert eng.sample_ws_bytes(32, 20, n) == out.value
        R = 32 * n
        assert out.value >= 2 * R * (512 + 2048 + 512) * 2 + 32 * 49 * 512 * 2 + R * 10000 * 4


BAD = [("n0", dict(num_samples=0)), ("n9", dict(num_samples=9)), ("k_neg", dict(top_k=-1)), ("k_gt_V", dict(top_k=65)),
       ("p_nan", dict(top_p=float("nan"))), ("p_zero", dict(top_p=0.0)), ("p_neg", dict(top_p=-0.5)), ("p_gt1", dict(top_p=1.01)),
       ("t_zero", dict(temperature=0.0)), ("t_neg", dict(temperature=-1.0)), ("t_inf", dict(temperature=float("inf"))),
       ("t_nan", dict(temperature=float("nan"))), ("eos", dict(eos_id=64)), ("eos_neg", dict(eos_id=-1)), ("pad", dict(pad_id=64)),
       ("pad_neg", dict(pad_id=-2)), ("L", dict(L=1025)), ("rows", dict(B=(1 << 21) + 1, num_samples=8)), ("ws_align", dict(ws=4100))]


def _opts(L, num_samples=3, top_k=0, top_p=1.0, temperature=1.0, eos_id=2, pad_id=0):
    o = L.SampleOpts()
    o.num_samples, o.top_k, o.top_p, o.temperature, o.eos_id, o.pad_id = num_samples, top_k, top_p, temperature, eos_id, pad_id
    return o


def _split(kw):
    kw = dict(kw)
    shape = dict(B=kw.pop("B", 4), L=kw.pop("L", 6))
    ws = kw.pop("ws", 4096)
    return shape, ws, kw


@pytest.mark.parametrize("case,kw", BAD, ids=[c for c, _ in BAD])
def test_decoder_sample_rejects_bad_arguments(case, kw):
    L, lib = _lib()
    shape, ws, o = _split(kw)
    d = L.DecoderDims(shape["B"], shape["L"], 64, 8, 16, 1, 0)
    p, s = L.DecoderParams(), L.DecoderShadow()
    p.embed = p.b_out = s.wout = 4096
    s.wcat[0] = s.bsum[0] = 4096
    fake = C.c_void_p(4096)
    rc = lib.gic_decoder_sample_captions(C.byref(d), C.byref(p), C.byref(s), C.byref(_opts(L, **o)), C.c_void_p(ws), fake, None, 1, fake,
                                         fake, fake, None)
    assert rc == -1, (case, lib.gic_last_error().decode())


@pytest.mark.parametrize("case,kw", BAD, ids=[c for c, _ in BAD])
def test_attn_sample_rejects_bad_arguments(case, kw):
    L, lib = _lib()
    shape, ws, o = _split(kw)
    d = L.AttnDims(shape["B"], shape["L"], 64, 8, 16, 8, 4, 8, 0)
    p, s = L.AttnParams(), L.AttnShadow()
    for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
        setattr(p, n, 4096)
    for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
        setattr(s, n, 4096)
    fake = C.c_void_p(4096)
    rc = lib.gic_attn_sample_captions(C.byref(d), C.byref(p), C.byref(s), C.byref(_opts(L, **o)), C.c_void_p(ws), fake, fake, None, 1,
                                      fake, fake, fake, None)
    assert rc == -1, (case, lib.gic_last_error().decode())


def test_ws_bytes_and_logits_reject_bad_arguments():
    L, lib = _lib()
    out = C.c_uint64(0)
    d = L.DecoderDims(4, 6, 64, 8, 16, 1, 0)
    for n in (0, 9, -1):
        assert lib.gic_decoder_sample_ws_bytes(C.byref(d), n, C.byref(out)) == -1
        assert lib.gic_attn_sample_ws_bytes(C.byref(L.AttnDims(4, 6, 64, 8, 16, 8, 4, 8, 0)), n, C.byref(out)) == -1
    assert lib.gic_decoder_sample_ws_bytes(C.byref(L.DecoderDims(4, 1025, 64, 8, 16, 1, 0)), 3, C.byref(out)) == -1
    assert lib.gic_decoder_sample_ws_bytes(C.byref(d), 3, None) == -1
    assert lib.gic_decoder_sample_captions(C.byref(d), None, None, None, None, None, None, 0, None, None, None, None) == -1
    fake = C.c_void_p(4096)
    for o in (_opts(L, top_k=-1), _opts(L, top_k=65), _opts(L, top_p=0.0), _opts(L, top_p=float("nan")), _opts(L, temperature=0.0),
              _opts(L, temperature=float("inf"))):
        assert lib.gic_sample_logits(fake, 64, 8, 64, C.byref(o), None, 0, 0, fake, None, None, None) == -1
    o = _opts(L)
    assert lib.gic_sample_logits(fake, 64, 8, 1, C.byref(o), None, 0, 0, fake, None, None, None) == -1        # V < 2
    assert lib.gic_sample_logits(fake, 32, 8, 64, C.byref(o), None, 0, 0, fake, None, None, None) == -1       # ld < V
    assert lib.gic_sample_logits(fake, 64, 0, 64, C.byref(o), None, 0, 0, fake, None, None, None) == -1       # no rows
    assert lib.gic_sample_logits(None, 64, 8, 64, C.byref(o), None, 0, 0, fake, None, None, None) == -1
    assert lib.gic_sample_logits(fake, 64, 8, 64, None, None, 0, 0, fake, None, None, None) == -1


def test_attention_decoder_needs_the_map():
    from gan_image_captioning_amd.generator import AttnDecoder
    with pytest.raises(NotImplementedError):
        AttnDecoder.sample_captions(None, None)


# ---------------------------------------------------------------- diversity metrics
def _utils():
    from gan_image_captioning_amd import utils
    return utils


def test_distinct_n_hand_worked():
    U = _utils()
    caps = [["a", "cat", "sat"], ["a", "dog", "sat"], ["a", "cat"]]
    # unigrams: a a a cat dog cat sat sat -> 4 unique of 8; bigrams: (a cat) (cat sat) (a dog) (dog sat) (a cat) -> 4 of 5
    assert U.distinct_n(caps, 1) == pytest.approx(4 / 8)
    assert U.distinct_n(caps, 2) == pytest.approx(4 / 5)
    assert U.distinct_n(caps, 3) == pytest.approx(2 / 2)
    assert U.distinct_n([["a"], []], 2) == 0.0
    same = [["the", "cat", "sat", "down"]] * 5
    assert U.distinct_n(same, 1) == pytest.approx(4 / 20)     # the minimum for these captions: every n-gram repeated 5 times
    assert U.distinct_n(same, 2) == pytest.approx(3 / 15)


def test_mbleu4_hand_worked():
    U = _utils()
    same = ["the", "cat", "sat", "on", "the", "mat"]
    assert U.mbleu4([[same] * 3, [["a", "b", "c", "d", "e"]] * 2]) == pytest.approx(1.0)
    assert U.mbleu4([[same]]) == 0.0                          # one sample: skipped, nothing left
    a, b = ["a", "b", "c", "d"], ["w", "x", "y", "z"]
    assert U.mbleu4([[a, b]]) == 0.0                          # no shared n-gram
    # two samples differing in the last token: each against the other, p1 = 6/8 ... as bleu_score of the pairs
    c1 = "the cat sat on the mat".split()
    c2 = "the cat sat on the rug".split()
    want = U.bleu_score([c1, c2], [[c2], [c1]])
    assert U.mbleu4([[c1, c2], [c1]]) == pytest.approx(want)
    assert want == pytest.approx(math.exp(0.25 * (math.log(10 / 12) + math.log(8 / 10) + math.log(6 / 8) + math.log(4 / 6))))


# ---------------------------------------------------------------- flags
def test_eval_sampling_flags_default_off():
    from gan_image_captioning_amd.args import build_parser
    a = build_parser().parse_args([])
    assert (a.eval_num_samples, a.eval_top_k, a.eval_top_p, a.eval_sample_temperature) == (0, 0, 1.0, 1.0)
    a = build_parser().parse_args(["--eval-num-samples", "5", "--eval-top-k", "50", "--eval-top-p", "0.9",
                                   "--eval-sample-temperature", "0.7"])
    assert (a.eval_num_samples, a.eval_top_k, a.eval_top_p, a.eval_sample_temperature) == (5, 50, 0.9, 0.7)
    flags = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_flags.json")))
    names = flags if isinstance(flags, list) else list(flags)
    opts = {a for act in build_parser()._actions for a in act.option_strings}
    for f in names:
        f = f if isinstance(f, str) else f[0]
        assert f in opts or ("--" + f.lstrip("-").replace("_", "-")) in opts, f
