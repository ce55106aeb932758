"""Beam search and BLEU-4 without a GPU: the C ABI (symbols, host-only workspace query, argument statuses), the CPU oracle
against brute force, utils.bleu_score on hand-worked cases, the --eval-beam-size flag."""
import ctypes as C
import itertools
import json
import math
import os
import re

import pytest
import torch

from tests import beam_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gic_decoder_beam_ws_bytes", "gic_decoder_beam_search")


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L


def test_symbols_declared_bound_exported():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "gic_decoder_beam_opts" in hdr
    assert lib.gic_abi_version() == 5


def _dims(B, Lc, V, E, H, NL, dt):
    return _lib().DecoderDims(B, Lc, V, E, H, NL, dt)


def test_workspace_query_is_host_only_and_matches_python():
    from gan_image_captioning_amd import engine
    L = _lib()
    for (B, Lc, V, E, H, NL, dt, k) in [(64, 20, 10000, 512, 512, 1, 1, 5), (4, 6, 50, 8, 16, 2, 0, 3), (600, 6, 50, 8, 16, 2, 0, 1)]:
        out = C.c_uint64(0)
        assert L.load().gic_decoder_beam_ws_bytes(C.byref(_dims(B, Lc, V, E, H, NL, dt)), k, C.byref(out)) == 0
        eng = engine.DecoderEngine(V, E, H, NL, dt)
        assert eng.beam_ws_bytes(B, Lc, k) == out.value > 0
        rows, nblk, asz = B * k, (V + 63) // 64, 4 if dt == 0 else 2
        floor = sum(2 * rows * ((E if l == 0 else H) + H) * asz + 2 * rows * H * 4 for l in range(NL)) + rows * nblk * (8 + 8 * k)
        assert out.value >= floor
    k3 = C.c_uint64(0)
    k5 = C.c_uint64(0)
    L.load().gic_decoder_beam_ws_bytes(C.byref(_dims(8, 10, 64, 32, 512, 1, 0)), 3, C.byref(k3))
    L.load().gic_decoder_beam_ws_bytes(C.byref(_dims(8, 10, 64, 32, 512, 1, 0)), 5, C.byref(k5))
    assert k5.value > k3.value


def test_invalid_arguments_return_statuses():
    L = _lib()
    lib = L.load()
    out = C.c_uint64(0)
    d = _dims(4, 6, 50, 8, 16, 2, 0)
    for k in (0, 9, -1):
        assert lib.gic_decoder_beam_ws_bytes(C.byref(d), k, C.byref(out)) == -1
    assert lib.gic_decoder_beam_ws_bytes(None, 3, C.byref(out)) == -1
    assert lib.gic_decoder_beam_ws_bytes(C.byref(d), 3, None) == -1
    small = _dims(4, 6, 4, 8, 16, 1, 0)
    assert lib.gic_decoder_beam_ws_bytes(C.byref(small), 5, C.byref(out)) == -1      # beam > V
    p, s = L.DecoderParams(), L.DecoderShadow()
    fake = C.c_void_p(4096)
    for beam, eos, pad in ((0, 2, 0), (9, 2, 0), (3, 50, 0), (3, -1, 0), (3, 2, 50), (3, 2, -3)):
        o = L.DecoderBeamOpts(beam, eos, pad, 0.0, None, None)
        st = lib.gic_decoder_beam_search(C.byref(d), C.byref(p), C.byref(s), C.byref(o), fake, fake, fake, fake, fake, None)
        assert st == -1, (beam, eos, pad)
    o = L.DecoderBeamOpts(3, 2, 0, 0.0, None, None)
    assert lib.gic_decoder_beam_search(C.byref(d), C.byref(p), C.byref(s), None, fake, fake, fake, fake, fake, None) == -1
    assert lib.gic_decoder_beam_search(C.byref(d), C.byref(p), C.byref(s), C.byref(o), None, fake, fake, fake, fake, None) == -1
    assert lib.gic_decoder_beam_search(C.byref(d), C.byref(p), C.byref(s), C.byref(o), fake, fake, fake, fake, fake, None) == -1  # null weights


def test_oracle_equals_brute_force_at_k_equal_v():
    V, E, H, NL, L = 50, 8, 16, 2, 2
    params = BO.random_params(V, E, H, NL, seed=1, scale=4.0)
    params[-1][2] += 2.0                                   # <E> likely enough that some first tokens end the caption
    feats = torch.randn(2, E, generator=torch.Generator().manual_seed(2))
    ids, scores, lengths, _ = BO.beam_search(params, feats, V, L)
    p = [t.double() for t in params]
    layers = [p[1 + 4 * l:5 + 4 * l] for l in range(NL)]

    def run(x, h, c):
        inp = x
        for l in range(NL):
            h[l], c[l] = BO.lstm_cell(inp, h[l], c[l], *layers[l])
            inp = h[l]
        return torch.log_softmax(inp @ p[-2].t() + p[-1], dim=-1), h, c

    for b in range(2):
        z = [torch.zeros(1, H, dtype=torch.float64) for _ in range(NL)]
        lp1, h1, c1 = run(feats[b:b + 1].double(), list(z), list(z))
        allseq = []
        for t1 in range(V):
            if t1 == 2:
                allseq.append((float(lp1[0, t1]), (t1, 0), 1))
                continue
            lp2, _, _ = run(p[0][t1:t1 + 1], list(h1), list(c1))
            for t2 in range(V):
                allseq.append((float(lp1[0, t1] + lp2[0, t2]), (t1, t2), 2 if t2 == 2 else 2))
        allseq.sort(key=lambda e: -e[0])
        best = allseq[:V]
        assert [tuple(r) for r in ids[b].tolist()] == [e[1] for e in best]
        torch.testing.assert_close(scores[b], torch.tensor([e[0] for e in best], dtype=torch.float64))
        assert lengths[b].tolist() == [e[2] for e in best]


def test_oracle_k1_equals_greedy():
    V, E, H, NL, L = 50, 8, 16, 2, 9
    params = BO.random_params(V, E, H, NL, seed=4, scale=3.0)
    params[-1][2] += 1.0
    feats = torch.randn(6, E, generator=torch.Generator().manual_seed(5))
    ids, _, _, _ = BO.beam_search(params, feats, 1, L)
    assert torch.equal(ids[:, 0], BO.greedy(params, feats, L))


def _bleu():
    from gan_image_captioning_amd.utils import bleu_score
    return bleu_score


def test_bleu_identical_and_disjoint():
    bleu = _bleu()
    c = [["a", "cat", "sat", "on", "the", "mat"], ["dogs", "run", "in", "the", "park", "today"]]
    assert bleu(c, [[x] for x in c]) == pytest.approx(1.0)
    assert bleu([["a", "b", "c", "d"]], [[["a", "b", "c", "e"]]]) == 0.0


def test_bleu_hand_worked_brevity_penalty():
    # candidate 6 tokens, reference 8: p1 = 6/6, p2 = 5/5, p3 = 4/4, p4 = 3/3; BP = exp(1 - 8/6)
    bleu = _bleu()
    cand = ["the", "cat", "sat", "on", "the", "mat"]
    ref = ["the", "cat", "sat", "on", "the", "mat", "at", "home"]
    assert bleu([cand], [[ref]]) == pytest.approx(math.exp(1 - 8 / 6), rel=1e-12)


def test_bleu_hand_worked_clipping_multiple_references():
    # cand "the the the cat sat down" (6), refs "the cat sat" (3) and "the the cat sat on" (5): closest length 5 -> BP 1.
    # 1-grams: the 3 -> clip max(1, 2) = 2, cat 1, sat 1, down 0 -> 4/6.  2-grams: (the the) 2 -> 1, (the cat) 1, (cat sat) 1,
    # (sat down) 0 -> 3/5.  3-grams: (the the the) 0, (the the cat) 1, (the cat sat) 1, (cat sat down) 0 -> 2/4.
    # 4-grams: (the the the cat) 0, (the the cat sat) 1, (the cat sat down) 0 -> 1/3.
    bleu = _bleu()
    cand = "the the the cat sat down".split()
    refs = ["the cat sat".split(), "the the cat sat on".split()]
    want = math.exp(0.25 * (math.log(4 / 6) + math.log(3 / 5) + math.log(2 / 4) + math.log(1 / 3)))
    assert bleu([cand], [refs]) == pytest.approx(want, rel=1e-12)
    assert want == pytest.approx(0.5081327, rel=1e-6)


def test_eval_beam_size_flag():
    from gan_image_captioning_amd.args import build_parser
    args = build_parser().parse_args([])
    assert args.eval_beam_size == 0
    assert build_parser().parse_args(["--eval-beam-size", "3"]).eval_beam_size == 3
    flags = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_flags.json")))
    names = flags if isinstance(flags, list) else list(flags)
    opts = {a for act in build_parser()._actions for a in act.option_strings}
    for f in names:
        f = f if isinstance(f, str) else f[0]
        assert f in opts or ("--" + f.lstrip("-").replace("_", "-")) in opts, f
