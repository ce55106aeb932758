"""Diverse beam search without a GPU: the C ABI (symbols, struct layout, argument statuses before any launch), the float64 oracle
(tests/diverse_beam_oracle.py) against plain beam search, greedy decoding and a brute-force enumeration, and the evaluation flags."""
import ctypes as C
import itertools
import math
import os
import re

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import diverse_beam_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gic_decoder_diverse_beam_search", "gic_attn_diverse_beam_search")


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


def test_symbols_declared_bound_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.gic_abi_version() == 5


def test_struct_matches_header():
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    body = re.search(r"typedef struct gic_diverse_beam_opts \{(.*?)\} gic_diverse_beam_opts;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*([a-z_0-9]+)\s+([a-z_]+);", re.sub(r"/\*.*?\*/", "", body), re.M)
    assert fields == [("gic_decoder_beam_opts", "beam"), ("int32_t", "groups"), ("float", "diversity")]
    assert [f[0] for f in L.DiverseBeamOpts._fields_] == ["beam", "groups", "diversity"]
    base = C.sizeof(L.DecoderBeamOpts)
    assert base == 16 + 2 * C.sizeof(C.c_void_p)
    assert L.DiverseBeamOpts.groups.offset == base and L.DiverseBeamOpts.diversity.offset == base + 4
    assert C.sizeof(L.DiverseBeamOpts) == base + 8


def _opts(L, beam=4, groups=2, diversity=0.5, eos=2, pad=0, lp=0.0):
    o = L.DiverseBeamOpts()
    o.beam.beam, o.beam.eos_id, o.beam.pad_id, o.beam.length_penalty = beam, eos, pad, lp
    o.groups, o.diversity = groups, diversity
    return o


def _lstm_call(L, lib, dims=(4, 6, 50, 8, 16, 2, 0), ws=256, **kw):
    d = L.DecoderDims(*dims)
    p, s = L.DecoderParams(), L.DecoderShadow()
    p.embed, p.w_out, p.b_out, s.wout = 256, 256, 256, 256
    for l in range(L.MAX_LAYERS):
        s.wcat[l], s.bsum[l] = 256, 256
    o = _opts(L, **kw)
    rc = lib.gic_decoder_diverse_beam_search(C.byref(d), C.byref(p), C.byref(s), C.byref(o), ws, 256, 256, 256, 256, None)
    return rc, lib.gic_last_error().decode()


def _attn_call(L, lib, dims=(2, 4, 64, 8, 8, 8, 4, 8, 0), ws=256, **kw):
    d = L.AttnDims(*dims)
    p, s = L.AttnParams(), L.AttnShadow()
    for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
        setattr(p, n, 256)
    for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
        setattr(s, n, 256)
    o = _opts(L, **kw)
    rc = lib.gic_attn_diverse_beam_search(C.byref(d), C.byref(p), C.byref(s), C.byref(o), ws, 256, 256, 256, 256, 256, None, None)
    return rc, lib.gic_last_error().decode()


@pytest.mark.parametrize("which", ["lstm", "attn"])
@pytest.mark.parametrize("case,kw,msg", [
    ("groups0", dict(groups=0), "groups"),
    ("groups_neg", dict(groups=-2), "groups"),
    ("groups_not_dividing", dict(beam=6, groups=4), "groups"),
    ("groups_gt_beam", dict(beam=2, groups=4), "groups"),
    ("nan", dict(diversity=float("nan")), "diversity"),
    ("negative", dict(diversity=-0.5), "diversity"),
    ("inf", dict(diversity=float("inf")), "diversity"),
    ("beam0", dict(beam=0, groups=1), "beam size"),
    ("beam9", dict(beam=9, groups=3), "beam size"),
    ("eos", dict(eos=64), "eos_id"),
    ("pad", dict(pad=-1), "pad_id"),
    ("lp_nan", dict(lp=float("nan")), "NaN"),
    ("ws_align", dict(ws=260), "256-byte aligned"),
    ("null_ws", dict(ws=None), "null argument"),
])
def test_invalid_arguments_return_a_status(which, case, kw, msg):
    L, lib = _lib()
    rc, err = (_lstm_call if which == "lstm" else _attn_call)(L, lib, **kw)
    assert rc == -1 and msg in err, (rc, err)


def test_null_options():
    L, lib = _lib()
    d, a = L.DecoderDims(4, 6, 50, 8, 16, 2, 0), L.AttnDims(2, 4, 64, 8, 8, 8, 4, 8, 0)
    assert lib.gic_decoder_diverse_beam_search(C.byref(d), None, None, None, 256, 256, 256, 256, 256, None) == -1
    assert "null options" in lib.gic_last_error().decode()
    assert lib.gic_attn_diverse_beam_search(C.byref(a), None, None, None, 256, 256, 256, 256, 256, 256, None, None) == -1
    assert "null options" in lib.gic_last_error().decode()


def _lstm_problem(seed, B=3, V=40, E=8, H=16, NL=2, eos_bias=1.5):
    params = BO.random_params(V, E, H, NL, seed=seed, scale=4.0)
    params[-1][2] += eos_bias
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(seed + 1))
    return params, feats


@pytest.mark.parametrize("lam", [0.0, 0.5, 3.0, 1e6])
@pytest.mark.parametrize("k", [2, 5])
def test_oracle_one_group_is_beam_search(k, lam):
    params, feats = _lstm_problem(k)
    for alpha in (0.0, 0.7):
        want = BO.beam_search(params, feats, k, 9, length_penalty=alpha)
        got = DO.diverse_beam_search(params, feats, k, 1, lam, 9, length_penalty=alpha)
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b)


def test_oracle_one_beam_per_group_without_penalty_is_greedy():
    params, feats = _lstm_problem(7, B=4)
    ids, _, _, _ = DO.diverse_beam_search(params, feats, 4, 4, 0.0, 9)
    greedy = BO.greedy(params, feats, 9)
    for j in range(4):
        assert torch.equal(ids[:, j], greedy)


def test_oracle_zero_penalty_groups_are_independent_beams():
    params, feats = _lstm_problem(8)
    ids, scores, lengths, _ = DO.diverse_beam_search(params, feats, 6, 2, 0.0, 8)
    ids3, scores3, lengths3, _ = BO.beam_search(params, feats, 3, 8)
    for g in range(2):
        assert torch.equal(ids[:, 3 * g:3 * g + 3], ids3)
        torch.testing.assert_close(scores[:, 3 * g:3 * g + 3], scores3)            # (six rows per matrix product against three)
        assert torch.equal(lengths[:, 3 * g:3 * g + 3], lengths3)


def test_oracle_large_penalty_separates_first_tokens():
    params, feats = _lstm_problem(9, B=4)
    ids, _, _, _ = DO.diverse_beam_search(params, feats, 8, 8, 1e4, 6)
    for b in range(4):
        assert len(set(ids[b, :, 0].tolist())) == 8


def _brute_group(score, fin, logp, rows, kg, lam, h, pad_id):
    """Every kg-subset of the group's candidates over the WHOLE vocabulary; the best by the sum of keys, ties to the lexicographically
    smallest (parent, rank in the full order) list."""
    V = logp.shape[1]
    cands = []
    for jl, j in enumerate(rows):
        if fin[j]:
            cands.append((score[j], j, jl, 0, pad_id, score[j]))
            continue
        order = torch.sort(-logp[j], stable=True).indices.tolist()
        for q, tok in enumerate(order[:V]):
            raw = score[j] + float(logp[j, tok])
            cands.append((raw, j, jl, q, tok, raw - lam * h.get(tok, 0)))
    best = None
    for sub in itertools.combinations(range(len(cands)), kg):
        tot = sum(cands[i][5] for i in sub)
        key = (-tot, sorted((cands[i][2], cands[i][3]) for i in sub))
        if best is None or key < best[0]:
            best = (key, sub)
    kept = sorted((cands[i] for i in best[1]), key=lambda e: (-e[5], e[2], e[3]))
    return kept


@pytest.mark.parametrize("lam", [0.0, 0.3, 2.0, 50.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_equals_brute_force_one_step(seed, lam):
    """V = 5, K = 4, G = 2: the step after a first step (two live or finished parents per group), enumerated over every token of the
    vocabulary and every K'-subset, against the oracle's two-step search from its top-K candidates."""
    V, E, H, NL, K, G = 5, 6, 8, 1, 4, 2
    kg = K // G
    params = BO.random_params(V, E, H, NL, seed=seed + 10, scale=4.0)
    params[-1][2] += 1.0
    feats = torch.randn(1, E, generator=torch.Generator().manual_seed(seed))
    ids, scores, lengths, _ = DO.diverse_beam_search(params, feats, K, G, lam, 2)
    # step 0 from the oracle's own first step (checked by the brute force below too), step 1 brute-forced
    p = [t.double() for t in params]
    st = DO._LstmStepper(p, feats[0].double(), K)
    score = [0.0 if j % kg == 0 else -math.inf for j in range(K)]
    fin = [False] * K
    seqs = [[] for _ in range(K)]
    ln = [0] * K
    for t in range(2):
        logits, _ = st.step()
        logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        h, sel = {}, []
        for g in range(G):
            kept = _brute_group(score, fin, logp, range(g * kg, (g + 1) * kg), kg, lam, h, 0)
            for e in kept:
                if not fin[e[1]]:
                    h[e[4]] = h.get(e[4], 0) + 1
            sel += kept
        seqs = [seqs[e[1]] + [e[4]] for e in sel]
        ln = [ln[e[1]] if fin[e[1]] else t + 1 for e in sel]
        fin = [fin[e[1]] or e[4] == 2 for e in sel]
        score = [e[0] for e in sel]
        st.reorder([e[1] for e in sel], [e[4] for e in sel])
    for g in range(G):
        order = sorted(range(g * kg, (g + 1) * kg), key=lambda j: (-score[j], j))
        assert [seqs[j] for j in order] == ids[0, g * kg:(g + 1) * kg].tolist(), (g, lam)
        torch.testing.assert_close(scores[0, g * kg:(g + 1) * kg], torch.tensor([score[j] for j in order], dtype=torch.float64))
        assert lengths[0, g * kg:(g + 1) * kg].tolist() == [ln[j] for j in order]


def test_attention_oracle_one_group_is_beam_search():
    params, feats, fmap = AO.random_problem(2, 24, 8, 16, 8, 5, 8, seed=3, scale=3.0)
    params[6] = params[6].clone()
    params[6][2] += 1.0
    want = AO.beam_search(params, feats, fmap, 3, 6, length_penalty=0.7)
    got = DO.attn_diverse_beam_search(params, feats, fmap, 3, 1, 2.0, 6, length_penalty=0.7)
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(a, b)
    ids, _, _, alphas, _ = DO.attn_diverse_beam_search(params, feats, fmap, 4, 4, 0.0, 6)
    ids1, _, _, alphas1, _ = AO.beam_search(params, feats, fmap, 1, 6)
    for j in range(4):
        assert torch.equal(ids[:, j], ids1[:, 0])
        assert torch.equal(alphas[:, j], alphas1[:, 0])


def test_diverse_beam_flags():
    from gan_image_captioning_amd.args import build_parser
    args = build_parser().parse_args([])
    assert args.eval_diverse_beam_size == 0
    assert args.eval_diverse_groups == 2 and args.eval_diversity_strength == 0.5
    a = build_parser().parse_args(["--eval-diverse-beam-size", "6", "--eval-diverse-groups", "3", "--eval-diversity-strength", "1.5"])
    assert (a.eval_diverse_beam_size, a.eval_diverse_groups, a.eval_diversity_strength) == (6, 3, 1.5)


def test_decoders_take_the_new_keywords():
    import inspect
    from gan_image_captioning_amd.engine import AttnDecoderEngine, DecoderEngine
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder, Generator
    from gan_image_captioning_amd.training import GANInstructor
    for f in (Decoder.beam_search, AttnDecoder.beam_search, Generator.caption):
        ps = inspect.signature(f).parameters
        assert ps["beam_groups"].default == 1 and ps["diversity"].default == 0.0
    for e in (DecoderEngine, AttnDecoderEngine):
        assert "groups" in inspect.signature(e.diverse_beam_search).parameters
    ps = inspect.signature(GANInstructor.evaluate_diverse_beam).parameters
    assert list(ps)[1:6] == ["what", "beam_size", "groups", "diversity", "length_penalty"]
