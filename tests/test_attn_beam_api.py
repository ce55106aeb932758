"""Attention-decoder beam search without a GPU: the float64 oracle (tests/attn_beam_oracle.py) against brute force and against the
greedy roll-out of oracle/cpu_attention.py, the host-only workspace query of gic_attn_beam_search and its argument checks."""
import ctypes
import itertools

import pytest
import torch

from oracle import cpu_attention as CA
from tests import attn_beam_oracle as AO


def _brute_force(params, features, fmap, L, eos_id=2, pad_id=0):
    """Every caption of at most L tokens (ending at its first <E>) of each image with its log-probability and attention maps:
    a list per image of (score, ids, length, alphas [L, P])."""
    gp = AO.as_dict(params)
    V = gp["decoder.linear.weight"].shape[0]
    P = fmap.shape[1]
    out = []
    for b in range(features.shape[0]):
        hyps = {}
        for seq in itertools.product(range(V), repeat=L):
            n = next((t + 1 for t, s in enumerate(seq) if s == eos_id), L)
            ids = tuple(seq[:n]) + (pad_id,) * (L - n)
            if ids in hyps:
                continue
            f = features[b:b + 1].double()
            logits, _, alphas = CA.attn_decoder_sample(gp, f, fmap[b:b + 1].double(), L, 1.0, pretrain=True,
                                                       force_ids=torch.tensor([ids]))
            logp = torch.log_softmax(logits[0], dim=-1)
            score = float(sum(logp[t, ids[t]] for t in range(n)))
            al = alphas[0].clone()
            al[n:] = 0
            hyps[ids] = (score, ids, n, al)
        out.append(list(hyps.values()))
    return out


@pytest.mark.parametrize("V,alpha", [(4, 0.0), (4, 1.0), (6, 0.5)])
def test_oracle_equals_brute_force_at_k_equal_V(V, alpha):
    """k = V and L = 2: every one-token prefix survives step 0, so the search keeps the exact top k of all captions."""
    B, L, E, H, C, P, A = 3, 2, 8, 8, 8, 5, 8
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=V)
    params[6] = params[6].clone()
    params[6][2] += 1.0                                   # some mass on <E>: finished beams compete with live ones
    ids, scores, lengths, alphas, _ = AO.beam_search(params, feats, fmap, V, L, length_penalty=alpha)
    for b, hyps in enumerate(_brute_force(params, feats, fmap, L)):
        hyps.sort(key=lambda e: -e[0] / e[2] ** alpha)
        for r in range(V):
            s, want, n, al = hyps[r]
            assert tuple(ids[b, r].tolist()) == want, (b, r)
            assert int(lengths[b, r]) == n
            assert float(scores[b, r]) == pytest.approx(s, rel=1e-12, abs=1e-12)
            torch.testing.assert_close(alphas[b, r], al, rtol=1e-12, atol=1e-12)


def test_oracle_k1_is_the_greedy_rollout():
    B, L, V, E, H, C, P, A = 5, 7, 12, 8, 16, 8, 9, 8
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=3)
    params[6] = params[6].clone()
    params[6][2] += 0.8
    ids, scores, lengths, alphas, _ = AO.beam_search(params, feats, fmap, 1, L)
    logits, gids, galph = CA.attn_decoder_sample(AO.as_dict(params), feats.double(), fmap.double(), L, 1.0, pretrain=True)
    logp = torch.log_softmax(logits, dim=-1)
    assert (gids == 2).any() and (lengths < L).any(), "the <E> offset should end some captions early"
    for b in range(B):
        hit = (gids[b] == 2).nonzero()
        n = int(hit[0]) + 1 if len(hit) else L
        want = gids[b].clone()
        want[n:] = 0
        assert torch.equal(ids[b, 0], want)
        assert int(lengths[b, 0]) == n
        assert float(scores[b, 0]) == pytest.approx(float(logp[b, torch.arange(n), gids[b, :n]].sum()), rel=1e-12)
        torch.testing.assert_close(alphas[b, 0, :n], galph[b, :n], rtol=1e-12, atol=1e-12)
        assert (alphas[b, 0, n:] == 0).all()
    torch.testing.assert_close(AO.sequence_logprob(params, feats, fmap, ids, lengths), scores, rtol=1e-12, atol=1e-12)


def _lib():
    from gan_image_captioning_amd import _lib
    return _lib, _lib.load()


def test_ws_bytes_is_host_only_and_python_agrees():
    from gan_image_captioning_amd import engine
    L_, lib = _lib()
    out = ctypes.c_uint64(0)
    d = L_.AttnDims(32, 20, 10000, 512, 512, 2048, 49, 512, 1)
    assert lib.gic_attn_beam_ws_bytes(ctypes.byref(d), 5, ctypes.byref(out)) == 0
    eng = engine.AttnDecoderEngine(10000, 512, 512, 2048, 49, 512, 1)
    assert eng.beam_ws_bytes(32, 20, 5) == out.value
    # the workspace holds at least the xh slots, the feature projection and the alpha history
    R = 32 * 5
    assert out.value >= 2 * R * (512 + 2048 + 512) * 2 + 32 * 49 * 512 * 2 + 20 * R * 49 * 4
    sizes = [eng.beam_ws_bytes(32, 20, k) for k in range(1, 9)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 8
    assert all(s % 256 == 0 for s in sizes)


def _call(lib, L_, dims, beam=3, eos=2, pad=0, lp=0.0, ws=256, ids=8, null_params=False, null_fmap=False):
    opts = L_.DecoderBeamOpts()
    opts.beam, opts.eos_id, opts.pad_id, opts.length_penalty = beam, eos, pad, lp
    p, s = L_.AttnParams(), L_.AttnShadow()
    if not null_params:
        for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
            setattr(p, n, 256)
        for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
            setattr(s, n, 256)
    rc = lib.gic_attn_beam_search(ctypes.byref(dims), ctypes.byref(p), ctypes.byref(s), ctypes.byref(opts), ws, 256,
                                  None if null_fmap else 256, ids, 256, 256, None, None)
    return rc, lib.gic_last_error().decode()


@pytest.mark.parametrize("case,kw,msg", [
    ("beam0", dict(beam=0), "beam size"),
    ("beam9", dict(beam=9), "beam size"),
    ("beam_gt_V", dict(beam=5, dims=(2, 4, 4, 8, 8, 8, 4, 8, 0)), "exceeds the vocabulary"),
    ("eos", dict(eos=64), "eos_id"),
    ("eos_neg", dict(eos=-1), "eos_id"),
    ("pad", dict(pad=64), "pad_id"),
    ("nan", dict(lp=float("nan")), "NaN"),
    ("ws_align", dict(ws=260), "256-byte aligned"),
    ("null_ws", dict(ws=None), "null argument"),
    ("null_ids", dict(ids=None), "null argument"),
    ("null_fmap", dict(null_fmap=True), "null argument"),
    ("null_weights", dict(null_params=True), "null weights"),
    ("L", dict(dims=(2, 1025, 64, 8, 8, 8, 4, 8, 0)), "1024 steps"),
    ("rows", dict(dims=((1 << 21) + 1, 4, 64, 8, 8, 8, 4, 8, 0)), "too many rows"),
    ("V4", dict(dims=(2, 4, 62, 8, 8, 8, 4, 8, 0)), "multiple of 4"),
    ("C8", dict(dims=(2, 4, 64, 8, 8, 12, 4, 8, 0)), "multiples of 8"),
    ("P", dict(dims=(2, 4, 64, 8, 8, 8, 1025, 8, 0)), "positions"),
    ("A", dict(dims=(2, 4, 64, 8, 8, 8, 4, 2056, 0)), "attention width"),
    ("dtype", dict(dims=(2, 4, 64, 8, 8, 8, 4, 8, 7)), "dtype"),
])
def test_invalid_arguments_return_a_status(case, kw, msg):
    L_, lib = _lib()
    dims = L_.AttnDims(*kw.pop("dims", (2, 4, 64, 8, 8, 8, 4, 8, 0)))
    beam = kw.pop("beam", 8 if case == "rows" else 3)
    rc, err = _call(lib, L_, dims, beam=beam, **kw)
    assert rc != 0 and msg in err, (rc, err)
    if case in ("beam0", "beam9", "beam_gt_V", "L", "rows", "V4", "C8", "P", "A", "dtype"):     # the shape checks of the size query too
        out = ctypes.c_uint64(0)
        assert lib.gic_attn_beam_ws_bytes(ctypes.byref(dims), beam, ctypes.byref(out)) != 0
        assert msg in lib.gic_last_error().decode()


def test_null_options_and_dims():
    L_, lib = _lib()
    d = L_.AttnDims(2, 4, 64, 8, 8, 8, 4, 8, 0)
    assert lib.gic_attn_beam_search(ctypes.byref(d), None, None, None, 256, 256, 256, 256, 256, 256, None, None) != 0
    assert "null options" in lib.gic_last_error().decode()
    assert lib.gic_attn_beam_ws_bytes(None, 3, None) != 0
    assert lib.gic_attn_beam_ws_bytes(ctypes.byref(d), 3, None) != 0


def test_beam_search_without_a_map_is_not_implemented():
    from gan_image_captioning_amd.generator import AttnDecoder
    with pytest.raises(NotImplementedError, match=r"beam_search\(features, fmap\)"):
        AttnDecoder.beam_search(None, torch.zeros(2, 8))
    with pytest.raises(NotImplementedError):
        AttnDecoder.beam_search(None, None)
