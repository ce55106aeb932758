"""Decode constraints without a GPU: the C ABI (symbols, struct layout, argument statuses before any launch, the feasibility bound),
the float64 oracle (tests/constrained_oracle.py) against the unconstrained oracles, brute force and its own invariants, the keywords
and flags, and the cases of tests/test_gpu_constrained.py: each is checked here to be decidable in float32 and to bind."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import diverse_beam_oracle as DO
from tests import sample_oracle as SO
from tests.test_diverse_beam_api import _lstm_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gic_decode_constraints_ws_bytes", "gic_decoder_constrained_beam_search", "gic_attn_constrained_beam_search",
       "gic_decoder_constrained_sample_captions", "gic_attn_constrained_sample_captions")


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
    assert lib.gic_abi_version() == 5


def test_struct_matches_header():
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    body = re.search(r"typedef struct gic_decode_constraints \{(.*?)\} gic_decode_constraints;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*([a-z_0-9]+)\s+([a-z_]+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body), re.M)
    assert fields == [("int32_t", "no_repeat_ngram", ""), ("int32_t", "min_length", ""), ("int32_t", "num_suppress", ""),
                      ("int32_t", "suppress", "16")]
    assert [f[0] for f in L.DecodeConstraints._fields_] == ["no_repeat_ngram", "min_length", "num_suppress", "suppress"]
    assert [getattr(L.DecodeConstraints, f).offset for f in ("no_repeat_ngram", "min_length", "num_suppress", "suppress")] == [0, 4, 8, 12]
    assert L.MAX_SUPPRESS == 16 and C.sizeof(L.DecodeConstraints) == (3 + 16) * 4


def _cons(L, n=0, min_length=0, suppress=(), S=None):
    c = L.DecodeConstraints()
    c.no_repeat_ngram, c.min_length = n, min_length
    c.num_suppress = len(suppress) if S is None else S
    for i, v in enumerate(suppress):
        c.suppress[i] = v
    return c


LSTM_DIMS = (4, 6, 50, 8, 16, 2, 0)          # B, L, V, E, H, NL, dtype
ATTN_DIMS = (2, 4, 64, 8, 8, 8, 4, 8, 0)     # B, L, V, E, H, C, P, A, dtype


def _call(L, lib, which, head, cons, dims=None, ws=256, cws=256, beam=4, groups=2, eos=2, opts=True, null_cons=False):
    """One constrained call on fake (non-null, aligned) pointers: every status comes back before any launch."""
    lstm = which == "lstm"
    d = (L.DecoderDims if lstm else L.AttnDims)(*(dims or (LSTM_DIMS if lstm else ATTN_DIMS)))
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
    cp = None if null_cons else C.byref(cons)
    if head == "beam":
        o = L.DiverseBeamOpts()
        o.beam.beam, o.beam.eos_id, o.beam.pad_id, o.groups, o.diversity = beam, eos, 0, groups, 0.5
        op = C.byref(o) if opts else None
        if lstm:
            rc = lib.gic_decoder_constrained_beam_search(C.byref(d), C.byref(p), C.byref(s), op, cp, ws, cws, 256, 256, 256, 256, None)
        else:
            rc = lib.gic_attn_constrained_beam_search(C.byref(d), C.byref(p), C.byref(s), op, cp, ws, cws, 256, 256, 256, 256, 256, None, None)
    else:
        o = L.SampleOpts()
        o.num_samples, o.top_k, o.top_p, o.temperature, o.eos_id, o.pad_id = beam, 0, 1.0, 1.0, eos, 0
        op = C.byref(o) if opts else None
        if lstm:
            rc = lib.gic_decoder_constrained_sample_captions(C.byref(d), C.byref(p), C.byref(s), op, cp, ws, cws, 256, None, 0, 256, 256, 256,
                                                             None)
        else:
            rc = lib.gic_attn_constrained_sample_captions(C.byref(d), C.byref(p), C.byref(s), op, cp, ws, cws, 256, 256, None, 0, 256, 256,
                                                          256, None)
    return rc, lib.gic_last_error().decode()


BOTH = pytest.mark.parametrize("which,head", [("lstm", "beam"), ("lstm", "sample"), ("attn", "beam"), ("attn", "sample")])


@BOTH
@pytest.mark.parametrize("case,kw,msg", [
    ("n_neg", dict(n=-1), "no_repeat_ngram"),
    ("n_gt_L", dict(n=99), "no_repeat_ngram"),
    ("min_neg", dict(min_length=-2), "min_length"),
    ("min_gt_L", dict(min_length=99), "min_length"),
    ("S_neg", dict(S=-1), "num_suppress"),
    ("S_17", dict(S=17), "num_suppress"),
    ("id_neg", dict(suppress=(1, -3)), "suppress[1]"),
    ("id_V", dict(suppress=(64,)), "suppress[0]"),
    ("eos", dict(suppress=(1, 3, 2)), "eos_id"),
])
def test_invalid_constraints_return_a_status(which, head, case, kw, msg):
    L, lib = _lib()
    rc, err = _call(L, lib, which, head, _cons(L, **kw))
    assert rc == -1 and msg in err, (rc, err)


@BOTH
def test_null_options_constraints_and_workspace(which, head):
    L, lib = _lib()
    rc, err = _call(L, lib, which, head, _cons(L, n=2), opts=False)
    assert rc == -1 and "null options" in err, err
    rc, err = _call(L, lib, which, head, None, null_cons=True)
    assert rc == -1 and "null constraints" in err, err
    rc, err = _call(L, lib, which, head, _cons(L, n=2), cws=None)
    assert rc == -1 and "constraint workspace" in err, err
    rc, err = _call(L, lib, which, head, _cons(L, n=2), cws=260)
    assert rc == -1 and "constraint workspace" in err, err
    rc, err = _call(L, lib, which, head, _cons(L, n=2), ws=260)
    assert rc == -1 and "256-byte aligned" in err, err


@pytest.mark.parametrize("head", ["beam", "sample"])
def test_feasibility_bound_at_its_edge(head):
    """V - (S + 1 + max(0, L - n)) >= K with n >= 1, V - (S + 1) >= K with n = 0 (K = 1 for the sampler): one token fewer than at
    equality is refused with the message; at equality the check passes and the call is refused by the NEXT check (the null
    constraint workspace)."""
    L, lib = _lib()
    K = 4 if head == "beam" else 1
    Lc, S = 6, 2
    for n in (0, 1, 3, 6):
        worst = S + 1 + (Lc - n if n else 0)
        for V, ok in ((K + worst, True), (K + worst - 1, False)):
            rc, err = _call(L, lib, "lstm", head, _cons(L, n=n, suppress=(0, 1)), dims=(4, Lc, V, 8, 16, 2, 0), beam=4, groups=2, cws=None)
            assert rc == -1
            assert ("infeasible" in err) == (not ok), (n, V, err)
            assert ok == ("constraint workspace" in err), (n, V, err)


def test_feasibility_bound_attention_edge():
    """The same edge for the attention decoder, whose V is a multiple of 4: S chosen so that equality falls on one."""
    L, lib = _lib()
    for head, K in (("beam", 4), ("sample", 1)):
        Lc, n = 6, 2
        for V in (16, 20):
            S = V - K - 1 - (Lc - n)                       # equality
            sup = tuple(v for v in range(3, 3 + S))
            dims = (2, Lc, V, 8, 8, 8, 4, 8, 0)
            rc, err = _call(L, lib, "attn", head, _cons(L, n=n, suppress=sup), dims=dims, cws=None)
            assert rc == -1 and "constraint workspace" in err, err
            rc, err = _call(L, lib, "attn", head, _cons(L, n=n, suppress=sup + (3 + S,)), dims=dims, cws=None)
            assert rc == -1 and "infeasible" in err, err


def test_constraints_ws_bytes():
    L, lib = _lib()
    out = C.c_uint64(0)
    for rows, Lc, S in ((1, 1, 0), (24, 12, 3), (512, 20, 16), (1 << 24, 1024, 16)):
        c = _cons(L, n=2, suppress=tuple(range(3, 3 + S)))
        assert lib.gic_decode_constraints_ws_bytes(rows, Lc, C.byref(c), C.byref(out)) == 0
        cap = S + 1 + Lc
        assert out.value % 256 == 0 and out.value >= 4 * rows * (1 + cap)
    assert lib.gic_decode_constraints_ws_bytes(0, 4, C.byref(c), C.byref(out)) == -1
    assert lib.gic_decode_constraints_ws_bytes(4, 4, None, C.byref(out)) == -1
    assert lib.gic_decode_constraints_ws_bytes(4, 4, C.byref(_cons(L, S=17)), C.byref(out)) == -1
    assert "num_suppress" in lib.gic_last_error().decode()


def test_engine_refuses_a_null_or_long_list():
    from gan_image_captioning_amd import engine
    assert engine.decode_constraints() is None and engine.decode_constraints(0, 0, []) is None
    with pytest.raises(ValueError, match="suppress_tokens"):
        engine.decode_constraints(2, 0, None)
    with pytest.raises(ValueError, match="num_suppress"):
        engine.decode_constraints(0, 0, range(17))
    c = engine.decode_constraints(2, 5, (1, 3))
    assert (c.no_repeat_ngram, c.min_length, c.num_suppress, list(c.suppress)[:2]) == (2, 5, 2, [1, 3])


# ---------------------------------------------------------------- the oracle against the existing oracles
@pytest.mark.parametrize("k", [2, 5])
def test_oracle_off_is_beam_search(k):
    params, feats = _lstm_problem(k)
    for alpha in (0.0, 0.7):
        want = BO.beam_search(params, feats, k, 9, length_penalty=alpha)
        got = CO.beam_search(params, feats, k, 9, length_penalty=alpha)
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("k,G,lam", [(4, 2, 0.5), (6, 3, 2.0), (4, 4, 0.0)])
def test_oracle_off_is_diverse_beam_search(k, G, lam):
    params, feats = _lstm_problem(k + G)
    want = DO.diverse_beam_search(params, feats, k, G, lam, 9, length_penalty=0.7)
    got = CO.beam_search(params, feats, k, 9, G, lam, length_penalty=0.7)
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert got[3] == want[3]


def test_oracle_off_is_the_attention_oracles():
    params, feats, fmap = AO.random_problem(2, 24, 8, 16, 8, 5, 8, seed=3, scale=3.0)
    params[6] = params[6].clone()
    params[6][2] += 1.0
    want = AO.beam_search(params, feats, fmap, 3, 6, length_penalty=0.7)
    got = CO.attn_beam_search(params, feats, fmap, 3, 6, length_penalty=0.7)
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(a, b)
    want = DO.attn_diverse_beam_search(params, feats, fmap, 4, 2, 1.0, 6)
    got = CO.attn_beam_search(params, feats, fmap, 4, 6, 2, 1.0)
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("opts", [(0, 1.0, 1.0), (5, 1.0, 0.8), (0, 0.9, 1.0), (8, 0.8, 1.5)], ids=["off", "k5", "p09", "k8p08"])
def test_oracle_off_is_the_sampling_oracle(opts):
    params, feats = _lstm_problem(5)
    n, Lc = 3, 9
    u = torch.rand(Lc, feats.shape[0] * n, 40, generator=torch.Generator().manual_seed(6))
    want = SO.decode(params, feats, n, Lc, u, *opts)
    got = CO.sample(params, feats, n, Lc, u, *opts)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    torch.testing.assert_close(got[1], want[1])
    torch.testing.assert_close(got[3], want[3], rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------- the oracle against brute force
def _admissible(seq, length, n, min_length, suppress, L):
    """The constraint tested on a whole sequence: seq[:length] repeats no n-gram, holds no suppressed id and does not end early."""
    return not CO.violates(seq, length, n, min_length, suppress)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("cons", [(1, 0, ()), (0, 2, ()), (0, 0, (1, 4)), (1, 2, (3,)), (2, 2, (0,))],
                         ids=["n1", "min2", "sup", "n1min2sup", "n2min2sup"])
def test_oracle_two_steps_equal_whole_search_brute_force(seed, cons):
    """L = 2 with K = V - (banned tokens at step 0): no candidate is pruned at step 0, so the oracle's beams are exactly the K best
    admissible two-token sequences (a caption that ends at step 0 counts with its one token)."""
    n, min_length, suppress = cons
    V, E, H = 7, 6, 8
    params = BO.random_params(V, E, H, 1, seed=seed + 30, scale=4.0)
    params[-1][2] += 1.0
    feats = torch.randn(1, E, generator=torch.Generator().manual_seed(seed))
    first = [v for v in range(V) if v not in CO.banned([], n, min_length, suppress)]
    K = len(first)
    assert K <= 8 and CO.feasible(V, 2, 1, n, suppress)
    p = [t.double() for t in params]
    st = DO._LstmStepper(p, feats[0].double(), V)
    l0, _ = st.step()
    lp0 = l0[0] - torch.logsumexp(l0[0], 0)
    st.reorder(list(range(V)), list(range(V)))
    l1, _ = st.step()
    lp1 = l1 - torch.logsumexp(l1, dim=-1, keepdim=True)
    seqs = []
    for a in range(V):
        if a == 2:
            if _admissible([a], 1, n, min_length, suppress, 2):
                seqs.append((float(lp0[a]), [a, 0], 1))
            continue
        for b in range(V):
            if _admissible([a, b], 2, n, min_length, suppress, 2) and _admissible([a], 1, 0, 0, suppress, 2):
                seqs.append((float(lp0[a] + lp1[a, b]), [a, b], 2))
    # every first token can be extended (feasibility), so the K-wide beam holds every admissible first token and prunes nothing
    seqs.sort(key=lambda e: -e[0])
    ids, scores, lengths, _ = CO.beam_search(params, feats, K, 2, no_repeat_ngram=n, min_length=min_length, suppress_tokens=suppress)
    want = seqs[:K]
    assert sorted(map(tuple, ids[0].tolist())) == sorted(tuple(e[1]) for e in want)
    torch.testing.assert_close(scores[0].sort(descending=True).values, torch.tensor([e[0] for e in want], dtype=torch.float64))
    assert sorted(lengths[0].tolist()) == sorted(e[2] for e in want)


@pytest.mark.parametrize("n", [2, 3])
def test_oracle_equals_brute_force_step_by_step_at_depth(n):
    """V = 10, K = 3, searches of 2..6 steps: every step t by brute force from the state the previous steps left -- the K best of ALL
    (parent, token) pairs over the whole vocabulary, after removing every pair whose extended history repeats an n-gram, ends too early
    or emits a suppressed id (tested on the extended sequence, not through banned()) -- against the oracle's search."""
    V, E, H, K, min_length, suppress = 10, 6, 8, 3, 3, (1,)
    removed = compared = 0
    for seed in range(4):
        params = BO.random_params(V, E, H, 1, seed=seed + 50, scale=1.0)
        feats = torch.randn(1, E, generator=torch.Generator().manual_seed(seed))
        p = [t.double() for t in params]
        for Lc in range(2, 7):
            assert CO.feasible(V, Lc, K, n, suppress)
            st = DO._LstmStepper(p, feats[0].double(), K)
            score = [0.0] + [-math.inf] * (K - 1)
            fin, seqs, ln = [False] * K, [[] for _ in range(K)], [0] * K
            for t in range(Lc):
                logits, _ = st.step()
                logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
                cands = []
                for j in range(K):
                    if fin[j]:
                        cands.append((score[j], j, 0, True, 0.0))
                        continue
                    for v in range(V):
                        ext = seqs[j] + [v]
                        if any(x in suppress for x in ext) or (v == 2 and len(ext) < min_length):
                            continue
                        grams = [tuple(ext[i:i + n]) for i in range(len(ext) - n + 1)]
                        if len(grams) != len(set(grams)):
                            removed += score[j] != -math.inf
                            continue
                        cands.append((score[j] + float(logp[j, v]), j, v, False, -float(logits[j, v])))
                cands.sort(key=lambda e: (-e[0], e[1], e[4], e[2]))
                kept = cands[:K]
                seqs = [seqs[e[1]] + [e[2]] for e in kept]
                ln = [ln[e[1]] if e[3] else t + 1 for e in kept]
                fin = [e[3] or e[2] == 2 for e in kept]
                score = [e[0] for e in kept]
                st.reorder([e[1] for e in kept], [e[2] for e in kept])
            order = sorted(range(K), key=lambda j: (-score[j], j))
            ids, scores, lengths, margins = CO.beam_search(params, feats, K, Lc, no_repeat_ngram=n, min_length=min_length,
                                                           suppress_tokens=suppress)
            if min(margins[0]) < 1e-9:
                continue                                   # (an exact tie: the two tie orders need not agree)
            compared += 1
            assert [seqs[j] for j in order] == ids[0].tolist(), (seed, Lc, n)
            torch.testing.assert_close(scores[0], torch.tensor([score[j] for j in order], dtype=torch.float64))
            assert lengths[0].tolist() == [ln[j] for j in order]
    assert compared >= 16 and removed >= 1, (compared, removed)          # the n-gram rule removed candidates of live parents


@pytest.mark.parametrize("cons", [(1, 0, ()), (2, 4, (1, 3)), (3, 0, ()), (4, 6, (4,)), (0, 3, (1,))])
def test_banned_equals_trying_every_token(cons):
    n, min_length, suppress = cons
    g = torch.Generator().manual_seed(n + min_length)
    V = 5
    for trial in range(200):
        t = int(torch.randint(0, 9, (1,), generator=g))
        y = torch.randint(0, V, (t,), generator=g).tolist()
        want = set()
        for v in range(V):
            ext = y + [v]
            grams = [tuple(ext[i:i + n]) for i in range(len(ext) - n + 1)] if n else []
            new_gram = n >= 1 and len(ext) >= n and tuple(ext[-n:]) in set(grams[:-1])
            if v in suppress or (v == 2 and len(ext) < min_length) or new_gram:
                want.add(v)
        assert CO.banned(y, n, min_length, suppress, 2) == want, (y, cons)


# ---------------------------------------------------------------- invariants of the oracle's output
def check_invariants(ids, lengths, L, n, min_length, suppress, eos_id=2, pad_id=0):
    """No repeated n-gram, no suppressed id, length >= min_length (or L), <E> only as the last token, pad behind: on every caption."""
    ids, lengths = ids.reshape(-1, L).tolist(), lengths.reshape(-1).tolist()
    for row, ln in zip(ids, lengths):
        s = row[:ln]
        assert 1 <= ln <= L and all(v == pad_id for v in row[ln:]), (row, ln)
        assert eos_id not in s[:-1], (row, ln)
        assert ln == L or s[-1] == eos_id, (row, ln)
        assert ln >= min(min_length, L), (row, ln)
        assert not any(v in suppress for v in s), (row, ln)
        if n >= 1:
            grams = [tuple(s[i:i + n]) for i in range(len(s) - n + 1)]
            assert len(grams) == len(set(grams)), (row, ln, n)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("cons", [(1, 0, ()), (2, 5, (1, 3)), (3, 0, (4,)), (0, 7, ()), (4, 9, (1,))])
def test_oracle_output_invariants(seed, cons):
    n, min_length, suppress = cons
    V, E, H, Lc = 40, 8, 16, 9
    params = BO.random_params(V, E, H, 2, seed=seed, scale=1.0 + seed)
    params[-1][2] += 0.5 * seed
    feats = torch.randn(3, E, generator=torch.Generator().manual_seed(seed + 1))
    kw = dict(no_repeat_ngram=n, min_length=min_length, suppress_tokens=suppress)
    ids, _, lengths, _ = CO.beam_search(params, feats, 4, Lc, **kw)
    check_invariants(ids, lengths, Lc, *cons)
    ids, _, lengths, _ = CO.beam_search(params, feats, 6, Lc, 3, 0.8, **kw)
    check_invariants(ids, lengths, Lc, *cons)
    u = torch.rand(Lc, 9, V, generator=torch.Generator().manual_seed(seed))
    ids, _, lengths, _ = CO.sample(params, feats, 3, Lc, u, 6, 0.9, 1.2, **kw)
    check_invariants(ids, lengths, Lc, *cons)


# ---------------------------------------------------------------- flags and signatures
def test_flags():
    from gan_image_captioning_amd.args import build_parser
    a = build_parser().parse_args([])
    assert (a.eval_no_repeat_ngram, a.eval_min_length, list(a.eval_suppress_tokens)) == (0, 0, [])
    a = build_parser().parse_args(["--eval-no-repeat-ngram", "2", "--eval-min-length", "5", "--eval-suppress-tokens", "1,3"])
    assert (a.eval_no_repeat_ngram, a.eval_min_length, list(a.eval_suppress_tokens)) == (2, 5, [1, 3])


def test_methods_take_the_new_keywords():
    from gan_image_captioning_amd.engine import AttnDecoderEngine, DecoderEngine
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder, Generator
    from gan_image_captioning_amd.training import GANInstructor
    fs = [e.__dict__[m] for e in (DecoderEngine, AttnDecoderEngine) for m in ("beam_search", "diverse_beam_search", "sample_captions")]
    fs += [d.__dict__[m] for d in (Decoder, AttnDecoder) for m in ("beam_search", "sample_captions")]
    fs += [Generator.caption, Generator.sample_captions]
    for f in fs:
        ps = inspect.signature(f).parameters
        assert list(ps)[-3:] == ["no_repeat_ngram", "min_length", "suppress_tokens"], f
        assert (ps["no_repeat_ngram"].default, ps["min_length"].default, ps["suppress_tokens"].default) == (0, 0, ()), f
    # the positions of the existing parameters
    assert list(inspect.signature(DecoderEngine.beam_search).parameters)[1:10] == \
        ["params", "features", "Lc", "beam", "eos_id", "pad_id", "length_penalty", "states", "ws"]
    assert list(inspect.signature(AttnDecoderEngine.diverse_beam_search).parameters)[1:14] == \
        ["params", "features", "fmap", "Lc", "beam", "groups", "diversity", "eos_id", "pad_id", "length_penalty", "states", "ws", "want_alphas"]
    assert list(inspect.signature(DecoderEngine.sample_captions).parameters)[1:14] == \
        ["params", "features", "Lc", "num_samples", "top_k", "top_p", "temperature", "eos_id", "pad_id", "seed", "noise_u", "states", "ws"]
    assert list(inspect.signature(Generator.caption).parameters)[1:10] == \
        ["images", "beam_size", "max_caption_len", "eos_id", "length_penalty", "return_beams", "return_alphas", "beam_groups", "diversity"]
    assert list(inspect.signature(Generator.sample_captions).parameters)[1:10] == \
        ["images", "num_samples", "top_k", "top_p", "temperature", "max_caption_len", "eos_id", "seed", "noise_u"]
    assert list(inspect.signature(GANInstructor.evaluate_diverse_beam).parameters)[1:6] == \
        ["what", "beam_size", "groups", "diversity", "length_penalty"]
    assert list(inspect.signature(GANInstructor.evaluate).parameters)[1:5] == ["what", "beam_size", "max_caption_len", "batch_size"]


# ---------------------------------------------------------------- the GPU cases (tests/test_gpu_constrained.py imports them)
# LSTM problems: BO.random_params(V, E, H, NL, seed, scale=1.0) without an <E> bias (captions of 6-12 tokens that repeat uni-, bi- and
# tri-grams); "generic" = the tiny_scaled shape, which the fused step kernels decline, "fused" = the cfg1 shape.  The seeds were picked
# by running the oracle; the tests below pin what made them eligible.
LSTM_SHAPES = {"generic": (8, 12, 50, 8, 16, 2), "fused": (8, 12, 64, 32, 512, 1)}       # B, L, V, E, H, NL
ATTN_SHAPE = (6, 10, 64, 16, 32, 40, 49, 24)                                                # B, L, V, E, H, C, P, A
ATTN_SCALE = 2.0
C_NGRAM2 = dict(no_repeat_ngram=2, min_length=0, suppress_tokens=())
C_ALL = dict(no_repeat_ngram=3, min_length=6, suppress_tokens=(1, 3))
C_MIN8 = dict(no_repeat_ngram=0, min_length=8, suppress_tokens=())
C_UNI = dict(no_repeat_ngram=1, min_length=4, suppress_tokens=(3,))

# (decoder, seed, k, groups, lambda, constraints)
BEAM_CASES = [
    ("generic", 2, 4, 1, 0.0, C_NGRAM2), ("generic", 1, 3, 1, 0.0, C_ALL), ("generic", 8, 5, 1, 0.0, C_MIN8),
    ("generic", 5, 6, 3, 0.8, C_ALL), ("generic", 1, 4, 2, 0.5, C_UNI),
    ("fused", 1, 4, 1, 0.0, C_NGRAM2), ("fused", 1, 3, 1, 0.0, C_ALL), ("fused", 10, 5, 1, 0.0, C_MIN8),
    ("fused", 10, 6, 3, 0.8, C_ALL), ("fused", 10, 4, 2, 0.5, C_UNI),
    ("attn", 2, 4, 1, 0.0, C_NGRAM2), ("attn", 2, 3, 1, 0.0, C_ALL), ("attn", 1, 5, 1, 0.0, C_MIN8),
    ("attn", 5, 6, 3, 0.8, C_ALL), ("attn", 6, 4, 2, 0.5, C_UNI),
]
# (decoder, seed, n, (top_k, top_p, temperature), constraints)
SAMPLE_CASES = [
    ("generic", 3, 3, (0, 1.0, 1.0), C_NGRAM2), ("generic", 1, 3, (8, 0.9, 0.8), C_ALL),
    ("fused", 1, 3, (0, 1.0, 1.0), C_NGRAM2), ("fused", 1, 3, (8, 0.9, 0.8), C_ALL),
    ("attn", 3, 3, (0, 1.0, 1.0), C_NGRAM2), ("attn", 1, 3, (8, 0.9, 0.8), C_ALL),
]


def lstm_problem(which, seed):
    B, Lc, V, E, H, NL = LSTM_SHAPES[which]
    params = BO.random_params(V, E, H, NL, seed=seed, scale=1.0)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(seed + 1))
    return params, feats


def attn_problem(seed):
    B, Lc, V, E, H, Cc, P, A = ATTN_SHAPE
    return AO.random_problem(B, V, E, H, Cc, P, A, seed=seed, scale=ATTN_SCALE)


def case_noise(which, seed, n):
    B, Lc, V = (ATTN_SHAPE if which == "attn" else LSTM_SHAPES[which])[:3]
    return torch.rand(Lc, B * n, V, generator=torch.Generator().manual_seed(seed + 7))


def beam_oracle(case, constrained=True):
    """(ids, scores, lengths, margins[, alphas]) of the oracle for one of BEAM_CASES."""
    which, seed, k, G, lam, cons = case
    kw = cons if constrained else {}
    if which == "attn":
        params, feats, fmap = attn_problem(seed)
        ids, sc, ln, al, margins = CO.attn_beam_search(params, feats, fmap, k, ATTN_SHAPE[1], G, lam, **kw)
        return ids, sc, ln, margins, al
    params, feats = lstm_problem(which, seed)
    return CO.beam_search(params, feats, k, LSTM_SHAPES[which][1], G, lam, **kw)


def sample_oracle(case, constrained=True):
    which, seed, n, opts, cons = case
    kw = cons if constrained else {}
    u = case_noise(which, seed, n)
    if which == "attn":
        params, feats, fmap = attn_problem(seed)
        return CO.attn_sample(params, feats, fmap, n, ATTN_SHAPE[1], u, *opts, **kw)
    params, feats = lstm_problem(which, seed)
    return CO.sample(params, feats, n, LSTM_SHAPES[which][1], u, *opts, **kw)


def _violations(ids, lengths, cons):
    Lc = ids.shape[-1]
    rows = zip(ids.reshape(-1, Lc).tolist(), lengths.reshape(-1).tolist())
    return sum(CO.violates(r, ln, cons["no_repeat_ngram"], cons["min_length"], cons["suppress_tokens"]) for r, ln in rows)


def _case_id(c):
    k = c[4] if len(c) == 5 else c[5]
    return f"{c[0]}-s{c[1]}-k{c[2]}-n{k['no_repeat_ngram']}m{k['min_length']}S{len(k['suppress_tokens'])}" + \
        (f"-g{c[3]}" if len(c) == 6 else f"-tk{c[3][0]}")


def test_the_gpu_cases_cover_the_ground():
    assert {(c[0], c[3] > 1) for c in BEAM_CASES} == {(w, d) for w in ("generic", "fused", "attn") for d in (False, True)}
    assert {c[0] for c in SAMPLE_CASES} == {"generic", "fused", "attn"}


@pytest.mark.parametrize("case", BEAM_CASES, ids=_case_id)
def test_gpu_beam_case_is_decidable_and_binds(case):
    which, seed, k, G, lam, cons = case
    B, Lc, V = (ATTN_SHAPE if which == "attn" else LSTM_SHAPES[which])[:3]
    assert CO.feasible(V, Lc, k, cons["no_repeat_ngram"], cons["suppress_tokens"])
    ids, _, lengths, margins = beam_oracle(case)[:4]
    check_invariants(ids, lengths, Lc, cons["no_repeat_ngram"], cons["min_length"], cons["suppress_tokens"])
    clear = sum(1 for sel, _ in margins if sel >= 1e-4)
    assert 4 * clear >= 3 * B, f"{clear} of {B} images with a selection margin >= 1e-4: {margins}"
    ids, _, lengths = beam_oracle(case, constrained=False)[:3]
    assert _violations(ids, lengths, cons) >= 1, "the unconstrained search already satisfies the constraints: they do not bind"


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=_case_id)
def test_gpu_sample_case_is_decidable_and_binds(case):
    which, seed, n, opts, cons = case
    B, Lc, V = (ATTN_SHAPE if which == "attn" else LSTM_SHAPES[which])[:3]
    assert CO.feasible(V, Lc, 1, cons["no_repeat_ngram"], cons["suppress_tokens"])
    ids, _, lengths, margin = sample_oracle(case)
    check_invariants(ids, lengths, Lc, cons["no_repeat_ngram"], cons["min_length"], cons["suppress_tokens"])
    assert 4 * int((margin > 1e-5).sum()) >= 3 * margin.numel(), margin
    ids, _, lengths, _ = sample_oracle(case, constrained=False)
    assert _violations(ids, lengths, cons) >= 1, "the unconstrained draws already satisfy the constraints: they do not bind"
