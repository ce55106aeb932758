"""Lexically constrained beam search (include/gicap.h gic_forced_words, gic_*_forced_beam_search) without a GPU: the oracle
(tests/forced_beam_oracle.py) against exhaustive search, the case table the GPU tests run (tests/test_gpu_forced_beam.py imports it)
and what makes each case eligible, every refusal's text from the Python layer and from the library, the list form's packing, the new
flags."""
import ctypes as C
import inspect
import itertools
import math
import os
import re

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import forced_beam_oracle as FO
from tests import test_constrained_api as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gic_decoder_forced_beam_ws_bytes", "gic_attn_forced_beam_ws_bytes", "gic_decoder_forced_beam_search", "gic_attn_forced_beam_search")
C_OFF = dict(no_repeat_ngram=0, min_length=0, suppress_tokens=())

# ---------------------------------------------------------------- the shared cases
# the three shapes of tests/test_constrained_api.py and one fused LSTM shape with several vocabulary tiles and a ragged last one
FUSED200 = (4, 8, 200, 32, 64, 1)                            # B, L, V, E, H, NL


def shape_of(which):
    if which == "attn":
        return T.ATTN_SHAPE[:3]
    return (FUSED200 if which == "fused200" else T.LSTM_SHAPES[which])[:3]


# (decoder, seed, C, K, D, decode constraints, length_penalty, pad_id, special hop ids): the seeds were picked by running the oracle;
# test_case_covers_the_ground pins what made them eligible.  pad_id 4 where 0 is a hop id (<PAD> itself is refused in a set)
CASES = [
    ("generic", 2, 1, 2, 1, C_OFF, 0.0, 0, (49,)), ("generic", 3, 1, 8, 4, T.C_ALL, 0.7, 4, (0,)),
    ("generic", 3, 2, 4, 4, C_OFF, 0.7, 0, (49,)), ("generic", 1, 2, 8, 1, T.C_ALL, 0.0, 0, ()),
    ("generic", 1, 3, 8, 4, T.C_ALL, 0.7, 4, (0, 49)),
    ("fused", 4, 1, 2, 4, T.C_ALL, 0.7, 4, (0, 63)), ("fused", 1, 1, 8, 1, C_OFF, 0.0, 0, (63,)),
    ("fused", 1, 2, 4, 1, T.C_ALL, 0.0, 0, ()), ("fused", 2, 2, 8, 4, C_OFF, 0.7, 4, (0,)),
    ("fused", 1, 3, 8, 4, C_OFF, 0.0, 0, (63,)),
    ("attn", 1, 1, 2, 1, C_OFF, 0.7, 0, (63,)), ("attn", 1, 1, 8, 4, T.C_ALL, 0.0, 4, (0,)),
    ("attn", 1, 2, 4, 4, T.C_ALL, 0.7, 0, (63,)), ("attn", 1, 2, 8, 1, C_OFF, 0.0, 0, ()),
    ("attn", 1, 3, 8, 4, T.C_ALL, 0.0, 4, (0, 63)),
    ("fused200", 1, 1, 2, 4, C_OFF, 0.0, 4, (0, 63, 64, 199)), ("fused200", 1, 1, 8, 1, T.C_ALL, 0.7, 0, (64,)),
    ("fused200", 1, 2, 4, 4, C_OFF, 0.0, 0, (63, 64)), ("fused200", 1, 2, 8, 4, T.C_ALL, 0.7, 4, (0, 199)),
    ("fused200", 1, 3, 8, 4, T.C_ALL, 0.0, 0, (63, 64, 199)),
]


def case_id(c):
    return f"{c[0]}-s{c[1]}-C{c[2]}K{c[3]}D{c[4]}-n{c[5]['no_repeat_ngram']}-a{c[6]}"


def case_force(case):
    """The case's constraint sets, int32 [B, C, D] padded with -1: image b carries C constraints, except b % 4 == 1 (one) and
    b % 4 == 2 (none); a set holds 1..D ids drawn from the ids that are neither special (<PAD>, <E>, the ids C_ALL suppresses) nor
    used by the image already; image 0's first sets start with the case's special hop ids; with C >= 2 image 3's second set repeats
    the first id of its first (a token in two sets)."""
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    B, L, V = shape_of(which)
    g = torch.Generator().manual_seed(1000 + seed)
    barred = {pad, 2, 1, 3} | set(special)
    force = torch.full((B, Cn, D), -1, dtype=torch.int32)
    for b in range(B):
        n = 1 if b % 4 == 1 else 0 if b % 4 == 2 else Cn
        used = set()
        for c in range(n):
            m = D if (b + c) % 2 == 0 else 1 + int(torch.randint(0, D, (1,), generator=g))
            ids = []
            while len(ids) < m:
                v = int(torch.randint(0, V, (1,), generator=g))
                if v not in barred and v not in used:
                    ids.append(v)
                    used.add(v)
            force[b, c, :m] = torch.tensor(ids, dtype=torch.int32)
    for i, v in enumerate(special):                          # image 0 carries C constraints: slot (i % C, i // C) of its sets
        if i // Cn < D:
            force[0, i % Cn, i // Cn] = v
    for c in range(Cn):                                      # (a special id may have left a gap behind it: keep the sets left-packed)
        row = [int(v) for v in force[0, c] if v >= 0]
        force[0, c] = torch.tensor(row + [-1] * (D - len(row)), dtype=torch.int32)
    if Cn >= 2 and B > 3 and D >= 2:
        force[3, 1, 1] = force[3, 0, 0]
    elif Cn >= 2 and B > 3:
        force[3, 1, 0] = force[3, 0, 0]
    return force


LSTM_SCALE, ATTN_SCALE = 3.0, 4.0                           # weight scales: logit gaps wide enough for float32 to decide most selections


def case_problem(case):
    """The case's decoder and inputs: tests/beam_oracle.py / tests/attn_beam_oracle.py random problems at the case's shape and seed."""
    which, seed = case[0], case[1]
    if which == "attn":
        B, Lc, V, E, H, Cc, P, A = T.ATTN_SHAPE
        return AO.random_problem(B, V, E, H, Cc, P, A, seed=seed, scale=ATTN_SCALE)
    B, Lc, V, E, H, NL = FUSED200 if which == "fused200" else T.LSTM_SHAPES[which]
    return BO.random_params(V, E, H, NL, seed=seed, scale=LSTM_SCALE), torch.randn(B, E, generator=torch.Generator().manual_seed(seed + 1))


_ORACLE = {}


def case_oracle(case):
    """(ids, scores, lengths, met, margins[, alphas]) of the oracle, computed once per case and shared (callers leave it unchanged)."""
    key = case_id(case)
    if key not in _ORACLE:
        which, seed, Cn, K, D, cons, alpha, pad, special = case
        L = shape_of(which)[1]
        force, kg = case_force(case), K >> Cn
        if which == "attn":
            params, feats, fmap = case_problem(case)
            ids, sc, ln, al, met, margins = FO.attn_beam_search(params, feats, fmap, force, kg, L, pad_id=pad, length_penalty=alpha, **cons)
            _ORACLE[key] = (ids, sc, ln, met, margins, al)
        else:
            params, feats = case_problem(case)
            _ORACLE[key] = FO.beam_search(params, feats, force, kg, L, pad_id=pad, length_penalty=alpha, **cons)
    return _ORACLE[key]


def case_plain(case):
    """(ids, lengths) of the oracle's plain (decode-constrained) beam search of the same K."""
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    L = shape_of(which)[1]
    if which == "attn":
        params, feats, fmap = case_problem(case)
        out = CO.attn_beam_search(params, feats, fmap, K, L, pad_id=pad, length_penalty=alpha, **cons)
    else:
        params, feats = case_problem(case)
        out = CO.beam_search(params, feats, K, L, pad_id=pad, length_penalty=alpha, **cons)
    return out[0], out[2]


def full_mask(Cn):
    return (1 << Cn) - 1


def test_the_cases_cover_the_ground():
    assert {(c[2], c[3]) for c in CASES} == {(1, 2), (1, 8), (2, 4), (2, 8), (3, 8)}
    for w in ("generic", "fused", "attn", "fused200"):
        mine = [c for c in CASES if c[0] == w]
        assert {(c[2], c[3]) for c in mine} == {(1, 2), (1, 8), (2, 4), (2, 8), (3, 8)}
        assert {c[4] for c in mine} == {1, 4} and {c[5]["no_repeat_ngram"] for c in mine} == {0, 3} and {c[6] for c in mine} == {0.0, 0.7}
    hops = set()
    for c in CASES:
        f = case_force(c)
        B, L, V = shape_of(c[0])
        hops |= {(int(v), V) for v in f[f >= 0]}
        n = [int((f[b] >= 0).any(dim=1).sum()) for b in range(B)]
        assert {0, 1, c[2]} <= set(n), n                     # images with no, one and C constraints in one batch
        if c[2] >= 2:                                        # a token in two sets
            assert any(len(set(f[b, 0][f[b, 0] >= 0].tolist()) & set(f[b, 1][f[b, 1] >= 0].tolist())) for b in range(B))
        for v in c[8]:
            assert (f[0] == v).any(), (case_id(c), v)
    assert {(0, 50), (49, 50), (0, 64), (63, 64), (0, 200), (63, 200), (64, 200), (199, 200)} <= hops


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_covers_the_ground(case):
    """What made the case's seed eligible: the oracle decides at least 3/4 of the images by >= 1e-4, plain beam search of the same K
    meets every constraint on at most 1/4 of the images that carry any, and the forced search's slot 0 meets them on every image."""
    from gan_image_captioning_amd import engine
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    B, L, V = shape_of(which)
    force = case_force(case)
    engine.check_force_words(engine.pack_force_words(force, B), V, K, 2, pad, cons["suppress_tokens"])
    assert V - (len(cons["suppress_tokens"]) + 1 + (max(0, L - cons["no_repeat_ngram"]) if cons["no_repeat_ngram"] else 0) + Cn * D) >= K
    ids, sc, ln, met, margins = case_oracle(case)[:5]
    clear = sum(1 for sel, _ in margins if sel >= 1e-4)
    assert 4 * clear >= 3 * B, f"{clear} of {B} images with a selection margin >= 1e-4: {margins}"
    sets = force.tolist()
    pid, pln = case_plain(case)
    carry = [b for b in range(B) if FO.absent_mask(sets[b]) != full_mask(Cn)]
    hit = sum(1 for b in carry if FO.met_mask(pid[b, 0].tolist(), int(pln[b, 0]), sets[b]) == full_mask(Cn))
    assert 4 * hit <= len(carry), f"plain beam search meets the constraints on {hit} of {len(carry)} images: they do not bind"
    assert L >= Cn
    for b in range(B):
        assert int(met[b, 0]) == full_mask(Cn), (b, met[b])
        for j in range(K):
            assert int(met[b, j]) == FO.met_mask(ids[b, j].tolist(), int(ln[b, j]), sets[b]), (b, j)
        if not cons["no_repeat_ngram"]:
            continue
        live = ln[b] > 0
        T.check_invariants(ids[b][live], ln[b][live], L, cons["no_repeat_ngram"], cons["min_length"], cons["suppress_tokens"], pad_id=pad)


# ---------------------------------------------------------------- 1. the oracle against exhaustive search
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_oracle_slot0_is_the_exhaustive_argmax(seed):
    """V = 5, L = 3, C = 2, kg = 125 >= V^L: nothing is ever pruned, so slot 0 is the best of ALL sequences that meet both
    constraints (a sequence ends at its first <E>; the model may emit id 0 like any token), and every returned beam reports the mask
    of what it holds."""
    V, E, H, L, kg = 5, 4, 8, 3, 125
    params = BO.random_params(V, E, H, 1, seed=seed, scale=2.0)
    feats = torch.randn(1, E, generator=torch.Generator().manual_seed(seed))
    sets = [[[1, 3], [4, -1]]] if seed % 2 == 0 else [[[3, -1], [3, 4]]]
    ids, sc, ln, met, margins = FO.beam_search(params, feats, sets, kg, L, eos_id=2, pad_id=0)
    p = [t.double() for t in params]
    best, arg = -math.inf, None
    for seq in itertools.product(range(V), repeat=L):
        n = seq.index(2) + 1 if 2 in seq else L
        if any(v != 0 for v in seq[n:]):                     # (one representative per caption: pad behind <E>)
            continue
        if FO.met_mask(seq, n, sets[0]) != 3:
            continue
        st = FO.DO._LstmStepper(p, feats[0].double(), 1)
        lp = 0.0
        for t in range(n):
            logits, _ = st.step()
            lp += float(logits[0, seq[t]] - torch.logsumexp(logits[0], 0))
            st.reorder([0], [seq[t]])
        if lp > best:
            best, arg = lp, (seq, n)
    assert int(met[0, 0]) == 3 and int(ln[0, 0]) == arg[1]
    assert ids[0, 0].tolist() == list(arg[0])
    assert abs(float(sc[0, 0]) - best) < 1e-9
    for j in range(ids.shape[1]):
        assert int(met[0, j]) == FO.met_mask(ids[0, j].tolist(), int(ln[0, j]), sets[0])
        if int(ln[0, j]) == 0:
            assert sc[0, j] == -math.inf and set(ids[0, j].tolist()) == {0}


def test_oracle_without_hops_is_beam_search():
    """An image whose sets are all absent searches like plain beam search of width kg in its last state group."""
    params, feats = T.lstm_problem("generic", 3)
    force = torch.full((feats.shape[0], 2, 2), -1, dtype=torch.int32)
    ids, sc, ln, met, _ = FO.beam_search(params, feats, force, 2, 9, length_penalty=0.7)
    want = BO.beam_search(params, feats, 2, 9, length_penalty=0.7)
    assert torch.equal(ids[:, :2], want[0]) and torch.equal(sc[:, :2], want[1]) and torch.equal(ln[:, :2], want[2])
    assert (met == 3).all() and (ln[:, 2:] == 0).all() and (sc[:, 2:] == -math.inf).all()


# ---------------------------------------------------------------- 3. refusals
def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


def test_symbols_declared_bound_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "gicap.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    body = re.search(r"typedef struct gic_forced_words \{(.*?)\} gic_forced_words;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in L.ForcedWords._fields_]
    assert L.ABI_VERSION == 5 and lib.gic_abi_version() == 5


def _call(L, lib, which, beam=4, Cn=2, D=2, groups=1, cons=None, cws=256, fw=True, dims=None, eos=2):
    """One forced call on fake (non-null, aligned) pointers: every status comes back before any launch."""
    lstm = which == "lstm"
    d = (L.DecoderDims if lstm else L.AttnDims)(*(dims or (T.LSTM_DIMS if lstm else T.ATTN_DIMS)))
    p, s = (L.DecoderParams(), L.DecoderShadow()) if lstm else (L.AttnParams(), L.AttnShadow())
    for st in (p, s):
        for name, typ in st._fields_:
            setattr(st, name, (typ(*([256] * typ._length_)) if hasattr(typ, "_length_") else 256))
    o = L.DiverseBeamOpts()
    o.beam.beam, o.beam.eos_id, o.beam.pad_id, o.groups = beam, eos, 0, groups
    f = L.ForcedWords()
    f.C, f.D, f.ids = Cn, D, 256
    args = [C.byref(d), C.byref(p), C.byref(s), C.byref(o), C.byref(f) if fw else None, C.byref(cons) if cons is not None else None, 256, cws,
            256] + ([] if lstm else [256]) + [256, 256, 256] + ([] if lstm else [None]) + [256, None]
    rc = getattr(lib, "gic_decoder_forced_beam_search" if lstm else "gic_attn_forced_beam_search")(*args)
    return rc, lib.gic_last_error().decode()


@pytest.mark.parametrize("which", ["lstm", "attn"])
def test_library_refusals(which):
    """Each refusal the library can make (the ids live on the device) has its own text and comes before any launch; a call that
    passes them all is refused by the last check, the missing constraint workspace."""
    L, lib = _lib()
    for kw, msg in ((dict(Cn=4), "C must be 1..3"), (dict(Cn=0), "C must be 1..3"), (dict(D=5), "D must be 1..4"), (dict(D=0), "D must be 1..4"),
                    (dict(beam=6, Cn=2), "2^C = 4 must divide the beam size 6"), (dict(beam=4, Cn=3), "2^C = 8 must divide the beam size 4"),
                    (dict(groups=2), "groups must be 1"), (dict(fw=False), "null argument"), (dict(beam=9), "beam size must be 1..8")):
        rc, err = _call(L, lib, which, **kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    rc, err = _call(L, lib, which, cons=T._cons(L, n=2), cws=None)
    assert rc == -1 and "constraint workspace" in err, err
    rc, err = _call(L, lib, which, cons=T._cons(L, suppress=(2,)))
    assert rc == -1 and "eos_id" in err, err


def test_feasibility_grows_by_the_hop_tokens():
    """V - (S + 1 + max(0, L - n) + C * D) >= K: LSTM_DIMS has V = 50, L = 6; with n = 2, S = 16: 50 - 21 - C * D >= K."""
    L, lib = _lib()
    sup = tuple(range(3, 19))
    rc, err = _call(L, lib, "lstm", beam=8, Cn=3, D=4, cons=T._cons(L, n=2, suppress=sup), cws=None)          # 50 - 21 - 12 = 17 >= 8
    assert rc == -1 and "constraint workspace" in err, err
    dims = (4, 6, 36, 8, 16, 2, 0)
    rc, err = _call(L, lib, "lstm", beam=4, Cn=2, D=4, cons=T._cons(L, n=2, suppress=sup), cws=None, dims=dims)     # 36 - 21 - 8 = 7 >= 4
    assert rc == -1 and "constraint workspace" in err, err
    rc, err = _call(L, lib, "lstm", beam=8, Cn=2, D=4, cons=T._cons(L, n=2, suppress=sup), cws=None, dims=dims)     # 7 < 8
    assert rc == -1 and "infeasible constraints" in err and "8 hop tokens" in err, err
    rc, err = _call(L, lib, "lstm", beam=8, Cn=3, D=4, dims=(4, 6, 20, 8, 16, 2, 0))                              # no constraints: 20 - 1 - 12 < 8
    assert rc == -1 and "infeasible constraints" in err, err


def test_forced_ws_bytes():
    L, lib = _lib()
    out, base = C.c_uint64(0), C.c_uint64(0)
    for dims, K in ((T.LSTM_DIMS, 4), ((64, 20, 10000, 512, 512, 1, 1), 8)):
        d = L.DecoderDims(*dims)
        assert lib.gic_decoder_forced_beam_ws_bytes(C.byref(d), K, C.byref(out)) == 0
        assert lib.gic_decoder_beam_ws_bytes(C.byref(d), K, C.byref(base)) == 0
        rows, Lc = dims[0] * K, dims[1]
        assert out.value % 256 == 0 and out.value > base.value + 3 * rows * 12 * 4 + 2 * rows * Lc * 4
    d = L.AttnDims(*T.ATTN_DIMS)
    assert lib.gic_attn_forced_beam_ws_bytes(C.byref(d), 4, C.byref(out)) == 0 and out.value % 256 == 0
    assert lib.gic_attn_forced_beam_ws_bytes(C.byref(d), 9, C.byref(out)) == -1
    assert lib.gic_decoder_forced_beam_ws_bytes(C.byref(L.DecoderDims(*T.LSTM_DIMS)), 4, None) == -1


def test_python_refusals():
    """Every refusal of the issue, each with its own text, from the Python layer and before anything touches a GPU."""
    from gan_image_captioning_amd import engine
    ok = [[(5, 6), 7], [8], [], [(9,)]]

    def check(fw, V=50, beam=4, eos=2, pad=0, sup=()):
        engine.check_force_words(engine.pack_force_words(fw, len(fw)), V, beam, eos, pad, sup)

    check(ok)
    for fw, kw, msg in (([[0]], {}, "<PAD>"), ([[2]], {}, "<E>"), ([[50]], {}, r"outside \[0, 50\)"), ([[-3]], {}, r"outside \[0, V\)"),
                        ([[7]], dict(sup=(7,)), "suppressed id"), ([[(5, 5)]], {}, "duplicate id within a constraint"),
                        ([[4, 5, 6, 7]], {}, "at most 3 constraints"), ([[(4, 5, 6, 7, 8)]], {}, "at most 4 ids"),
                        ([[4, 5]], dict(beam=6), r"2\^C = 4 must divide the beam size 6"), ([[4, 5, 6]], dict(beam=4), r"2\^C = 8 must divide"),
                        ([[], []], {}, "every constraint of every image is absent")):
        with pytest.raises(ValueError, match=msg):
            check(fw, **kw)
    with pytest.raises(ValueError, match="one list of constraints per image"):
        engine.pack_force_words(ok, 3)
    with pytest.raises(ValueError, match=r"int32 \[B=2, C, D\]"):
        engine.pack_force_words(torch.zeros(2, 2, 2, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match=r"outside \[0, 50\)"):
        check(torch.tensor([[[-2, 5]]], dtype=torch.int32))


class _Dec:
    """A decoder stand-in whose engine must never be reached."""
    max_seq_length = 8

    def param_list(self):
        return []

    def engine(self):
        raise AssertionError("the refusal must come before the engine")


def test_refused_combinations():
    from gan_image_captioning_amd import generator as G
    feats = torch.zeros(2, 4)
    for kw in (dict(beam_groups=2), dict(diversity=0.5)):
        with pytest.raises(ValueError, match="beam_groups > 1"):
            G._beam_search(_Dec(), feats, (), 4, None, 2, 0.0, None, True, kw.get("beam_groups", 1), kw.get("diversity", 0.0), force_words=[[5], [6]])
    with pytest.raises(ValueError, match="return_met needs force_words"):
        G._beam_search(_Dec(), feats, (), 4, None, 2, 0.0, None, True, 1, 0.0, return_met=True)
    src = inspect.getsource(G.Generator.caption)
    assert "force_words with rerank_disc or consensus" in src
    gen = G.Generator.__new__(G.Generator)
    torch.nn.Module.__init__(gen)
    gen.decoder = _Dec()
    for kw in (dict(rerank_disc=object()), dict(consensus=object())):
        with pytest.raises(ValueError, match="force_words with rerank_disc or consensus"):
            G.Generator.caption(gen, None, beam_size=4, force_words=[[5]], **kw)
    with pytest.raises(ValueError, match="return_met needs force_words"):
        G.Generator.caption(gen, None, beam_size=4, return_met=True)
    ens = G.Ensemble.__new__(G.Ensemble)
    with pytest.raises(ValueError, match="force_words with an ensemble"):
        G.Ensemble.caption(ens, None, beam_size=4, force_words=[[5]])


# ---------------------------------------------------------------- 4. packing
def test_packing_of_the_list_form():
    from gan_image_captioning_amd import engine
    t = engine.pack_force_words([[(5, 6, 9), 7], [8], [], [(9,), 4, (3, 1)]], 4)
    assert t.dtype == torch.int32 and t.shape == (4, 3, 3)
    assert t.tolist() == [[[5, 6, 9], [7, -1, -1], [-1, -1, -1]], [[8, -1, -1], [-1, -1, -1], [-1, -1, -1]],
                          [[-1, -1, -1]] * 3, [[9, -1, -1], [4, -1, -1], [3, 1, -1]]]
    assert engine.pack_force_words([[], []], 2).shape == (2, 1, 1)
    same = torch.tensor([[[5, -1]], [[6, 7]]], dtype=torch.int32)
    assert engine.pack_force_words(same, 2) is same


def test_methods_take_the_keyword():
    from gan_image_captioning_amd.engine import AttnDecoderEngine, DecoderEngine
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder, Generator
    for f in (DecoderEngine.beam_search, AttnDecoderEngine.beam_search, Decoder.beam_search, AttnDecoder.beam_search, Generator.caption):
        ps = inspect.signature(f).parameters
        names = list(ps)
        assert names[-3:] == ["no_repeat_ngram", "min_length", "suppress_tokens"], f
        assert "force_words" in names and names.index("force_words") < names.index("no_repeat_ngram") and ps["force_words"].default is None, f
    ps = inspect.signature(Generator.caption).parameters
    assert ps["return_met"].default is False


# ---------------------------------------------------------------- 5. the flags
def test_flags_parse_and_combinations_are_refused():
    from gan_image_captioning_amd.args import build_parser, check_eval_forced, default_args
    from gan_image_captioning_amd.training import GANInstructor
    a = build_parser().parse_args([])
    assert (a.eval_force_words, a.eval_force_beam_size) == (0, 8) and check_eval_forced(a) is None
    a = build_parser().parse_args(["--eval-force-words", "2", "--eval-force-beam-size", "4", "--eval-min-length", "3"])
    assert check_eval_forced(a) == (2, 4)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--eval-force-words", "4"])
    for kw, msg in ((dict(eval_force_words=2, eval_force_beam_size=6), r"multiple of 2\^N = 4"),
                    (dict(eval_force_words=3, eval_force_beam_size=4), r"multiple of 2\^N = 8"),
                    (dict(eval_force_words=1, eval_force_beam_size=10), "must be 1..8"),
                    (dict(eval_force_words=5), "must be 0..3"),
                    (dict(eval_force_words=1, eval_ensemble="a.ckpt"), "the forced search runs one model"),
                    (dict(eval_force_words=1, eval_ensemble_ema=1), "the forced search runs one model"),
                    (dict(eval_force_words=1, eval_rerank_weight=0.5), "keeps its own order")):
        with pytest.raises(ValueError, match=msg):
            check_eval_forced(default_args(**kw))
    assert check_eval_forced(default_args(eval_force_words=0, eval_ensemble="a.ckpt")) is None
    ps = inspect.signature(GANInstructor.evaluate_forced).parameters
    assert list(ps)[1:] == ["what", "num_words", "beam_size", "length_penalty", "max_caption_len", "batch_size"]


def test_oracle_tags():
    """The N tokens of lowest document frequency among those in at least half of the references; ties to the lower id; barred ids
    and rarer-than-half tokens never; fewer candidates, fewer words."""
    from gan_image_captioning_amd.training import GANInstructor
    refs = [[1, 5, 6, 7, 2], [1, 5, 7, 9, 2], [1, 5, 8, 2], [1, 9, 2]]
    df = {5: 10, 7: 3, 9: 3, 6: 1, 8: 1}
    assert GANInstructor.oracle_tags(refs, 2, df, {0, 1, 2}) == [7, 9]           # 6 and 8 are rarer but in one reference of four
    assert GANInstructor.oracle_tags(refs, 3, df, {0, 1, 2}) == [7, 9, 5]
    assert GANInstructor.oracle_tags(refs, 3, df, {0, 1, 2, 9}) == [7, 5]
    assert GANInstructor.oracle_tags([[1, 2]], 2, df, {0, 1, 2}) == []


def test_list_form_takes_integer_scalars_of_any_kind():
    """Tagger output arrives as numpy or torch integers as often as Python ints."""
    import numpy as np
    from gan_image_captioning_amd import engine
    want = engine.pack_force_words([[(5, 6), 7], [8]], 2)
    got = engine.pack_force_words([[(np.int64(5), np.int32(6)), np.int64(7)], [torch.tensor(8)]], 2)
    assert torch.equal(want, got)
    assert torch.equal(engine.pack_force_words([np.array([5, 6]), np.array([8])], 2), torch.tensor([[[5], [6]], [[8], [-1]]], dtype=torch.int32))


def test_unigram_df_reads_the_tables_own_keys():
    from gan_image_captioning_amd.cider import document_frequency, unigram_df, unpack_key
    corpus = [[[1, 5, 6, 2], [1, 5, 7, 2]], [[1, 5, 9, 2]], [[1, 7, 7, 2]]]
    keys, df = document_frequency(corpus)
    got = unigram_df(keys, df)
    assert got == {5: 2, 6: 1, 7: 2, 9: 1}                   # images, not occurrences; the specials are stripped before the table
    assert got == {unpack_key(k)[0]: int(d) for k, d in zip(keys, df) if len(unpack_key(k)) == 1}


def test_ensemble_caption_keeps_generator_captions_keywords():
    from gan_image_captioning_amd.generator import Ensemble, Generator
    g, e = list(inspect.signature(Generator.caption).parameters), list(inspect.signature(Ensemble.caption).parameters)
    assert e[:-1] == g and e[-1] == "states"
    with pytest.raises(ValueError, match="force_words with an ensemble"):
        Ensemble.caption(Ensemble.__new__(Ensemble), None, beam_size=4, return_met=True)
