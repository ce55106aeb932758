"""Long-search cases for the float64 search oracles (tests/beam_oracle.py, tests/diverse_beam_oracle.py, tests/attn_beam_oracle.py):
problems whose searches run for many steps, mix finished and live beams, reorder their parents and stop image by image, so that a
float32 search on the device can be compared with the oracle well past step 1.  tests/test_search_cases.py pins, on the oracle alone,
what makes every case eligible; tests/test_gpu_search_long.py runs them on the device.

A case is (problem, search, seed, <E> bias, comparable, steps): ``search`` = ("beam", k, alpha) or ("diverse", k, G, lambda);
``comparable`` is the number of images whose selection margin is >= 1e-4 in the oracle's run (the images a float32 search must
reproduce) and ``steps`` the number of search steps those images ran.

LSTM problems: BO.random_params(V, E, H, NL, seed, scale=6.0) with the bias added to b_out[<E>], features randn(B, E) of seed + 1.
Attention problems: AO.random_problem(..., seed, scale=6.0) with the bias added likewise, at the dimensions of
tests/test_gpu_attn_beam.py's ORACLE_SHAPE and WIDE_SHAPE with L = 10.  With that generator's own inputs every image gets nearly the
same caption and a batch returns too few distinct tokens for the last floor of ``eligible``; the inputs are the test's to choose, so
the image features are scaled by FEAT_SCALE and the batch holds 24 images, which gives captions that differ by image.  Seed and
bias are per case: the first pair, seeds in ascending order, that meets every floor."""
from __future__ import annotations

import functools

import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import diverse_beam_oracle as DO

EOS, PAD = 2, 0
SCALE = 6.0
# B, L, V, E, H, NL
LSTM_PROBLEMS = {
    "generic": (16, 12, 50, 8, 16, 2),          # V % 4 != 0: the generic path (library GEMM + beam_tile_topk)
    "fused1": (16, 12, 68, 8, 16, 1),           # V = 68: one full 64-wide tile and a ragged tile of 4
    "fused2": (16, 12, 68, 8, 16, 2),
}
# B, L, V, E, H, C, P, A: the dimensions of tests/test_gpu_attn_beam.py's ORACLE_SHAPE and WIDE_SHAPE, 24 images, L = 10
ATTN_PROBLEMS = {"attn": (24, 10, 64, 16, 32, 40, 49, 24), "wide": (24, 10, 64, 8, 16, 136, 70, 264)}
FEAT_SCALE = 12.0                                # the image features of AO.random_problem, scaled: captions that differ by image
PLAIN = [("beam", k, a) for k in (2, 3, 5, 8) for a in (0.0, 0.7)]
DIVERSE = [("diverse", 4, 2, 1.0), ("diverse", 6, 3, 2.0), ("diverse", 8, 4, 0.5), ("diverse", 8, 8, 0.7)]
SEARCHES = PLAIN + DIVERSE

# (problem, search) -> (seed, <E> bias, comparable images, search steps those images ran)
TABLE = {
    ("generic", ("beam", 2, 0.0)): (7, 1.0, 16, 157),
    ("generic", ("beam", 2, 0.7)): (7, 1.0, 16, 157),
    ("generic", ("beam", 3, 0.0)): (7, 1.0, 16, 169),
    ("generic", ("beam", 3, 0.7)): (7, 1.0, 16, 169),
    ("generic", ("beam", 5, 0.0)): (7, 1.0, 16, 165),
    ("generic", ("beam", 5, 0.7)): (7, 1.0, 16, 165),
    ("generic", ("beam", 8, 0.0)): (7, 1.0, 15, 167),
    ("generic", ("beam", 8, 0.7)): (7, 1.0, 15, 167),
    ("generic", ("diverse", 4, 2, 1.0)): (7, 1.0, 16, 172),
    ("generic", ("diverse", 6, 3, 2.0)): (7, 1.0, 16, 187),
    ("generic", ("diverse", 8, 4, 0.5)): (7, 1.0, 16, 181),
    ("generic", ("diverse", 8, 8, 0.7)): (7, 1.0, 16, 189),
    ("fused1", ("beam", 2, 0.0)): (7, 1.0, 16, 139),
    ("fused1", ("beam", 2, 0.7)): (7, 1.0, 16, 139),
    ("fused1", ("beam", 3, 0.0)): (7, 1.0, 16, 159),
    ("fused1", ("beam", 3, 0.7)): (7, 1.0, 16, 159),
    ("fused1", ("beam", 5, 0.0)): (7, 1.0, 16, 169),
    ("fused1", ("beam", 5, 0.7)): (7, 1.0, 16, 169),
    ("fused1", ("beam", 8, 0.0)): (7, 1.0, 16, 180),
    ("fused1", ("beam", 8, 0.7)): (7, 1.0, 16, 180),
    ("fused1", ("diverse", 4, 2, 1.0)): (7, 1.0, 16, 181),
    ("fused1", ("diverse", 6, 3, 2.0)): (5, 1.0, 16, 184),
    ("fused1", ("diverse", 8, 4, 0.5)): (7, 1.0, 16, 191),
    ("fused1", ("diverse", 8, 8, 0.7)): (5, 1.0, 16, 184),
    ("fused2", ("beam", 2, 0.0)): (7, 1.0, 16, 154),
    ("fused2", ("beam", 2, 0.7)): (7, 1.0, 16, 154),
    ("fused2", ("beam", 3, 0.0)): (7, 1.0, 16, 157),
    ("fused2", ("beam", 3, 0.7)): (7, 1.0, 16, 157),
    ("fused2", ("beam", 5, 0.0)): (7, 1.0, 16, 181),
    ("fused2", ("beam", 5, 0.7)): (7, 1.0, 16, 181),
    ("fused2", ("beam", 8, 0.0)): (7, 1.0, 16, 184),
    ("fused2", ("beam", 8, 0.7)): (7, 1.0, 16, 184),
    ("fused2", ("diverse", 4, 2, 1.0)): (7, 1.0, 16, 185),
    ("fused2", ("diverse", 6, 3, 2.0)): (7, 1.0, 16, 186),
    ("fused2", ("diverse", 8, 4, 0.5)): (7, 1.0, 15, 173),
    ("fused2", ("diverse", 8, 8, 0.7)): (2, 1.0, 15, 176),
    ("attn", ("beam", 2, 0.0)): (2, 0.5, 23, 188),
    ("attn", ("beam", 2, 0.7)): (2, 0.5, 23, 188),
    ("attn", ("beam", 3, 0.0)): (1, 0.125, 23, 195),
    ("attn", ("beam", 3, 0.7)): (1, 0.125, 23, 195),
    ("attn", ("beam", 5, 0.0)): (1, 0.125, 24, 220),
    ("attn", ("beam", 5, 0.7)): (1, 0.125, 24, 220),
    ("attn", ("beam", 8, 0.0)): (0, 0.375, 23, 224),
    ("attn", ("beam", 8, 0.7)): (0, 0.375, 23, 224),
    ("attn", ("diverse", 4, 2, 1.0)): (0, 0.375, 24, 220),
    ("attn", ("diverse", 6, 3, 2.0)): (1, 0.125, 24, 235),
    ("attn", ("diverse", 8, 4, 0.5)): (3, 0.375, 24, 220),
    ("attn", ("diverse", 8, 8, 0.7)): (0, 0.5, 21, 208),
    ("wide", ("beam", 2, 0.0)): (1, 0.25, 24, 173),
    ("wide", ("beam", 2, 0.7)): (1, 0.25, 24, 173),
    ("wide", ("beam", 3, 0.0)): (0, 0.75, 24, 185),
    ("wide", ("beam", 3, 0.7)): (0, 0.75, 24, 185),
    ("wide", ("beam", 5, 0.0)): (0, 0.75, 24, 196),
    ("wide", ("beam", 5, 0.7)): (0, 0.75, 24, 196),
    ("wide", ("beam", 8, 0.0)): (0, 0.75, 24, 198),
    ("wide", ("beam", 8, 0.7)): (0, 0.75, 24, 198),
    ("wide", ("diverse", 4, 2, 1.0)): (0, 0.75, 24, 220),
    ("wide", ("diverse", 6, 3, 2.0)): (0, 0.75, 24, 235),
    ("wide", ("diverse", 8, 4, 0.5)): (0, 0.75, 24, 236),
    ("wide", ("diverse", 8, 8, 0.7)): (0, 0.75, 23, 228),
}

CASES = [(p, s) + TABLE[(p, s)] for p in list(LSTM_PROBLEMS) + list(ATTN_PROBLEMS) for s in SEARCHES]


def case_id(case):
    p, s = case[:2]
    tail = f"k{s[1]}a{s[2]}" if s[0] == "beam" else f"k{s[1]}g{s[2]}l{s[3]}"
    return f"{p}-{tail}"


def shape(problem):
    return LSTM_PROBLEMS[problem] if problem in LSTM_PROBLEMS else ATTN_PROBLEMS[problem]


def problem(name, seed, bias):
    """LSTM: (params, features); attention: (params, features, fmap) -- float32 CPU tensors in the library's order."""
    if name in LSTM_PROBLEMS:
        B, L, V, E, H, NL = LSTM_PROBLEMS[name]
        params = BO.random_params(V, E, H, NL, seed=seed, scale=SCALE)
        params[-1] = params[-1].clone()
        params[-1][EOS] += bias
        return params, torch.randn(B, E, generator=torch.Generator().manual_seed(seed + 1))
    B, L, V, E, H, C, P, A = ATTN_PROBLEMS[name]
    params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=SCALE)
    params[6] = params[6].clone()
    params[6][EOS] += bias
    return params, feats * FEAT_SCALE, fmap


@functools.lru_cache(maxsize=None)
def oracle(name, search, seed, bias):
    """The oracle's run of one case: dict(ids, scores, lengths, margins, trace[, alphas]); computed once and shared (read-only)."""
    prob = problem(name, seed, bias)
    L = shape(name)[1]
    trace, out = [], {}
    if name in LSTM_PROBLEMS:
        if search[0] == "beam":
            ids, sc, ln, margins = BO.beam_search(*prob, search[1], L, length_penalty=search[2], trace=trace)
        else:
            ids, sc, ln, margins = DO.diverse_beam_search(*prob, search[1], search[2], search[3], L, trace=trace)
    else:
        if search[0] == "beam":
            ids, sc, ln, out["alphas"], margins = AO.beam_search(*prob, search[1], L, length_penalty=search[2], trace=trace)
        else:
            ids, sc, ln, out["alphas"], margins = DO.attn_diverse_beam_search(*prob, search[1], search[2], search[3], L, trace=trace)
    out.update(ids=ids, scores=sc, lengths=ln, margins=margins, trace=trace)
    return out


def groups_of(search):
    return 1 if search[0] == "beam" else search[2]


def eligibility(name, search, seed, bias):
    """What the oracle's run of a case offers, as a dict of the quantities tests/test_search_cases.py puts a floor under."""
    r = oracle(name, search, seed, bias)
    B, L = shape(name)[:2]
    k = search[1]
    ln = r["lengths"]
    comparable = sum(1 for sel, _ in r["margins"] if sel >= 1e-4)
    # ran[b, j]: beam j never emitted <E> (length L and another last token); a beam that ends with <E> at step L - 1 has length L too
    ran = (ln == L) & (r["ids"][..., L - 1] != EOS)
    # a beam that finished at step t <= L - 4 (length <= L - 3) is carried, finished, for >= 3 steps beside one that runs to L
    mixed = sum(1 for b in range(B) if int(ln[b].min()) <= L - 3 and bool(ran[b].any()))
    early = sum(1 for b in range(B) if int(ln[b].max()) < L)           # every beam finished before L: the image stops early
    late = sum(1 for b in range(B) if bool(ran[b].any()))              # a beam is still live after the last step
    moved = sum(1 for pars in r["trace"] for t, par in enumerate(pars) if t >= 2 and par != list(range(k)))
    live = torch.arange(L)[None, None] < ln[..., None]
    return dict(comparable=comparable, mean_len=float(ln.double().mean()), mixed=mixed, early=early, late=late, moved=moved,
                tokens=int(r["ids"][live].unique().numel()), steps=sum(len(p) for p in r["trace"]),
                compared_steps=sum(len(p) for p, (sel, _) in zip(r["trace"], r["margins"]) if sel >= 1e-4))


def eligible(name, search, e):
    """The floors of tests/test_search_cases.py on ``e`` = eligibility(...).  With one beam per group (G = k) every beam's parent is the
    group's only beam, so the parents are the identity by construction and that floor does not apply."""
    B, L = shape(name)[:2]
    k = search[1]
    return (4 * e["comparable"] >= 3 * B and e["mean_len"] >= L / 2 and e["mixed"] >= 1 and e["early"] >= 1 and e["late"] >= 1
            and (e["moved"] >= 1 or groups_of(search) == k) and e["tokens"] >= 20)
