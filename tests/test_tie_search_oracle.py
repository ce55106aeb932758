"""tests/tie_search_oracle.py without a GPU: the tables are what they claim, every table's runs meet the tie situations it is there
for, the emulation agrees with the float64 oracles where no tie decides, and each of the three tie rules is pinned -- reversing it
changes the result on at least one table."""
import math

import numpy as np
import pytest
import torch

from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import tie_search_oracle as TO

VOCABS = (50, 64, 68, 4100)          # generic / attention / fused with a ragged tile / 65 tiles
EOS = 2


def _lse(t):
    return np.float32(TO.lse64(t))


def _run_all(t, flip=None):
    lse = _lse(t)
    return {label: TO.search(t, lse, flip=flip, **kw) for label, kw in TO.runs(t)}


@pytest.fixture(scope="module")
def results():
    """Every run of every table at every vocabulary, computed once and shared (read-only)."""
    return {(V, name): _run_all(t) for V in VOCABS for name, t in TO.tables(V).items()}


def _met(runs):
    out = {}
    for r in runs.values():
        for k, v in r["stats"].items():
            out[k] = out.get(k, 0) + int(v)
    return out


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("V", VOCABS)
def test_tables_are_dyadic_with_maximum_zero(V):
    for name, t in TO.tables(V).items():
        assert t.dtype == np.float32 and t.shape == (V,) and float(t.max()) == 0.0, name
        assert np.array_equal(t * 4, np.round(t * 4)) and float(t.min()) >= -4.0, name       # multiples of 1/4: every x - max is exact
        # bf16 holds them too (8 significant bits), so a bf16 store of the teacher-forced logits shows them unchanged
        assert np.array_equal(torch.from_numpy(t).bfloat16().float().numpy(), t), name
        s = TO.suppressed_id(t)
        assert s != EOS and t[s] == max(t[v] for v in range(V) if v != EOS), name      # tied for the top (<E> aside)


@pytest.mark.parametrize("V", VOCABS)
def test_first_proposals_are_the_id_order_of_the_maxima(V):
    T = TO.tables(V)
    assert TO.proposals(T["all_equal"], 8) == list(range(8))
    assert all((EOS in TO.proposals(T["all_equal"], K)) == (K >= 3) for K in TO.PLAIN_K)
    assert TO.proposals(T["seam8"], 3) == [7, 8, 0]                       # the seam of two 8-entry lane segments, then the id order
    assert TO.proposals(T["eos_top"], 3) == [2, 9, 17]
    assert TO.proposals(T["eos_tied"], 5) == [2, 5, 11, 1, 3]
    assert TO.proposals(T["two_level"], 5) == [6, 2, 21, 30, 31]
    seam = {50: [49, 47, 48], 64: [0, 63, 31, 32], 68: [60, 63, 64, 67, 0], 4100: [5, 63, 4032, 4095, 4096, 4099, 64, 4031]}[V]
    assert TO.proposals(T["tile_seam"], len(seam)) == seam
    if V == 4100:
        # 65 tiles: lane 0 of beam_select merges tiles 0 and 64; the maxima sit in tiles 0, 63 and 64, on both sides of two seams
        assert -(-V // 64) == 65 and {v // 64 for v in np.nonzero(T["tile_seam"] == 0.0)[0]} == {0, 63, 64}
    if V == 68:
        assert {v // 64 for v in (60, 63, 64, 67)} == {0, 1} and V % 64 == 4
    # a banned id proposes nothing: the next id of the level moves up
    assert TO.proposals(T["seam8"], 2, ban={7}) == [8, 0]


# ---------------------------------------------------------------- what the runs of each table meet
MEETS = {
    "all_equal": ("row_ties", "sel_ties", "sel_ties_perm", "final_ties", "final_ties_fin_live", "eos_steps"),
    "seam8": ("row_ties", "sel_ties_cross", "sel_ties_perm", "final_ties"),
    "eos_top": ("row_ties", "sel_ties", "final_ties", "eos_steps"),
    "eos_tied": ("row_ties", "sel_ties_cross", "final_ties", "eos_steps"),
    "two_level": ("row_ties", "sel_ties_cross", "sel_ties_perm", "final_ties", "final_ties_fin_live", "eos_steps"),
    "tile_seam": ("row_ties", "sel_ties_cross", "final_ties"),
}


@pytest.mark.parametrize("V", VOCABS)
def test_every_table_meets_its_ties(results, V):
    for name in TO.tables(V):
        met = _met(results[(V, name)])
        for prop in MEETS[name]:
            assert met[prop] >= 1, (V, name, prop, met)


@pytest.mark.parametrize("V", VOCABS)
def test_named_situations(results, V):
    R = {name: results[(V, name)] for name in TO.tables(V)}
    # histories (a, b) and (b, a) from different parents, bit-equal at the boundary between the K-th and the (K+1)-th candidate
    for label in ("k5a0", "k8a0", "k4g2cons"):
        assert R["two_level"][label]["stats"]["sel_ties_perm"] >= 1, label
    # a beam that ended with <E> at the last step and a live one, equal score and equal length, under alpha = 1 -- and in slots of
    # their own, so the GPU test asserts their order (the beam index decides) and not just their set
    r = R["two_level"]["k8a1"]
    assert r["stats"]["final_ties_fin_live"] >= 1
    pairs = [(a, a + 1) for a in range(7) if r["scores"][a] == r["scores"][a + 1] and r["lengths"][a] == r["lengths"][a + 1]
             and (r["ids"][a, -1] == EOS) != (r["ids"][a + 1, -1] == EOS)]
    assert pairs and all([a] in r["clusters"] and [b] in r["clusters"] for a, b in pairs)
    # all_equal meets the same tie, but there every normalised score is -lse: the whole final order is one cluster
    r = R["all_equal"]["k8a1"]
    assert r["stats"]["final_ties_fin_live"] >= 1 and r["clusters"] == [list(range(8))]
    # <E> alone at the top: k = 1 stops after one step
    r = R["eos_top"]["k1a0"]
    assert r["ids"].tolist() == [[2, 0, 0, 0, 0, 0]] and r["lengths"].tolist() == [1] and r["stats"]["steps"] == 1
    # a finished beam is carried beside live ones to the last step
    r = R["all_equal"]["k5a0"]
    assert r["lengths"].min() == 1 and r["lengths"].max() == TO.L_TIES and r["stats"]["steps"] == TO.L_TIES
    # the constrained runs: no suppressed id, no repeated bigram, no <E> before min_length
    for name, t in TO.tables(V).items():
        s = TO.suppressed_id(t)
        for label in ("k3g1cons", "k5g1cons", "k4g2cons"):
            r = R[name][label]
            for row, n in zip(r["ids"].tolist(), r["lengths"].tolist()):
                assert not CO.violates(row, n, 2, 3, (s,)), (name, label, row)
    # alpha = 1: some run holds beams whose normalised scores are too close to call without powf (compared as a set, together with
    # the true ties that adjoin them), and alpha = 0 never does
    assert any(len(c) > 1 for runs in R.values() for label, r in runs.items() for c in r["clusters"])
    assert all(len(c) == 1 for runs in R.values() for label, r in runs.items() if label.endswith("a0") for c in r["clusters"])
    for runs in R.values():
        for r in runs.values():
            assert sorted(s for c in r["clusters"] for s in c) == list(range(len(r["lengths"])))


# ---------------------------------------------------------------- each tie rule is pinned
@pytest.mark.parametrize("flip", ["id", "lane", "beam"])
def test_reversing_a_tie_rule_changes_the_result(results, flip):
    """The mutation check: with equal logits going to the higher id, equal keys to the higher lane or equal normalised scores to the
    higher beam index, at least one table's runs differ from the unreversed ones -- on every vocabulary."""
    for V in VOCABS:
        changed = []
        for name, t in TO.tables(V).items():
            mut = _run_all(t, flip)
            for label, r in results[(V, name)].items():
                m = mut[label]
                if not all(np.array_equal(m[k], r[k]) for k in ("ids", "scores", "lengths")):
                    changed.append((name, label))
        assert changed, (V, flip)


# ---------------------------------------------------------------- against the float64 oracles, where no tie decides
def _problem(V, seed):
    """A table without equal entries as the b_out of an LSTM decoder whose w_out is zero: the float64 oracles then search that table."""
    g = torch.Generator().manual_seed(seed)
    tab = -3.0 * torch.rand(V, generator=g)
    tab[EOS] = -0.3
    tab[int(torch.argmax(tab))] = 0.0
    params = BO.random_params(V, 8, 16, 1, seed=seed)
    params[-2] = torch.zeros_like(params[-2])
    params[-1] = tab.float()
    return params, torch.randn(1, 8, generator=g), tab.float().numpy()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_one_beam_per_group_agrees_with_the_float64_oracle(seed):
    """G = K: every group keeps the best candidate of its only row, so no two histories compete and the same table at every step
    brings no permutation ties; the float64 oracle's margins are then those of the table and the penalty."""
    params, feats, t = _problem(50, seed)
    lse = _lse(t)
    held = dict(no_repeat_ngram=2, min_length=3, suppress_tokens=(int(np.argmax(t)),))
    for K, lam, cons in ((1, 0.0, {}), (4, 0.5, {}), (8, 1.0, {}), (4, 0.25, held)):
        ids, sc, ln, margins = CO.beam_search(params, feats, K, TO.L_TIES, K, lam, **cons)
        assert margins[0][0] >= 1e-4, (K, margins)
        kw = dict(cons)
        if kw:
            kw["suppress"] = kw.pop("suppress_tokens")
        r = TO.search(t, lse, K, TO.L_TIES, groups=K, lam=lam, **kw)
        assert np.array_equal(r["ids"], ids[0].numpy()) and np.array_equal(r["lengths"], ln[0].numpy()), (K, lam)
        np.testing.assert_allclose(r["scores"], sc[0].numpy(), rtol=0, atol=TO.L_TIES * 2.0 ** -21)      # (6 sums of |logp| < 8)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_two_steps_agree_with_the_float64_oracle(seed, K):
    """L = 2: the only exact ties are histories (a, b) and (b, a), whose sums are equal bit for bit in float64 and in float32 alike
    (addition commutes), and both oracles give them to the lower (parent, rank) -- so they agree although the reported margin is 0."""
    params, feats, t = _problem(68, seed)
    lse = _lse(t)
    ids, sc, ln, _ = BO.beam_search(params, feats, K, 2)
    r = TO.search(t, lse, K, 2)
    assert np.array_equal(r["ids"], ids[0].numpy()) and np.array_equal(r["lengths"], ln[0].numpy())
    np.testing.assert_allclose(r["scores"], sc[0].numpy(), rtol=0, atol=2 * 2.0 ** -21)


# ---------------------------------------------------------------- the bound on the device's logsumexp
@pytest.mark.parametrize("V", VOCABS)
def test_lse_bound_is_a_few_ulps(V):
    for name, t in TO.tables(V).items():
        ref = TO.lse64(t)
        b = TO.lse_bound(V, t)
        assert ref == pytest.approx(math.log(np.exp(t.astype(np.float64)).sum()), rel=1e-14)
        # (19 + 6 * (7 or 8)) u on the sum, 6 u on the logarithm: a few millionths, and wide enough for a float32 rounding of lse
        n = 19 + 6 * (-(-(-(-V // 64)) // 64) + 6)
        assert n == (67 if V == 4100 else 61)
        assert n * 2.0 ** -24 <= b <= (n * 1.01 + 6 * abs(ref)) * 2.0 ** -24, (name, b)
        assert abs(float(np.float32(ref)) - ref) <= b
