"""The search semantics of include/gicap.h (gic_decoder_beam_search, gic_*_diverse_beam_search, gic_decode_constraints) restated in
numpy float32 arithmetic over ONE table of logits that every row sees at every step -- what the device computes when w_out is all
zero and the logits are b_out.  Unlike the float64 oracles (tests/beam_oracle.py and its kin), which skip whatever a tie decides,
this one exists to decide ties: every comparison is the header's, in the header's order, and the scores are formed with the device's
roundings, so ids, lengths and the float32 bits of the scores are compared exactly.  The header is the authority; a difference between
header and kernel is a finding.

  proposals   a live row proposes its top K ids by (logit descending, id ascending) among the ids outside its banned set
              (tests/constrained_oracle.banned); banned ids propose nothing but stay in the logsumexp.
  scores      a live parent's candidate: f32(score + f32(x - lse)); a finished parent proposes itself once, score unchanged, token PAD.
  ranking     per group, candidates by (key descending, lane ascending), lane = (parent within the group) * K + rank; key = score for
              a finished parent's proposal, else f32(score - lambda * h), h = the earlier groups' picks of the token from live parents
              at this step (lambda dyadic and h a small integer: the product is exact with or without contraction).  The kept score
              is the unpenalised one.
  start       beam 0 of every group at score 0, the others at -inf.
  finish      finished = parent finished or token == <E>; length = t + 1, or the parent's if it had finished; an image whose K beams
              have all finished stops.
  order       within each group by f32(score / f32(len) ** alpha) descending, ties to the lower beam index.

``lse`` is the one thing taken from outside: the device's expf / logf cannot be emulated, so the GPU test reads the device's value
(a one-step search returns score[:, 0] = -lse exactly when the table's maximum is 0) and bounds it against float64 separately.

``flip`` reverses one tie rule ("id": equal logits to the HIGHER id, "lane": equal keys to the HIGHER lane, "beam": equal normalised
scores to the HIGHER beam index) -- the mutations of tests/test_tie_search_oracle.py, which show that each rule is pinned."""
from __future__ import annotations

import math

import numpy as np

from tests.constrained_oracle import banned

F = np.float32
NEG = F(-np.inf)


def lse64(table):
    """float64 logsumexp of the table (the reference the device's lse is bounded against)."""
    x = np.asarray(table, dtype=np.float64)
    m = x.max()
    return float(m + math.log(np.exp(x - m).sum()))


def lse_bound(V, table):
    """|lse_device - lse64| <= this, from operation counts in the rounding model of tests/aux_cases.py (u = 2^-24 per inexact f32
    operation on the magnitudes of its operands, a sum of positive terms with a longest chain of n roundings: (n + 4) u of the sum),
    expf and logf taken at 2 ulp = 4 u each.  With S = sum_v exp(x_v - max) (all terms positive, no cancellation):
      tile sums        x - m is exact for the dyadic tables; expf: 4 u per term; 8 adds per lane + 3 shuffle levels: (11 + 4) u
      merges           beam_select combines ceil(nblk / 64) tile partials per lane and 6 butterfly levels; a combine is
                       s * expf(m - mn) + s2 * expf(m2 - mn): expf 4 u, the product 1 u, the add 1 u = 6 u per combine on a chain
      lse = m + logf(s)  d(log S) = dS / S; logf: 4 u |log S|; the add: 1 u |lse|
    so |err| <= u * (4 + 15 + 6 * (ceil(nblk / 64) + 6)) * (1 + 2^-10) + 5 u |lse - max| + u |lse|."""
    u = 2.0 ** -24
    nblk = -(-V // 64)
    x = np.asarray(table, dtype=np.float64)
    ref = lse64(x)
    rel_s = u * (4 + 15 + 6 * (-(-nblk // 64) + 6)) * (1 + 2.0 ** -10)
    return rel_s + 5 * u * abs(ref - x.max()) + u * abs(ref)


def proposals(table, K, ban=(), flip=None):
    """The top K admissible ids of a row by (logit descending, id ascending)."""
    x = np.asarray(table)
    ids = np.arange(len(x))
    order = np.lexsort((-ids if flip == "id" else ids, -x))          # (the last key is the primary one)
    out = []
    for v in order.tolist():
        if v not in ban:
            out.append(v)
            if len(out) == K:
                break
    return out


def search(table, lse, K, L, groups=1, lam=0.0, alpha=0.0, eos=2, pad=0, no_repeat_ngram=0, min_length=0, suppress=(), flip=None):
    """One image's search.  Returns dict(ids int64 [K, L], scores f32 [K], lengths int64 [K], norm f32 [K] (the final order's keys, in
    the returned order), clusters (see below), stats).

    clusters: the returned slots as a list of lists.  With alpha = 0 every slot is its own cluster (the order is exact).  With
    alpha != 0 powf and the division are not emulated: consecutive beams of a group that are neither a true tie (equal score and
    equal length) nor more than 4 ulp apart in their normalised scores share a cluster, together with the true ties that adjoin them,
    and a cluster is compared as a set.

    stats (what the run exercised): row_ties = (step, live row) pairs whose proposals hold equal logits or end at a tie that the id
    decides; sel_ties = (step, group) selections whose last kept and first dropped candidate have equal keys; sel_ties_cross = those
    between different parents; sel_ties_perm = those between two live histories that hold the same tokens in another order;
    final_ties = true ties between consecutive beams of the final order; final_ties_fin_live = those between a beam that emitted <E>
    and one that did not; steps = steps that ran; eos_steps = (step, live row) pairs whose proposals hold <E>."""
    x = np.asarray(table, dtype=F)
    lse = F(lse)
    lam = F(lam)
    V = len(x)
    Kg = K // groups
    assert Kg * groups == K and K <= V
    lane_sign = -1 if flip == "lane" else 1
    score = [F(0.0) if j % Kg == 0 else NEG for j in range(K)]
    fin, ln, seqs = [False] * K, [0] * K, [[] for _ in range(K)]
    stats = dict(row_ties=0, sel_ties=0, sel_ties_cross=0, sel_ties_perm=0, final_ties=0, final_ties_fin_live=0, steps=0, eos_steps=0)
    for t in range(L):
        if all(fin):
            for j in range(K):
                seqs[j].append(pad)
            continue
        stats["steps"] += 1
        props = {}
        for j in range(K):
            if fin[j]:
                continue
            ban = banned(seqs[j], no_repeat_ngram, min_length, suppress, eos)
            props[j] = proposals(x, K, ban, flip)
            adm = [float(x[v]) for v in proposals(x, min(K + 1, V - len(ban)), ban)]
            if len(set(adm)) < len(adm):
                stats["row_ties"] += 1
            stats["eos_steps"] += eos in props[j]
        h = {}
        picks = []
        for g in range(groups):
            cands = []                                       # (key, lane, raw score, parent, token)
            for pl in range(Kg):
                p = g * Kg + pl
                if fin[p]:
                    cands.append((score[p], pl * K, score[p], p, pad))
                    continue
                for q, v in enumerate(props[p]):
                    raw = F(score[p] + F(x[v] - lse))
                    cands.append((F(raw - F(lam * F(h.get(v, 0)))), pl * K + q, raw, p, v))
            cands.sort(key=lambda e: (-float(e[0]), lane_sign * e[1]))
            kept = cands[:Kg]
            if len(cands) > Kg and cands[Kg][0] == cands[Kg - 1][0] and cands[Kg][0] != NEG:
                stats["sel_ties"] += 1
                stats["sel_ties_cross"] += cands[Kg][3] != cands[Kg - 1][3]
                ha, hb = (seqs[e[3]] + [e[4]] for e in (cands[Kg - 1], cands[Kg]))
                stats["sel_ties_perm"] += ha != hb and sorted(ha) == sorted(hb) and not fin[cands[Kg][3]] and not fin[cands[Kg - 1][3]]
            for e in kept:
                if not fin[e[3]]:
                    h[e[4]] = h.get(e[4], 0) + 1
            picks += kept
        score = [e[2] for e in picks]
        seqs = [seqs[e[3]] + [e[4]] for e in picks]
        ln = [ln[e[3]] if fin[e[3]] else t + 1 for e in picks]
        fin = [fin[e[3]] or e[4] == eos for e in picks]
    # ---- the final order, group by group
    beam_sign = -1 if flip == "beam" else 1
    norm = [F(score[j] / F(F(ln[j]) ** F(alpha))) for j in range(K)]
    order, clusters = [], []
    for g in range(groups):
        og = sorted(range(g * Kg, (g + 1) * Kg), key=lambda j: (-float(norm[j]), beam_sign * j))
        # links between consecutive beams: "far" (normalised scores more than 4 ulp apart: the order holds on the device), "tie" (equal
        # score and equal length: whatever powf returns, both get the same value and the beam index decides) or "near" (anything
        # else, a bit-equal quotient of different operands included: the device's powf and division may order them either way)
        links = []
        for i in range(1, Kg):
            a, j = og[i - 1], og[i]
            true_tie = score[a] == score[j] and ln[a] == ln[j]
            if true_tie:
                stats["final_ties"] += 1
                stats["final_ties_fin_live"] += fin[a] != fin[j]
            gap = abs(float(norm[a]) - float(norm[j]))
            ulp = float(np.spacing(np.abs(norm[a]))) if np.isfinite(norm[a]) else 0.0
            links.append("tie" if true_tie else "far" if alpha == 0.0 or gap > 4 * ulp or not np.isfinite(gap) else "near")
        # a run of beams joined by near and tie links moves as a whole if one of its near pairs swaps (a tied twin moves with its
        # partner), so such a run is one cluster; runs of ties alone keep one slot per beam
        start = 0
        for i in range(1, Kg + 1):
            if i == Kg or links[i - 1] == "far":
                run = list(range(g * Kg + start, g * Kg + i))
                clusters += [run] if "near" in links[start:i - 1] else [[slot] for slot in run]
                start = i
        order += og
    return dict(ids=np.array([seqs[j] for j in order], dtype=np.int64).reshape(K, L), scores=np.array([score[j] for j in order], dtype=F),
                lengths=np.array([ln[j] for j in order], dtype=np.int64), norm=np.array([norm[j] for j in order], dtype=F),
                clusters=clusters, stats=stats)


# ---------------------------------------------------------------- the tables (dyadic logits, maximum 0; <E> = 2, PAD = 0)
def _table(V, base, levels):
    x = np.full(V, base, dtype=F)
    for value, ids in levels:
        x[list(ids)] = value
    return x


def tables(V):
    """name -> logits f32 [V] for the vocabularies of the GPU test (50, 64, 68, 4100).  Every value is a small dyadic number, so the
    bias add, x - max and lambda * h are exact, and the maximum is 0."""
    last = V - 1
    out = {
        # every logit 0: pure id order; <E> is among the first K from K = 3 on
        "all_equal": _table(V, 0.0, []),
        # maxima at the seam of two 8-entry lane segments of tile 0
        "seam8": _table(V, -1.0, [(0.0, (7, 8))]),
        # <E> alone at the top
        "eos_top": _table(V, -1.0, [(0.0, (2,)), (-0.5, (9, 17))]),
        # <E> tied with other ids, a second level below
        "eos_tied": _table(V, -2.0, [(0.0, (2, 5, 11)), (-0.25, (1, 3, 20))]),
        # levels {0, -1, -1.5}: the histories (6, 21) and (21, 6) reach bit-equal scores from different parents, and with <E> beside 21
        # on the second level a beam that ends with <E> at the last step ties a live one (equal score, equal length) under alpha = 1
        "two_level": _table(V, -4.0, [(0.0, (6,)), (-1.0, (2, 21)), (-1.5, (30, 31))]),
    }
    if V == 68:          # the tile seam (63 | 64) and the ragged tile of 4 (64..67)
        out["tile_seam"] = _table(V, -1.0, [(0.0, (60, 63, 64, 67))])
    elif V == 50:        # the last entry of a ragged tile
        out["tile_seam"] = _table(V, -1.0, [(0.0, (49,)), (-0.5, (47, 48))])
    elif V == 4100:      # nblk = 65: lane 0 of beam_select merges tiles 0 and 64; maxima in tiles 0, 63 and 64
        out["tile_seam"] = _table(V, -3.0, [(0.0, (5, 63, 4032, 4095, 4096, 4099)), (-0.25, (64, 4031))])
    else:
        out["tile_seam"] = _table(V, -1.0, [(0.0, (0, last)), (-0.5, (31, 32))])
    assert all(float(t.max()) == 0.0 for t in out.values())
    return out


# ---------------------------------------------------------------- the searches of tests/test_gpu_search_ties.py
L_TIES = 6
PLAIN_K = (1, 2, 3, 5, 8)
ALPHAS = (0.0, 1.0)
DIVERSE = ((4, 2, 0.5), (6, 3, 0.25), (8, 8, 1.0))          # (K, G, lambda): lambda dyadic
# constrained: a no-repeat bigram, min_length 3 and one suppressed id that is tied for the top (suppressed_id); (K, G, lambda)
CONSTRAINED = ((3, 1, 0.0), (5, 1, 0.0), (4, 2, 0.5))


def suppressed_id(table, eos=2):
    """The lowest id tied for the table's maximum that is not <E>, else the lowest id of the next level."""
    x = np.asarray(table)
    for level in sorted(set(x.tolist()), reverse=True):
        ids = [int(v) for v in np.nonzero(x == level)[0] if v != eos]
        if ids:
            return ids[0]
    raise ValueError("no id to suppress")


def runs(table):
    """Every search of one table as (label, keyword arguments of ``search`` without lse)."""
    out = []
    for K in PLAIN_K:
        for a in ALPHAS:
            out.append((f"k{K}a{a:g}", dict(K=K, L=L_TIES, alpha=a)))
    for K, G, lam in DIVERSE:
        for a in ALPHAS:
            out.append((f"k{K}g{G}a{a:g}", dict(K=K, L=L_TIES, groups=G, lam=lam, alpha=a)))
    cons = dict(no_repeat_ngram=2, min_length=3, suppress=(suppressed_id(table),))
    for K, G, lam in CONSTRAINED:
        out.append((f"k{K}g{G}cons", dict(K=K, L=L_TIES, groups=G, lam=lam, alpha=0.0, **cons)))
    return out
