"""CPU oracle (float64 torch) of the lexically constrained beam search (include/gicap.h gic_forced_words, gic_*_forced_beam_search), on
the steppers of tests/diverse_beam_oracle.py (the recurrences of tests/beam_oracle.py / tests/attn_beam_oracle.py) and the banned sets
of tests/constrained_oracle.py.

Image b carries C constraint sets (``force`` [B][C][D], -1 padded; an all -1 set is absent and met from the start).  A hypothesis'
state is the bitmask of met sets; the k = 2^C * kg beams of an image are 2^C state groups of kg beams, beam j in state j // kg.  The
oracle puts no limit on kg.  State group g keeps the kg best of
  stay  the top-k admissible non-hop tokens of each live parent of g (hop tokens: the ids of the sets outside the parent's state),
  pad   the single proposal of each finished parent of g,
  hop   token w of a live parent in state s != g with s | m(w) == g.
Tie order: score, the lower parent beam, stay before hop, the rank in the parent's row (stay) or the slot c * D + d of the token's
first unmet set (hop).  Final order: real constraints met (descending), score / length**alpha (descending), beam index; dead beams
last (all pad, length 0, score -inf, met = the initial state).

Per image it returns (selection margin, order margin): the smallest gap between the kg-th and the next candidate of any group at any
step, and the smallest gap between consecutive normalised scores of live beams that meet the same number of real constraints."""
from __future__ import annotations

import math

import torch

from tests import attn_beam_oracle as AO
from tests import constrained_oracle as CO
from tests import diverse_beam_oracle as DO


def absent_mask(sets):
    """The initial state: the bits of the all -1 sets."""
    return sum(1 << c for c, ids in enumerate(sets) if all(v < 0 for v in ids))


def met_mask(seq, length, sets):
    """The state of a caption: the absent sets plus every set one of whose ids it has emitted."""
    toks = set(int(v) for v in seq[:length])
    return absent_mask(sets) | sum(1 << c for c, ids in enumerate(sets) if any(v >= 0 and v in toks for v in ids))


def hop_slots(sets, s):
    """[(slot, token, target state)] of a row in state s: slot c * D + d of the token's first unmet set."""
    D = len(sets[0]) if sets else 0
    out, seen = [], set()
    for c, ids in enumerate(sets):
        if (s >> c) & 1:
            continue
        for d, v in enumerate(ids):
            if v < 0 or v in seen:
                continue
            seen.add(v)
            m = sum(1 << c2 for c2, ids2 in enumerate(sets) if v in ids2)
            out.append((c * D + d, int(v), s | m))
    return out


def _search_image(stepper, sets, kg, L, eos_id, pad_id, length_penalty, cons, P=0):
    n, min_length, suppress = cons
    C = len(sets)
    S = 1 << C
    k = S * kg
    init = absent_mask(sets)
    score = [0.0 if j == init * kg else -math.inf for j in range(k)]
    fin = [False] * k
    ln = [0] * k
    seqs = [[] for _ in range(k)]
    alph = [[] for _ in range(k)]
    zero = torch.zeros(P, dtype=torch.float64)
    margin = order_margin = math.inf
    for t in range(L):
        if all(fin):
            for j in range(k):
                seqs[j].append(pad_id)
                alph[j].append(zero)
            continue
        logits, alpha = stepper.step()
        logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        cands = [[] for _ in range(S)]                      # (score, parent, kind, rank or slot, token)
        for j in range(k):
            s = j // kg
            if score[j] == -math.inf:
                continue
            if fin[j]:
                cands[s].append((score[j], j, 0, 0, pad_id))
                continue
            hops = hop_slots(sets, s)
            out = set(CO.banned(seqs[j], n, min_length, suppress, eos_id)) | set(h[1] for h in hops)
            adm = logits[j].clone()
            if out:
                adm[torch.tensor(sorted(out))] = -math.inf
            order = torch.sort(-adm, stable=True).indices[:k].tolist()
            for q, tok in enumerate(order):
                if adm[tok] != -math.inf:
                    cands[s].append((score[j] + float(logp[j, tok]), j, 0, q, tok))
            for slot, tok, tgt in hops:
                cands[tgt].append((score[j] + float(logp[j, tok]), j, 1, slot, tok))
        sel = []
        for g in range(S):
            cg = sorted(cands[g], key=lambda e: (-e[0], e[1], e[2], e[3]))
            if len(cg) > kg:
                margin = min(margin, cg[kg - 1][0] - cg[kg][0])
            sel += cg[:kg] + [None] * (kg - min(kg, len(cg)))
        new = []
        for j, e in enumerate(sel):
            if e is None:                                   # a dead beam: its own parent, pad, finished
                new.append((-math.inf, True, 0, [pad_id] * (t + 1), [zero] * (t + 1), j, pad_id))
                continue
            sc, p, _, _, tok = e
            new.append((sc, fin[p] or tok == eos_id, ln[p] if fin[p] else t + 1, seqs[p] + [tok],
                        alph[p] + [zero if (fin[p] or alpha is None) else alpha[p]], p, tok))
        score = [e[0] for e in new]
        fin = [e[1] for e in new]
        ln = [e[2] for e in new]
        seqs = [e[3] for e in new]
        alph = [e[4] for e in new]
        stepper.reorder([e[5] for e in new], [e[6] for e in new])
    dead = [score[j] == -math.inf for j in range(k)]
    nreal = [bin((j // kg) & ~init).count("1") for j in range(k)]
    norm = [-math.inf if dead[j] else score[j] / (ln[j] ** length_penalty) for j in range(k)]
    order = sorted(range(k), key=lambda j: (dead[j], -nreal[j], -norm[j], j))
    for i in range(k - 1):
        a_, b_ = order[i], order[i + 1]
        if not dead[a_] and not dead[b_] and nreal[a_] == nreal[b_]:
            order_margin = min(order_margin, abs(norm[a_] - norm[b_]))
    met = [init if dead[j] else j // kg for j in range(k)]
    for j in range(k):
        if dead[j]:
            seqs[j], ln[j], alph[j] = [pad_id] * L, 0, [zero] * L
    return order, seqs, score, ln, alph, met, (margin, order_margin)


def _collect(res, B, k, L, P=None):
    ids, scores, lengths, alphas, margins = DO._collect([r[:5] + (r[6],) for r in res], B, k, L, P)
    met = torch.zeros(B, k, dtype=torch.int64)
    for b, r in enumerate(res):
        for slot, j in enumerate(r[0]):
            met[b, slot] = r[5][j]
    return ids, scores, lengths, alphas, met, margins


def _sets(force):
    return [[[int(v) for v in ids] for ids in img] for img in (force.tolist() if isinstance(force, torch.Tensor) else force)]


def beam_search(params, features, force, kg, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None, no_repeat_ngram=0, min_length=0,
                suppress_tokens=()):
    """The LSTM decoder (beam_oracle's parameter order); ``force`` int [B][C][D], k = 2^C * kg.  Returns (ids int64 [B, k, L], scores
    f64 [B, k], lengths int64 [B, k], met int64 [B, k], margins: B (selection, order) pairs)."""
    cons = CO._cons(no_repeat_ngram, min_length, suppress_tokens)
    p = [t.detach().double().cpu() for t in params]
    feats = features.detach().double().cpu()
    sets = _sets(force)
    B = feats.shape[0]
    k = (1 << len(sets[0])) * kg
    res = []
    for b in range(B):
        h0 = c0 = None
        if states is not None:
            h0, c0 = states[0][:, b].double().cpu(), states[1][:, b].double().cpu()
        res.append(_search_image(DO._LstmStepper(p, feats[b], k, h0, c0), sets[b], kg, L, eos_id, pad_id, length_penalty, cons))
    ids, scores, lengths, _, met, margins = _collect(res, B, k, L)
    return ids, scores, lengths, met, margins


def attn_beam_search(params, features, fmap, force, kg, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None, no_repeat_ngram=0,
                     min_length=0, suppress_tokens=()):
    """The attention decoder: (ids, scores, lengths, alphas f64 [B, k, L, P], met, margins)."""
    cons = CO._cons(no_repeat_ngram, min_length, suppress_tokens)
    gp = AO.as_dict(params)
    feats = features.detach().double().cpu()
    fm = fmap.detach().double().cpu()
    sets = _sets(force)
    B, P = feats.shape[0], fm.shape[1]
    k = (1 << len(sets[0])) * kg
    H = gp["decoder.lstm.weight_hh_l0"].shape[1]
    res = []
    for b in range(B):
        h0 = c0 = None
        if states is not None:
            h0, c0 = states[0].reshape(B, H)[b].double(), states[1].reshape(B, H)[b].double()
        res.append(_search_image(DO._AttnStepper(gp, feats[b], fm[b], k, h0, c0), sets[b], kg, L, eos_id, pad_id, length_penalty, cons, P))
    return _collect(res, B, k, L, P)
