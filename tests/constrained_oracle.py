"""CPU oracle (float64 torch) of the constrained decodes (include/gicap.h gic_decode_constraints, gic_*_constrained_beam_search,
gic_*_constrained_sample_captions): beam search, diverse beam search and sampling for both decoders, built from the steppers of
tests/diverse_beam_oracle.py and the truncation and draw of tests/sample_oracle.py.

A live row about to emit its token of step t may not emit a token of ``banned(history, ...)``: the suppressed ids, <E> while
t + 1 < min_length, and with n >= 1 every token that would complete an n-gram the row's history already holds.  The beam heads take
each row's top-K among the admissible tokens and keep logp = logit - logsumexp(all logits); the sampler removes the banned tokens
before top-k / top-p and keeps the score's logsumexp over the full vocabulary.

The margins are those of the unconstrained oracles: per image the selection margin and the order margin of the beam searches, per
row the smallest draw / nucleus margin of the sampler (over the admissible tokens)."""
from __future__ import annotations

import math

import torch

from tests import attn_beam_oracle as AO
from tests import diverse_beam_oracle as DO
from tests import sample_oracle as SO


def banned(y, n=0, min_length=0, suppress=(), eos_id=2):
    """The banned set of a row with history y (a list of t tokens) about to emit token t, written the naive way."""
    t = len(y)
    out = set(int(v) for v in suppress)
    if t + 1 < min_length:
        out.add(eos_id)
    if n >= 1 and t >= n - 1:
        prefix = y[t - n + 1:t] if n > 1 else []
        for i in range(0, t - n + 1):
            if y[i:i + n - 1] == prefix:
                out.add(y[i + n - 1])
    return out


def violates(seq, length, n=0, min_length=0, suppress=()):
    """True if the caption seq[:length] breaks a constraint: a repeated n-gram, a suppressed id, or fewer than min_length tokens
    (min_length <= L, so a caption of L tokens is never too short)."""
    s = [int(v) for v in seq[:length]]
    if any(v in set(suppress) for v in s):
        return True
    if length < min_length:
        return True
    if n >= 1:
        grams = [tuple(s[i:i + n]) for i in range(len(s) - n + 1)]
        if len(grams) != len(set(grams)):
            return True
    return False


def feasible(V, L, k, n=0, suppress=()):
    """The feasibility bound of gicap.h: every row can always propose k admissible tokens."""
    worst = len(suppress) + 1 + (max(0, L - n) if n >= 1 else 0)
    return V - worst >= k


def _search_image(stepper, k, G, lam, L, eos_id, pad_id, length_penalty, cons, P=0):
    """diverse_beam_oracle._search_image with each live row's banned tokens removed from its proposals."""
    n, min_length, suppress = cons
    kg = k // G
    score = [0.0 if j % kg == 0 else -math.inf for j in range(k)]
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
        # a banned token is proposed by nobody: -inf as a logit (the rank within the row) and as a candidate score, so a row left with
        # fewer than k admissible tokens fills up with candidates that no finite one loses to; the others keep their raw logp
        admissible, adm_logp = logits.clone(), logp.clone()
        for j in range(k):
            if not fin[j]:
                ban = sorted(banned(seqs[j], n, min_length, suppress, eos_id))
                if ban:
                    admissible[j, torch.tensor(ban)] = -math.inf
                    adm_logp[j, torch.tensor(ban)] = -math.inf
        h = {}
        sel = []
        for g in range(G):
            kept, m = DO.select_group(score, fin, admissible, adm_logp, range(g * kg, (g + 1) * kg), k, kg, lam, h, pad_id)
            margin = min(margin, m)
            for (_, j, _, tok, _) in kept:
                if not fin[j]:
                    h[tok] = h.get(tok, 0) + 1
            sel += kept
        new_fin, new_len, new_seqs, new_alph = [], [], [], []
        for (s, j, q, tok, _) in sel:
            new_fin.append(fin[j] or tok == eos_id)
            new_len.append(ln[j] if fin[j] else t + 1)
            new_seqs.append(seqs[j] + [tok])
            new_alph.append(alph[j] + [zero if (fin[j] or alpha is None) else alpha[j]])
        score = [e[0] for e in sel]
        fin, ln, seqs, alph = new_fin, new_len, new_seqs, new_alph
        stepper.reorder([e[1] for e in sel], [e[3] for e in sel])
    norm = [score[j] / (ln[j] ** length_penalty) for j in range(k)]
    order = []
    for g in range(G):
        og = sorted(range(g * kg, (g + 1) * kg), key=lambda j: (-norm[j], j))
        for i in range(kg - 1):
            a_, b_ = norm[og[i]], norm[og[i + 1]]
            if a_ != -math.inf:
                order_margin = min(order_margin, abs(a_ - b_))
        order += og
    return order, seqs, score, ln, alph, (margin, order_margin)


def _cons(no_repeat_ngram, min_length, suppress_tokens):
    return int(no_repeat_ngram), int(min_length), tuple(int(v) for v in suppress_tokens)


def beam_search(params, features, k, L, groups=1, diversity=0.0, eos_id=2, pad_id=0, length_penalty=0.0, states=None,
                no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    """The LSTM decoder's constrained (diverse) beam search: diverse_beam_oracle.diverse_beam_search's arguments and outputs (ids
    int64 [B, k, L], scores f64 [B, k], lengths int64 [B, k], margins: B (selection, order) pairs); groups = 1 is beam search."""
    cons = _cons(no_repeat_ngram, min_length, suppress_tokens)
    p = [t.detach().double().cpu() for t in params]
    feats = features.detach().double().cpu()
    B = feats.shape[0]
    res = []
    for b in range(B):
        h0 = c0 = None
        if states is not None:
            h0, c0 = states[0][:, b].double().cpu(), states[1][:, b].double().cpu()
        res.append(_search_image(DO._LstmStepper(p, feats[b], k, h0, c0), k, groups, diversity, L, eos_id, pad_id, length_penalty, cons))
    ids, scores, lengths, _, margins = DO._collect(res, B, k, L)
    return ids, scores, lengths, margins


def attn_beam_search(params, features, fmap, k, L, groups=1, diversity=0.0, eos_id=2, pad_id=0, length_penalty=0.0, states=None,
                     no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    """The attention decoder's: (ids, scores, lengths, alphas f64 [B, k, L, P], margins) as diverse_beam_oracle.attn_diverse_beam_search."""
    cons = _cons(no_repeat_ngram, min_length, suppress_tokens)
    gp = AO.as_dict(params)
    feats = features.detach().double().cpu()
    fm = fmap.detach().double().cpu()
    B, P = feats.shape[0], fm.shape[1]
    H = gp["decoder.lstm.weight_hh_l0"].shape[1]
    res = []
    for b in range(B):
        h0 = c0 = None
        if states is not None:
            h0, c0 = states[0].reshape(B, H)[b].double(), states[1].reshape(B, H)[b].double()
        res.append(_search_image(DO._AttnStepper(gp, feats[b], fm[b], k, h0, c0), k, groups, diversity, L, eos_id, pad_id,
                                 length_penalty, cons, P))
    return DO._collect(res, B, k, L, P)


def draw(l, u, ban, top_k=0, top_p=1.0, temperature=1.0):
    """sample_oracle.draw over the admissible tokens of one row: (token, l_tok - logsumexp(all of l), draw margin, nucleus margin)."""
    l = l.double()
    idx = torch.tensor([v for v in range(l.numel()) if v not in ban])
    tok, _, _, dm, pm = SO.draw(l[idx], u[idx], top_k, top_p, temperature)          # (top_k >= the admissible count: top-k is off)
    tok = int(idx[tok])
    return tok, float(l[tok] - torch.logsumexp(l, 0)), dm, pm


def _sample_image(stepper, n, L, u, top_k, top_p, temperature, eos_id, pad_id, cons):
    ngram, min_length, suppress = cons
    seqs = [[] for _ in range(n)]
    ids = torch.full((n, L), pad_id, dtype=torch.int64)
    scores = torch.zeros(n, dtype=torch.float64)
    lengths = torch.zeros(n, dtype=torch.int64)
    margin = torch.full((n,), math.inf, dtype=torch.float64)
    fin = [False] * n
    for t in range(L):
        logits, _ = stepper.step()
        toks = []
        for r in range(n):
            if fin[r]:
                toks.append(pad_id)
                continue
            ban = banned(seqs[r], ngram, min_length, suppress, eos_id)
            tok, lp, dm, pm = draw(logits[r], u[t, r], ban, top_k, top_p, temperature)
            seqs[r].append(tok)
            ids[r, t] = tok
            scores[r] += lp
            lengths[r] = t + 1
            margin[r] = min(float(margin[r]), dm, pm)
            fin[r] = tok == eos_id
            toks.append(tok)
        if all(fin):
            break
        stepper.reorder(list(range(n)), toks)
    return ids, scores, lengths, margin


def sample(params, features, n, L, noise_u, top_k=0, top_p=1.0, temperature=1.0, eos_id=2, pad_id=0, no_repeat_ngram=0, min_length=0,
           suppress_tokens=()):
    """The LSTM decoder's constrained sampling decode with explicit noise u [L, B*n, V]: sample_oracle.decode's outputs (ids int64
    [B, n, L], scores f64 [B, n], lengths int64 [B, n], margin f64 [B, n])."""
    cons = _cons(no_repeat_ngram, min_length, suppress_tokens)
    p = [t.detach().double().cpu() for t in params]
    feats = features.detach().double().cpu()
    B = feats.shape[0]
    u = noise_u.detach().double().cpu()
    out = [_sample_image(DO._LstmStepper(p, feats[b], n), n, L, u[:, b * n:(b + 1) * n], top_k, top_p, temperature, eos_id, pad_id, cons)
           for b in range(B)]
    return tuple(torch.stack([o[i] for o in out]) for i in range(4))


def attn_sample(params, features, fmap, n, L, noise_u, top_k=0, top_p=1.0, temperature=1.0, eos_id=2, pad_id=0, no_repeat_ngram=0,
                min_length=0, suppress_tokens=()):
    """The attention decoder's constrained sampling decode: the outputs of ``sample``."""
    cons = _cons(no_repeat_ngram, min_length, suppress_tokens)
    gp = AO.as_dict(params)
    feats = features.detach().double().cpu()
    fm = fmap.detach().double().cpu()
    B = feats.shape[0]
    u = noise_u.detach().double().cpu()
    out = [_sample_image(DO._AttnStepper(gp, feats[b], fm[b], n), n, L, u[:, b * n:(b + 1) * n], top_k, top_p, temperature, eos_id, pad_id,
                         cons) for b in range(B)]
    return tuple(torch.stack([o[i] for o in out]) for i in range(4))
