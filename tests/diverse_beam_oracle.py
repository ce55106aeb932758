"""CPU diverse-beam-search oracle (float64 torch) restating gic_decoder_diverse_beam_search and gic_attn_diverse_beam_search
(include/gicap.h) for both decoders, with the steps of tests/beam_oracle.py (lstm_cell) and tests/attn_beam_oracle.py (step).

Besides the outputs it reports, per image, two decision margins as the beam oracles do: the selection margin, the smallest gap over
every step and group between the K'-th and the (K'+1)-th candidate's ranking key score + logp - lambda * h (penalty included), and the
order margin, the smallest gap between consecutive normalised scores score / length**alpha within a group of the final order.  Where a
margin is tiny a float32 search may legitimately decide differently."""
from __future__ import annotations

import math

import torch

from oracle import cpu_attention as CA
from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO


def select_group(score, fin, logits, logp, rows, k, kg, lam, h, pad_id):
    """One group's selection at one step: ``rows`` its parent beams, h {token: count} the earlier groups' picks from live parents.
    Returns (the kept candidates (raw score, parent, rank, token, key), the margin between the kg-th and the next key)."""
    cands = []
    for jl, j in enumerate(rows):
        if fin[j]:
            cands.append((score[j], j, jl, 0, pad_id, score[j]))
            continue
        order = torch.sort(-logits[j], stable=True).indices[:k].tolist()
        for q, tok in enumerate(order):
            raw = score[j] + float(logp[j, tok])
            cands.append((raw, j, jl, q, tok, raw - lam * h.get(tok, 0)))
    cands.sort(key=lambda e: (-e[5], e[2], e[3]))
    margin = math.inf
    if len(cands) > kg and cands[kg][5] != -math.inf:
        margin = cands[kg - 1][5] - cands[kg][5]
    return [(e[0], e[1], e[3], e[4], e[5]) for e in cands[:kg]], margin


def _search_image(stepper, k, G, lam, L, eos_id, pad_id, length_penalty, P=0, trace=None):
    kg = k // G
    score = [0.0 if j % kg == 0 else -math.inf for j in range(k)]
    fin = [False] * k
    ln = [0] * k
    seqs = [[] for _ in range(k)]
    alph = [[] for _ in range(k)]
    zero = torch.zeros(P, dtype=torch.float64)
    margin = order_margin = math.inf
    pars = []
    for t in range(L):
        if all(fin):
            for j in range(k):
                seqs[j].append(pad_id)
                alph[j].append(zero)
            continue
        logits, alpha = stepper.step()
        logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        h = {}
        sel = []
        for g in range(G):
            kept, m = select_group(score, fin, logits, logp, range(g * kg, (g + 1) * kg), k, kg, lam, h, pad_id)
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
        pars.append([e[1] for e in sel])
        stepper.reorder([e[1] for e in sel], [e[3] for e in sel])
    if trace is not None:
        trace.append(pars)
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


class _LstmStepper:
    def __init__(self, p, feat, k, h0=None, c0=None):
        NL = (len(p) - 3) // 4
        self.embed, self.w_out, self.b_out = p[0], p[-2], p[-1]
        self.layers = [p[1 + 4 * l:5 + 4 * l] for l in range(NL)]
        H = self.layers[0][1].shape[1]
        self.h = [(h0[l] if h0 is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1) for l in range(NL)]
        self.c = [(c0[l] if c0 is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1) for l in range(NL)]
        self.x = feat.repeat(k, 1)

    def step(self):
        inp = self.x
        for l in range(len(self.layers)):
            self.h[l], self.c[l] = BO.lstm_cell(inp, self.h[l], self.c[l], *self.layers[l])
            inp = self.h[l]
        return inp @ self.w_out.t() + self.b_out, None

    def reorder(self, par, toks):
        self.h = [hl[par] for hl in self.h]
        self.c = [cl[par] for cl in self.c]
        self.x = self.embed[toks]


class _AttnStepper:
    def __init__(self, gp, feat, fm, k, h0=None, c0=None):
        self.gp = gp
        H = gp["decoder.lstm.weight_hh_l0"].shape[1]
        self.fmb = fm.unsqueeze(0).expand(k, -1, -1)
        self.fpb = (fm @ gp["decoder.attn.w_f"].t() + gp["decoder.attn.b_f"]).unsqueeze(0).expand(k, -1, -1)
        self.h = (h0 if h0 is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1)
        self.c = (c0 if c0 is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1)
        self.x = feat.repeat(k, 1)

    def step(self):
        z, alpha = CA.attention(self.gp, self.fmb, self.fpb, self.h)
        self.h, self.c, logits = AO.step(self.gp, self.x, z, self.h, self.c)
        return logits, alpha

    def reorder(self, par, toks):
        self.h, self.c = self.h[par], self.c[par]
        self.x = self.gp["decoder.embed.weight"][toks]


def _collect(results, B, k, L, P=None):
    ids = torch.zeros(B, k, L, dtype=torch.int64)
    scores = torch.zeros(B, k, dtype=torch.float64)
    lengths = torch.zeros(B, k, dtype=torch.int64)
    alphas = torch.zeros(B, k, L, P, dtype=torch.float64) if P is not None else None
    margins = []
    for b, (order, seqs, score, ln, alph, m) in enumerate(results):
        margins.append(m)
        for r, j in enumerate(order):
            ids[b, r] = torch.tensor(seqs[j])
            scores[b, r] = score[j]
            lengths[b, r] = ln[j]
            if alphas is not None:
                alphas[b, r] = torch.stack(alph[j])
    return ids, scores, lengths, alphas, margins


def diverse_beam_search(params, features, k, groups, diversity, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None, trace=None):
    """The LSTM decoder (beam_oracle's parameter order).  Returns (ids int64 [B, k, L], scores f64 [B, k], lengths int64 [B, k],
    margins: list of B (selection, order) pairs), in group-major order.  ``trace`` as in tests/beam_oracle.py."""
    p = [t.detach().double().cpu() for t in params]
    feats = features.detach().double().cpu()
    B = feats.shape[0]
    res = []
    for b in range(B):
        h0 = c0 = None
        if states is not None:
            h0, c0 = states[0][:, b].double().cpu(), states[1][:, b].double().cpu()
        res.append(_search_image(_LstmStepper(p, feats[b], k, h0, c0), k, groups, diversity, L, eos_id, pad_id, length_penalty,
                                 trace=trace))
    ids, scores, lengths, _, margins = _collect(res, B, k, L)
    return ids, scores, lengths, margins


def attn_diverse_beam_search(params, features, fmap, k, groups, diversity, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None,
                             trace=None):
    """The attention decoder (attn_beam_oracle's parameter order).  Returns (ids, scores, lengths, alphas f64 [B, k, L, P], margins)
    as attn_beam_oracle.beam_search, in group-major order."""
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
        res.append(_search_image(_AttnStepper(gp, feats[b], fm[b], k, h0, c0), k, groups, diversity, L, eos_id, pad_id, length_penalty,
                                 P, trace))
    return _collect(res, B, k, L, P)
