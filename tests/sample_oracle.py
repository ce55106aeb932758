"""CPU oracle (float64 torch) of caption sampling: the truncation and the draw of gic_sample_logits and the decode of
gic_decoder_sample_captions (include/gicap.h), restated from their definitions.

Besides its outputs it reports each decision's margins: the draw margin, the gap between the two largest perturbed values
l_v / tau + g(u_v) over the kept set (which token is drawn), and the nucleus margin, |cumulative mass - top_p| at the nucleus
boundary (the mass of the kept set minus top_p, and top_p minus the mass of the next smaller set).  Where a margin is tiny a
float32 kernel may legitimately decide differently."""
from __future__ import annotations

import math

import torch

from tests.beam_oracle import lstm_cell


def gumbel(u):
    return -torch.log(-torch.log(u.double() + 1e-10) + 1e-10)


def truncate(l, top_k=0, top_p=1.0, temperature=1.0):
    """(kept bool [V], nucleus margin) for one row of logits l [V]: top-k (ties kept), then top-p over the renormalised
    softmax(l / temperature) of the top-k set (ties kept)."""
    l = l.double()
    V = l.numel()
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        kth = torch.sort(l, descending=True).values[top_k - 1]
        keep = l >= kth
    margin = math.inf
    if top_p < 1.0:
        q = torch.softmax(torch.where(keep, l / temperature, torch.full_like(l, -math.inf)), 0)
        vals = torch.unique(l[keep], sorted=True).flip(0)          # distinct kept values, descending
        prev = None
        for beta in vals:
            mass = float(q[l >= beta].sum())
            if mass >= top_p:
                margin = mass - top_p if prev is None else min(mass - top_p, top_p - prev)
                keep = keep & (l >= beta)
                break
            prev = mass
    return keep, margin


def kept_brute_force(l, top_k=0, top_p=1.0, temperature=1.0):
    """The kept set from a full sort: walk the entries in descending order (ties in any order); after top-k the set is every entry
    whose value is at least the k-th one; top-p then keeps the shortest prefix, extended over the ties of its last value, whose
    renormalised mass reaches top_p."""
    l = l.double()
    V = l.numel()
    order = sorted(range(V), key=lambda v: -float(l[v]))
    k = V if top_k == 0 else min(top_k, V)
    kth = float(l[order[k - 1]])
    cand = [v for v in order if float(l[v]) >= kth]
    if top_p >= 1.0:
        return set(cand)
    w = {v: math.exp((float(l[v]) - float(l[cand[0]])) / temperature) for v in cand}
    z = sum(w.values())
    for i in range(len(cand)):
        pre = [v for v in cand if float(l[v]) >= float(l[cand[i]])]
        if sum(w[v] for v in pre) / z >= top_p:
            return set(pre)
    return set(cand)


def draw(l, u, top_k=0, top_p=1.0, temperature=1.0):
    """(token, log-probability l_tok - logsumexp(l), kept count, draw margin, nucleus margin) for one row."""
    l = l.double()
    keep, pm = truncate(l, top_k, top_p, temperature)
    y = torch.where(keep, l / temperature + gumbel(u), torch.full_like(l, -math.inf))
    tok = int(torch.argmax(y))                  # first maximal index
    top2 = torch.topk(y, 2).values if int(keep.sum()) > 1 else None
    dm = float(top2[0] - top2[1]) if top2 is not None else math.inf
    lp = float(l[tok] - torch.logsumexp(l, 0))
    return tok, lp, int(keep.sum()), dm, pm


def decode(params, features, n, L, noise_u, top_k=0, top_p=1.0, temperature=1.0, eos_id=2, pad_id=0):
    """The LSTM decoder's sampling decode with explicit noise u [L, B*n, V].  Params in the library's order
    [embed, (w_ih, w_hh, b_ih, b_hh) * NL, w_out, b_out].  Returns (ids int64 [B, n, L], scores f64 [B, n], lengths int64 [B, n],
    margin f64 [B, n]: the smallest draw / nucleus margin of the row's live steps)."""
    p = [t.detach().double().cpu() for t in params]
    NL = (len(p) - 3) // 4
    layers = [p[1 + 4 * l:5 + 4 * l] for l in range(NL)]
    feats = features.detach().double().cpu()
    B, H = feats.shape[0], layers[0][1].shape[1]
    R = B * n
    u = noise_u.detach().double().cpu()
    x = feats.repeat_interleave(n, 0)
    h = [torch.zeros(R, H, dtype=torch.float64) for _ in range(NL)]
    c = [torch.zeros(R, H, dtype=torch.float64) for _ in range(NL)]
    ids = torch.full((R, L), pad_id, dtype=torch.int64)
    scores = torch.zeros(R, dtype=torch.float64)
    lengths = torch.zeros(R, dtype=torch.int64)
    margin = torch.full((R,), math.inf, dtype=torch.float64)
    fin = [False] * R
    for t in range(L):
        inp = x
        for l in range(NL):
            h[l], c[l] = lstm_cell(inp, h[l], c[l], *layers[l])
            inp = h[l]
        logits = inp @ p[-2].t() + p[-1]
        toks = []
        for r in range(R):
            if fin[r]:
                toks.append(pad_id)
                continue
            tok, lp, _, dm, pm = draw(logits[r], u[t, r], top_k, top_p, temperature)
            ids[r, t] = tok
            scores[r] += lp
            lengths[r] = t + 1
            margin[r] = min(float(margin[r]), dm, pm)
            fin[r] = tok == eos_id
            toks.append(tok)
        if all(fin):
            break
        x = p[0][torch.tensor(toks)]
    return ids.reshape(B, n, L), scores.reshape(B, n), lengths.reshape(B, n), margin.reshape(B, n)
