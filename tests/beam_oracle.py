"""CPU beam-search oracle (float64 torch) restating the semantics of gic_decoder_beam_search (include/gicap.h).

Parameters come in the library's order: [embed, (w_ih, w_hh, b_ih, b_hh) * NL, w_out, b_out] (nn.LSTM gate order i, f, g, o).
Besides the outputs it reports, per image, two decision margins: the selection margin, the smallest gap between the k-th and the
(k+1)-th candidate score over every step (which hypotheses survive), and the order margin, the smallest gap between consecutive
normalised scores score / length**alpha of the final order.  The order of the kept candidates within a step only breaks exact ties
later, so it has no margin of its own.  Where a margin is tiny a float32 search may legitimately decide differently."""
from __future__ import annotations

import math

import torch


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    g = x @ w_ih.t() + h @ w_hh.t() + b_ih + b_hh
    i, f, gg, o = g.chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def beam_search(params, features, k, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None, trace=None):
    """Returns (ids int64 [B, k, L], scores f64 [B, k], lengths int64 [B, k], margins: list of B (selection, order) pairs).
    ``trace``: a list that receives, per image, the chosen parent beams of every step that ran (a list of k-lists)."""
    p = [t.detach().double().cpu() for t in params]
    NL = (len(p) - 3) // 4
    embed, w_out, b_out = p[0], p[-2], p[-1]
    layers = [p[1 + 4 * l:5 + 4 * l] for l in range(NL)]
    feats = features.detach().double().cpu()
    B, H = feats.shape[0], layers[0][1].shape[1]
    ids = torch.full((B, k, L), pad_id, dtype=torch.int64)
    scores = torch.zeros(B, k, dtype=torch.float64)
    lengths = torch.zeros(B, k, dtype=torch.int64)
    margins = []
    for b in range(B):
        margin = order_margin = math.inf
        h = [(states[0][l, b].double().cpu() if states is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1) for l in range(NL)]
        c = [(states[1][l, b].double().cpu() if states is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1) for l in range(NL)]
        score = [0.0] + [-math.inf] * (k - 1)
        fin = [False] * k
        ln = [0] * k
        seqs = [[] for _ in range(k)]
        x = feats[b].repeat(k, 1)
        pars = []
        for t in range(L):
            if all(fin):
                for j in range(k):
                    seqs[j].append(pad_id)
                continue
            inp = x
            for l in range(NL):
                h[l], c[l] = lstm_cell(inp, h[l], c[l], *layers[l])
                inp = h[l]
            logits = inp @ w_out.t() + b_out
            logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
            cands = []
            for j in range(k):
                if fin[j]:
                    cands.append((score[j], j, 0, pad_id))
                    continue
                # top-k by raw logit, ties to the lower id (stable sort of the negated logits)
                order = torch.sort(-logits[j], stable=True).indices[:k].tolist()
                for q, tok in enumerate(order):
                    cands.append((score[j] + float(logp[j, tok]), j, q, tok))
            cands.sort(key=lambda e: (-e[0], e[1], e[2]))
            sel = cands[:k]
            if len(cands) > k and cands[k][0] != -math.inf:
                margin = min(margin, cands[k - 1][0] - cands[k][0])
            par = [e[1] for e in sel]
            pars.append(par)
            h = [hl[par] for hl in h]
            c = [cl[par] for cl in c]
            new_fin, new_len, new_seqs = [], [], []
            for (s, j, q, tok) in sel:
                new_fin.append(fin[j] or tok == eos_id)
                new_len.append(ln[j] if fin[j] else t + 1)
                new_seqs.append(seqs[j] + [tok])
            score = [e[0] for e in sel]
            fin, ln, seqs = new_fin, new_len, new_seqs
            x = embed[[e[3] for e in sel]]
        norm = [score[j] / (ln[j] ** length_penalty) for j in range(k)]
        order = sorted(range(k), key=lambda j: (-norm[j], j))
        for i in range(k - 1):
            a_, b_ = norm[order[i]], norm[order[i + 1]]
            if a_ != -math.inf:
                order_margin = min(order_margin, abs(a_ - b_))
        margins.append((margin, order_margin))
        if trace is not None:
            trace.append(pars)
        for r, j in enumerate(order):
            ids[b, r] = torch.tensor(seqs[j])
            scores[b, r] = score[j]
            lengths[b, r] = ln[j]
    return ids, scores, lengths, margins


def greedy(params, features, L, eos_id=2, pad_id=0):
    """Argmax decode (ties to the lower id), PAD after the first <E>: ids [B, L]."""
    p = [t.detach().double().cpu() for t in params]
    NL = (len(p) - 3) // 4
    layers = [p[1 + 4 * l:5 + 4 * l] for l in range(NL)]
    x = features.detach().double().cpu()
    B, H = x.shape[0], layers[0][1].shape[1]
    h = [torch.zeros(B, H, dtype=torch.float64) for _ in range(NL)]
    c = [torch.zeros(B, H, dtype=torch.float64) for _ in range(NL)]
    out = torch.full((B, L), pad_id, dtype=torch.int64)
    done = torch.zeros(B, dtype=torch.bool)
    for t in range(L):
        inp = x
        for l in range(NL):
            h[l], c[l] = lstm_cell(inp, h[l], c[l], *layers[l])
            inp = h[l]
        tok = torch.argmax(inp @ p[-2].t() + p[-1], dim=-1)
        out[:, t] = torch.where(done, torch.full_like(tok, pad_id), tok)
        done |= tok == eos_id
        x = p[0][tok]
    return out


def random_params(V, E, H, NL, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / math.sqrt(H)
    ps = [torch.randn(V, E, generator=g)]
    for l in range(NL):
        din = E if l == 0 else H
        ps += [(torch.rand(4 * H, din, generator=g) * 2 - 1) * k * scale, (torch.rand(4 * H, H, generator=g) * 2 - 1) * k * scale,
               (torch.rand(4 * H, generator=g) * 2 - 1) * k, (torch.rand(4 * H, generator=g) * 2 - 1) * k]
    ps += [(torch.rand(V, H, generator=g) * 2 - 1) * k * scale, (torch.rand(V, generator=g) * 2 - 1) * k]
    return [t.float() for t in ps]
