"""CPU beam-search oracle (float64 torch) for the attention decoder: the semantics of gic_decoder_beam_search (tests/beam_oracle.py)
with the step of oracle/cpu_attention.attn_decoder_sample(pretrain=True), restated for gic_attn_beam_search (include/gicap.h).

Parameters come in the library's order (engine.AttnDecoderEngine.NAMES): [embed, w_ih, w_hh, b_ih, b_hh, w_out, b_out, w_f, b_f, w_h,
w_a].  Margins as in tests/beam_oracle.py: per image the smallest gap between the k-th and the (k+1)-th candidate over every step
(selection) and between consecutive normalised final scores (order)."""
from __future__ import annotations

import math

import torch

from oracle import cpu_attention as CA
from oracle import cpu_step as O

NAMES = ("embed.weight", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "linear.weight", "linear.bias",
         "attn.w_f", "attn.b_f", "attn.w_h", "attn.w_a")


def as_dict(params, prefix="decoder."):
    """The library-ordered parameter list as oracle.cpu_attention's float64 dict."""
    return {prefix + n: t.detach().double().cpu() for n, t in zip(NAMES, params)}


def step(gp, x, z_in, h, c):
    """One LSTM cell + output layer: (h, c, logits) for the rows of x [n, E], z [n, C]."""
    h, c = O.lstm_cell(torch.cat([x, z_in], 1), h, c, gp["decoder.lstm.weight_ih_l0"], gp["decoder.lstm.weight_hh_l0"],
                       gp["decoder.lstm.bias_ih_l0"], gp["decoder.lstm.bias_hh_l0"])
    return h, c, h @ gp["decoder.linear.weight"].t() + gp["decoder.linear.bias"]


def beam_search(params, features, fmap, k, L, eos_id=2, pad_id=0, length_penalty=0.0, states=None, trace=None):
    """Returns (ids int64 [B, k, L], scores f64 [B, k], lengths int64 [B, k], alphas f64 [B, k, L, P], margins: list of B
    (selection, order) pairs).  ``states`` = (h0, c0), each [1, B, H] or [B, H].  ``trace`` as in tests/beam_oracle.py."""
    gp = as_dict(params)
    feats = features.detach().double().cpu()
    fm = fmap.detach().double().cpu()
    B, P = feats.shape[0], fm.shape[1]
    H = gp["decoder.lstm.weight_hh_l0"].shape[1]
    embed = gp["decoder.embed.weight"]
    ids = torch.full((B, k, L), pad_id, dtype=torch.int64)
    scores = torch.zeros(B, k, dtype=torch.float64)
    lengths = torch.zeros(B, k, dtype=torch.int64)
    alphas = torch.zeros(B, k, L, P, dtype=torch.float64)
    margins = []
    for b in range(B):
        margin = order_margin = math.inf
        fmb = fm[b:b + 1].expand(k, -1, -1)
        fpb = fm[b] @ gp["decoder.attn.w_f"].t() + gp["decoder.attn.b_f"]
        fpb = fpb.unsqueeze(0).expand(k, -1, -1)
        h = (states[0].reshape(B, H)[b].double() if states is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1)
        c = (states[1].reshape(B, H)[b].double() if states is not None else torch.zeros(H, dtype=torch.float64)).repeat(k, 1)
        score = [0.0] + [-math.inf] * (k - 1)
        fin = [False] * k
        ln = [0] * k
        seqs = [[] for _ in range(k)]
        alph = [[] for _ in range(k)]
        x = feats[b].repeat(k, 1)
        zero = torch.zeros(P, dtype=torch.float64)
        pars = []
        for t in range(L):
            if all(fin):
                for j in range(k):
                    seqs[j].append(pad_id)
                    alph[j].append(zero)
                continue
            z, alpha = CA.attention(gp, fmb, fpb, h)
            h, c, logits = step(gp, x, z, h, c)
            logp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
            cands = []
            for j in range(k):
                if fin[j]:
                    cands.append((score[j], j, 0, pad_id))
                    continue
                order = torch.sort(-logits[j], stable=True).indices[:k].tolist()
                for q, tok in enumerate(order):
                    cands.append((score[j] + float(logp[j, tok]), j, q, tok))
            cands.sort(key=lambda e: (-e[0], e[1], e[2]))
            sel = cands[:k]
            if len(cands) > k and cands[k][0] != -math.inf:
                margin = min(margin, cands[k - 1][0] - cands[k][0])
            par = [e[1] for e in sel]
            pars.append(par)
            h, c = h[par], c[par]
            new_fin, new_len, new_seqs, new_alph = [], [], [], []
            for (s, j, q, tok) in sel:
                new_fin.append(fin[j] or tok == eos_id)
                new_len.append(ln[j] if fin[j] else t + 1)
                new_seqs.append(seqs[j] + [tok])
                new_alph.append(alph[j] + [zero if fin[j] else alpha[j]])
            score = [e[0] for e in sel]
            fin, ln, seqs, alph = new_fin, new_len, new_seqs, new_alph
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
            alphas[b, r] = torch.stack(alph[j])
    return ids, scores, lengths, alphas, margins


def sequence_logprob(params, features, fmap, ids, lengths):
    """Teacher-forced log-probability of each caption ids [B, n, L] up to its length [B, n] (float64 [B, n])."""
    gp = as_dict(params)
    B, n, L = ids.shape
    feats = features.detach().double().cpu().repeat_interleave(n, 0)
    fm = fmap.detach().double().cpu().repeat_interleave(n, 0)
    logits, _, _ = CA.attn_decoder_sample(gp, feats, fm, L, 1.0, pretrain=True, force_ids=ids.reshape(B * n, L).cpu())
    logp = torch.log_softmax(logits, dim=-1).gather(2, ids.reshape(B * n, L, 1).cpu())[..., 0]
    keep = torch.arange(L)[None] < lengths.reshape(B * n, 1).cpu()
    return torch.where(keep, logp, torch.zeros_like(logp)).sum(1).reshape(B, n)


def random_problem(B, V, E, H, C, P, A, seed=0, scale=6.0):
    """(params in library order, features [B, E], fmap [B, P, C]) as float32 CPU tensors (tests/test_gpu_attention.py's problem)."""
    g = torch.Generator().manual_seed(seed)
    gp = CA.make_attn_params(V, E, H, C, A, g)
    params = [gp["decoder." + n] * scale for n in NAMES]
    feats = torch.randn(B, E, generator=g) * 0.5
    fmap = torch.relu(torch.randn(B, P, C, generator=g))
    return [t.float().contiguous() for t in params], feats.float(), fmap.float()
