"""CPU oracle (float64 torch) of the ensemble caption decodes (include/gicap.h gic_*_ensemble_*): M members of one decoder kind, each
in its own recurrent state, around one search.  At a step member m gives logits l_m; with lp_m = l_m - logsumexp(l_m) and weights
normalised to sum 1 the search runs on
    prob     z = log sum_m w_m exp(lp_m)
    logprob  z = sum_m w_m lp_m
exactly as the single-model oracles run on one model's logits, and every member advances with the chosen tokens and parents.

Nothing of the searches is restated here: a member is a stepper of tests/diverse_beam_oracle.py (beam_oracle.lstm_cell, or the
attention step of attn_beam_oracle), the ensemble is a stepper that mixes their logits, and the search and the sampling decode are
tests/constrained_oracle.py's own loops (diverse groups, decode constraints and sample_oracle.draw included; every constraint off and
one group is the plain search).  The margins are theirs: per image the selection margin (the smallest gap between the last kept and
the first dropped candidate over the steps) and the order margin (of the final order); per sampled row the smaller of the draw and
nucleus margins."""
from __future__ import annotations

import torch

from tests import attn_beam_oracle as AO
from tests import constrained_oracle as CO
from tests import diverse_beam_oracle as DO

MODES = ("prob", "logprob")


def normalise(weights, M):
    """The weights as the library forms them: the f32 values it reads, normalised in double."""
    w = torch.ones(M, dtype=torch.float64) if weights is None else torch.tensor([float(v) for v in weights], dtype=torch.float32).double()
    if w.numel() != M or not bool((w > 0).all()):
        raise ValueError("one positive weight per member")
    return w / w.sum()


def mix(logits, w, mode):
    """logits f64 [M, rows, V], w f64 [M] summing to 1 -> z [rows, V]."""
    lp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
    if mode == "prob":
        return torch.logsumexp(lp + w.log().view(-1, 1, 1), dim=0)
    if mode == "logprob":
        return (lp * w.view(-1, 1, 1)).sum(0)
    raise ValueError(mode)


class _EnsembleStepper:
    """M steppers behind the interface of one: step() -> (the mixed logits, None), reorder() moves every member alike."""

    def __init__(self, steppers, w, mode):
        self.steppers, self.w, self.mode = steppers, w, mode

    def step(self):
        return mix(torch.stack([s.step()[0] for s in self.steppers]), self.w, self.mode), None

    def reorder(self, par, toks):
        for s in self.steppers:
            s.reorder(par, toks)


def _lstm_steppers(members, features, b, k):
    return [DO._LstmStepper([t.detach().double().cpu() for t in p], f[b].detach().double().cpu(), k) for p, f in zip(members, features)]


def _attn_steppers(members, features, fmaps, b, k):
    return [DO._AttnStepper(AO.as_dict(p), f[b].detach().double().cpu(), fm[b].detach().double().cpu(), k)
            for p, f, fm in zip(members, features, fmaps)]


def _beam(steppers_of, B, M, k, L, weights, mode, groups, diversity, eos_id, pad_id, length_penalty, cons):
    w = normalise(weights, M)
    res = [CO._search_image(_EnsembleStepper(steppers_of(b), w, mode), k, groups, diversity, L, eos_id, pad_id, length_penalty, cons)
           for b in range(B)]
    ids, scores, lengths, _, margins = DO._collect(res, B, k, L)
    return ids, scores, lengths, margins


def beam_search(members, features, k, L, weights=None, mode="prob", groups=1, diversity=0.0, eos_id=2, pad_id=0, length_penalty=0.0,
                no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    """The LSTM decoder: ``members`` a list of M parameter lists (beam_oracle's order), ``features`` a list of M [B, E] tensors.
    Returns (ids int64 [B, k, L], scores f64 [B, k], lengths int64 [B, k], margins: B (selection, order) pairs); with groups > 1 in
    group-major order (diverse_beam_oracle)."""
    B = features[0].shape[0]
    return _beam(lambda b: _lstm_steppers(members, features, b, k), B, len(members), k, L, weights, mode, groups, diversity, eos_id,
                 pad_id, length_penalty, CO._cons(no_repeat_ngram, min_length, suppress_tokens))


def attn_beam_search(members, features, fmaps, k, L, weights=None, mode="prob", groups=1, diversity=0.0, eos_id=2, pad_id=0,
                     length_penalty=0.0, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    """The attention decoder: ``members`` in attn_beam_oracle's parameter order, ``fmaps`` a list of M [B, P, C] tensors."""
    B = features[0].shape[0]
    return _beam(lambda b: _attn_steppers(members, features, fmaps, b, k), B, len(members), k, L, weights, mode, groups, diversity, eos_id,
                 pad_id, length_penalty, CO._cons(no_repeat_ngram, min_length, suppress_tokens))


def _sample(steppers_of, B, M, n, L, noise_u, weights, mode, top_k, top_p, temperature, eos_id, pad_id, cons):
    w = normalise(weights, M)
    u = noise_u.detach().double().cpu()
    out = [CO._sample_image(_EnsembleStepper(steppers_of(b), w, mode), n, L, u[:, b * n:(b + 1) * n], top_k, top_p, temperature, eos_id,
                            pad_id, cons) for b in range(B)]
    return tuple(torch.stack([o[i] for o in out]) for i in range(4))


def sample(members, features, n, L, noise_u, weights=None, mode="prob", top_k=0, top_p=1.0, temperature=1.0, eos_id=2, pad_id=0,
           no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    """The LSTM decoder's sampling decode with explicit noise u [L, B*n, V]: (ids int64 [B, n, L], scores f64 [B, n], lengths int64
    [B, n], margin f64 [B, n]) as sample_oracle.decode."""
    B = features[0].shape[0]
    return _sample(lambda b: _lstm_steppers(members, features, b, n), B, len(members), n, L, noise_u, weights, mode, top_k, top_p,
                   temperature, eos_id, pad_id, CO._cons(no_repeat_ngram, min_length, suppress_tokens))


def attn_sample(members, features, fmaps, n, L, noise_u, weights=None, mode="prob", top_k=0, top_p=1.0, temperature=1.0, eos_id=2,
                pad_id=0, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
    B = features[0].shape[0]
    return _sample(lambda b: _attn_steppers(members, features, fmaps, b, n), B, len(members), n, L, noise_u, weights, mode, top_k, top_p,
                   temperature, eos_id, pad_id, CO._cons(no_repeat_ngram, min_length, suppress_tokens))


def sequence_logprob(members, features, ids, lengths, weights=None, mode="prob", fmaps=None):
    """The ensemble's teacher-forced log-probability of given captions: sum_{t < length} (z - logsumexp(z))[ids[b, t]] with z the mixed
    logits along the caption, f64 [B].  ``fmaps``: the attention decoder's."""
    M, B = len(members), ids.shape[0]
    w = normalise(weights, M)
    out = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        st = _EnsembleStepper(_lstm_steppers(members, features, b, 1) if fmaps is None else _attn_steppers(members, features, fmaps, b, 1),
                              w, mode)
        for t in range(int(lengths[b])):
            z = st.step()[0][0]
            tok = int(ids[b, t])
            out[b] += float(z[tok] - torch.logsumexp(z, 0))
            st.reorder([0], [tok])
    return out
