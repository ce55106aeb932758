"""CPU oracle (float64 torch) of scheduled sampling inside the teacher-forced decodes, gic_decoder_forward_ss / gic_attn_forward_ss
(include/gicap.h): the step loop of the definition on top of oracle.cpu_step.decoder_forward_tf and tests/attn_tf_oracle.forward_tf.
The logits of step t-1 are those of the teacher-forced decode of the inputs realised so far with every length cut to t (a prefix
decode: the packed semantics make a cut row's last output its step t-1), so neither decode is copied here.

Differentiable plain torch: the returned pred / alphas are functions of the parameters with ``inputs`` detached, so autograd of this
file is the gradient oracle of gic_*_forward_tf_bwd run over ``inputs``."""
from __future__ import annotations

import torch

from oracle import cpu_step as O
from tests import attn_tf_oracle as TF


def decode(gp, features, fmap, caps, lengths):
    """(pred, (h_n, c_n), alphas or None): the teacher-forced pretrain decode of ``caps``, LSTM (fmap None) or attention."""
    lens = [int(v) for v in lengths]
    if fmap is None:
        pred, hc = O.decoder_forward_tf(gp, features, caps, lens, 1.0, pretrain=True)
        return pred, hc, None
    pred, hc, alphas = TF.forward_tf(gp, features, fmap, caps, lens, pretrain=True)
    return pred, hc, alphas


def scheduled(gp, features, fmap, caps, lengths, p, pick, coin, u, inputs=None):
    """The definition of gic_decoder_forward_ss (``fmap`` None) / gic_attn_forward_ss.  ``caps`` int64 [B, T-1], ``lengths`` B values in
    1..T, ``coin`` f32 [B, T-1], ``u`` f32 [T-1, B, V] (unread for pick = "argmax").  With ``inputs`` (a run's own, int64 [B, T-1]) the
    decode follows those instead of its own choices, which factors the discrete picks out; ``picks`` is then what this oracle would
    have picked from that same prefix.  Returns a dict: inputs, replaced (bool), picks (int64 [B, T-1], -1 where nothing was
    maximised), min_gap (the smallest top-2 gap of the maximised quantity over the replaced positions; inf without one), pred
    [B, Tmax, V], h_n, c_n, alphas ([B, Tmax, P] or None)."""
    assert pick in ("sample", "argmax")
    B, Lc = caps.shape
    V = gp["decoder.linear.bias"].shape[0]
    lens = torch.as_tensor([int(v) for v in lengths], dtype=torch.long)
    Tmax = int(lens.max())
    p32 = torch.tensor(float(p), dtype=torch.float32)
    follow = inputs is not None
    inp = caps.clone()
    inp[:, :Tmax - 1] = caps[:, :Tmax - 1].clamp(0, V - 1)        # positions >= Tmax - 1 stay copies of caps
    replaced = torch.zeros(B, Lc, dtype=torch.bool)
    picks = torch.full((B, Lc), -1, dtype=torch.long)
    min_gap = float("inf")
    with torch.no_grad():
        for t in range(1, Tmax):
            rep = (coin[:, t - 1].to(torch.float32) < p32) & (t < lens)
            if bool(rep.any()):
                pred, _, _ = decode(gp, features, fmap, inp.clamp(0, V - 1), lens.clamp(max=t).tolist())
                y = pred[:, t - 1]                                 # the logits of step t-1 (rows with lengths >= t)
                if pick == "sample":
                    y = y + O.gumbel_from_uniform(u[t - 1].to(y.dtype))
                top = y.topk(2, dim=1).values
                m = y.max(1)[1]                                    # first maximal index
                picks[rep, t - 1] = m[rep]
                min_gap = min(min_gap, float((top[:, 0] - top[:, 1])[rep].min()))
                inp[rep, t - 1] = m[rep]
            replaced[:, t - 1] = rep
            if follow:
                inp[:, t - 1] = inputs[:, t - 1]
    pred, (h_n, c_n), alphas = decode(gp, features, fmap, inp.clamp(0, V - 1), lens.tolist())
    return {"inputs": inp, "replaced": replaced, "picks": picks, "min_gap": min_gap, "pred": pred, "h_n": h_n, "c_n": c_n,
            "alphas": alphas}
