"""Plain-torch definition of the SeqGAN step with the attention decoder (--adv-mode seqgan --decoder attention): oracle/cpu_seqgan.py's
step, called as it is, with oracle/cpu_attention.py's decoder as the sampler.  Test infrastructure, no reference counterpart; nothing here is used by
the package."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from oracle import cpu_attention as A
from oracle import cpu_seqgan as S
from oracle import cpu_step as O

Tensor = torch.Tensor


def attn_rollouts(gp: O.Params, feats: Tensor, fmap: Tensor, Y: Tensor, N: int, u_mc: Tensor) -> Tuple[Tensor, float]:
    """Monte-Carlo roll-outs of the captions Y [B, L]: cpu_attention.attn_decoder_sample's loop at temperature 1 over (L-1)*N*B rows,
    row (t-1)*N*B + n*B + b = roll-out n of caption b, forced along Y[b, :t] and sampled (Gumbel-max on u_mc [L, rows, V]) from step t
    on.  Returns (ids [rows, L], the smallest gap between the best and the second-best perturbed logit over all sampled row-steps)."""
    B, L = Y.shape
    reps = (L - 1) * N
    p = "decoder."
    f_big, m_big, y_big = feats.repeat(reps, 1), fmap.repeat(reps, 1, 1), Y.repeat(reps, 1)
    flen = torch.arange(1, L).repeat_interleave(N * B)
    rows = reps * B
    hid = gp[p + "lstm.weight_hh_l0"].shape[1]
    fproj = m_big @ gp[p + "attn.w_f"].t() + gp[p + "attn.b_f"]
    h, c, x = f_big.new_zeros(rows, hid), f_big.new_zeros(rows, hid), f_big
    ids = []
    gap = float("inf")
    for t in range(L):
        z, _ = A.attention(gp, m_big, fproj, h, p)
        h, c = O.lstm_cell(torch.cat([x, z], 1), h, c, gp[p + "lstm.weight_ih_l0"], gp[p + "lstm.weight_hh_l0"],
                           gp[p + "lstm.bias_ih_l0"], gp[p + "lstm.bias_hh_l0"])
        y = h @ gp[p + "linear.weight"].t() + gp[p + "linear.bias"] + O.gumbel_from_uniform(u_mc[t])
        forced = t < flen
        idx = torch.where(forced, y_big[:, t], y.argmax(1))
        if not bool(forced.all()):
            top = y[~forced].topk(2, dim=1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
        ids.append(idx)
        x = gp[p + "embed.weight"][idx]
    return torch.stack(ids, 1), gap


class _AttnStep:
    """oracle/cpu_step.py as oracle/cpu_seqgan.py sees it, with the attention decoder as its sampler: decoder_sample(gp, features, L,
    T, us, pretrain, force_ids, force_len) attends over ``fmap`` (repeated for the roll-out batch); everything else is cpu_step's."""

    def __init__(self, fmap: Tensor):
        self.fmap, self.gap = fmap, float("inf")

    def __getattr__(self, name):
        return getattr(O, name)

    def decoder_sample(self, gp, features, max_caption_len, temperature, us=None, pretrain=False, force_ids=None, force_len=None):
        B = self.fmap.shape[0]
        if force_len is None:
            out, ids, _ = A.attn_decoder_sample(gp, features, self.fmap, max_caption_len, temperature, us, pretrain=pretrain, force_ids=force_ids)
            return out, ids
        # the roll-out batch: features and force_ids are B-row blocks repeated (L-1)*N times, force_len = the prefix lengths
        N = features.shape[0] // (B * (max_caption_len - 1))
        ids, self.gap = attn_rollouts(gp, features[:B], self.fmap, force_ids[:B], N, torch.stack(list(us)))
        return None, ids


def attn_seqgan_step(gp: O.Params, dp: O.Params, captions: Tensor, u_sample: Sequence[Tensor], u_mc: Tensor, n_rollouts: int,
                     masks: Optional[Sequence[Tensor]], trunk_feat: Tensor, fmap: Tensor, clip_norm: float = 5.0,
                     gen_opt: Optional[O.AdamState] = None, disc_opt: Optional[O.AdamState] = None, num_rep: int = 64,
                     force_Y: Optional[Tensor] = None) -> Dict[str, object]:
    """cpu_seqgan.seqgan_step itself -- its rewards, losses, gradients and optimizer steps -- with the attention sampler in the place of
    cpu_step.decoder_sample: features = encoder head(trunk_feat), the decoder attends over ``fmap`` [B, P, C].  Arguments and the
    returned dict as there, plus "mc_gap" (attn_rollouts' smallest top-2 gap)."""
    step = _AttnStep(fmap)
    saved, S.O = S.O, step
    try:
        out = S.seqgan_step(gp, dp, captions, u_sample, u_mc, n_rollouts, masks, clip_norm, gen_opt, disc_opt, trunk_feat, num_rep, force_Y)
    finally:
        S.O = saved
    out["mc_gap"] = step.gap
    return out
