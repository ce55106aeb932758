"""CPU oracle (float64 torch) of the attention decoder's teacher-forced decode, gic_attn_forward_tf (include/gicap.h): the packed-sequence
semantics of Decoder.forward with the step of oracle/cpu_attention.attn_decoder_sample.  Differentiable plain torch: autograd of this
file is the gradient oracle of gic_attn_forward_tf_bwd.

Parameters come as oracle.cpu_attention's dict (tests/attn_beam_oracle.as_dict turns the library-ordered list into one)."""
from __future__ import annotations

import torch

from oracle import cpu_attention as CA
from oracle import cpu_step as O


def forward_tf(gp, features, fmap, caps, lengths, temperature=1.0, pretrain=False, u=None, prefix="decoder."):
    """Returns (pred [B, Tmax, V], (h_n, c_n) [B, H], alphas [B, Tmax, P]) with Tmax = max(lengths).  Step 0 is fed ``features``,
    step t > 0 embed(caps[:, t-1]); a row with t >= lengths[b] keeps (h, c), outputs a zero h (its pred row is b_out, or the
    Gumbel-softmax of b_out) and a zero alpha row.  ``u`` [B, Tmax, V]: the uniforms of the Gumbel noise (pretrain=False)."""
    lens = torch.as_tensor(lengths).long().cpu()
    B = features.shape[0]
    Tmax = int(lens.max())
    hid = gp[f"{prefix}lstm.weight_hh_l0"].shape[1]
    fproj = fmap @ gp[f"{prefix}attn.w_f"].t() + gp[f"{prefix}attn.b_f"]
    h = features.new_zeros(B, hid)
    c = features.new_zeros(B, hid)
    hs, alphas = [], []
    for t in range(Tmax):
        x = features if t == 0 else gp[f"{prefix}embed.weight"][caps[:, t - 1]]
        z, alpha = CA.attention(gp, fmap, fproj, h, prefix)
        h_new, c_new = O.lstm_cell(torch.cat([x, z], 1), h, c, gp[f"{prefix}lstm.weight_ih_l0"], gp[f"{prefix}lstm.weight_hh_l0"],
                                   gp[f"{prefix}lstm.bias_ih_l0"], gp[f"{prefix}lstm.bias_hh_l0"])
        live = (t < lens).to(features.device).unsqueeze(1)
        h = torch.where(live, h_new, h)
        c = torch.where(live, c_new, c)
        hs.append(h_new * live.to(h_new.dtype))
        alphas.append(alpha * live.to(alpha.dtype))
    o = torch.stack(hs, 1) @ gp[f"{prefix}linear.weight"].t() + gp[f"{prefix}linear.bias"]
    pred = o if pretrain else torch.softmax((o + O.gumbel_from_uniform(u)) * temperature, dim=-1)
    return pred, (h, c), torch.stack(alphas, 1)


def attn_reg(alphas, lam):
    """The doubly stochastic attention penalty lam * mean_b sum_i (1 - sum_t alpha_bti)^2 (Xu et al., 2015, eq. 14)."""
    return lam * ((1.0 - alphas.sum(1)) ** 2).sum(1).mean()
