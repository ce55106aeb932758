"""Host oracle of the caption decoder's output dropout (include/gicap.h gic_decoder_dropout; csrc/gen_dropout.hip): the map from an
element to its draw, built on tests/philox_ref.py, the stage itself, and differentiable float64 restatements of both teacher-forced
decodes with the mask in front of the vocabulary projection.  numpy / CPU torch only.

Philox maps (the list of tests/philox_ref.py, continued).  Element (row r, entry h) of a launch gets (stream, counter, lane):

  decoder output dropout             stream "gdro" << 32, row r = b Tmax + t of hout [B, Tmax, H], flat index i = r H + h,
    csrc/gen_dropout.hip               counter i >> 2, lane i & 3, keep = u >= p (the convention of highway_keep4)      dropout_u
      hidden_dropout_fwd_vec_kernel    H % 4 == 0 (f32) / H % 8 == 0 (bf16), 16-byte aligned bases: a piece of 4 elements is
                                       one counter, lanes = entries 4 q .. 4 q + 3 (bf16: two counters per 16-byte piece)
      hidden_dropout_fwd_kernel        any H, any base: idx = r H + h, gen(idx >> 2)[idx & 3]
      hidden_dropout_bwd_vec_kernel /  the same two forms over d hout f32 [B, Tmax, H]; rows with t >= lengths[b] draw nothing
      hidden_dropout_bwd_kernel
    The all-rows launch (after the loop of gic_*_forward_tf_drop) and the per-step launches (the B rows b Tmax + t of step t, inside
    the loop of gic_*_forward_ss_drop) index alike: the mask depends on (seed, p, i) alone.

The stream tag is far above every roll-out step index and differs from the other tags of tests/philox_ref.py."""
import numpy as np
import torch

from oracle import cpu_attention as CA
from oracle import cpu_step as O
from tests import philox_ref as PR

STREAM_GEN_DROP = 0x6764726F << 32     # "gdro"


# ------------------------------------------------------------------------------------------ the map
def dropout_triples(B, Tmax, H):
    """(stream, counter, lane) of every element of hout [B, Tmax, H]: the map written down (philox_ref.from_triples draws it)."""
    idx = np.arange(B * Tmax * H, dtype=np.uint64).reshape(B, Tmax, H)
    return np.full(idx.shape, STREAM_GEN_DROP, dtype=np.uint64), idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64)


def dropout_u(seed, B, Tmax, H):
    """float32 [B, Tmax, H]: the uniform behind each keep flag, one Philox call per counter (four elements, across row ends)."""
    n = B * Tmax * H
    return PR._lanes(seed, STREAM_GEN_DROP, np.arange((n + 3) // 4, dtype=np.uint64)).reshape(-1)[:n].reshape(B, Tmax, H)


def dropout_keep(seed, B, Tmax, H, p):
    """bool [B, Tmax, H]: keep = u >= p, compared in float32."""
    return dropout_u(seed, B, Tmax, H) >= np.float32(p)


def keep_of(u, p):
    """bool tensor: the keep mask of given uniforms (a float32 tensor or array), compared in float32."""
    u = torch.as_tensor(u, dtype=torch.float32)
    return u >= torch.tensor(p, dtype=torch.float32)


def scale(p):
    """s = 1.0f / (1.0f - p), formed in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ------------------------------------------------------------------------------------------ the stage
def apply(hout, keep, p, dtype=None):
    """hdrop = keep ? hout * s : 0 in ``dtype`` (default hout's): the f32 product, rounded once to bf16 in the bf16 mode."""
    keep = torch.as_tensor(np.asarray(keep)) if not torch.is_tensor(keep) else keep
    dtype = hout.dtype if dtype is None else dtype
    s = float(scale(p))                                            # a float32 value: x.float() * s is the f32 product
    y = (hout.float() * torch.tensor(s, dtype=torch.float32)).to(dtype)
    return torch.where(keep.to(hout.device), y, torch.zeros_like(y))


def apply_bwd(dhout, keep, lengths, p):
    """d hout f32 [B, Tmax, H] after the backward stage: (t < lengths[b] && keep) ? dhout * s : 0."""
    keep = torch.as_tensor(np.asarray(keep)) if not torch.is_tensor(keep) else keep
    B, Tmax, _ = dhout.shape
    live = torch.arange(Tmax)[None, :] < torch.as_tensor(lengths).long()[:, None]
    y = dhout.float() * torch.tensor(float(scale(p)), dtype=torch.float32)
    return torch.where(keep & live[..., None], y, torch.zeros_like(y))


# ------------------------------------------------------------------------------------------ the decodes, float64, differentiable
def _drop64(h, keep, p):
    """The oracle's own stage: exact s in the tensor's dtype (float64)."""
    return torch.where(keep, h / (1.0 - float(np.float32(p))), torch.zeros_like(h))


def lstm_forward_tf(gp, features, caps, lengths, keep, p, temperature=1.0, pretrain=True, u=None, prefix="decoder."):
    """oracle.cpu_step.decoder_forward_tf with keep bool [B, Tmax, H] in front of the projection: (pred, (h_n, c_n))."""
    nl = O.num_lstm_layers(gp, prefix)
    bsz = features.shape[0]
    hid = gp[f"{prefix}lstm.weight_hh_l0"].shape[1]
    emb = gp[f"{prefix}embed.weight"][caps]
    xs = torch.cat((features.unsqueeze(1), emb), 1)
    lens = torch.as_tensor(list(lengths), dtype=torch.long)
    tmax = int(lens.max())
    h = [features.new_zeros(bsz, hid) for _ in range(nl)]
    c = [features.new_zeros(bsz, hid) for _ in range(nl)]
    outs = []
    for t in range(tmax):
        live = (lens > t).unsqueeze(1)
        inp = xs[:, t]
        for l in range(nl):
            hn, cn = O.lstm_cell(inp, h[l], c[l], gp[f"{prefix}lstm.weight_ih_l{l}"], gp[f"{prefix}lstm.weight_hh_l{l}"],
                                 gp[f"{prefix}lstm.bias_ih_l{l}"], gp[f"{prefix}lstm.bias_hh_l{l}"])
            h[l] = torch.where(live, hn, h[l])
            c[l] = torch.where(live, cn, c[l])
            inp = h[l]
        outs.append(torch.where(live, inp, torch.zeros_like(inp)))
    output = _drop64(torch.stack(outs, 1), keep, p)                # the recurrence above kept the undropped h
    o = output @ gp[f"{prefix}linear.weight"].t() + gp[f"{prefix}linear.bias"]
    pred = o if pretrain else torch.softmax((o + O.gumbel_from_uniform(u)) * temperature, dim=-1)
    return pred, (torch.stack(h, 0), torch.stack(c, 0))


def attn_forward_tf(gp, features, fmap, caps, lengths, keep, p, temperature=1.0, pretrain=True, u=None, prefix="decoder."):
    """tests/attn_tf_oracle.forward_tf with keep bool [B, Tmax, H] in front of the projection: (pred, (h_n, c_n), alphas)."""
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
        live = (t < lens).unsqueeze(1)
        h = torch.where(live, h_new, h)
        c = torch.where(live, c_new, c)
        hs.append(h_new * live.to(h_new.dtype))
        alphas.append(alpha * live.to(alpha.dtype))
    o = _drop64(torch.stack(hs, 1), keep, p) @ gp[f"{prefix}linear.weight"].t() + gp[f"{prefix}linear.bias"]
    pred = o if pretrain else torch.softmax((o + O.gumbel_from_uniform(u)) * temperature, dim=-1)
    return pred, (h, c), torch.stack(alphas, 1)
