"""float64 CPU oracle of gic_xent_seq (include/gicap.h): the definition written out with plain torch, from the very values the kernel gets
(a bf16 input is upcast, not regenerated)."""
import torch


def counted_mask(targets, group, lengths=None, ignore_index=-100):
    rows = targets.numel()
    t = targets.reshape(-1).cpu()
    m = t != ignore_index
    if lengths is not None:
        pos = torch.arange(rows) % group
        m &= pos < lengths.reshape(-1).cpu().long().repeat_interleave(group)
    return m


def xent_seq(logits, targets, group, lengths=None, ignore_index=-100, smoothing=0.0, row_weight=None):
    """{"loss", "count", "row_nll" [rows], "cap_nll" [rows / group], "cap_tokens" [rows / group], "d_logits" [rows, V]} in float64 (counts
    int64).  count = 0: loss 0 and a zero gradient.  A counted target outside [0, V): its row_nll, its cap_nll and the loss are NaN."""
    x = logits.detach().cpu().double()
    rows, V = x.shape
    t = targets.reshape(-1).cpu().long()
    w = torch.ones(rows, dtype=torch.float64) if row_weight is None else row_weight.detach().cpu().double().reshape(-1)
    m = counted_mask(t, group, lengths, ignore_index)
    lp = torch.log_softmax(x, 1)
    bad = m & ((t < 0) | (t >= V))
    tc = t.clamp(0, V - 1)
    nll = -lp.gather(1, tc[:, None])[:, 0]
    nll = torch.where(bad, torch.full_like(nll, float("nan")), nll)
    row = (1.0 - smoothing) * nll + smoothing * (-lp.mean(1))
    zero = torch.zeros_like(nll)
    row_nll = torch.where(m, nll, zero)
    cap_nll = row_nll.view(-1, group).sum(1)
    cap_tokens = m.view(-1, group).sum(1)
    count = int(cap_tokens.sum())
    loss = torch.where(m, w * row, zero).sum() / count if count else torch.zeros((), dtype=torch.float64)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), tc] = 1.0
    d = w[:, None] * (lp.exp() - (1.0 - smoothing) * onehot - smoothing / V) / max(count, 1)
    d = torch.where(m[:, None], d, torch.zeros_like(d))
    return {"loss": loss, "count": count, "row_nll": row_nll, "cap_nll": cap_nll, "cap_tokens": cap_tokens, "d_logits": d}
