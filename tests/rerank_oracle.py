"""D-guided re-ranking (gic_rerank, discriminator.rerank) on the CPU in fp64: there is no reference counterpart, the oracle is this
build's own definition.  Nothing here touches the GPU.

  d[b, k]     = (1/R) sum_r d_logits[(b K + k) R + r]
  final[b, k] = lm[b, k] / max(len[b, k], 1) ** length_penalty + weight d[b, k]          (weight == 0: the first term alone)
  order[b, :] = the input indices by final descending, ties to the lower input index, a NaN final last

The bounds are those the issue sets, with eps = 2^-24 the f32 unit round-off: |d - d'| <= (R + 2) eps mean_r |logit| (R - 1 additions and
one division), |final - final'| <= (R + 6) eps (|lm term| + |weight| mean_r |logit|) (the power, the division, the product and the sum on
top).  An image is `clear` when every gap between distinct oracle finals is at least four bounds: then no rounding of that size can
swap two beams, and the order is the oracle's; otherwise only the multiset of (input index, final) is compared."""
import math

import torch

from tests import disc_cond_oracle as DC                                  # the match term the scored logits come from

EPS = 2.0 ** -24


def d_scores(d_logits, B, K, R):
    """fp64 [B, K] and the magnitude mean_r |logit| the bounds scale with."""
    g = d_logits.double().view(B, K, R)
    return g.sum(-1) / R, g.abs().sum(-1) / R


def lm_terms(lm, lengths, length_penalty):
    return lm.double() / lengths.double().clamp(min=1.0) ** float(length_penalty)


def finals(lm, lengths, length_penalty, d_logits, R, weight):
    """(final, d, bound of final, bound of d), each fp64 [B, K]."""
    B, K = lm.shape
    d, mag = d_scores(d_logits, B, K, R)
    term = lm_terms(lm, lengths, length_penalty)
    final = term.clone() if weight == 0 else term + float(weight) * d
    share = torch.zeros_like(mag) if weight == 0 else abs(float(weight)) * mag          # weight 0: D has no share (a NaN logit included)
    return final, d, (R + 6) * EPS * (term.abs() + share), (R + 2) * EPS * mag


def order_of(final_row):
    """Input indices by final descending, stable (ties to the lower index), NaN last."""
    vals = [float(v) for v in final_row]
    return sorted(range(len(vals)), key=lambda k: (1, 0.0, k) if math.isnan(vals[k]) else (0, -vals[k], k))


def rerank(lm, lengths, length_penalty, d_logits, R, weight):
    """{"order" int64 [B, K], "final", "d" (fp64, in the new order), "bound", "d_bound" (in INPUT order), "final_in", "d_in"}."""
    final, d, bound, d_bound = finals(lm, lengths, length_penalty, d_logits, R, weight)
    order = torch.tensor([order_of(row) for row in final], dtype=torch.int64).view(final.shape)
    return {"order": order, "final": final.gather(1, order), "d": d.gather(1, order), "bound": bound, "d_bound": d_bound,
            "final_in": final, "d_in": d}


def clear(final_row, bound_row):
    """Every gap between distinct (non-NaN) oracle finals of the image is at least 4 bounds (the larger of the two neighbours')."""
    pairs = sorted((float(f), float(b)) for f, b in zip(final_row, bound_row) if not math.isnan(float(f)))
    for (f0, b0), (f1, b1) in zip(pairs, pairs[1:]):
        if f1 != f0 and not (f1 - f0 >= 4.0 * max(b0, b1)):
            return False
    return True


def clear_images(ref):
    return [clear(f, b) for f, b in zip(ref["final_in"], ref["bound"])]


def check(ref, order, final, d):
    """The GPU's (order int [B, K], final / d f32 [B, K] in the new order) against ``ref``.  Returns (number of images that are not clear,
    largest err / bound seen over final and d).  Raises AssertionError on a miss."""
    B, K = ref["order"].shape
    order = order.long().cpu()
    final, d = final.double().cpu(), d.double().cpu()
    unclear, worst = 0, 0.0
    for b in range(B):
        got = order[b].tolist()
        assert sorted(got) == list(range(K)), f"image {b}: order {got} is no permutation"
        fin_ref, d_ref = ref["final_in"][b][order[b]], ref["d_in"][b][order[b]]
        bnd, dbnd = ref["bound"][b][order[b]], ref["d_bound"][b][order[b]]
        for name, g, r, bd in (("final", final[b], fin_ref, bnd), ("d", d[b], d_ref, dbnd)):
            nan = torch.isnan(r)
            assert torch.equal(torch.isnan(g), nan), f"image {b}: NaN pattern of {name} differs"
            err = (g - r).abs()[~nan]
            lim = bd[~nan]
            assert bool((err <= lim).all()), f"image {b}: {name} err {err.tolist()} above bound {lim.tolist()}"
            if err.numel():
                worst = max(worst, float((err / lim.clamp(min=1e-300)).max()))
        if clear(ref["final_in"][b], ref["bound"][b]):
            assert got == ref["order"][b].tolist(), f"image {b} is clear: order {got}, oracle {ref['order'][b].tolist()}"
        else:
            unclear += 1
            # not clear: the order still has to be one that the GPU's own finals justify (descending, ties by index, NaN last)
            assert got == [got[i] for i in order_of_pairs(final[b].tolist(), got)], f"image {b}: order {got} contradicts its own finals"
    return unclear, worst


def order_of_pairs(vals, idx):
    """Positions 0..K-1 sorted by (value descending, input index ascending, NaN last): the identity for a consistent result."""
    return sorted(range(len(vals)), key=lambda p: (1, 0.0, idx[p]) if math.isnan(vals[p]) else (0, -vals[p], idx[p]))


def match_term_indexed(y, q, q_index, R):
    """The grouped match term s <y[b R + r, :], q[q_index[b], :]> for y [B*R, F], q [q_rows, F] (disc_cond_oracle.match_term on the
    gathered rows)."""
    return DC.match_term(y, q[q_index.long()], R)


# ------------------------------------------------------------------------------------------------ the synthetic cases of the GPU test
SYN_B, SYN_L = 3, 7
SYN_K, SYN_R, SYN_P = (1, 2, 5, 8, 64), (1, 4), (0, 4)
SYN_LP, SYN_W = (0.0, 0.7), (0.0, 0.5, -1.0)
SYN_SEED = 1908           # chosen so that every image of every case is clear in the oracle alone (tests/test_rerank_api.py checks it)


def synthetic(K, R, P, seed=SYN_SEED):
    """Inputs of gic_rerank as a search leaves them: lm descending per image (so that weight 0 with no length penalty must give the
    identity), lengths in 1..L, Gaussian logits, random ids / alphas.  f32 / int tensors on the CPU."""
    g = torch.Generator().manual_seed(seed + 1000 * K + 10 * R + P)
    B, L = SYN_B, SYN_L
    lm = -(10.0 * torch.rand(B, K, generator=g)).sort(1).values
    lengths = torch.randint(1, L + 1, (B, K), generator=g, dtype=torch.int32)
    d_logits = torch.randn(B * K * R, generator=g)
    ids = torch.randint(0, 50, (B, K, L), generator=g)
    alphas = torch.rand(B, K, L, P, generator=g) if P else None
    return lm, lengths, d_logits, ids, alphas


def synthetic_cases():
    for K in SYN_K:
        for R in SYN_R:
            for P in SYN_P:
                yield K, R, P
