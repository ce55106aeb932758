"""Image-caption retrieval with the conditioned discriminator (gic_disc_rep_mean, gic_match_ranks, GANInstructor.evaluate_retrieval) on
the CPU: there is no reference counterpart, the oracle is this build's own definition.  Nothing here touches
the GPU.

  ybar[c, :] = (1/R) sum_r y[c R + r, :F]      lbar[c] = (1/R) sum_r logits[c R + r]       (y = the dropped highway output, eval mode)
  T[c, j]    = lbar[c] + s <ybar[c], q[j]>      s = F^-1/2 (disc_cond_oracle.scale): the mean over r of D's logit for (caption c, image j)
  rank_c2i[c] = #{j != c : not T[c, j] < T[c, c]}      rank_i2c[j] = #{c != j : not T[c, j] < T[j, j]}       (a tie or a NaN counts against)

`ranks_exact` is the integer oracle of gic_match_ranks: the same f32 inputs, one f32 addition and comparisons, so there is no tolerance.
`rank_intervals` is the end-to-end oracle: T in fp64 and, per item, the interval [lo, hi] of ranks that an error of at most `bound` per
score allows.  Bounds with eps = 2^-24: ybar (R + 2) eps mean_r |y| (a bf16 input is exact in f32), lbar likewise; the f32 GEMM
2 F eps s sum_n |ybar||q|; the addition of the bias one more rounding of the result."""
import torch

from tests import disc_cond_oracle as DC

EPS = 2.0 ** -24


def rep_mean(y, logits, R, F):
    """(ybar, lbar, bound of ybar, bound of lbar) in fp64 for y [C*R, >= F] (f32 or bf16) and logits [C*R] (or None)."""
    yd = y[:, :F].double().view(-1, R, F)
    ybar, ymag = yd.sum(1) / R, yd.abs().sum(1) / R
    if logits is None:
        return ybar, None, (R + 2) * EPS * ymag, None
    ld = logits.double().view(-1, R)
    return ybar, ld.sum(1) / R, (R + 2) * EPS * ymag, (R + 2) * EPS * ld.abs().sum(1) / R


def pair_scores(ybar, lbar, q, ybar_bound=None, lbar_bound=None):
    """(T fp64 [N, N], bound [N, N]) of T[c, j] = lbar[c] + s <ybar[c], q[j]> as evaluate_retrieval forms it in f32."""
    F = q.shape[1]
    s = DC.scale(F)
    qd = q.double()
    # element by element (no BLAS blocking): two images with the same q row get the same bits in their columns
    S = s * (ybar[:, None, :] * qd[None, :, :]).sum(-1)
    mag = s * (ybar.abs()[:, None, :] * qd.abs()[None, :, :]).sum(-1)
    T = S + lbar[:, None]
    bound = 2 * F * EPS * mag + EPS * (S.abs() + lbar.abs()[:, None])
    if ybar_bound is not None:
        bound = bound + s * ybar_bound @ qd.abs().t()
    if lbar_bound is not None:
        bound = bound + lbar_bound[:, None]
    return T, bound


def ranks_exact(S, row_bias=None):
    """(rank_c2i, rank_i2c) int64 [N] of a given f32 S [N, N]: T = S + row_bias[c] in f32, then comparisons only."""
    S = S.float()
    N = S.shape[0]
    T = S if row_bias is None else S + row_bias.float()[:, None]
    diag = T.diagonal()
    off = ~torch.eye(N, dtype=torch.bool)
    c2i = (~(T < diag[:, None]) & off).sum(1)
    i2c = (~(T < diag[None, :]) & off).sum(0)
    return c2i, i2c


def rank_intervals(T, bound):
    """{"c2i": (lo, hi), "i2c": (lo, hi)}: lo counts the competitors that beat the true pair by more than the two scores' bounds, hi also
    those within them (and every NaN)."""
    N = T.shape[0]
    diag, dbound = T.diagonal(), bound.diagonal()
    off = ~torch.eye(N, dtype=torch.bool)
    out = {}
    for name, dg, db, dim in (("c2i", diag[:, None], dbound[:, None], 1), ("i2c", diag[None, :], dbound[None, :], 0)):
        diff, tol = T - dg, bound + db
        nan = torch.isnan(diff)
        lo = (((diff > tol) | nan) & off).sum(dim)
        hi = ((~(diff < -tol) | nan) & off).sum(dim)
        out[name] = (lo, hi)
    return out


def recall_at(ranks, k):
    """The share of 0-based ranks below k."""
    r = [int(v) for v in ranks]
    return sum(v < k for v in r) / len(r)


def median_rank(ranks):
    """1-based median: the mean of the two middle ranks of an even count."""
    r = sorted(int(v) for v in ranks)
    n = len(r)
    return 1.0 + (r[n // 2] if n % 2 else 0.5 * (r[n // 2 - 1] + r[n // 2]))


def summary(ranks):
    r = [int(v) for v in ranks]
    return {"r1": recall_at(r, 1), "r5": recall_at(r, 5), "r10": recall_at(r, 10), "medr": median_rank(r), "meanr": 1.0 + sum(r) / len(r)}
