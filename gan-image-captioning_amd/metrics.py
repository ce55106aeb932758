"""The n-gram overlap metrics of a captioning results table -- BLEU-1..4 (Papineni et al. 2002) and ROUGE-L (Lin 2004, the coco-caption
``Rouge`` with beta = 1.2) -- on token ids, scored on the GPU by ``gic_caption_overlap`` (csrc/overlap.hip), and mixed SCST rewards
(Rennie et al. 2017: CIDEr-D + BLEU-4 + ROUGE-L).  No reference counterpart.  Definitions: gicap.h and DESIGN.md section 16.

The kernel gives, per candidate, the ten integers of corpus BLEU (``STAT_COLUMNS``), ROUGE-L and an add-one smoothed sentence BLEU-4;
``OverlapScorer.score`` leaves them on the device without a host sync.  Corpus BLEU is a function of the summed integers alone
(``corpus_bleu``, float64 on the host): BLEU-n equals ``utils.bleu_score`` with ``max_n = n`` and uniform weights.  Captions use the
references (``cider.RefBatch``) and the stripping rule (<PAD>, <S>, <E> dropped) of CIDEr-D; METEOR and SPICE are out of scope."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from . import _lib, engine
from .cider import RefBatch, flat_candidates

STAT_COLUMNS = ("clipped1", "clipped2", "clipped3", "clipped4", "total1", "total2", "total3", "total4", "cand_len", "ref_len")
assert len(STAT_COLUMNS) == _lib.OVERLAP_STATS


class OverlapScorer:
    """BLEU statistics, ROUGE-L and smoothed sentence BLEU-4 of candidates against a RefBatch; needs no corpus table.  ``vocab_size``
    above 32768 is refused (15-bit n-gram windows, as CIDEr-D)."""

    def __init__(self, vocab_size: int, device=None):
        if int(vocab_size) > _lib.CIDER_MAX_VOCAB:
            raise ValueError(f"n-gram windows hold 15-bit token ids: vocabulary size {vocab_size} > {_lib.CIDER_MAX_VOCAB} is not supported")
        self.V = int(vocab_size)
        self.device = device

    def score(self, cand_ids: torch.Tensor, cand_lengths: torch.Tensor, refs: RefBatch,
              cand_img: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Candidates int64 [B, n, L] (n per image, image-major) or [rows, L] with ``cand_img`` int [rows] (None with rows = B: one per
        image) against ``refs`` (a RefBatch on the device, B images); ``cand_lengths`` as in ``CiderD.score``.  Returns device tensors
        (stats int32 [*cand_lengths.shape, 10] in the order of ``STAT_COLUMNS``, rouge_l f32, sbleu f32, both of ``cand_lengths``'s
        shape); no host sync."""
        flat, img = flat_candidates(cand_ids, refs, cand_img)
        if flat.shape[1] > _lib.CIDER_MAX_LEN:
            raise ValueError(f"candidates of {flat.shape[1]} ids: the overlap metrics score at most {_lib.CIDER_MAX_LEN}")
        stats, rouge, sbleu = engine.caption_overlap(flat, cand_lengths.reshape(-1), img, refs.ids, refs.lengths, refs.offsets,
                                                     refs.max_refs, self.V)
        shape = tuple(cand_lengths.shape)
        return stats.view(*shape, _lib.OVERLAP_STATS), rouge.view(shape), sbleu.view(shape)


def corpus_bleu(stats_sum) -> List[float]:
    """[BLEU-1, BLEU-2, BLEU-3, BLEU-4] of a corpus from its ten summed stats (``STAT_COLUMNS``; a tensor, array or sequence): BLEU-n =
    BP * exp(mean_{k <= n} log(clipped_k / total_k)), BP = exp(min(1 - ref_len / cand_len, 0)), and 0.0 from the first order without a
    clipped match on -- ``utils.bleu_score(max_n=n, weights=(1/n,)*n)`` over the same integers, in float64 on the host."""
    s = [int(v) for v in (stats_sum.tolist() if hasattr(stats_sum, "tolist") else stats_sum)]
    if len(s) != _lib.OVERLAP_STATS:
        raise ValueError(f"corpus_bleu takes the {_lib.OVERLAP_STATS} summed stats, got {len(s)}")
    clipped, total, c_len, r_len = s[0:4], s[4:8], s[8], s[9]
    out = []
    for n in range(1, 5):
        if min(clipped[:n]) == 0:
            out.append(0.0)
            continue
        log_p = sum((1.0 / n) * math.log(clipped[i] / total[i]) for i in range(n))
        out.append(math.exp(min(1.0 - r_len / c_len, 0.0)) * math.exp(log_p))
    return out


def retrieval_summary(ranks) -> dict:
    """{"r1", "r5", "r10", "medr", "meanr"} of 0-based retrieval ranks (GANInstructor.evaluate_retrieval): R@K = the share of items whose
    true pair is among the K best (rank < K), the median (the mean of the two middle ranks of an even count) and mean rank 1-based."""
    r = sorted(int(v) for v in (ranks.tolist() if hasattr(ranks, "tolist") else ranks))
    n = len(r)
    if n == 0:
        return {"r1": 0.0, "r5": 0.0, "r10": 0.0, "medr": 0.0, "meanr": 0.0}
    out = {f"r{k}": sum(v < k for v in r) / n for k in (1, 5, 10)}
    out["medr"] = 1.0 + (r[n // 2] if n % 2 else 0.5 * (r[n // 2 - 1] + r[n // 2]))
    out["meanr"] = 1.0 + sum(r) / n
    return out


def _check_weights(w_cider, w_bleu, w_rouge) -> Tuple[float, float, float]:
    w = (float(w_cider), float(w_bleu), float(w_rouge))
    if any(not math.isfinite(v) or v < 0.0 for v in w):
        raise ValueError(f"reward weights must be finite and >= 0, got {w}")
    if not any(w):
        raise ValueError("reward weights are all zero: there is nothing to optimise")
    return w


class RewardMix:
    """SCST reward ``w_cider * CIDEr-D + w_bleu * sbleu + w_rouge * ROUGE-L`` with ``CiderD.score``'s signature; the scores keep their
    native units (CIDEr-D in 0..10, the other two in 0..1), as in self-critical.pytorch.  ``cider``: a ``CiderD``; ``overlap``: an
    ``OverlapScorer``.  A scorer whose weights are 0 may be None and is never launched."""

    def __init__(self, cider=None, overlap: Optional[OverlapScorer] = None, w_cider: float = 1.0, w_bleu: float = 0.0,
                 w_rouge: float = 0.0):
        w = _check_weights(w_cider, w_bleu, w_rouge)
        if w[0] > 0.0 and cider is None:
            raise ValueError("a CIDEr-D weight needs a CiderD scorer")
        if (w[1] > 0.0 or w[2] > 0.0) and overlap is None:
            raise ValueError("a BLEU or ROUGE-L weight needs an OverlapScorer")
        self.cider, self.overlap = cider, overlap
        self.w_cider, self.w_bleu, self.w_rouge = w

    def score(self, cand_ids: torch.Tensor, cand_lengths: torch.Tensor, refs: RefBatch, cand_img: torch.Tensor = None) -> torch.Tensor:
        """The weighted sum as device f32 of ``cand_lengths``'s shape: at most one launch per scorer, no host sync."""
        out = None
        if self.w_cider > 0.0:
            out = self.cider.score(cand_ids, cand_lengths, refs, cand_img=cand_img) * self.w_cider
        if self.w_bleu > 0.0 or self.w_rouge > 0.0:
            _, rouge, sbleu = self.overlap.score(cand_ids, cand_lengths, refs, cand_img=cand_img)
            for w, term in ((self.w_bleu, sbleu), (self.w_rouge, rouge)):
                if w > 0.0:
                    out = term * w if out is None else out + term * w
        return out

