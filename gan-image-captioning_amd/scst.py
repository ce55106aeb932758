"""Self-critical sequence training (Rennie et al., CVPR 2017) with CIDEr-D rewards scored on the GPU.  No reference counterpart: the
reference trains with MLE and the Gumbel-softmax GAN only.  DESIGN.md section 13.

One step (every tensor stays on the device; the caller reads the returned scalars with one sync):
  1. features         GANInstructor._features with autograd, in the current train mode (encoder head / embed(<S>) / attention map)
  2. n samples        sample_captions at temperature 1, no truncation (the policy itself), up to max_caption_len steps
  3. baseline         greedy: beam search k = 1 on the detached features; mean: the mean reward of the image's other n - 1 samples
  4. rewards          ONE gic_cider_d launch for the B*n samples (and the B greedy captions); with --scst-bleu-weight / --scst-rouge-weight
                      a metrics.RewardMix adds one gic_caption_overlap launch (smoothed sentence BLEU-4, ROUGE-L) and the weighted sum
  5. teacher-forced   decoder.forward over the B*n samples (caps = ids[:, :-1], the sampled lengths, features repeated per sample),
                      max_length = L so that the device lengths are never read back
  6. loss             -(1/(B n)) sum_i (r_i - b_i) sum_{t < len_i} log p(y_it): gic_xent with row weights (r_i - b_i) * L (zero past a
                      caption's length) -- its mean over the B*n*L rows is the loss
  7. update           GANInstructor.optimize: clip + Adam, the data-parallel reducer
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Optional, Union

import torch

from . import engine
from .cider import CiderD, RefBatch
from .generator import SEEDS

if TYPE_CHECKING:
    from .metrics import RewardMix


class _WeightedNLLFn(torch.autograd.Function):
    """mean_r w_r * nll_r over the rows of logits [rows, V] (gic_xent with row_weight); the weights are constants."""

    @staticmethod
    def forward(ctx, logits, targets, weights):
        loss, dlog = engine.xent(logits.detach().contiguous(), targets, want_grad=ctx.needs_input_grad[0], row_weight=weights)
        ctx.dlog = dlog
        return loss[0]

    @staticmethod
    def backward(ctx, d):
        return ctx.dlog * d.to(ctx.dlog.dtype), None, None


class SCSTStep:
    """SCST generator update bound to a GANInstructor (its generator, ``_features``, ``optimize`` and reducer) and a reward scorer: a
    CIDEr-D scorer whose table holds the training references' document frequencies, or anything with its ``score`` (metrics.RewardMix)."""

    def __init__(self, inst, scorer: Union[CiderD, "RewardMix"], num_samples: int = 5, baseline: str = "greedy", lr: float = 5e-5):
        from .optim import FusedClipAdam
        if baseline not in ("greedy", "mean"):
            raise ValueError(f"--scst-baseline must be greedy or mean, got {baseline!r}")
        if not 1 <= int(num_samples) <= 8:
            raise ValueError("--scst-samples must be in 1..8")
        if baseline == "mean" and int(num_samples) < 2:
            raise ValueError("--scst-baseline mean needs --scst-samples >= 2 (the other samples of the image)")
        self.inst, self.scorer = inst, scorer
        self.n, self.baseline = int(num_samples), baseline
        # the constant --scst-lr, with the generator's weight decay and weight EMA (one per arena) where the instructor has them
        self.opt = FusedClipAdam(inst.gen_arena, float(lr), inst.args.clip_norm, weight_decay=getattr(inst, "gen_weight_decay", 0.0),
                                 ema=getattr(inst, "ema", None))

    def __call__(self, images, refs: RefBatch, max_caption_len: int, opt_step: bool = True, noise_u: Optional[torch.Tensor] = None,
                 seed: Optional[int] = None) -> dict:
        """One step on B images with their references (a RefBatch on the device).  ``noise_u`` f32 [L, B*n, V] fixes the draw (tests);
        otherwise Philox(``seed``, default the next of SEEDS).  With ``opt_step`` False the gradients are left in the generator's arena
        and no update runs.  Returns device tensors: loss, reward (mean sampled reward), baseline (mean baseline reward), ids [B, n, L],
        lengths [B, n], rewards [B, n], baselines [B, n]."""
        inst, n, L = self.inst, self.n, int(max_caption_len)
        B = refs.num_images
        dec = inst.gen.decoder
        feats = inst._features(images, B)
        fmap = None
        if inst.attention:
            feats, fmap = feats
        extra = (fmap,) if fmap is not None else ()
        seed = (0 if noise_u is not None else SEEDS.next()) if seed is None else int(seed)
        ids, _, lengths = dec.sample_captions(feats, *extra, num_samples=n, temperature=1.0, max_caption_len=L, seed=seed, noise_u=noise_u)
        dev = ids.device
        img = torch.arange(B, device=dev, dtype=torch.int32)
        if self.baseline == "greedy":
            g_ids, _, g_len = dec.beam_search(feats.detach(), *extra, beam_size=1, max_caption_len=L)
            cand = torch.cat([ids.reshape(B * n, L), g_ids], 0)
            clen = torch.cat([lengths.reshape(-1), g_len.reshape(-1)], 0)
            cimg = torch.cat([img.repeat_interleave(n), img], 0)
        else:
            cand, clen, cimg = ids.reshape(B * n, L), lengths.reshape(-1), img.repeat_interleave(n)
        scores = self.scorer.score(cand, clen, refs, cand_img=cimg)           # one launch: samples (+ greedy captions)
        rewards = scores[:B * n].view(B, n)
        if self.baseline == "greedy":
            base = scores[B * n:].view(B, 1).expand(B, n)
        else:
            base = (rewards.sum(1, keepdim=True) - rewards) / (n - 1)
        # teacher-forced rescoring of the samples with autograd: row (i, t) predicts ids[i, t]
        flat = ids.reshape(B * n, L)
        f_rep = feats.repeat_interleave(n, 0)
        rep = (fmap.repeat_interleave(n, 0),) if fmap is not None else ()
        pred = dec(f_rep, *rep, flat[:, :-1], lengths.reshape(-1), pretrain=True, max_length=L)[0]
        live = torch.arange(L, device=dev)[None, :] < lengths.reshape(-1, 1)
        w = torch.where(live, ((rewards - base).reshape(-1, 1) * float(L)).expand(B * n, L), torch.zeros((), device=dev))
        loss = _WeightedNLLFn.apply(pred.reshape(B * n * L, pred.shape[-1]), flat.reshape(-1), w.reshape(-1).contiguous())
        if opt_step:
            inst.optimize(self.opt, loss)
        else:
            self.opt.zero_grad()
            loss.backward()
        return {"loss": loss.detach(), "reward": rewards.mean(), "baseline": base.mean(), "ids": ids, "lengths": lengths,
                "rewards": rewards, "baselines": base}
