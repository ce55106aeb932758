"""RelGAN-style multi-representation CNN discriminator with the reference's module API and
state-dict keys (src/discriminator.py:9-86), computing through libgicap.so.

``forward(inp)`` accepts the reference's dense ``[B, L, V]`` float tensor (soft captions or a
one-hot) and, as an extension, ``int64 [B, L]`` token ids (the one-hot product evaluated as a
gather).  Gradients flow to the parameters and to a dense ``inp``.

``--disc-cond projection`` (no reference counterpart) makes D score (image, caption) pairs in the
projection form of Miyato & Koyama: ``logits += F^-1/2 <y, img_proj(pooled trunk feature)>`` with
``y`` the dropped highway output that ``feature2out`` consumes.  ``forward`` then takes the pooled
trunk features as ``image_features`` (detached: no gradient reaches the trunk or G's encoder head).
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Optional

import torch
import torch.nn as nn

from . import engine
from .generator import SEEDS, _LinearParams, _compute_dtype


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, train, keep_mask, seed, want_param_grads, inp, *params):
        dparams = [p.detach() for p in params]
        is_ids = inp.dtype == torch.int64
        soft = None if is_ids else eng.soft_input(inp.detach())
        ids = inp if is_ids else None
        logits, st = eng.fwd(dparams, soft, ids, train, keep_mask, seed)
        ctx.eng, ctx.train, ctx.st, ctx.dparams = eng, train, st, dparams
        ctx.soft, ctx.ids = soft, ids
        ctx.in_dtype = inp.dtype
        ctx.want_param_grads = want_param_grads
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        want_inp = ctx.needs_input_grad[5] and ctx.soft is not None
        want_par = ctx.want_param_grads and any(ctx.needs_input_grad[6:])
        grads, d_inp = ctx.eng.bwd(ctx.dparams, ctx.st, ctx.soft, ctx.ids, ctx.train, d_logits, want_par, want_inp)
        ctx.st = None
        if d_inp is not None and d_inp.dtype != ctx.in_dtype:
            d_inp = d_inp.to(ctx.in_dtype)
        pg = grads if grads is not None else [None] * len(ctx.dparams)
        return (None, None, None, None, None, d_inp, *pg)


class _DiscCondFn(torch.autograd.Function):
    """_DiscFn with the projection match term: q = img_proj(pooled), logits += F^-1/2 <ydrop, q>."""

    @staticmethod
    def forward(ctx, eng, train, keep_mask, seed, want_param_grads, inp, pooled, proj_w, proj_b, *params):
        dparams = [p.detach() for p in params]
        is_ids = inp.dtype == torch.int64
        soft = None if is_ids else eng.soft_input(inp.detach())
        ids = inp if is_ids else None
        q, pooled_act = eng.img_proj_fwd(proj_w.detach(), proj_b.detach(), pooled.detach())
        logits, st = eng.fwd(dparams, soft, ids, train, keep_mask, seed, cond=q)
        ctx.eng, ctx.train, ctx.st, ctx.dparams = eng, train, st, dparams
        ctx.soft, ctx.ids, ctx.q, ctx.pooled = soft, ids, q, pooled_act
        ctx.in_dtype = inp.dtype
        ctx.want_param_grads = want_param_grads
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        want_inp = ctx.needs_input_grad[5] and ctx.soft is not None
        want_par = ctx.want_param_grads and any(ctx.needs_input_grad[7:])
        grads, d_inp, d_q = ctx.eng.bwd(ctx.dparams, ctx.st, ctx.soft, ctx.ids, ctx.train, d_logits, want_par, want_inp, cond=ctx.q)
        ctx.st = None
        if d_inp is not None and d_inp.dtype != ctx.in_dtype:
            d_inp = d_inp.to(ctx.in_dtype)
        d_w = d_b = None
        if want_par:
            d_w = torch.empty(ctx.q.shape[1], ctx.pooled.shape[1], device=d_q.device, dtype=torch.float32)
            d_b = torch.empty(ctx.q.shape[1], device=d_q.device, dtype=torch.float32)
            ctx.eng.img_proj_bwd(d_q, ctx.pooled, d_w, d_b)
        pg = grads if grads is not None else [None] * len(ctx.dparams)
        return (None, None, None, None, None, d_inp, None, d_w, d_b, *pg)


DISC_COND = ("none", "projection")


def check_disc_cond(args) -> str:
    """--disc-cond and what it needs, before any module is built."""
    cond = getattr(args, "disc_cond", "none") or "none"
    if cond not in DISC_COND:
        raise ValueError(f"--disc-cond must be one of {DISC_COND}, got {cond!r}")
    if cond == "projection":
        if int(getattr(args, "conditional_gan", 0)) != 1:
            raise ValueError("--disc-cond projection scores (image, caption) pairs: it needs --conditional-gan 1")
        if getattr(args, "adv_mode", "relgan") == "seqgan":
            raise ValueError("--disc-cond projection is not available with --adv-mode seqgan: the conditioned roll-out reward "
                             "(reward rows that carry an image index) is a follow-up")
        if not int(getattr(args, "real_as_ids", 1)):
            raise ValueError("--disc-cond projection needs --real-as-ids 1: the conditioned step scores the real captions from token ids")
        w = float(getattr(args, "disc_mismatch_weight", 0.5))
        if not 0.0 <= w < 1.0:
            raise ValueError(f"--disc-mismatch-weight must be in [0, 1), got {w}")
    return cond


class _ConvParams(nn.Module):
    """nn.Conv2d(1, n, (f, s), stride=(1, s)) parameter container (discriminator.py:22-25)."""

    def __init__(self, n: int, f: int, s: int):
        super().__init__()
        k = 1.0 / math.sqrt(f * s)
        self.weight = nn.Parameter(torch.empty(n, 1, f, s).uniform_(-k, k))
        self.bias = nn.Parameter(torch.empty(n).uniform_(-k, k))


class Discriminator(nn.Module):
    def __init__(self, args, gpu=False, dropout=0.2):
        super().__init__()
        if not 0.0 <= float(dropout) < 1.0:            # nn.Dropout(dropout), discriminator.py:10,30 (p = 1 would zero every feature)
            raise ValueError("dropout probability has to be in [0, 1), but got {}".format(dropout))
        self.dropout_p = float(dropout)
        self.vocab_size = args.vocab_size
        self.embed_dim = args.disc_embed_dim
        self.padding_idx = args.padding_idx
        self.feature_dim = sum(args.disc_num_filters)
        self.emb_dim_single = int(args.disc_embed_dim / args.disc_num_rep)
        self.gpu = gpu
        self.embeddings = _LinearParams(self.vocab_size, self.embed_dim, bias=False)
        self.convs = nn.ModuleList([_ConvParams(n, f, self.emb_dim_single)
                                    for n, f in zip(args.disc_num_filters, args.disc_filter_sizes)])
        self.highway = _LinearParams(self.feature_dim, self.feature_dim)
        self.feature2out = _LinearParams(self.feature_dim, 100)
        self.out2logits = _LinearParams(100, 1)
        self.cond = check_disc_cond(args)
        if self.cond == "projection":               # exists (state dict, param_list, arena) only when the flag is on
            from .trunk import ARCHS
            _, _, widths, expansion = ARCHS[getattr(args, "encoder_arch", "resnet18")]
            self.img_proj = _LinearParams(widths[-1] * expansion, self.feature_dim)
        self.args = args
        self._engine: Optional[engine.DiscEngine] = None
        self._param_grads = True
        self.init_params()

    def engine(self) -> engine.DiscEngine:
        if self._engine is None:
            a = self.args
            self._engine = engine.DiscEngine(a.vocab_size, a.disc_embed_dim, a.disc_num_rep, a.disc_filter_sizes,
                                             a.disc_num_filters, _compute_dtype(a), dropout=self.dropout_p)
        return self._engine

    def param_list(self) -> List[nn.Parameter]:
        ps = [self.embeddings.weight]
        for c in self.convs:
            ps += [c.weight, c.bias]
        ps += [self.highway.weight, self.highway.bias, self.feature2out.weight, self.feature2out.bias,
               self.out2logits.weight, self.out2logits.bias]
        if self.cond == "projection":               # behind the engine's parameters (DiscEngine.nparams() of them)
            ps += [self.img_proj.weight, self.img_proj.bias]
        return ps

    def text_param_list(self) -> List[nn.Parameter]:
        """The parameters of the caption path in the engine's order: param_list() without img_proj."""
        return self.param_list()[:7 + 2 * len(self.convs)]

    @contextlib.contextmanager
    def input_grad_only(self):
        """Inside this context forward() records no parameter gradients: the generator's path through D
        (training.py:164,169) only needs d(loss)/d(input); the parameter gradients the reference computes
        there are discarded by the next zero_grad (training.py:195)."""
        prev, self._param_grads = self._param_grads, False
        try:
            yield self
        finally:
            self._param_grads = prev

    def forward(self, inp, image_features=None, keep_mask=None):
        """inp: float [B, L, V] (or int64 ids [B, L]) -> logits [B * num_rep] (discriminator.py:34-62).
        image_features: the frozen trunk's pooled features [B, C] of the captions' images -- required by a module built with
        --disc-cond projection, refused by any other."""
        seed = 0 if keep_mask is not None else SEEDS.next()
        if self.cond != "projection":
            if image_features is not None:
                raise ValueError("image_features given to a discriminator built without --disc-cond projection")
            return _DiscFn.apply(self.engine(), self.training, keep_mask, seed, self._param_grads, inp, *self.param_list())
        if image_features is None:
            raise ValueError("a discriminator built with --disc-cond projection needs image_features")
        if image_features.shape[0] != inp.shape[0]:
            raise ValueError(f"image_features has {image_features.shape[0]} rows for {inp.shape[0]} captions")
        return _DiscCondFn.apply(self.engine(), self.training, keep_mask, seed, self._param_grads, inp, image_features.detach(),
                                 self.img_proj.weight, self.img_proj.bias, *self.text_param_list())

    def score(self, image_features, ids, image_index=None):
        """Eval-mode score of (image, caption) pairs: the mean logit over the num_rep representations.  Three forms:
        ``ids`` [B, L] against ``image_features`` [B, C] -> [B];  ``ids`` [B, K, L], K captions per image -> [B, K] (image b serves its K
        captions through an index, nothing is repeated);  ``ids`` [N, L] with ``image_index`` int [N] into ``image_features`` [G, C] -> [N].
        A module built without --disc-cond projection takes ``image_features=None`` and scores the captions alone.  Runs under no-grad
        on a forward-only state and restores the module's mode."""
        logits, shape = self.score_logits(image_features, ids, image_index)
        return logits.view(-1, int(self.args.disc_num_rep)).mean(1).view(shape)

    def score_logits(self, image_features, ids, image_index=None):
        """The logits behind ``score``: (f32 [captions * num_rep] in caption-major order, the shape of the score)."""
        if ids.dtype != torch.int64 or ids.dim() not in (2, 3):
            raise ValueError(f"score takes int64 token ids [B, L] or [B, K, L], got {ids.dtype} {tuple(ids.shape)}")
        shape = tuple(ids.shape[:-1])
        flat = ids.reshape(-1, ids.shape[-1])
        if self.cond != "projection":
            if image_features is not None:
                raise ValueError("image_features given to a discriminator built without --disc-cond projection")
            if image_index is not None:
                raise ValueError("image_index given to a discriminator built without --disc-cond projection")
        else:
            if image_features is None:
                raise ValueError("a discriminator built with --disc-cond projection needs image_features")
            G = image_features.shape[0]
            if ids.dim() == 3:
                if image_index is not None:
                    raise ValueError("image_index goes with ids [N, L]: ids [B, K, L] are indexed by their first dimension")
                if G != ids.shape[0]:
                    raise ValueError(f"image_features has {G} rows for {ids.shape[0]} images")
                K = ids.shape[1]
                image_index = None if K == 1 else torch.arange(G * K, device=ids.device, dtype=torch.int32) // K
            elif image_index is not None:
                if image_index.dim() != 1 or image_index.shape[0] != flat.shape[0] or image_index.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"image_index must be an int tensor [{flat.shape[0]}], got {image_index.dtype} {tuple(image_index.shape)}")
                image_index = image_index.to(device=ids.device, dtype=torch.int32).contiguous()
            elif G != flat.shape[0]:
                raise ValueError(f"image_features has {G} rows for {flat.shape[0]} captions")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                eng = self.engine()
                q = None
                if self.cond == "projection":
                    q, _ = eng.img_proj_fwd(self.img_proj.weight.detach(), self.img_proj.bias.detach(), image_features.detach())
                logits, _ = eng.fwd([p.detach() for p in self.text_param_list()], None, flat, False, forward_only=True, cond=q,
                                    cond_index=image_index)
        finally:
            self.train(was_training)
        return logits, shape

    def get_feature(self, inp):
        raise NotImplementedError("get_feature is unused by the reference trainer and broken there for num_rep > 1 "
                                  "(discriminator.py:64-77)")

    def init_params(self):
        """discriminator.py:79-86."""
        for param in self.parameters():
            if param.requires_grad and len(param.shape) > 0:
                if self.args.disc_init == "uniform":
                    torch.nn.init.uniform_(param, a=-0.05, b=0.05)
                elif self.args.disc_init == "normal":
                    torch.nn.init.normal_(param, std=1 / math.sqrt(param.shape[0]))


def rerank(disc, image_features, ids, scores, lengths, weight=1.0, length_penalty=0.0, alphas=None):
    """Re-rank K candidate captions per image with a discriminator's score (Dai et al. 2017): ``ids`` int64 [B, K, L], ``scores`` f32
    [B, K] (G's log-probabilities), ``lengths`` int32 [B, K], ``alphas`` f32 [B, K, L, P] or None; ``image_features`` [B, C] the pooled
    trunk features of the images (None for a D built without --disc-cond projection).
      final[b, k] = scores[b, k] / max(lengths[b, k], 1) ** length_penalty + weight * disc.score(...)[b, k]
    One D forward over the B*K captions (no repeat of the features: Discriminator.score's [B, K, L] form) and one gic_rerank launch.
    Returns a dict in the new order (final descending, ties to the lower input index, NaN last): ``ids``, ``scores`` (G's raw
    log-probabilities), ``lengths``, ``alphas`` (None without), ``order`` int32 [B, K] (input indices), ``final`` and ``d`` f32 [B, K]."""
    if ids.dim() != 3:
        raise ValueError(f"rerank takes ids [B, K, L], got {tuple(ids.shape)}")
    K = ids.shape[1]
    if not 1 <= K <= 64:
        raise ValueError(f"rerank orders 1..64 candidates per image, got {K}")
    logits, _ = disc.score_logits(image_features, ids)
    return engine.rerank(scores, lengths, logits, int(disc.args.disc_num_rep), float(weight), float(length_penalty), ids=ids, alphas=alphas)
