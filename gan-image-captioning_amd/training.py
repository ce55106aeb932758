"""GANInstructor: drop-in for the reference trainer (src/training.py:15-235).

Same public surface (``GANInstructor(args, train_dataset, dev_dataset)``, ``_run``,
``pretrain_generator``, ``genpretrain_loop``, ``adv_loop``, ``optimize``, ``update_temperature``),
same batch contract and logging, with these deliberate fixes:
  * step order: both backward passes on pre-update weights, then both optimizer steps -- the literal
    order (training.py:168-169) raises on every torch >= 1.5; losses are unaffected;
  * ``_run`` logs ``adv_epoch`` where the reference hits ``NameError: epoch`` (training.py:227);
  * the six per-batch host syncs (training.py:171-181) collapse into one;
  * data parallelism: one process per GPU, flat-gradient all-reduce over RCCL (parallel.py).
"""
from __future__ import annotations

import contextlib
import functools
import json
import math
import os
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader
from tqdm import tqdm

from . import engine, parallel
from .args import check_eval_ensemble, check_eval_forced, check_image_pipeline
from .discriminator import Discriminator
from .fused_step import FusedAdvStep
from .seqgan import SeqGANStep
from .generator import Ensemble, Generator
from .optim import ArenaEMA, FusedClipAdam, LRSchedule, ParamArena
from .tasks import make_collate, stack_images
from .utils import create_logger, get_fixed_temperature, get_losses


class _ScalarWriter:
    """SummaryWriter stand-in (tensorboard is optional): add_scalar -> <save_dir>/scalars.jsonl, buffered."""

    def __init__(self, logdir: Optional[str]):
        self._fh = None
        self._tb = None
        if logdir:
            try:
                from torch.utils.tensorboard import SummaryWriter      # noqa: WPS433
                self._tb = SummaryWriter(logdir)
            except Exception:
                os.makedirs(logdir, exist_ok=True)
                self._fh = open(os.path.join(logdir, "scalars.jsonl"), "a")

    def add_scalar(self, tag, value, step):
        value = float(value)
        if self._tb is not None:
            self._tb.add_scalar(tag, value, step)
        elif self._fh is not None:
            self._fh.write(json.dumps({"tag": tag, "value": value, "step": int(step)}) + "\n")

    def flush(self):
        if self._fh is not None:
            self._fh.flush()


def _lookahead(loader, device):
    """(batch on device, next batch on device or None): the adversarial loop hands the next images to the step so that
    their trunk forward overlaps this step (FusedAdvStep._prefetch_trunk)."""
    def to_dev(b):
        return (b[0].to(device), b[1].to(device), b[2], b[3])
    it = iter(loader)
    try:
        cur = to_dev(next(it))
    except StopIteration:
        return
    for b in it:
        nxt = to_dev(b)
        yield cur, nxt
        cur = nxt
    yield cur, None


def scst_reward_scorer(args, corpus):
    """The reward scorer of SCST from --scst-cider-weight / --scst-bleu-weight / --scst-rouge-weight, with document frequencies from
    ``corpus`` (per-image lists of reference token lists): at the defaults (1, 0, 0) the plain ``CiderD`` -- the launches and the bits
    of a CIDEr-only step -- else a ``metrics.RewardMix`` that builds only the scorers its weights use."""
    from .cider import CiderD
    from .metrics import OverlapScorer, RewardMix, _check_weights
    w = _check_weights(getattr(args, "scst_cider_weight", 1.0), getattr(args, "scst_bleu_weight", 0.0),
                       getattr(args, "scst_rouge_weight", 0.0))              # a bad weight fails before any table is built
    if w == (1.0, 0.0, 0.0):
        return CiderD(corpus, args.vocab_size, args.device)
    cider = CiderD(corpus, args.vocab_size, args.device) if w[0] > 0.0 else None
    overlap = OverlapScorer(args.vocab_size, args.device) if w[1] > 0.0 or w[2] > 0.0 else None
    return RewardMix(cider, overlap, *w)


def check_modes(args):
    """The instructor's checks of the mode flags, before anything touches the device: (pretrain_mode, attn_reg).  Either decoder
    (--decoder lstm | attention) trains with either adversarial update (--adv-mode relgan | seqgan)."""
    pretrain_mode = getattr(args, "pretrain_mode", "sample")
    attn_reg = float(getattr(args, "attn_reg", 0.0))
    if pretrain_mode not in ("sample", "teacher"):
        raise ValueError(f"--pretrain-mode must be sample or teacher, got {pretrain_mode!r}")
    if attn_reg != 0.0 and not (getattr(args, "decoder", "lstm") == "attention" and pretrain_mode == "teacher"):
        raise ValueError("--attn-reg applies to --decoder attention --pretrain-mode teacher only")
    return pretrain_mode, attn_reg


def check_scheduled_sampling(args):
    """The instructor's checks of the scheduled-sampling flags, before anything touches the device: (prob, ramp_epochs, pick)."""
    p = float(getattr(args, "scheduled_sampling_prob", 0.0))
    n = int(getattr(args, "scheduled_sampling_ramp_epochs", 0))
    pick = getattr(args, "scheduled_sampling_pick", "sample")
    if not 0.0 <= p <= 1.0:                       # false for NaN too
        raise ValueError(f"--scheduled-sampling-prob must be in [0, 1], got {p}")
    if n < 0:
        raise ValueError(f"--scheduled-sampling-ramp-epochs must be >= 0, got {n}")
    if pick not in ("sample", "argmax"):
        raise ValueError(f"--scheduled-sampling-pick must be sample or argmax, got {pick!r}")
    if p > 0.0 and getattr(args, "pretrain_mode", "sample") != "teacher":
        raise ValueError("--scheduled-sampling-prob mixes the decoder's own tokens into teacher forcing: it needs --pretrain-mode teacher")
    return p, n, pick


def check_gen_dropout(args) -> float:
    """The instructor's check of --gen-dropout, before anything touches the device: p."""
    p = float(getattr(args, "gen_dropout", 0.0))
    if not 0.0 <= p < 1.0:                        # false for NaN too
        raise ValueError(f"--gen-dropout must be in [0, 1), got {p}")
    if p > 0.0 and getattr(args, "pretrain_mode", "sample") != "teacher":
        raise ValueError("--gen-dropout drops the decoder's output in the teacher-forced decode: it needs --pretrain-mode teacher")
    return p


def check_seq_loss(args):
    """The instructor's checks of the sequence-loss flags, before anything touches the device: (ignore_pad, label_smoothing)."""
    eps = float(getattr(args, "label_smoothing", 0.0))
    if not 0.0 <= eps < 1.0:                      # false for NaN too
        raise ValueError(f"--label-smoothing must be in [0, 1), got {eps}")
    return bool(int(getattr(args, "pretrain_ignore_pad", 0))), eps


def check_optimizer(args) -> dict:
    """The instructor's checks of the optimizer flags, before anything touches the device: the schedules' shapes (their horizons come
    from the loaders), the weight decays, the EMA decay / warm-up and --eval-ema.  The horizon check (linear / cosine need more
    steps than their warm-up) is LRSchedule.validate's, at the optimizer's construction."""
    r = float(getattr(args, "lr_min_ratio", 0.0))
    if not 0.0 <= r <= 1.0:                       # false for NaN too
        raise ValueError(f"--lr-min-ratio must be in [0, 1], got {r}")
    S, gamma = int(getattr(args, "lr_step_size", 0)), float(getattr(args, "lr_step_gamma", 0.1))
    shapes = {}
    for phase in ("pretrain", "adv"):
        kind, W = getattr(args, f"{phase}_lr_schedule", "none"), int(getattr(args, f"{phase}_lr_warmup_steps", 0))
        if W < 0:
            raise ValueError(f"--{phase}-lr-warmup-steps must be >= 0, got {W}")
        if kind == "step" and S <= 0:
            raise ValueError(f"--{phase}-lr-schedule step needs a positive --lr-step-size, got {S}")
        shapes[phase] = LRSchedule(kind, W, 0, r, S, gamma)
        if kind not in ("linear", "cosine"):
            shapes[phase].validate()
    wd = {}
    for who in ("gen", "disc"):
        wd[who] = float(getattr(args, f"{who}_weight_decay", 0.0))
        if not wd[who] >= 0.0:
            raise ValueError(f"--{who}-weight-decay must be >= 0, got {wd[who]}")
    d = float(getattr(args, "gen_ema_decay", 0.0))
    if not 0.0 <= d < 1.0:
        raise ValueError(f"--gen-ema-decay must be in [0, 1), got {d}")
    eval_ema = bool(int(getattr(args, "eval_ema", 0)))
    if eval_ema and d == 0.0:
        raise ValueError("--eval-ema 1 evaluates the averaged generator: it needs --gen-ema-decay > 0")
    return {"pretrain": shapes["pretrain"], "adv": shapes["adv"], "gen_wd": wd["gen"], "disc_wd": wd["disc"], "ema_decay": d,
            "ema_warmup": bool(int(getattr(args, "gen_ema_warmup", 1))), "eval_ema": eval_ema}


def build_optimizers(args, oc, gen_arena, disc_arena, pretrain_steps, adv_steps):
    """(pretrain_opt, gen_opt, disc_opt, ema) of the instructor (training.py:24-26) from ``oc = check_optimizer(args)`` and the two
    phases' step counts, the schedules' horizons.  One ArenaEMA on gen_arena, advanced by every generator optimizer (SCST's too); D
    gets schedule and decay and no EMA.  Neutral flags give neutral keywords: plain clip + Adam."""
    pre_sched, adv_sched = oc["pretrain"]._replace(total=pretrain_steps), oc["adv"]._replace(total=adv_steps)
    ema = ArenaEMA(gen_arena, oc["ema_decay"], oc["ema_warmup"]) if oc["ema_decay"] > 0.0 else None
    g_kw = {"weight_decay": oc["gen_wd"], "ema": ema}
    pretrain_opt = FusedClipAdam(gen_arena, args.pretrain_lr, args.clip_norm, schedule=pre_sched, **g_kw)
    gen_opt = FusedClipAdam(gen_arena, args.gen_lr, args.clip_norm, schedule=adv_sched, **g_kw)
    disc_opt = FusedClipAdam(disc_arena, args.disc_lr, args.clip_norm, schedule=adv_sched, weight_decay=oc["disc_wd"])
    return pretrain_opt, gen_opt, disc_opt, ema


def _on_eval_weights(method):
    """An evaluate* method of GANInstructor: under --eval-ema 1 it runs with the averaged generator in the live parameters."""
    @functools.wraps(method)
    def run(self, *a, **kw):
        with self._eval_weights():
            return method(self, *a, **kw)
    return run


def scheduled_sampling_prob(p: float, ramp_epochs: int, epoch: int) -> float:
    """p_e = p * min(1, e / n) of epoch e (0-based); n = 0: p throughout."""
    return p if ramp_epochs <= 0 else p * min(1.0, epoch / ramp_epochs)


class GANInstructor:
    ema = None              # ArenaEMA of gen_arena under --gen-ema-decay
    eval_ema = False        # --eval-ema
    _ema_held = False       # True: evaluate* stays on the weights that are live now (nested evaluations, checkpoint selection)
    eval_ensemble = None    # --eval-ensemble*: what check_eval_ensemble returned
    eval_forced = None      # --eval-force-words / --eval-force-beam-size: what check_eval_forced returned
    _ensemble = None        # the evaluations' Ensemble, built at the first evaluation that needs it
    _ensemble_ema = None    # its EMA member, refreshed at the start of every evaluation
    _live_only = False      # True: evaluate* stays on the live generator alone (checkpoint selection)
    scst_opt = None         # SCST's own optimizer over gen_arena, once scst_train has built it
    _train_state = None     # a loaded --resume-train-state, for the optimizers built later (SCST)

    def __init__(self, args, train_dataset, dev_dataset):
        self.args = args
        self.pretrain_mode, self.attn_reg = check_modes(args)
        self.ss_prob, self.ss_ramp, self.ss_pick = check_scheduled_sampling(args)
        self.ss_prob_now = scheduled_sampling_prob(self.ss_prob, self.ss_ramp, 0)      # pretrain_generator sets it per epoch
        self.gen_dropout = check_gen_dropout(args)
        self.ignore_pad, self.label_smoothing = check_seq_loss(args)
        check_image_pipeline(args)
        oc = check_optimizer(args)
        self.eval_ensemble = check_eval_ensemble(args)       # None: the evaluations run on the one generator
        self.eval_forced = check_eval_forced(args)           # None: no forced-words evaluation; else (N, beam size)
        self.dist = parallel.DistInfo.from_env()
        from .generator import SEEDS
        SEEDS.rank = self.dist.rank            # replicas share weights and the torch seed, not the device noise streams
        self.gen = Generator(args).to(args.device)                        # training.py:19
        self.disc = Discriminator(args).to(args.device)                   # training.py:20
        self.cgan = (args.conditional_gan == 1)
        self.attention = getattr(args, "decoder", "lstm") == "attention"
        if int(getattr(args, "deterministic", 0)):
            engine.set_deterministic(True)
        if self.attention and engine.deterministic():
            # the attention decoder's split-K products (attention.hip) still add f32 partials atomically
            raise ValueError("--decoder attention is not available with --deterministic 1 (or GIC_DETERMINISTIC=1)")
        if self.dist.world_size > 1:
            parallel.broadcast_module(self.gen, self.dist)
            parallel.broadcast_module(self.disc, self.dist)
        rank0 = self.dist.rank == 0
        self.log = create_logger(__name__ + str(id(self)), silent=not rank0, to_disk=rank0 and bool(getattr(args, "log_file", None)),
                                 log_file=(args.log_file + ".txt") if getattr(args, "log_file", None) else None)

        # Trainable generator parameters: the decoder, plus the encoder head under --conditional-gan 1.  The
        # ResNet trunk runs under no_grad (generator.py:21) so Adam never touches it (grad is None there).
        g_params = list(self.gen.decoder.parameters())
        if self.cgan:
            g_params += list(self.gen.encoder.linear.parameters()) + list(self.gen.encoder.bn.parameters())
        self.gen_arena = ParamArena(g_params)
        self.disc_arena = ParamArena(self.disc.parameters())
        self.train_dataset, self.dev_dataset = train_dataset, dev_dataset
        nw = int(getattr(args, "num_workers", 4))
        dp = self.dist.world_size > 1
        # training.py:28-32 (shuffle=True for the two train loaders).  Under data parallelism the shuffling moves into the
        # DistributedSampler (the DataLoader itself must not shuffle when it is given a sampler); set_epoch() in the loops.
        mk = lambda ds, bs, shuffle: None if ds is None else DataLoader(   # noqa: E731
            ds, shuffle=shuffle and not dp, batch_size=bs, collate_fn=make_collate(ds), num_workers=nw,
            sampler=parallel.shard_sampler(ds, self.dist, shuffle) if dp else None)
        self.pre_train_loader = mk(train_dataset, args.pre_train_batch_size, True)
        self.pre_eval_loader = mk(dev_dataset, args.pre_eval_batch_size, False)
        self.adv_train_loader = mk(train_dataset, args.adv_train_batch_size, True)
        self.adv_eval_loader = mk(dev_dataset, args.adv_eval_batch_size, False)
        self._sampler_epoch = 0

        # LR schedules over the phases' step counts, decoupled weight decay and G's weight EMA; with every flag at its default the
        # optimizers are plain clip + Adam
        steps = lambda epochs, loader: int(epochs) * (len(loader) if loader is not None else 0)      # noqa: E731
        self.gen_weight_decay, self.eval_ema = oc["gen_wd"], oc["eval_ema"]
        self.pretrain_opt, self.gen_opt, self.disc_opt, self.ema = build_optimizers(
            args, oc, self.gen_arena, self.disc_arena, steps(args.pretrain_epochs, self.pre_train_loader),
            steps(args.adv_epochs, self.adv_train_loader))
        self.reducer = parallel.GradReducer(self.dist) if self.dist.world_size > 1 else None
        self.fused = FusedAdvStep(self.gen, self.disc, self.gen_arena, self.disc_arena, args, self.reducer
                                  ).bind_optimizers(self.gen_opt, self.disc_opt)
        # --adv-mode seqgan: policy gradient + Monte-Carlo roll-outs (no reference counterpart; seqgan.py)
        self.seqgan = SeqGANStep(self.gen, self.disc, self.gen_arena, self.disc_arena, args, self.reducer
                                 ).bind_optimizers(self.gen_opt, self.disc_opt)

        self.model_dir = getattr(args, "model_dir", None)
        self.writer = _ScalarWriter(getattr(args, "save_dir", None) if rank0 and getattr(args, "log_file", None) else None)
        self.pretrain_steps = 0
        self.gen_steps = 0
        self.disc_steps = 0
        self.adv_epoch = -1
        self.scst_steps = 0
        self._cider = {}

    # ------------------------------------------------------------------ shared pieces
    def _features(self, images, batch, next_images=None):
        if self.attention:
            return self.gen.encoder.forward_with_map(images, next_images=next_images)      # (features, feature map)
        if self.cgan:
            return self.gen.encoder(images, next_images=next_images)       # training.py:66,145
        ones = torch.ones(batch, dtype=torch.long, device=self.args.device)
        return self.gen.decoder.embed(ones)                                # training.py:68,147

    def _reshuffle(self, loader, what) -> None:
        """Data parallel: a new permutation per pass over the training set (DistributedSampler.set_epoch), same on every rank."""
        if what == "train" and self.dist.world_size > 1 and hasattr(getattr(loader, "sampler", None), "set_epoch"):
            loader.sampler.set_epoch(self._sampler_epoch)
            self._sampler_epoch += 1

    def update_temperature(self, i, N):
        self.gen.decoder.temperature = get_fixed_temperature(self.args.temperature, i, N, self.args.temp_adpt)

    def optimize(self, opt, loss, model=None, retain_graph=False):
        """training.py:194-199; the clip_grad_norm_ of :198 is fused into ``opt.step()``."""
        opt.zero_grad()
        loss.backward(retain_graph=retain_graph)
        if self.reducer is not None:
            self.reducer.start(opt.arena.grad)
            self.reducer.wait_all()
        opt.step()

    # ------------------------------------------------------------------ MLE pre-training (training.py:48-126)
    def pretrain_step(self, images, captions, max_caption_len, train=True, next_images=None, lengths=None):
        feats = self._features(images, captions.shape[0], next_images)
        if self.pretrain_mode == "teacher":
            return self._pretrain_step_teacher(feats, captions, lengths, train)
        if self.attention:
            gen_captions, _ids = self.gen.decoder.sample(feats[0], fmap=feats[1], pretrain=True, max_caption_len=max_caption_len)
        else:
            gen_captions, _ids = self.gen.decoder.sample(feats, pretrain=True, max_caption_len=max_caption_len)
        loss = self._pretrain_loss(gen_captions, captions, train)         # nn.CrossEntropyLoss(), training.py:81-83
        if train:
            self.optimize(self.pretrain_opt, loss, self.gen)
        return loss

    def _pretrain_loss(self, pred, targets, train):
        """The pre-training loss of pred [B, T, V] against targets [B, T]: the reference's mean over all positions (_XentFn), or with
        --pretrain-ignore-pad 1 / --label-smoothing > 0 the mean over the tokens that are not <PAD>, label-smoothed (_SeqXentFn).
        Only training batches are smoothed: the validation loss stays comparable."""
        flat = pred.reshape(-1, pred.size(-1))
        eps = self.label_smoothing if train else 0.0
        if not self.ignore_pad and self.label_smoothing == 0.0:
            return _XentFn.apply(flat, targets.reshape(-1))
        ignore = int(self.args.padding_idx) if self.ignore_pad else -100        # -100: no token has it, nothing is ignored
        return _SeqXentFn.apply(flat, targets.reshape(-1), int(pred.shape[1]), None, ignore, eps)[0]

    def _pretrain_step_teacher(self, feats, captions, lengths, train):
        """--pretrain-mode teacher: pred = decoder.forward(features[, fmap], captions[:, :-1], lengths, pretrain=True), the same
        cross entropy against captions as the free-running step; with --attn-reg lam, + lam * mean_b sum_i (1 - sum_t alpha_bti)^2.
        With --scheduled-sampling-prob, a training step decodes through decoder.forward_scheduled at this epoch's probability; with
        --gen-dropout, a training step drops the decoder's output in front of the vocabulary projection."""
        if lengths is None:
            lengths = torch.full((captions.shape[0],), captions.shape[1], dtype=torch.int32)
        caps = captions[:, :-1]
        p = self.ss_prob_now if train else 0.0        # only training batches are mixed: the validation loss stays comparable
        drop = self.gen_dropout if train else 0.0     # ... and only training batches are dropped
        if p > 0.0:
            if self.attention:
                pred, _, alphas = self.gen.decoder.forward_scheduled(feats[0], feats[1], caps, lengths, p, pick=self.ss_pick,
                                                                     return_alphas=True, dropout=drop)
            else:
                pred, _ = self.gen.decoder.forward_scheduled(feats, caps, lengths, p, pick=self.ss_pick, dropout=drop)
                alphas = None
        elif self.attention:
            pred, _, alphas = self.gen.decoder(feats[0], feats[1], caps, lengths, pretrain=True, return_alphas=True, dropout=drop)
        else:
            pred, _ = self.gen.decoder(feats, caps, lengths, pretrain=True, dropout=drop)
            alphas = None
        loss = self._pretrain_loss(pred, captions[:, :pred.shape[1]], train)
        if self.attn_reg:
            loss = loss + self.attn_reg * ((1.0 - alphas.sum(1)) ** 2).sum(1).mean()
        if train:
            self.optimize(self.pretrain_opt, loss, self.gen)
        return loss

    def genpretrain_loop(self, what):
        gen_loss = []
        loader = self.pre_train_loader if what == "train" else self.pre_eval_loader
        total = len(self.train_dataset) if what == "train" else len(self.dev_dataset)
        self._reshuffle(loader, what)
        with (torch.enable_grad() if what == "train" else torch.no_grad()), \
                tqdm(total=total, disable=self.dist.rank != 0) as progress:
            for (images, captions, lengths, max_caption_len), nxt in _lookahead(loader, self.args.device):
                loss = self.pretrain_step(images, captions, max_caption_len, train=(what == "train"),
                                          next_images=nxt[0] if nxt is not None and nxt[0].shape == images.shape else None,
                                          lengths=lengths)
                val = loss.item()
                if val != val:      # gic_xent poisons the loss when a target is outside [0, V) (nn.CrossEntropyLoss would raise)
                    raise ValueError("pre-train loss is NaN: a caption token is outside [0, vocab_size=%d) or the logits overflowed"
                                     % self.args.vocab_size)
                gen_loss.append(val)
                self.writer.add_scalar("GenPreTraining_train_loss" if what == "train" else "GenPreTraining_val_loss",
                                       val, self.pretrain_steps)
                if what == "train":        # lr * lambda(s) of the next step, against the number s of steps taken
                    self.writer.add_scalar("GenPreTraining_lr", self.pretrain_opt.current_lr(), self.pretrain_opt.steps)
                progress.update(len(images) * self.dist.world_size)
                progress.set_postfix(loss=val)
        return gen_loss

    def pretrain_generator(self, epochs):
        self.log.info("Pretraining Generator")
        total_loss, best_loss = 0, None
        for epoch in range(self.args.pretrain_epochs):
            if self.ss_prob > 0.0:
                self.ss_prob_now = scheduled_sampling_prob(self.ss_prob, self.ss_ramp, epoch)
                self.log.info("Epoch {}: scheduled sampling probability {}".format(epoch, self.ss_prob_now))
                self.writer.add_scalar("GenPreTraining_sched_prob", self.ss_prob_now, self.pretrain_steps)
            self.gen.train()
            train_epoch_loss = np.mean(self.genpretrain_loop("train"))
            total_loss += train_epoch_loss
            self.gen.eval()
            val_epoch_loss = np.mean(self.genpretrain_loop("val"))
            if int(getattr(self.args, "eval_perplexity", 0)) and self.dist.rank == 0:
                self.evaluate_perplexity("val")
            if best_loss is None or val_epoch_loss < best_loss:
                best_loss = val_epoch_loss
                self._save(self.gen.state_dict(), "pretrained_model.ckpt")                    # training.py:118
                self.log.info("Saving Best model [Gen Loss = {}] at Epoch {}".format(best_loss, epoch))
            if epoch % self.args.pre_log_step == 0:
                self.log.info("Epoch {}: \n \t Train: {} \n\t Val: {} ".format(epoch, train_epoch_loss, val_epoch_loss))
            self.pretrain_steps += 1
        return total_loss / epochs if epochs != 0 else 0

    # ------------------------------------------------------------------ adversarial step (training.py:136-183)
    def adv_step(self, images, captions, max_caption_len, train=True, noise_u=None, keep_masks=None, next_images=None):
        """One minibatch.  Returns (g_loss, d_loss) as a 2-element device tensor (one host sync to read).
        ``next_images`` (optional): the next batch's images on the device, for the trunk prefetch of the fused step."""
        impl = getattr(self.args, "step_impl", "fused")
        if getattr(self.args, "adv_mode", "relgan") == "seqgan":
            return self.seqgan(images, captions, max_caption_len, train, next_images=next_images)["losses"]
        if impl == "fused":
            return self.fused(images, captions, max_caption_len, train, noise_u, keep_masks, next_images=next_images)["losses"]
        return self._adv_step_autograd(images, captions, max_caption_len, train, noise_u, keep_masks, next_images=next_images)

    def _adv_step_autograd(self, images, captions, max_caption_len, train, noise_u=None, keep_masks=None, next_images=None):
        """The reference's flow through the module API + autograd, with the fixed order."""
        km = tuple(keep_masks) if keep_masks is not None else (None, None, None)
        km = km + (None,) * (4 - len(km))
        cond = self.disc.cond == "projection"
        w = float(getattr(self.args, "disc_mismatch_weight", 0.5)) if cond else 0.0
        if w > 0.0 and captions.shape[0] < 2:
            raise ValueError("--disc-mismatch-weight > 0 needs at least two captions per batch: the wrong pair is the next image of the batch")
        with (torch.enable_grad() if train else torch.no_grad()):
            features = self._features(images, captions.shape[0], next_images if self.cgan else None)
            if self.attention:
                gen_captions, _ids = self.gen.decoder.sample(features[0], fmap=features[1], max_caption_len=max_caption_len, noise_u=noise_u)
            else:
                gen_captions, _ids = self.gen.decoder.sample(features, max_caption_len=max_caption_len, noise_u=noise_u)
            fake_captions = gen_captions.detach()                                            # training.py:151
            if int(getattr(self.args, "real_as_ids", 1)):
                real = captions
            else:
                real = F.one_hot(captions, self.args.vocab_size).float()                     # training.py:158
            # --disc-cond projection: every D pass also sees the pooled trunk features of the batch's images (detached)
            img = {"image_features": self.gen.encoder.last_trunk} if cond else {}
            d_out_real = self.disc(real, keep_mask=km[0], **img)                             # training.py:162
            d_out_fake = self.disc(fake_captions, keep_mask=km[1], **img)                    # training.py:163
            with self.disc.input_grad_only():
                g_out = self.disc(gen_captions, keep_mask=km[2], **img)                      # training.py:164
            g_loss, d_loss = get_losses(d_out_real, d_out_fake, g_out, self.args.adv_loss_type, detach_d_for_g=True)
            if w > 0.0:         # mismatched pairs: the real captions against the batch's images rolled by one, its own dropout draw
                d_out_wrong = self.disc(real, image_features=torch.roll(img["image_features"], -1, 0), keep_mask=km[3])
                _, d_wrong = get_losses(d_out_real, d_out_wrong, g_out, self.args.adv_loss_type, detach_d_for_g=True)
                d_loss = (1.0 - w) * d_loss + w * d_wrong
        if train:
            self.disc_opt.zero_grad()
            self.gen_opt.zero_grad()
            d_loss.backward()                       # reaches D's parameters only (fake is detached)
            if self.reducer is not None:
                self.reducer.start(self.disc_arena.grad)
            if g_loss.requires_grad:
                g_loss.backward()                   # reaches G through D's input gradient; D records no param grads here
            if self.reducer is not None:
                self.reducer.start(self.gen_arena.grad)
                self.reducer.wait_all()
            self.disc_opt.step()
            self.gen_opt.step()
        return torch.stack([g_loss.detach(), d_loss.detach()])

    def adv_loop(self, what):
        loader = self.adv_train_loader if what == "train" else self.adv_eval_loader
        total = len(self.train_dataset) if what == "train" else len(self.dev_dataset)
        self._reshuffle(loader, what)
        float_epoch = 0.0
        gen_loss, disc_loss = [], []
        with tqdm(total=total, disable=self.dist.rank != 0) as progress:
            for (images, captions, lengths, max_caption_len), nxt in _lookahead(loader, self.args.device):
                float_epoch += 1
                losses = self.adv_step(images, captions, max_caption_len, train=(what == "train"),
                                       next_images=nxt[0] if nxt is not None and nxt[0].shape == images.shape else None)
                g_val, d_val = losses.tolist()                                   # the step's single host sync
                self.writer.add_scalar("Discriminator_train_loss" if what == "train" else "Discriminator_val_loss", d_val, self.disc_steps)
                self.disc_steps += 1
                self.writer.add_scalar("Generator_train_loss" if what == "train" else "Generator_val_loss", g_val, self.gen_steps)
                self.gen_steps += 1
                if what == "train":
                    self.writer.add_scalar("Generator_lr", self.gen_opt.current_lr(), self.gen_opt.steps)
                    self.writer.add_scalar("Discriminator_lr", self.disc_opt.current_lr(), self.disc_opt.steps)
                gen_loss.append(g_val)
                disc_loss.append(d_val)
                progress.update(len(images) * self.dist.world_size)
                progress.set_postfix(disc_loss=d_val, gen_loss=g_val)
                self.update_temperature(self.adv_epoch + float_epoch / len(loader), self.args.adv_epochs)   # training.py:183
        return np.mean(gen_loss), np.mean(disc_loss)

    def load_checkpoint(self, path: str) -> str:
        """Load weights written by ``_run`` here or by the reference (training.py:118: the generator's state dict;
        training.py:225-226: {"generator", "discriminator"}).  Values are copied into the existing parameter storage (the flat
        arenas stay in place); optimizer moments start from zero, as after the reference's own cold start, and the EMA restarts from the
        loaded weights, unless ``load_train_state`` follows (--resume-train-state).  Returns the kind."""
        ckpt = torch.load(path, map_location=self.args.device)
        if isinstance(ckpt, dict) and set(ckpt) == {"generator", "discriminator"}:
            self.gen.load_state_dict(ckpt["generator"])
            d_state = ckpt["discriminator"]
            proj = ("img_proj.weight", "img_proj.bias")
            if self.disc.cond == "projection" and not any(k in d_state for k in proj):
                # a checkpoint of an unconditioned D: the text path loads, the image projection keeps its fresh initialisation
                # (every other key mismatch stays an error)
                own = self.disc.state_dict()
                d_state = dict(d_state, **{k: own[k] for k in proj})
                self.log.info("checkpoint %s holds no img_proj.*: the discriminator's image projection keeps its fresh initialisation", path)
            self.disc.load_state_dict(d_state)
            kind = "adversarial"
        else:
            self.gen.load_state_dict(ckpt)
            kind = "pretrained"
        from . import engine
        engine.bump_param_epoch()          # compute-dtype weight images are stale
        if self.ema is not None:
            self.ema.reset()
        self.log.info("resumed %s weights from %s", kind, path)
        return kind

    def _optimizers(self) -> dict:
        opts = {"pretrain_opt": self.pretrain_opt, "gen_opt": self.gen_opt, "disc_opt": self.disc_opt}
        if self.scst_opt is not None:
            opts["scst_opt"] = self.scst_opt
        return opts

    def train_state(self) -> dict:
        """What a model checkpoint leaves out: every optimizer's moments and step count, and the EMA's buffer and counter.  The
        loops' epoch counters are not part of it."""
        state = {name: opt.state_dict() for name, opt in self._optimizers().items()}
        if self.ema is not None:
            state["ema"] = self.ema.state_dict()
        return state

    def load_train_state(self, path: str) -> None:
        """Restore a ``*.train_state`` file (after ``load_checkpoint``): the schedules' positions, Adam's bias correction and the
        average continue where they were.  Optimizers absent from the file keep their fresh state; an EMA absent from it stays reset."""
        state = torch.load(path, map_location=self.args.device)
        for name, opt in self._optimizers().items():
            if name in state:
                opt.load_state_dict(state[name])
        if self.ema is not None and "ema" in state:
            self.ema.load_state_dict(state["ema"])
        self._train_state = state
        self.log.info("resumed optimizer state from %s", path)

    @contextlib.contextmanager
    def _eval_weights(self):
        if self.eval_ensemble is not None and not self._live_only and self._ensemble_ema is not None:
            self._load_ema_member(self._ensemble_ema)             # the average has moved since the last evaluation
        if not self.eval_ema or self._ema_held:
            yield
            return
        self._ema_held = True
        try:
            with self.ema.swapped():
                yield
        finally:
            self._ema_held = False

    @contextlib.contextmanager
    def _live_weights(self):
        """Evaluations inside the block stay on the live weights (checkpoint selection)."""
        held, self._ema_held = self._ema_held, True
        live, self._live_only = self._live_only, True
        try:
            yield
        finally:
            self._ema_held, self._live_only = held, live

    # ------------------------------------------------------------------ decode-time ensembles (generator.Ensemble)
    def _member_copy(self, share_trunk: bool = False):
        """A generator of the live one's configuration for an ensemble member, in the live one's mode.  ``share_trunk``: on the live
        trunk module itself (the frozen trunk is not averaged), so that an Ensemble runs the trunk once for both."""
        g = Generator(self.args).to(self.args.device)
        if share_trunk:
            g.encoder.resnet = self.gen.encoder.resnet
        g.train(self.gen.training)
        return g

    def _load_ema_member(self, g) -> None:
        with self.ema.swapped():
            g.load_state_dict(self.gen.state_dict())
        engine.bump_param_epoch()

    def ensemble(self, paths=(), with_ema=False, weights=None, mode="prob"):
        """An Ensemble (generator.py) of, in this order, the live generator, one copy per checkpoint of ``paths`` (load_checkpoint's
        formats: a generator state dict, or {"generator", "discriminator"}) and, with ``with_ema``, a copy that holds the averaged
        weights as they are now, on the live trunk.  ``weights`` (None: uniform) in the same order; ``mode`` "prob" / "logprob"."""
        if with_ema and self.ema is None:
            raise ValueError("ensemble(with_ema=True) needs --gen-ema-decay > 0")
        members = [self.gen]
        for path in paths:
            ckpt = torch.load(path, map_location=self.args.device)
            g = self._member_copy()
            g.load_state_dict(ckpt["generator"] if isinstance(ckpt, dict) and set(ckpt) == {"generator", "discriminator"} else ckpt)
            members.append(g)
        if with_ema:
            g = self._member_copy(share_trunk=True)
            self._load_ema_member(g)
            members.append(g)
        engine.bump_param_epoch()
        return Ensemble(members, weights, mode)

    def _eval_gen(self):
        """The generator the evaluations decode and score with: the live one, or under --eval-ensemble* (and outside checkpoint
        selection) the ensemble around it."""
        if self.eval_ensemble is None or self._live_only:
            return self.gen
        if self._ensemble is None:
            self._ensemble = self.ensemble(**self.eval_ensemble)
            self._ensemble_ema = self._ensemble.members[-1] if self.eval_ensemble["with_ema"] else None
        return self._ensemble

    def _save(self, obj, name):
        """A model checkpoint, its ``<stem>.train_state`` and, with an EMA, ``<stem>_ema.ckpt``: the same format with the averaged
        generator (buffers outside the arena, BatchNorm running statistics among them, are the live ones)."""
        if self.model_dir and self.dist.rank == 0:
            torch.save(obj, os.path.join(self.model_dir, name))
            stem = name[:-len(".ckpt")] if name.endswith(".ckpt") else name
            torch.save(self.train_state(), os.path.join(self.model_dir, stem + ".train_state"))
            if self.ema is not None:
                with self.ema.swapped():
                    gen = self.gen.state_dict()
                    avg = dict(obj, generator=gen) if set(obj) == {"generator", "discriminator"} else gen
                    torch.save(avg, os.path.join(self.model_dir, stem + "_ema.ckpt"))

    # ------------------------------------------------------------------ self-critical sequence training (scst.py)
    def scst_train(self, epochs):
        """``epochs`` SCST epochs over the training images (grouped by image, --adv-train-batch-size images per step): CIDEr-D
        rewards with df from the training references, or the mix of --scst-cider-weight / --scst-bleu-weight / --scst-rouge-weight
        (``scst_reward_scorer``).  After each epoch the greedy CIDEr-D on val decides whether the generator is
        saved as ``scst_model.ckpt`` (the generator's state dict: --resume loads it as pretrained weights).  Returns the best val
        CIDEr-D."""
        from .cider import RefBatch
        from .scst import SCSTStep
        from .tasks import ImageGroups
        args = self.args
        groups = ImageGroups(self.train_dataset)
        step = SCSTStep(self, scst_reward_scorer(args, groups.references()), int(getattr(args, "scst_samples", 5)),
                        getattr(args, "scst_baseline", "greedy"), float(getattr(args, "scst_lr", 5e-5)))
        self.scst_opt = step.opt
        if self._train_state is not None and "scst_opt" in self._train_state:
            step.opt.load_state_dict(self._train_state["scst_opt"])
        dp = self.dist.world_size > 1
        loader = DataLoader(groups, shuffle=not dp, batch_size=args.adv_train_batch_size,
                            collate_fn=make_collate(self.train_dataset, groups=True),
                            num_workers=int(getattr(args, "num_workers", 4)),
                            sampler=parallel.shard_sampler(groups, self.dist, True) if dp else None)
        L = int(args.max_seq_len)
        best = None
        self.log.info("Starting SCST (%d samples, %s baseline)...", step.n, step.baseline)
        for epoch in range(epochs):
            self.gen.train()
            self._reshuffle(loader, "train")
            rewards = []
            with torch.enable_grad(), tqdm(total=len(groups), disable=self.dist.rank != 0) as progress:
                for images, (ids, lens, off, max_refs) in loader:
                    refs = RefBatch(ids, lens, off, max_refs).to(args.device)
                    out = step(images.to(args.device) if self.cgan else None, refs, L)
                    loss, r, b = torch.stack([out["loss"].float(), out["reward"], out["baseline"]]).tolist()   # the step's one sync
                    rewards.append(r)
                    self.writer.add_scalar("SCST_train_reward", r, self.scst_steps)
                    self.scst_steps += 1
                    progress.update(len(images) * self.dist.world_size)
                    progress.set_postfix(reward=r, baseline=b, loss=loss)
            self.gen.eval()
            with self._live_weights():         # checkpoint selection stays on the live weights
                val = self.evaluate_cider("val", beam_size=1) if self.dist.rank == 0 else 0.0
            self.writer.add_scalar("SCST_val_cider", val, epoch)
            if best is None or val > best:
                best = val
                self._save(self.gen.state_dict(), "scst_model.ckpt")
                self.log.info("Saving Best model [CIDEr-D = {}] at SCST epoch {}".format(best, epoch))
            self.log.info("[SCST] epoch %d: train reward %.4f | val CIDEr-D (greedy) %.4f", epoch, float(np.mean(rewards)), val)
            self.writer.flush()
        return best

    def _run(self):
        self.pretrain_generator(self.args.pretrain_epochs)
        if int(getattr(self.args, "scst_epochs", 0)) > 0:
            self.scst_train(int(self.args.scst_epochs))
        self.log.info("Starting Adversarial Training...")
        best_loss = None
        for adv_epoch in range(self.args.adv_epochs):
            self.adv_epoch = adv_epoch
            self.disc.train()
            self.gen.train()
            train_g_loss, train_d_loss = self.adv_loop("train")
            self.disc.eval()
            self.gen.eval()
            val_g_loss, val_d_loss = self.adv_loop("val")
            if best_loss is None or val_g_loss < best_loss:
                best_loss = val_g_loss
                self._save({"generator": self.gen.state_dict(), "discriminator": self.disc.state_dict()}, "adv_model.ckpt")
                self.log.info("Saving Best model [Gen Loss = {}] at Epoch {}".format(best_loss, adv_epoch))
            if adv_epoch % self.args.adv_log_step == 0 or adv_epoch == self.args.adv_epochs - 1:
                self.log.info("[ADV] epoch %d (temperature: %.4f):\n\t g_loss: %.4f | %.4f \n\t d_loss: %.4f | %.4f" % (
                    adv_epoch, self.gen.decoder.temperature, train_g_loss, val_g_loss, train_d_loss, val_d_loss))
            if int(getattr(self.args, "eval_beam_size", 0)) > 0 and self.dist.rank == 0:
                self.evaluate("val", beam_size=int(self.args.eval_beam_size))
            if int(getattr(self.args, "eval_cider_beam_size", 0)) > 0 and self.dist.rank == 0:
                self.evaluate_cider("val", beam_size=int(self.args.eval_cider_beam_size))
            if int(getattr(self.args, "eval_metrics_beam_size", 0)) > 0 and self.dist.rank == 0:
                self.evaluate_metrics("val", beam_size=int(self.args.eval_metrics_beam_size))
            if int(getattr(self.args, "eval_num_samples", 0)) > 0 and self.dist.rank == 0:
                self.evaluate_diversity("val", num_samples=int(self.args.eval_num_samples), top_k=int(getattr(self.args, "eval_top_k", 0)),
                                        top_p=float(getattr(self.args, "eval_top_p", 1.0)),
                                        temperature=float(getattr(self.args, "eval_sample_temperature", 1.0)))
            if int(getattr(self.args, "eval_match", 0)) and self.dist.rank == 0:
                self.evaluate_match("val")
            if int(getattr(self.args, "eval_retrieval", 0)) and self.dist.rank == 0:
                self.evaluate_retrieval("val", max_items=int(getattr(self.args, "eval_retrieval_items", 1000)))
            if int(getattr(self.args, "eval_perplexity", 0)) and self.dist.rank == 0:
                self.evaluate_perplexity("val")
            if int(getattr(self.args, "eval_diverse_beam_size", 0)) > 0 and self.dist.rank == 0:
                self.evaluate_diverse_beam("val", beam_size=int(self.args.eval_diverse_beam_size),
                                           groups=int(getattr(self.args, "eval_diverse_groups", 2)),
                                           diversity=float(getattr(self.args, "eval_diversity_strength", 0.5)))
            if self.eval_forced is not None and self.dist.rank == 0:
                self.evaluate_forced("val", num_words=self.eval_forced[0], beam_size=self.eval_forced[1])
            if int(getattr(self.args, "eval_consensus_samples", 0)) > 0 and self.dist.rank == 0:
                self.evaluate_consensus("val", num_samples=int(self.args.eval_consensus_samples), top_k=int(getattr(self.args, "eval_top_k", 0)),
                                        top_p=float(getattr(self.args, "eval_top_p", 1.0)),
                                        temperature=float(getattr(self.args, "eval_sample_temperature", 1.0)),
                                        weight=float(getattr(self.args, "eval_consensus_weight", 1.0)))
            self.writer.flush()

    @_on_eval_weights
    def evaluate(self, what="val", beam_size=3, max_caption_len=None, batch_size=None):
        """BLEU-4 of beam-search captions against the dev (``what="val"``) or train captions: the captions are grouped by image
        (``filepath`` + ``filename`` for COCO_data, one image per item otherwise), every image is loaded and decoded once in eval
        mode, ids map through ``index_to_word`` with <S>, <E>, <PAD> stripped.  Captions are decoded up to ``max_caption_len``
        steps, by default max(args.max_seq_len, longest reference of the batch + 2): a batch's collate length, so that a short
        --max-seq-len cannot truncate every candidate below its references.  --eval-no-repeat-ngram / --eval-min-length /
        --eval-suppress-tokens constrain the decode (``_eval_constraints``), here and in the other evaluations.  Logs the score and
        writes the scalar ``BLEU4_<what>``."""
        from .utils import bleu_score
        words = self._eval_groups(what)[-1]
        cands, refs = [], []
        for ids, lengths, caps in self._beam_decode(what, beam_size, max_caption_len, batch_size):
            ids, lengths = ids.cpu(), lengths.cpu()
            for b, group in enumerate(caps):
                cands.append(words(ids[b, :int(lengths[b])].tolist()))
                refs.append([words(c) for c in group])
        score = bleu_score(cands, refs)
        self.log.info("[EVAL] BLEU-4 (%s, %s): %.4f", what, self._beam_label(beam_size), score)
        self.writer.add_scalar(f"BLEU4_{what}", score, max(self.adv_epoch, 0))
        return score

    @_on_eval_weights
    def evaluate_match(self, what="val"):
        """Image-caption match of the conditioned D (--disc-cond projection) over the adversarial eval (``what="val"``) or train loader:
        per caption the match term F^-1/2 <y, q> (mean over the representations) with its own image against the batch's next image
        (rolled by one).  Returns {"pair_acc": the share of captions whose own image scores strictly higher (a tie is no win),
        "margin": the mean difference}.  Per batch one eval forward of D (forward only) and two gic_disc_match_fwd; the sums stay on the
        device and are read with one sync.  Logs the values and writes the scalars ``MatchAcc_<what>`` / ``MatchMargin_<what>``."""
        if self.disc.cond != "projection":
            raise ValueError("evaluate_match needs a discriminator built with --disc-cond projection")
        loader = self.adv_eval_loader if what == "val" else self.adv_train_loader
        dev = self.args.device
        den = self.disc.engine()
        R = int(self.args.disc_num_rep)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)           # wins, sum of differences
        n = 0
        with torch.no_grad():
            dparams = [p.detach() for p in self.disc.text_param_list()]
            wp, bp = self.disc.img_proj.weight.detach(), self.disc.img_proj.bias.detach()
            for batch in loader:
                images, captions = batch[0].to(dev), batch[1].to(dev)
                main = torch.cuda.current_stream(images.device)
                q, _ = den.img_proj_fwd(wp, bp, self.gen.encoder.take_trunk(images, False, main))
                _, st = den.fwd(dparams, None, captions, False, forward_only=True)
                own = den.match_logits(st, q).view(-1, R).mean(1)
                other = den.match_logits(st, torch.roll(q, -1, 0)).view(-1, R).mean(1)
                diff = (own - other).double()
                sums += torch.stack([(diff > 0).sum().double(), diff.sum()])
                n += captions.shape[0]
        wins, total = sums.tolist() if n else (0.0, 0.0)                  # the one sync
        out = {"pair_acc": wins / n if n else 0.0, "margin": total / n if n else 0.0}
        self.log.info("[EVAL] match (%s): pair accuracy %.4f | margin %.6f", what, out["pair_acc"], out["margin"])
        step = max(self.adv_epoch, 0)
        self.writer.add_scalar(f"MatchAcc_{what}", out["pair_acc"], step)
        self.writer.add_scalar(f"MatchMargin_{what}", out["margin"], step)
        return out

    @_on_eval_weights
    def evaluate_perplexity(self, what="val"):
        """Teacher-forced per-token perplexity of the generator over the pre-training eval (``what="val"``) or train loader: one
        decoder.log_likelihood per batch (features as pretrain_step forms them, with the generator in eval mode for the pass, whatever mode
        it was in, and put back afterwards; no label smoothing), the captions' negative
        log-likelihoods and token counts (the positions t < length, <S> and <E> included) summed on the device and read with one
        sync.  Returns {"nll_per_token", "perplexity" = exp(sum nll / sum tokens), "tokens", "captions"}; logs them and writes the scalar
        ``Perplexity_<what>``."""
        loader = self.pre_eval_loader if what == "val" else self.pre_train_loader
        dev = self.args.device
        sums = torch.zeros(2, dtype=torch.float64, device=dev)           # nll, tokens
        n = 0
        gen = self._eval_gen()
        was_training = gen.training
        gen.eval()                                   # the encoder's BatchNorm on its running statistics, which stay as they are
        try:
            with torch.no_grad():
                for batch in loader:
                    images, captions, lengths = batch[0].to(dev), batch[1].to(dev), batch[2]
                    if gen is not self.gen:          # an ensemble scores through its own members' features
                        logp, tokens = gen.score_captions(images, captions, lengths)
                        sums += torch.stack([-logp.double().sum(), tokens.double().sum()])
                        n += captions.shape[0]
                        continue
                    feats = self._features(images, captions.shape[0])
                    if self.attention:
                        logp, tokens = self.gen.decoder.log_likelihood(feats[0], feats[1], captions, lengths)
                    else:
                        logp, tokens = self.gen.decoder.log_likelihood(feats, captions, lengths)
                    sums += torch.stack([-logp.double().sum(), tokens.double().sum()])
                    n += captions.shape[0]
        finally:
            gen.train(was_training)
        nll, tokens = sums.tolist() if n else (0.0, 0.0)                  # the one sync
        per_token = nll / tokens if tokens else 0.0
        out = {"nll_per_token": per_token, "perplexity": math.exp(per_token) if per_token < 700.0 else float("inf"),
               "tokens": int(tokens), "captions": n}
        self.log.info("[EVAL] perplexity (%s): %.4f | nll per token %.6f | %d tokens in %d captions", what, out["perplexity"],
                      out["nll_per_token"], out["tokens"], out["captions"])
        self.writer.add_scalar(f"Perplexity_{what}", out["perplexity"], self.adv_epoch if self.adv_epoch >= 0 else self.pretrain_steps)
        return out

    RETRIEVAL_MAX_ITEMS = 8192

    @_on_eval_weights
    def evaluate_retrieval(self, what="val", max_items=None):
        """Image-caption retrieval of the conditioned D (--disc-cond projection) over the first N = min(max_items, len) items of the
        adversarial eval (``what="val"``) or train loader (len = what the loader yields on this rank: its sampler's length, the shard
        under data parallelism); item i is (image i, caption i).  The pair score of caption c and image j is
        the mean over the representations of D's eval logit, T[c, j] = lbar[c] + F^-1/2 <ybar[c], q[j]> (linear in the logits).  Per
        batch one trunk pass, one img_proj_fwd, one forward-only D forward and one gic_disc_rep_mean into [N, F] / [N] buffers; at the
        end one f32 gic_gemm S = F^-1/2 Ybar Q^T, one gic_match_ranks and one sync.  A tie or a NaN counts against the true pair.
        Returns {"n": N, "c2i": {"r1", "r5", "r10", "medr", "meanr"}, "i2c": {...}} (caption -> image and image -> caption, recalls as
        fractions, ranks 1-based); logs them and writes the scalars ``Retr_c2i_R1_<what>`` ...  Refuses (ValueError, before anything
        runs) a D without --disc-cond projection, --captions-per-image != 1 (a repeated image ties with itself) and N > 8192."""
        from .metrics import retrieval_summary
        if self.disc.cond != "projection":
            raise ValueError("evaluate_retrieval needs a discriminator built with --disc-cond projection")
        if int(getattr(self.args, "captions_per_image", 1)) != 1:
            raise ValueError("evaluate_retrieval needs --captions-per-image 1: a repeated image ties with itself, and every tie counts "
                             "against the true pair")
        loader = self.adv_eval_loader if what == "val" else self.adv_train_loader
        N = self._loader_items(loader)
        N = N if max_items is None else min(int(max_items), N)
        if N > self.RETRIEVAL_MAX_ITEMS:
            raise ValueError(f"evaluate_retrieval: {N} items exceed {self.RETRIEVAL_MAX_ITEMS} (the score matrix would be "
                             f"{4 * N * N / 1e6:.0f} MB): set max_items / --eval-retrieval-items")
        if N < 1:
            raise ValueError("evaluate_retrieval: no items")
        dev = self.args.device
        den = self.disc.engine()
        nF = den.F
        ybar = torch.empty(N, nF, dtype=torch.float32, device=dev)
        lbar = torch.empty(N, dtype=torch.float32, device=dev)
        qall = torch.empty(N, nF, dtype=torch.float32, device=dev)
        n = 0
        with torch.no_grad():
            dparams = [p.detach() for p in self.disc.text_param_list()]
            wp, bp = self.disc.img_proj.weight.detach(), self.disc.img_proj.bias.detach()
            for batch in loader:
                if n >= N:
                    break
                k = min(int(batch[1].shape[0]), N - n)
                images, captions = batch[0][:k].to(dev), batch[1][:k].to(dev)
                main = torch.cuda.current_stream(images.device)
                den.img_proj_fwd(wp, bp, self.gen.encoder.take_trunk(images, False, main), out=qall[n:n + k])
                logits, st = den.fwd(dparams, None, captions, False, forward_only=True)
                den.rep_mean(st, logits, ybar=ybar[n:n + k], lbar=lbar[n:n + k])
                n += k
            if n < 1:
                raise ValueError("evaluate_retrieval: the loader gave no items")
            if n < N:                                                    # a loader that yields fewer items than it announced: rank those
                self.log.info("[EVAL] retrieval (%s): the loader gave %d of %d items", what, n, N)
                N, ybar, lbar, qall = n, ybar[:n], lbar[:n], qall[:n]
            S = torch.empty(N, N, dtype=torch.float32, device=dev)
            engine.gemm(ybar, qall, S, N, N, nF, nF, nF, N, True, True, alpha=den.match_scale())
            c2i, i2c = engine.match_ranks(S, lbar)
            ranks = torch.stack([c2i, i2c]).cpu()                        # the one sync
        out = {"n": N, "c2i": retrieval_summary(ranks[0]), "i2c": retrieval_summary(ranks[1])}
        step = max(self.adv_epoch, 0)
        for d in ("c2i", "i2c"):
            o = out[d]
            self.log.info("[EVAL] retrieval %s (%s, %d items): R@1 %.4f | R@5 %.4f | R@10 %.4f | median rank %.1f | mean rank %.2f",
                          d, what, N, o["r1"], o["r5"], o["r10"], o["medr"], o["meanr"])
            for name, key in (("R1", "r1"), ("R5", "r5"), ("R10", "r10"), ("MedR", "medr"), ("MeanR", "meanr")):
                self.writer.add_scalar(f"Retr_{d}_{name}_{what}", o[key], step)
        return out

    @staticmethod
    def _loader_items(loader) -> int:
        """The items ``loader`` will yield on this rank: the length of its sampler where it has one (under data parallelism the
        DistributedSampler's shard, not the dataset), else of its dataset, else counted from its batches."""
        for name in ("sampler", "dataset"):
            src = getattr(loader, name, None)
            if src is not None and hasattr(src, "__len__"):
                return len(src)
        return sum(int(b[1].shape[0]) for b in loader)

    def _eval_constraints(self):
        """The decode constraints of every evaluation (--eval-no-repeat-ngram, --eval-min-length, --eval-suppress-tokens) as the
        keywords of Generator.caption / sample_captions."""
        return dict(no_repeat_ngram=int(getattr(self.args, "eval_no_repeat_ngram", 0) or 0),
                    min_length=int(getattr(self.args, "eval_min_length", 0) or 0),
                    suppress_tokens=tuple(int(v) for v in (getattr(self.args, "eval_suppress_tokens", ()) or ())))

    def _eval_rerank(self):
        """--eval-rerank-weight as the keywords of Generator.caption: nothing when it is 0 (the search's own order, no D pass)."""
        w = float(getattr(self.args, "eval_rerank_weight", 0.0) or 0.0)
        return dict(rerank_disc=self.disc, rerank_weight=w) if w != 0.0 else {}

    def _beam_label(self, beam_size):
        """'beam k' of the evaluations' log lines, with the re-rank weight next to it when one is set."""
        w = float(getattr(self.args, "eval_rerank_weight", 0.0) or 0.0)
        return "beam %d" % beam_size if w == 0.0 else "beam %d, rerank weight %g" % (beam_size, w)

    def _beam_decode(self, what, beam_size, max_caption_len=None, batch_size=None):
        """The decode of ``evaluate`` / ``evaluate_cider``: the best beam of each image (``_decode_batches``)."""
        def decode(images, L, _):
            ids, _, lengths = self._eval_gen().caption(images, beam_size=beam_size, max_caption_len=L, **self._eval_constraints(),
                                                        **self._eval_rerank())
            return ids, lengths
        return self._decode_batches(what, decode, max_caption_len, batch_size)

    def _decode_batches(self, what, decode, max_caption_len=None, batch_size=None, with_caps=False):
        """The decode loop of the evaluations: every image of the split once (``_eval_groups``), the generator in eval mode;
        ``decode(images, L, batch_index)`` gives (ids, lengths) of the batch (``with_caps``: decode(images, L, batch_index, the
        images' reference token lists)).  Yields per batch (ids and lengths on the device, the images' reference token lists)."""
        ds, groups, order, coco, coco_ids, _ = self._eval_groups(what)
        gen = self._eval_gen()
        was_training = gen.training
        gen.eval()
        bs = int(batch_size or getattr(self.args, "adv_eval_batch_size", 32))
        try:
            for bi, s in enumerate(range(0, len(order), bs)):
                keys = order[s:s + bs]
                firsts = [ds[groups[k][0]] for k in keys]          # one image load per image
                images = stack_images([it[0] for it in firsts], getattr(ds, "image_size", None)).to(self.args.device)
                caps = [[coco_ids(ds.captions[j]) for j in groups[k]] if coco else [it[1]] for k, it in zip(keys, firsts)]
                L = max_caption_len or max(int(getattr(self.args, "max_seq_len", 0) or 0),
                                           max(len(c) for group in caps for c in group) + 2)
                ids, lengths = decode(images, L, bi, caps) if with_caps else decode(images, L, bi)
                yield ids, lengths, caps
        finally:
            gen.train(was_training)

    @_on_eval_weights
    def evaluate_cider(self, what="val", beam_size=3, max_caption_len=None, batch_size=None):
        """CIDEr-D of the beam-search captions of ``evaluate`` (the same images, grouping and caption length rule), scored on the GPU
        (gic_cider_d) with document frequencies from the evaluated split's references (the coco-caption convention).  Logs the score
        and writes the scalar ``CIDErD_<what>``."""
        from .cider import CiderD, RefBatch
        from .tasks import ImageGroups
        if what not in self._cider:
            ds = self.dev_dataset if what == "val" else self.train_dataset
            self._cider[what] = CiderD(ImageGroups(ds).references(), self.args.vocab_size, self.args.device)
        scorer = self._cider[what]
        scores = []
        for ids, lengths, caps in self._beam_decode(what, beam_size, max_caption_len, batch_size):
            scores.append(scorer.score(ids, lengths, RefBatch.pack(caps).to(self.args.device)))
        score = float(torch.cat(scores).double().mean()) if scores else 0.0
        self.log.info("[EVAL] CIDEr-D (%s, %s): %.4f", what, self._beam_label(beam_size), score)
        self.writer.add_scalar(f"CIDErD_{what}", score, max(self.adv_epoch, 0))
        return score

    @_on_eval_weights
    def evaluate_metrics(self, what="val", beam_size=3, max_caption_len=None, batch_size=None):
        """The metrics table of the beam-search captions of ``evaluate`` (the same images, grouping, caption length rule and decode
        constraints) from ONE decode pass, scored on the GPU: per batch one gic_caption_overlap launch (metrics.OverlapScorer) and one
        gic_cider_d launch (the scorer of ``evaluate_cider``); the BLEU statistics accumulate on the device in int64 and the sums are
        read with one sync at the end.  Returns {"bleu1", "bleu2", "bleu3", "bleu4", "rouge_l", "cider_d"}: corpus BLEU-n
        (metrics.corpus_bleu), mean ROUGE-L and mean CIDEr-D.  Logs them on one line and writes the scalars ``BLEU1M_<what>`` ..
        ``BLEU4M_<what>``, ``ROUGEL_<what>`` and ``CIDErDM_<what>``."""
        from .cider import CiderD, RefBatch
        from .metrics import STAT_COLUMNS, OverlapScorer, corpus_bleu
        from .tasks import ImageGroups
        dev = self.args.device
        if what not in self._cider:                                          # the scorer of evaluate_cider, and its cache
            ds = self.dev_dataset if what == "val" else self.train_dataset
            self._cider[what] = CiderD(ImageGroups(ds).references(), self.args.vocab_size, dev)
        cider = self._cider[what]
        overlap = OverlapScorer(self.args.vocab_size, dev)
        stats = torch.zeros(len(STAT_COLUMNS), dtype=torch.int64, device=dev)
        rouge, cd = [], []
        for ids, lengths, caps in self._beam_decode(what, beam_size, max_caption_len, batch_size):
            refs = RefBatch.pack(caps).to(dev)
            st, rl, _ = overlap.score(ids, lengths, refs)
            rouge.append(rl)
            cd.append(cider.score(ids, lengths, refs))
            stats += st.sum(0, dtype=torch.int64)
        if rouge:                                                            # the one sync: the sums (exact in float64) and the two means
            means = torch.stack([torch.cat(rouge).double().mean(), torch.cat(cd).double().mean()])
            *sums, rouge_l, cider_d = torch.cat([stats.double(), means]).tolist()
        else:
            sums, rouge_l, cider_d = [0] * len(STAT_COLUMNS), 0.0, 0.0
        bleu = corpus_bleu(sums)
        out = {"bleu1": bleu[0], "bleu2": bleu[1], "bleu3": bleu[2], "bleu4": bleu[3], "rouge_l": rouge_l, "cider_d": cider_d}
        self.log.info("[EVAL] metrics (%s, %s): BLEU-1 %.4f | BLEU-2 %.4f | BLEU-3 %.4f | BLEU-4 %.4f | ROUGE-L %.4f | CIDEr-D %.4f",
                      what, self._beam_label(beam_size), out["bleu1"], out["bleu2"], out["bleu3"], out["bleu4"], out["rouge_l"], out["cider_d"])
        step = max(self.adv_epoch, 0)
        for name, key in (("BLEU1M", "bleu1"), ("BLEU2M", "bleu2"), ("BLEU3M", "bleu3"), ("BLEU4M", "bleu4"), ("ROUGEL", "rouge_l"),
                          ("CIDErDM", "cider_d")):
            self.writer.add_scalar(f"{name}_{what}", out[key], step)
        return out

    @staticmethod
    def oracle_tags(refs, n, df, barred=()):
        """The oracle-tags protocol's forced words of one image: among the tokens that occur in at least half of its references
        ``refs`` (token lists) and are not ``barred``, the ``n`` with the lowest document frequency ``df`` {token: count}, ties to the
        lower id.  Fewer than ``n`` such tokens give fewer words."""
        counts = {}
        for r in refs:
            for t in set(int(v) for v in r):
                counts[t] = counts.get(t, 0) + 1
        ok = [t for t, c in counts.items() if 2 * c >= len(refs) and t not in barred]
        return sorted(ok, key=lambda t: (df.get(t, 0), t))[:int(n)]

    @_on_eval_weights
    def evaluate_forced(self, what="val", num_words=1, beam_size=8, length_penalty=0.0, max_caption_len=None, batch_size=None):
        """The forced-words evaluation (--eval-force-words N, --eval-force-beam-size K), the "oracle tags" protocol of Anderson et al.
        (2017): per image of ``evaluate`` the ``num_words`` reference tokens of ``oracle_tags`` (document frequencies from the CiderD
        table of ``evaluate_cider``; the specials and the suppressed ids are barred) are forced into the caption by lexically constrained
        beam search (Generator.caption force_words; one constraint per word), next to plain beam search of the same ``beam_size``.
        The decode constraints of the evaluations apply to both.  Returns {"bleu4", "cider_d": corpus BLEU-4 and mean CIDEr-D of the
        forced search's best captions, scored on the GPU as in ``evaluate_metrics``; "satisfied": the share of images whose best forced
        caption holds all its words; "satisfied_plain": the same share for plain beam search}.  The sums stay on the device and are read
        with one sync at the end; the words are chosen on the host from the scorer's host copy of its table, and the ids are checked on
        the host before they are uploaded.  The plain search runs for every batch; a batch in which no image has a word to force runs
        it alone and counts its captions as the forced ones.  Logs them and
        writes the scalars ``BLEU4F_<what>``, ``CIDErDF_<what>``, ``ForcedSat_<what>``, ``PlainSat_<what>``."""
        from .cider import CiderD, RefBatch, unigram_df
        from .metrics import STAT_COLUMNS, OverlapScorer, corpus_bleu
        from .tasks import SPECIALS, ImageGroups
        N, K = int(num_words), int(beam_size)
        if not 1 <= N <= 3 or K % (1 << N):
            raise ValueError(f"evaluate_forced: num_words must be 1..3 and 2^num_words must divide beam_size, got {N} and {K}")
        gen = self._eval_gen()
        if gen is not self.gen:
            raise ValueError("evaluate_forced with an ensemble: the forced search runs one model")
        dev = self.args.device
        ds = self.dev_dataset if what == "val" else self.train_dataset
        if what not in self._cider:
            self._cider[what] = CiderD(ImageGroups(ds).references(), self.args.vocab_size, dev)
        cider = self._cider[what]
        df = unigram_df(cider.keys_host, cider.df)                   # (the table's host copy: no device read)
        cons = self._eval_constraints()
        barred = {ds.word_to_index[w] for w in SPECIALS if w in ds.word_to_index} | {0, 1, 2} | set(cons["suppress_tokens"])
        overlap = OverlapScorer(self.args.vocab_size, dev)
        stats = torch.zeros(len(STAT_COLUMNS), dtype=torch.int64, device=dev)
        sat = torch.zeros(2, dtype=torch.int64, device=dev)             # images satisfied: forced, plain
        cd, n_img = [], 0

        def held(ids, lengths, tags):
            pos = torch.arange(ids.shape[1], device=ids.device)[None, :, None] < lengths.long()[:, None, None]
            return (((ids[:, :, None] == tags[:, None, :]) & pos).any(1) | (tags < 0)[:, :]).all(1)

        def decode(images, L, bi, caps):
            words = [self.oracle_tags(group, N, df, barred) for group in caps]
            tags = torch.full((len(caps), N), -1, dtype=torch.int32)
            for b, w in enumerate(words):
                tags[b, :len(w)] = torch.tensor(w, dtype=torch.int32)
            pid, _, plen = gen.caption(images, beam_size=K, max_caption_len=L, length_penalty=length_penalty, **cons)
            tags_d = tags.to(dev)
            if any(words):
                ids, _, lengths, met = gen.caption(images, beam_size=K, max_caption_len=L, length_penalty=length_penalty,
                                                   force_words=tags[:, :, None].contiguous(), return_met=True, **cons)   # (host ids: checked without a sync)
                ok = met == (1 << N) - 1
            else:                                                        # no image of the batch has a word to force: the plain search
                ids, lengths = pid, plen
                ok = torch.ones(len(caps), dtype=torch.bool, device=dev)
            sat.add_(torch.stack([ok.sum(), held(pid, plen, tags_d.long()).sum()]))
            return ids, lengths

        for ids, lengths, caps in self._decode_batches(what, decode, max_caption_len, batch_size, with_caps=True):
            refs = RefBatch.pack(caps).to(dev)
            st, _, _ = overlap.score(ids, lengths, refs)
            cd.append(cider.score(ids, lengths, refs))
            stats += st.sum(0, dtype=torch.int64)
            n_img += len(caps)
        if cd:                                                           # the one sync
            *sums, fs, ps, cider_d = torch.cat([stats.double(), sat.double(), torch.cat(cd).double().mean()[None]]).tolist()
        else:
            sums, fs, ps, cider_d = [0] * len(STAT_COLUMNS), 0.0, 0.0, 0.0
        out = {"bleu4": corpus_bleu(sums)[3], "cider_d": cider_d, "satisfied": fs / n_img if n_img else 0.0,
               "satisfied_plain": ps / n_img if n_img else 0.0}
        self.log.info("[EVAL] forced words (%s, %d words, beam %d): BLEU-4 %.4f | CIDEr-D %.4f | satisfied %.4f | plain beam satisfied %.4f",
                      what, N, K, out["bleu4"], out["cider_d"], out["satisfied"], out["satisfied_plain"])
        step = max(self.adv_epoch, 0)
        for name, key in (("BLEU4F", "bleu4"), ("CIDErDF", "cider_d"), ("ForcedSat", "satisfied"), ("PlainSat", "satisfied_plain")):
            self.writer.add_scalar(f"{name}_{what}", out[key], step)
        return out

    def _eval_groups(self, what):
        """The evaluation's dataset and its captions grouped by image (``filepath`` + ``filename`` for COCO_data, one image per item
        otherwise): (ds, groups {key: [item]}, keys in first-seen order, is_coco, a COCO entry's token ids as __getitem__ forms them
        (no image load), ids -> words with <S>, <E>, <PAD> stripped)."""
        from .tasks import COCO_data, SPECIALS, group_by_image
        ds = self.dev_dataset if what == "val" else self.train_dataset
        groups, order = group_by_image(ds)
        coco = isinstance(ds, COCO_data)
        unk = ds.word_to_index.get("<UNK>", 3)
        coco_ids = lambda e: [t if isinstance(t, int) else ds.word_to_index.get(t, unk) for t in e["tokens"]]   # noqa: E731
        i2w = ds.index_to_word
        strip = {ds.word_to_index[w] for w in SPECIALS[:3] if w in ds.word_to_index}
        words = lambda ids: [i2w.get(int(t), str(int(t))) for t in ids if int(t) not in strip]   # noqa: E731
        return ds, groups, order, coco, coco_ids, words

    @_on_eval_weights
    def evaluate_diversity(self, what="val", num_samples=5, top_k=0, top_p=1.0, temperature=1.0, seed=1234, max_caption_len=None,
                           batch_size=None):
        """Caption diversity of ``num_samples`` sampled captions per image (Generator.sample_captions), on the images of ``evaluate``
        (grouped and loaded once each, the generator in eval mode, the same caption length rule): ``bleu4`` = BLEU-4 of each image's
        first sample against its references, ``mbleu4`` = each sample against the other samples of its image (lower = more diverse),
        ``distinct1`` / ``distinct2`` = unique / total uni- and bigrams over all samples, ``vocab`` = distinct words used.  Logs the
        values and writes the scalars ``<Name>_<what>`` (BLEU4S, mBLEU4, Distinct1, Distinct2, Vocab).  ``seed`` fixes the draws."""
        def decode(images, L, bi):
            ids, _, lengths = self._eval_gen().sample_captions(images, num_samples=num_samples, top_k=top_k, top_p=top_p, temperature=temperature,
                                                               max_caption_len=L, seed=int(seed) + bi, **self._eval_constraints())
            return ids, lengths
        out = self._diversity(what, decode, max_caption_len, batch_size)
        self.log.info("[EVAL] diversity (%s, n %d, top-k %d, top-p %.3f, temperature %.3f): BLEU-4 %.4f | mBLEU-4 %.4f | distinct-1 %.4f"
                      " | distinct-2 %.4f | vocab %d", what, num_samples, top_k, top_p, temperature, out["bleu4"], out["mbleu4"],
                      out["distinct1"], out["distinct2"], out["vocab"])
        self._write_diversity(out, what, ("BLEU4S", "mBLEU4", "Distinct1", "Distinct2", "Vocab"))
        return out

    @_on_eval_weights
    def evaluate_diverse_beam(self, what="val", beam_size=4, groups=2, diversity=0.5, length_penalty=0.0, max_caption_len=None,
                              batch_size=None):
        """The metrics of ``evaluate_diversity`` for the ``beam_size`` captions per image of diverse beam search (Generator.caption
        with ``groups`` groups and the Hamming penalty ``diversity``), on the same images with the same caption length rule:
        ``bleu4`` of slot 0 (group 0's best beam), ``mbleu4`` / ``distinct1`` / ``distinct2`` / ``vocab`` over the beams.  Logs the
        values and writes the scalars ``<Name>_<what>`` (BLEU4DBS, mBLEU4DBS, Distinct1DBS, Distinct2DBS, VocabDBS)."""
        def decode(images, L, _):
            ids, _, lengths = self._eval_gen().caption(images, beam_size=beam_size, max_caption_len=L, length_penalty=length_penalty,
                                                       return_beams=True, beam_groups=groups, diversity=diversity, **self._eval_constraints())
            return ids, lengths
        out = self._diversity(what, decode, max_caption_len, batch_size)
        self.log.info("[EVAL] diverse beam (%s, beam %d, groups %d, diversity %.3f): BLEU-4 %.4f | mBLEU-4 %.4f | distinct-1 %.4f"
                      " | distinct-2 %.4f | vocab %d", what, beam_size, groups, diversity, out["bleu4"], out["mbleu4"],
                      out["distinct1"], out["distinct2"], out["vocab"])
        self._write_diversity(out, what, ("BLEU4DBS", "mBLEU4DBS", "Distinct1DBS", "Distinct2DBS", "VocabDBS"))
        return out

    @_on_eval_weights
    def evaluate_consensus(self, what="val", num_samples=8, top_k=0, top_p=1.0, temperature=1.0, weight=1.0, seed=1234, max_caption_len=None,
                           batch_size=None):
        """Consensus (minimum-Bayes-risk) selection among ``num_samples`` sampled captions per image, and their Self-CIDEr diversity, on
        the images, grouping, caption length rule and decode constraints of ``evaluate``, all scored on the GPU.  Per batch: one
        sample_captions pass, one gic_cider_pairwise launch (each sample's consensus = its mean CIDEr-D against the image's other
        samples, and the set's Self-CIDEr), the pick = the first of gic_rerank's order under log-probability + ``weight`` * consensus,
        and one gic_cider_d launch (the scorer of ``evaluate_cider``) over the first draw and the pick.  Returns {"cider_d_first": the
        mean CIDEr-D of the first draw, "cider_d_consensus": of the pick, "self_cider": the mean Self-CIDEr}; the sums accumulate on
        the device and are read with one sync at the end.  Logs them on one line and writes the scalars ``CIDErDFirst_<what>``,
        ``CIDErDConsensus_<what>`` and ``SelfCIDEr_<what>``.  ``seed`` fixes the draws."""
        from .cider import CiderD, RefBatch
        from .tasks import ImageGroups
        dev = self.args.device
        if what not in self._cider:                                          # the scorer of evaluate_cider, and its cache
            ds = self.dev_dataset if what == "val" else self.train_dataset
            self._cider[what] = CiderD(ImageGroups(ds).references(), self.args.vocab_size, dev)
        scorer = self._cider[what]
        drawn = {}

        def decode(images, L, bi):
            ids, drawn["scores"], lengths = self._eval_gen().sample_captions(images, num_samples=num_samples, top_k=top_k, top_p=top_p,
                                                                             temperature=temperature, max_caption_len=L, seed=int(seed) + bi,
                                                                             **self._eval_constraints())
            return ids, lengths
        sums = torch.zeros(3, dtype=torch.float64, device=dev)              # CIDEr-D of the first draw, of the pick, Self-CIDEr
        n_images = 0
        for ids, lengths, caps in self._decode_batches(what, decode, max_caption_len, batch_size):
            pw = scorer.pairwise(ids, lengths, want_matrix=False)
            r = engine.rerank(drawn["scores"], lengths, pw["consensus"].view(-1), 1, float(weight), 0.0, ids=ids)
            cand = torch.stack([ids[:, 0], r["ids"][:, 0]], 1)
            cand_len = torch.stack([lengths[:, 0], r["lengths"][:, 0]], 1)
            cd = scorer.score(cand, cand_len, RefBatch.pack(caps).to(dev))
            sums += torch.cat([cd.double().sum(0), pw["self_cider"].double().sum().view(1)])
            n_images += ids.shape[0]
        first, picked, self_cider = (sums / max(n_images, 1)).tolist()         # the one sync
        out = {"cider_d_first": first, "cider_d_consensus": picked, "self_cider": self_cider}
        self.log.info("[EVAL] consensus (%s, n %d, top-k %d, top-p %.3f, temperature %.3f, weight %g): CIDEr-D first %.4f | CIDEr-D consensus"
                      " %.4f | Self-CIDEr %.4f", what, num_samples, top_k, top_p, temperature, weight, first, picked, self_cider)
        step = max(self.adv_epoch, 0)
        for name, key in (("CIDErDFirst", "cider_d_first"), ("CIDErDConsensus", "cider_d_consensus"), ("SelfCIDEr", "self_cider")):
            self.writer.add_scalar(f"{name}_{what}", out[key], step)
        return out

    def _diversity(self, what, decode, max_caption_len, batch_size):
        """The metrics of ``evaluate_diversity`` over the captions [b, n, L] that ``decode`` gives per batch (``_decode_batches``)."""
        from .utils import bleu_score, distinct_n, mbleu4
        words = self._eval_groups(what)[-1]
        firsts_c, refs, samples = [], [], []
        for ids, lengths, caps in self._decode_batches(what, decode, max_caption_len, batch_size):
            ids, lengths = ids.cpu(), lengths.cpu()
            for b, group in enumerate(caps):
                smp = [words(ids[b, j, :int(lengths[b, j])].tolist()) for j in range(ids.shape[1])]
                samples.append(smp)
                firsts_c.append(smp[0])
                refs.append([words(c) for c in group])
        flat = [c for group in samples for c in group]
        return {"bleu4": bleu_score(firsts_c, refs), "mbleu4": mbleu4(samples), "distinct1": distinct_n(flat, 1),
                "distinct2": distinct_n(flat, 2), "vocab": len({w for c in flat for w in c})}

    def _write_diversity(self, out, what, names):
        step = max(self.adv_epoch, 0)
        for name, key in zip(names, ("bleu4", "mbleu4", "distinct1", "distinct2", "vocab")):
            self.writer.add_scalar(f"{name}_{what}", out[key], step)


class _XentFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean over all rows, PAD included; training.py:81-83) via gic_xent."""

    @staticmethod
    def forward(ctx, logits, targets):
        loss, dlog = engine.xent(logits.detach().contiguous(), targets, want_grad=ctx.needs_input_grad[0])
        ctx.dlog = dlog
        return loss[0]

    @staticmethod
    def backward(ctx, d):
        return ctx.dlog * d, None


class _SeqXentFn(torch.autograd.Function):
    """F.cross_entropy(ignore_index, label_smoothing) over the counted rows via gic_xent_seq (engine.xent_seq): returns (loss, cap_nll
    [rows / group], cap_tokens [rows / group]); only the loss is differentiable."""

    @staticmethod
    def forward(ctx, logits, targets, group, lengths=None, ignore_index=-100, smoothing=0.0):
        out = engine.xent_seq(logits.detach().contiguous(), targets, group, lengths=lengths, ignore_index=ignore_index, smoothing=smoothing,
                              want_grad=ctx.needs_input_grad[0])
        ctx.dlog = out["d_logits"]
        ctx.mark_non_differentiable(out["cap_nll"], out["cap_tokens"])
        return out["loss"], out["cap_nll"], out["cap_tokens"]

    @staticmethod
    def backward(ctx, d, _d_nll, _d_tokens):
        return ctx.dlog * d, None, None, None, None, None
