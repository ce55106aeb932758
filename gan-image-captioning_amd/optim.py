"""Flat parameter arenas + fused clip_grad_norm_ / Adam (reference src/training.py:24-26,194-199).

A ``ParamArena`` re-homes a list of ``nn.Parameter``s into one contiguous float32 buffer (each
parameter becomes a view, so state-dicts / checkpoints keep the reference's keys) with a matching
flat gradient buffer.  One flat buffer per model means: one norm reduction, one Adam kernel, and one
RCCL all-reduce per optimizer under data parallelism.
"""
from __future__ import annotations

import contextlib
import math
from typing import Iterable, List, NamedTuple, Optional

import torch
import torch.nn as nn

from . import engine


def slot_ranges(params, predicate=lambda p: p.ndim >= 2) -> List[tuple]:
    """Half-open element ranges [start, end) of the padded arena slots of the parameters ``predicate`` selects, in a ParamArena of
    ``params``: sorted, adjacent slots merged, every boundary a multiple of 4 (the slots are 16-byte aligned).  The default takes
    matrices, embeddings and conv filters and leaves biases and BatchNorm affine parameters alone.  Shapes only: works on any device."""
    out: List[List[int]] = []
    off = 0
    for p in params:
        end = off + (p.numel() + 3) // 4 * 4
        if predicate(p):
            if out and out[-1][1] == off:
                out[-1][1] = end
            else:
                out.append([off, end])
        off = end
    return [tuple(r) for r in out]


class ParamArena:
    def __init__(self, params: Iterable[nn.Parameter]):
        self.params: List[nn.Parameter] = [p for p in params]
        if not self.params:
            raise ValueError("ParamArena needs at least one parameter")
        dev = self.params[0].device
        engine.require_gpu(*self.params)
        self.sizes = [p.numel() for p in self.params]
        # 16-byte aligned slots so every view can be a 16-B vector-load operand
        self.offsets, off = [], 0
        for n in self.sizes:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4
        self.numel = off
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o, n in zip(self.params, self.offsets, self.sizes):
                if p.dtype != torch.float32:
                    raise ValueError("master weights must be float32")
                view = self.flat[o:o + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[o:o + n].view(p.shape)
        engine.bump_param_epoch()

    def span(self, params) -> Optional[tuple]:
        """(start, end) of the arena slots of ``params`` if they are one contiguous run (in any order), else None."""
        want = {id(p) for p in params}
        idx = sorted(i for i, p in enumerate(self.params) if id(p) in want)
        if len(idx) != len(want) or not idx or idx != list(range(idx[0], idx[-1] + 1)):
            return None
        end = self.offsets[idx[-1] + 1] if idx[-1] + 1 < len(self.params) else self.numel
        return self.offsets[idx[0]], end

    def decay_ranges(self, predicate=lambda p: p.ndim >= 2) -> List[tuple]:
        """The arena ranges decoupled weight decay multiplies (``slot_ranges``): by default matrices, embeddings and conv filters."""
        return slot_ranges(self.params, predicate)

    def grad_views(self) -> List[torch.Tensor]:
        return [self.grad[o:o + n].view(p.shape) for p, o, n in zip(self.params, self.offsets, self.sizes)]

    def zero_grad(self) -> None:
        self.grad.zero_()
        for p, g in zip(self.params, self.grad_views()):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g


LR_SCHEDULES = ("none", "linear", "cosine", "invsqrt", "step")
MAX_DECAY_RANGES = 256          # GIC_ADAMW_MAX_RANGES


class LRSchedule(NamedTuple):
    """A learning-rate multiplier lambda(s) over the number s of completed optimizer steps (torch's LambdaLR: the t-th step uses
    lambda(t - 1)).  ``warmup`` W linear warm-up steps, ``total`` T the horizon (linear, cosine), ``min_ratio`` r the floor,
    ``step_size`` S and ``gamma`` of the step schedule.  The update kernel evaluates the same formulas on the device from its own
    step counter (gic_clip_adamw); ``multiplier`` restates them on the host in float64."""
    kind: str = "none"
    warmup: int = 0
    total: int = 0
    min_ratio: float = 0.0
    step_size: int = 0
    gamma: float = 0.1

    def validate(self) -> "LRSchedule":
        if self.kind not in LR_SCHEDULES:
            raise ValueError(f"LR schedule must be one of {'|'.join(LR_SCHEDULES)}, got {self.kind!r}")
        if self.warmup < 0:
            raise ValueError(f"LR warm-up steps must be >= 0, got {self.warmup}")
        if not 0.0 <= self.min_ratio <= 1.0:             # false for NaN too
            raise ValueError(f"the LR floor ratio must be in [0, 1], got {self.min_ratio}")
        if self.kind in ("linear", "cosine") and not self.total > self.warmup:
            raise ValueError(f"the {self.kind} LR schedule needs a horizon beyond its warm-up: {self.total} total steps, {self.warmup} warm-up steps")
        if self.kind == "step" and not (self.step_size > 0 and self.gamma > 0.0):
            raise ValueError(f"the step LR schedule needs a positive step size and gamma, got {self.step_size} and {self.gamma}")
        return self

    @property
    def neutral(self) -> bool:
        return self.kind == "none" and self.warmup == 0

    def multiplier(self, s: int) -> float:
        W, r = self.warmup, self.min_ratio
        if s < W:
            return (s + 1) / W
        u = s - W
        if self.kind == "linear":
            return r + (1.0 - r) * max(0.0, 1.0 - u / (self.total - W))
        if self.kind == "cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * min(1.0, u / (self.total - W))))
        if self.kind == "invsqrt":
            return max(r, math.sqrt(max(W, 1) / (s + 1)))
        if self.kind == "step":
            return max(r, self.gamma ** (u // self.step_size))
        return 1.0


class ArenaEMA:
    """Exponential moving average of an arena's parameters: one shadow buffer and one device update counter per arena, advanced
    inside the update kernel by whichever optimizer steps (pretrain_opt, gen_opt and SCST's optimizer share ``gen_arena``).  The
    k-th update (k from 0) uses d_k = min(decay, (1 + k) / (10 + k)) with ``warmup``, else ``decay``.  Buffers outside the arena
    (BatchNorm running statistics) are not averaged."""

    def __init__(self, arena: ParamArena, decay: float, warmup: bool = True):
        if not 0.0 <= decay < 1.0:                       # false for NaN too
            raise ValueError(f"the EMA decay must be in [0, 1), got {decay}")
        self.arena, self.decay, self.warmup = arena, float(decay), bool(warmup)
        self.shadow = arena.flat.clone()
        self.count = torch.zeros(1, dtype=torch.int64, device=arena.flat.device)

    def reset(self) -> None:
        self.shadow.copy_(self.arena.flat)
        self.count.zero_()

    def _exchange(self) -> None:
        tmp = self.arena.flat.clone()
        self.arena.flat.copy_(self.shadow)
        self.shadow.copy_(tmp)
        engine.bump_param_epoch()          # compute-dtype weight images are stale

    @contextlib.contextmanager
    def swapped(self):
        """The averaged weights in the live parameters for the duration of the block (pointers never change: the contents of
        ``arena.flat`` and the shadow are exchanged, and exchanged back on exit, also on an exception)."""
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def state_dict(self):
        return {"shadow": self.shadow, "count": self.count}

    def load_state_dict(self, sd) -> None:
        self.shadow.copy_(sd["shadow"])
        self.count.copy_(sd["count"])


class FusedClipAdam:
    """``opt.zero_grad(); loss.backward(); clip_grad_norm_(params, clip); opt.step()`` of the reference's
    ``optimize`` (training.py:194-199) with clip + Adam as two kernels over the arena.  Several optimizers
    may share one arena with separate moments (pretrain_opt / gen_opt, training.py:24-25).

    ``weight_decay`` (decoupled, torch.optim.AdamW) applies inside ``decay_ranges`` (default ``arena.decay_ranges()``),
    ``schedule`` (an ``LRSchedule``) scales ``lr`` on the device from the step counter, ``ema`` (an ``ArenaEMA`` of the same arena)
    is advanced by every step.  With all of them neutral ``step()`` is gic_clip_adam as before; otherwise gic_clip_adamw, still two
    launches.  ``lr`` stays the base rate either way."""

    def __init__(self, arena: ParamArena, lr: float, clip_norm: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decay_ranges=None, schedule: Optional[LRSchedule] = None, ema: Optional[ArenaEMA] = None):
        self.arena, self.lr, self.clip_norm, self.betas, self.eps = arena, lr, clip_norm, betas, eps
        if not weight_decay >= 0.0:                      # false for NaN too
            raise ValueError(f"weight decay must be >= 0, got {weight_decay}")
        if ema is not None and ema.arena is not arena:
            raise ValueError("the EMA belongs to another arena")
        self.weight_decay, self.ema = float(weight_decay), ema
        self.schedule = (schedule or LRSchedule()).validate()
        self.steps = 0                                   # host count of step() calls, for current_lr()
        dev = arena.flat.device
        self.exp_avg = torch.zeros_like(arena.flat)
        self.exp_avg_sq = torch.zeros_like(arena.flat)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)       # pre-clip global L2 norm of the last step
        self._partials = torch.zeros(engine.clip_adam_partials(arena.numel), dtype=torch.float32, device=dev)
        self._opts = None
        if self.weight_decay > 0.0 or not self.schedule.neutral or ema is not None:
            ranges = list(arena.decay_ranges() if decay_ranges is None else decay_ranges) if self.weight_decay > 0.0 else []
            if len(ranges) > MAX_DECAY_RANGES:
                raise ValueError(f"{len(ranges)} weight-decay ranges, at most {MAX_DECAY_RANGES} are accepted")
            flat = [int(x) for r in ranges for x in r]
            sc = self.schedule
            self.sched_out = torch.zeros(2, dtype=torch.float32, device=dev)    # lr_t and the EMA's 1 - d_k of the last step
            self._opts = engine.adamw_opts(
                self.weight_decay, flat, torch.tensor(flat, dtype=torch.int64, device=dev) if flat else None, sc.kind, sc.warmup,
                sc.total, sc.min_ratio, sc.step_size, sc.gamma, ema.shadow if ema else None, ema.count if ema else None,
                ema.decay if ema else 0.0, ema.warmup if ema else True, self.sched_out)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.arena.zero_grad()

    def step(self) -> None:
        a = self.arena
        args = (a.flat, a.grad, self.exp_avg, self.exp_avg_sq, self.lr, self.betas[0], self.betas[1], self.eps,
                self.clip_norm, self.step_count, self.grad_norm, self._partials)
        if self._opts is None:
            engine.clip_adam(*args)
        else:
            engine.clip_adamw(*args, self._opts)
        self.steps += 1

    def current_lr(self) -> float:
        """The learning rate of the next ``step()``: lr * lambda(steps so far), from the host's count of calls (no sync)."""
        return self.lr * self.schedule.multiplier(self.steps)

    def state_dict(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count, "lr": self.lr}

    def load_state_dict(self, sd) -> None:
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count.copy_(sd["step"])
        self.steps = int(sd["step"])                     # the schedule position follows the device counter
        self.lr = sd.get("lr", self.lr)
