"""Generator: Encoder / Decoder / Generator with the reference's module API
(src/generator.py:8-123) and state-dict key names, computing through libgicap.so.

Differences a caller can observe (all documented in DESIGN.md):
  * ``Decoder.sample`` returns its probabilities in the compute dtype (bf16 when
    ``--compute-dtype bf16``; float32 in parity mode), laid out [B, L, V] contiguous.
  * ``sample`` / ``Discriminator.forward`` take optional explicit noise (``noise_u``,
    ``keep_mask``) so a run can be replayed bit-for-bit against the CPU reference; without it
    noise comes from an on-device Philox stream seeded from ``torch.initial_seed()``.
  * ``Generator.forward`` reads ``args.conditional_gan`` (the reference reads a non-existent
    ``args.cgan``, generator.py:109, and is never called by training.py).
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn

from . import engine
from .trunk import ResNetTrunk, encoder_head_bwd, encoder_head_fwd


def _compute_dtype(args) -> int:
    return engine.parse_dtype(getattr(args, "compute_dtype", "bf16"))


class _SeedStream:
    """Host-side counter that hands a fresh Philox seed to every stochastic kernel launch."""

    def __init__(self):
        self._n = 0

    rank = 0        # data-parallel rank (set by GANInstructor): replicas draw DIFFERENT Gumbel noise / dropout masks

    def reset(self, n: int = 0) -> None:
        """Restart the counter (tests: two runs that must draw the same device noise)."""
        self._n = int(n)

    def next(self) -> int:
        self._n += 1
        return (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._n * 0xD1B54A32D192ED03
                + self.rank * 0xA0761D6478BD642F) & (2 ** 64 - 1)


SEEDS = _SeedStream()


# ------------------------------------------------------------------------------------------ embedding
class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, ids):
        ctx.save_for_backward(ids)
        ctx.vocab = weight.shape[0]
        return engine.embedding_fwd(weight.detach(), ids)

    @staticmethod
    def backward(ctx, d_out):
        (ids,) = ctx.saved_tensors
        return engine.embedding_bwd(d_out, ids, ctx.vocab), None


class Embedding(nn.Module):
    """nn.Embedding(V, E) stand-in (same parameter name / init) used as a callable (training.py:68,147)."""

    def __init__(self, num_embeddings: int, embedding_dim: int):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        nn.init.normal_(self.weight)

    def forward(self, ids):
        return _EmbeddingFn.apply(self.weight, ids)


class _LSTMParams(nn.Module):
    """Parameter container with nn.LSTM's names, shapes and default init (generator.py:32)."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        k = 1.0 / math.sqrt(hidden_size)
        for l in range(num_layers):
            din = input_size if l == 0 else hidden_size
            for name, shape in ((f"weight_ih_l{l}", (4 * hidden_size, din)), (f"weight_hh_l{l}", (4 * hidden_size, hidden_size)),
                                (f"bias_ih_l{l}", (4 * hidden_size,)), (f"bias_hh_l{l}", (4 * hidden_size,))):
                self.register_parameter(name, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def layer_params(self, l: int) -> List[nn.Parameter]:
        return [getattr(self, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


class _LinearParams(nn.Module):
    """Parameter container with nn.Linear's names, shapes and default init."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        k = 1.0 / math.sqrt(in_features)
        self.weight = nn.Parameter(torch.empty(out_features, in_features).uniform_(-k, k))
        self.bias = nn.Parameter(torch.empty(out_features).uniform_(-k, k)) if bias else None


# ------------------------------------------------------------------------------------------ decoder
class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, temperature, pretrain, max_len, noise_u, seed, h0, c0, features, *params):
        dparams = [p.detach() for p in params]
        states = None if h0 is None else (h0.detach(), c0.detach())
        out, ids, st = eng.sample_fwd(dparams, features.detach().float(), max_len, temperature, pretrain, noise_u, seed, states=states)
        ctx.eng, ctx.temperature, ctx.pretrain = eng, temperature, pretrain
        ctx.st, ctx.dparams = st, dparams
        ctx.has_states = states is not None
        ctx.save_for_backward(out, ids)
        ctx.mark_non_differentiable(ids)
        return out, ids

    @staticmethod
    def backward(ctx, d_out, _d_ids):
        out, ids = ctx.saved_tensors
        ws = ctx.eng.alloc_bwd_ws(ids.shape[0], ids.shape[1], out.device)
        grads = ctx.eng.sample_bwd(ctx.dparams, ctx.st, out, ids, d_out, ctx.temperature, ctx.pretrain, ws=ws,
                                   phases=7 if ctx.has_states else 3)
        ctx.st = None
        d_h0 = d_c0 = None
        if ctx.has_states:        # gradients into the initial states: slot 0 of the recurrent input-gradient buffers
            d_h0, d_c0 = ctx.eng.state_grads(ws)
        return (None, None, None, None, None, None, d_h0, d_c0, grads[-1], *grads[:-1])


class _ForwardTfFn(torch.autograd.Function):
    """Decoder.forward with autograd (generator.py:39-53): gic_decoder_forward_tf / gic_decoder_forward_tf_bwd."""

    @staticmethod
    def forward(ctx, eng, drop, temperature, pretrain, caps, lengths, noise_u, seed, tmax, features, *params):
        dparams = [p.detach() for p in params]
        pred, (h_n, c_n), saved = eng.forward_tf(dparams, features.detach().float(), caps, lengths, temperature, pretrain, noise_u, seed,
                                                 keep_state=True, tmax=tmax, **_drop_kw(drop))
        ctx.eng, ctx.temperature, ctx.pretrain, ctx.saved, ctx.dparams = eng, temperature, pretrain, saved, dparams
        ctx.save_for_backward(pred)
        ctx.mark_non_differentiable(h_n, c_n)
        return pred, h_n, c_n

    @staticmethod
    def backward(ctx, d_pred, _d_h, _d_c):
        (pred,) = ctx.saved_tensors
        grads = ctx.eng.forward_tf_bwd(ctx.dparams, ctx.saved, pred, d_pred, ctx.temperature, ctx.pretrain)
        ctx.saved = None
        return (None, None, None, None, None, None, None, None, None, grads[-1], *grads[:-1])


class _ForwardSsFn(torch.autograd.Function):
    """Decoder.forward_scheduled with autograd: gic_decoder_forward_ss, then gic_decoder_forward_tf_bwd over the inputs it realised."""

    @staticmethod
    def forward(ctx, eng, drop, sample_prob, pick, caps, lengths, coin_u, noise_u, seed, tmax, features, *params):
        dparams = [p.detach() for p in params]
        pred, (h_n, c_n), saved, inputs, replaced = eng.forward_scheduled(dparams, features.detach().float(), caps, lengths, sample_prob,
                                                                           pick, coin_u, noise_u, seed, tmax=tmax, **_drop_kw(drop))
        ctx.eng, ctx.saved, ctx.dparams = eng, saved, dparams
        ctx.save_for_backward(pred)
        ctx.mark_non_differentiable(h_n, c_n, inputs, replaced)
        return pred, h_n, c_n, inputs, replaced

    @staticmethod
    def backward(ctx, d_pred, _d_h, _d_c, _d_in, _d_rep):
        (pred,) = ctx.saved_tensors
        grads = ctx.eng.forward_tf_bwd(ctx.dparams, ctx.saved, pred, d_pred, 1.0, True)
        ctx.saved = None
        return (None, None, None, None, None, None, None, None, None, None, grads[-1], *grads[:-1])


def _ss_args(sample_prob, pick, coin_u, noise_u, seed):
    """(p, seed) of a forward_scheduled call, checked: ``seed`` None = the next of SEEDS (0 with both draws given)."""
    p = float(sample_prob)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"sample_prob must be in [0, 1], got {sample_prob}")
    if pick not in engine.SS_PICKS:
        raise ValueError(f"pick must be one of {engine.SS_PICKS}, got {pick!r}")
    if seed is None:
        seed = 0 if (coin_u is not None and (noise_u is not None or pick == "argmax")) or p == 0.0 else SEEDS.next()
    return p, int(seed)


def _drop_args(dropout, dropout_seed, keep_u):
    """(p, seed, keep_u) of a decode's output dropout, checked: ``dropout_seed`` None = the next of SEEDS when a mask is drawn (p > 0
    and no ``keep_u``) -- taken after the call's other seeds, so a call with ``dropout`` = 0 leaves the seed sequence as it was."""
    p = float(dropout)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout must be in [0, 1), got {dropout}")
    if dropout_seed is None:
        dropout_seed = SEEDS.next() if p > 0.0 and keep_u is None else 0
    return p, int(dropout_seed), keep_u


def _drop_kw(drop):
    """The engine keywords of ``_drop_args``' triple."""
    return {"dropout": drop[0], "dropout_seed": drop[1], "keep_u": drop[2]}


def _teacher_inputs(caps, vocab: int):
    """(inputs, replaced) of a decode that replaced nothing: the clamped captions (embed_rows_tf's clamp) and zeros."""
    return caps.clamp(0, vocab - 1), torch.zeros(caps.shape, dtype=torch.int32, device=caps.device)


def _beam_search(dec, features, maps, beam_size, max_caption_len, eos_id, length_penalty, states, return_beams, beam_groups, diversity,
                 force_words=None, return_met=False, **kw):
    """Decoder.beam_search / AttnDecoder.beam_search: ``maps`` = () or (fmap,), ``kw`` = the engine's further keywords (the decode
    constraints, want_alphas).  One group without diversity is the plain search; ``force_words`` the forced one (met comes last)."""
    L = int(dec.max_seq_length if max_caption_len is None else max_caption_len)
    if force_words is None and return_met:
        raise ValueError("return_met needs force_words")
    with torch.no_grad():
        args = ([p.detach() for p in dec.param_list()], features.detach().float(), *(m.detach() for m in maps), L, int(beam_size))
        if force_words is not None:
            if int(beam_groups) != 1 or float(diversity) != 0.0:
                raise ValueError("force_words with beam_groups > 1 or diversity: forced words do not combine with diverse beam search")
            out = dec.engine().beam_search(*args, int(eos_id), 0, float(length_penalty), states=states, force_words=force_words, **kw)
            if not return_met:
                out = out[:-1]
        elif int(beam_groups) == 1 and float(diversity) == 0.0:
            out = dec.engine().beam_search(*args, int(eos_id), 0, float(length_penalty), states=states, **kw)
        else:
            out = dec.engine().diverse_beam_search(*args, int(beam_groups), float(diversity), int(eos_id), 0, float(length_penalty),
                                                   states=states, **kw)
    return out if return_beams else tuple(t[:, 0] for t in out)


def _sample_captions(dec, features, maps, num_samples, top_k, top_p, temperature, max_caption_len, eos_id, seed, noise_u, states, **cons):
    """Decoder.sample_captions / AttnDecoder.sample_captions: ``maps`` = () or (fmap,)."""
    L = int(dec.max_seq_length if max_caption_len is None else max_caption_len)
    seed = (0 if noise_u is not None else SEEDS.next()) if seed is None else int(seed)
    with torch.no_grad():
        return dec.engine().sample_captions([p.detach() for p in dec.param_list()], features.detach().float(), *(m.detach() for m in maps), L,
                                            int(num_samples), int(top_k), float(top_p), float(temperature), int(eos_id), 0, seed, noise_u,
                                            states=states, **cons)


def _log_likelihood(dec, features, maps, ids, lengths):
    """Decoder.log_likelihood / AttnDecoder.log_likelihood: ``maps`` = () or (fmap,).  ``forward(features[, fmap], ids[:, :-1], lengths,
    pretrain=True)``'s own no-grad decode (``_forward_no_grad``: logits need no device draw, so none is taken from SEEDS) over all L
    positions with device lengths (no host sync), then gic_xent_seq masked by ``lengths``."""
    if ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[1] < 2:
        raise ValueError("log_likelihood: ids must be int64 [B, L] with L >= 2")
    B, L = ids.shape
    lengths = torch.as_tensor(lengths).to(device=ids.device, dtype=torch.int32).reshape(-1)
    if lengths.numel() != B:
        raise ValueError(f"log_likelihood: lengths must hold one value per caption ({B})")
    with torch.no_grad():
        pred = dec._forward_no_grad(features, *maps, ids[:, :-1].contiguous(), lengths.clamp(1, L), True, None, 0, L)[0]
        out = engine.xent_seq(pred.reshape(B * L, pred.shape[-1]), ids.reshape(-1), L, lengths=lengths, want_grad=False)
        return -out["cap_nll"], out["cap_tokens"]


class Decoder(nn.Module):
    """Embedding + LSTM + Linear caption decoder (generator.py:27-96)."""

    def __init__(self, args):
        super().__init__()
        self.embed = Embedding(args.vocab_size, args.gen_embed_dim)
        self.lstm = _LSTMParams(args.gen_embed_dim, args.gen_hidden_dim, args.gen_num_layers)
        self.linear = _LinearParams(args.gen_hidden_dim, args.vocab_size)
        self.max_seq_length = args.max_seq_len
        self.temperature = args.temperature          # mutated from outside (training.py:191)
        self.args = args
        self._engine: Optional[engine.DecoderEngine] = None

    def engine(self) -> engine.DecoderEngine:
        if self._engine is None:
            a = self.args
            self._engine = engine.DecoderEngine(a.vocab_size, a.gen_embed_dim, a.gen_hidden_dim, a.gen_num_layers, _compute_dtype(a))
        return self._engine

    def param_list(self) -> List[nn.Parameter]:
        ps = [self.embed.weight]
        for l in range(self.lstm.num_layers):
            ps += self.lstm.layer_params(l)
        return ps + [self.linear.weight, self.linear.bias]

    def sample(self, features, states=None, pretrain=False, max_caption_len=34, noise_u=None):
        """Greedy Gumbel-softmax roll-out (generator.py:55-81): returns (outputs [B,L,V], ids int64 [B,L]).
        Gradients flow through ``outputs`` to the decoder parameters and ``features``; never through ``ids``."""
        h0 = c0 = None
        if states is not None:          # (h0, c0), each [num_layers, B, H], as nn.LSTM takes them (generator.py:61)
            h0, c0 = states
        seed = 0 if noise_u is not None else SEEDS.next()
        return _SampleFn.apply(self.engine(), float(self.temperature), bool(pretrain), int(max_caption_len), noise_u, seed,
                               h0, c0, features, *self.param_list())

    def forward(self, features, caps, lengths, pretrain=False, noise_u=None, max_length=None, dropout=0.0, dropout_seed=None, keep_u=None):
        """Teacher-forced decode (generator.py:39-53): inputs [features ; embed(caps)] packed with ``lengths``; returns
        (pred [B, max(lengths), V], (h_n, c_n)) with pred = logits (pretrain) or softmax((logits + gumbel) * temperature).
        Dead on the reference's training path (training.py never calls it), kept for the module surface.  Gradients flow through
        ``pred`` to the decoder parameters and ``features`` (padded positions reach the projection's bias only, as
        pad_packed_sequence's zeros do); the returned hidden state is not differentiated.  ``noise_u`` [B, max(lengths), V]
        replaces the device draw (parity runs).  ``max_length``: decode that many steps with ``lengths`` a device tensor that is not
        read back (no host sync; pred is [B, max_length, V], rows past a length as above).  ``dropout`` p in [0, 1): output dropout --
        the LSTM output is dropped with probability p (and the rest scaled by 1 / (1 - p)) in front of the vocabulary projection; the
        recurrence and (h_n, c_n) keep the undropped h.  The mask is Philox(``dropout_seed``; None = the next of SEEDS) or ``keep_u`` f32
        [B, max(lengths), H] (keep = u >= p).  It is the caller's switch, not the module's training flag: a no-grad call drops too."""
        seed = 0 if noise_u is not None else SEEDS.next()
        drop = _drop_args(dropout, dropout_seed, keep_u)
        params = self.param_list()
        if not torch.is_grad_enabled() or not (features.requires_grad or any(p.requires_grad for p in params)):
            return self._forward_no_grad(features, caps, lengths, pretrain, noise_u, seed, max_length, drop)
        pred, h_n, c_n = _ForwardTfFn.apply(self.engine(), drop, float(self.temperature), bool(pretrain), caps, lengths, noise_u, seed,
                                            max_length, features, *params)
        return pred, (h_n, c_n)

    def _forward_no_grad(self, features, caps, lengths, pretrain, noise_u, seed, max_length, drop=(0.0, 0, None)):
        """``forward`` without autograd, with the seed of its device draw given: (pred, (h_n, c_n)).  Also log_likelihood's decode
        (which never drops)."""
        with torch.no_grad():
            return self.engine().forward_tf([p.detach() for p in self.param_list()], features, caps, lengths, float(self.temperature),
                                            bool(pretrain), noise_u, seed, tmax=max_length, **_drop_kw(drop))

    def forward_scheduled(self, features, caps, lengths, sample_prob, pick="sample", coin_u=None, noise_u=None, seed=None, max_length=None,
                          return_inputs=False, dropout=0.0, dropout_seed=None, keep_u=None):
        """``forward(features, caps, lengths, pretrain=True)`` with scheduled sampling (Bengio et al., 2015; gicap.h
        gic_decoder_forward_ss): the input of step t >= 1 is caps[:, t-1] with probability 1 - ``sample_prob``, else a token the decoder
        picks from its own logits of step t-1 -- ``pick`` = "sample" (a draw from softmax(logits), by Gumbel-max) or "argmax"; positions
        past a caption's length are never replaced.  Returns (pred = logits [B, max(lengths), V], (h_n, c_n)); ``return_inputs`` appends
        (inputs int64 [B, L], replaced int32 [B, L]), the inputs the decode realised.  Gradients flow as in ``forward`` over those
        inputs; none flows through the choice.  ``coin_u`` f32 [B, L] and ``noise_u`` f32 [L, B, V] replace the device draws
        (Philox(``seed``); None = the next of SEEDS).  ``sample_prob`` = 0 is ``forward`` itself: nothing else is launched.
        ``dropout`` / ``dropout_seed`` / ``keep_u`` as ``forward``: the picks are made from the dropped logits."""
        p, seed = _ss_args(sample_prob, pick, coin_u, noise_u, seed)
        if p == 0.0:
            pred, hc = self.forward(features, caps, lengths, pretrain=True, max_length=max_length, dropout=dropout,
                                    dropout_seed=dropout_seed, keep_u=keep_u)
            return (pred, hc, _teacher_inputs(caps, self.args.vocab_size)) if return_inputs else (pred, hc)
        drop = _drop_args(dropout, dropout_seed, keep_u)
        params = self.param_list()
        if not torch.is_grad_enabled() or not (features.requires_grad or any(q.requires_grad for q in params)):
            with torch.no_grad():
                pred, hc, _, inputs, replaced = self.engine().forward_scheduled([q.detach() for q in params], features.detach().float(), caps,
                                                                               lengths, p, pick, coin_u, noise_u, seed, tmax=max_length,
                                                                               **_drop_kw(drop))
        else:
            pred, h_n, c_n, inputs, replaced = _ForwardSsFn.apply(self.engine(), drop, p, pick, caps, lengths, coin_u, noise_u, seed, max_length,
                                                                  features, *params)
            hc = (h_n, c_n)
        return (pred, hc, (inputs, replaced)) if return_inputs else (pred, hc)

    def beam_search(self, features, beam_size=3, max_caption_len=None, eos_id=2, length_penalty=0.0, states=None, return_beams=False,
                    beam_groups=1, diversity=0.0, force_words=None, return_met=False, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
        """Beam-search caption decode (gicap.h gic_decoder_beam_search): token log-probabilities of sample(pretrain=True)'s
        distribution, ``beam_size`` (1..8) hypotheses per image, <E> = ``eos_id`` ends a beam, <PAD> (0) after it; final order by
        score / length**length_penalty.  Returns detached (ids int64 [B, L], scores f32 [B], lengths int32 [B]) of the best beam, or
        all beams ([B, k, L], [B, k], [B, k]) with ``return_beams``.  ``max_caption_len`` None = args.max_seq_len.  ``beam_groups``
        > 1 or ``diversity`` > 0: diverse beam search (gic_decoder_diverse_beam_search), ``beam_groups`` groups of beam_size /
        beam_groups beams with the Hamming penalty ``diversity``; the beams come in group-major order, the best beam is group 0's.
        ``no_repeat_ngram`` (n: no n-gram occurs twice in a caption; 0 = off), ``min_length`` (<E> not before that many
        tokens; 0 = off) and ``suppress_tokens`` (up to 16 ids never emitted): decode constraints (gicap.h gic_decode_constraints),
        applied inside the search.
        ``force_words`` (None = off): lexically constrained beam search (gicap.h gic_forced_words) -- an int32 tensor [B, C, D] padded
        with -1, or a list per image of constraints, each an int or a tuple of ints (a caption meets a constraint by emitting any id
        of it); C <= 3, D <= 4, 2^C must divide ``beam_size``, one beam group.  The beams come ordered by constraints met, then
        score / length**length_penalty: the best beam is the best caption that meets everything, if the search found one.
        ``return_met`` appends met int32 [B] ([B, k]): the bitmask of constraints each caption meets (absent ones set)."""
        return _beam_search(self, features, (), beam_size, max_caption_len, eos_id, length_penalty, states, return_beams, beam_groups, diversity,
                            force_words=force_words, return_met=return_met, no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=suppress_tokens)

    def sample_captions(self, features, num_samples=5, top_k=0, top_p=1.0, temperature=1.0, max_caption_len=None, eos_id=2, seed=None,
                        noise_u=None, states=None, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
        """Caption sampling (gicap.h gic_decoder_sample_captions): ``num_samples`` (1..8) captions per image drawn from softmax(logits /
        ``temperature``) truncated to the ``top_k`` largest logits (0 = off) and then to the nucleus of mass ``top_p`` (1 = off); ties at
        either boundary are kept.  <E> = ``eos_id`` ends a caption, <PAD> (0) after it.  ``temperature`` is the sampling temperature,
        not args.temperature.  ``noise_u`` f32 [L, B*n, V] replaces the device draw (Philox(seed); ``seed`` None = the next of SEEDS).
        Returns detached (ids int64 [B, n, L], scores f32 [B, n] = the model's log-probability of each caption, lengths int32 [B, n]),
        in draw order.  ``max_caption_len`` None = args.max_seq_len.  ``no_repeat_ngram`` (n: no n-gram occurs twice in a caption; 0 =
        off), ``min_length`` (<E> not before that many tokens; 0 = off) and ``suppress_tokens`` (up to 16 ids never emitted): decode
        constraints (gicap.h gic_decode_constraints), the banned tokens leave the distribution before top-k / top-p."""
        return _sample_captions(self, features, (), num_samples, top_k, top_p, temperature, max_caption_len, eos_id, seed, noise_u, states,
                                no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=suppress_tokens)

    def log_likelihood(self, features, ids, lengths):
        """The decoder's log-probability of given captions, in the units of the beam and sample scores: (logp f32 [B], tokens int32 [B])
        with logp[b] = sum_{t < lengths[b]} log p(ids[b, t] | features, ids[b, <t]) (position 0 included) and tokens[b] the positions
        summed.  ``ids`` int64 [B, L], ``lengths`` [B].  Teacher-forced: ``forward(features, ids[:, :-1], lengths, pretrain=True)``
        followed by gic_xent_seq, under no-grad; detached."""
        return _log_likelihood(self, features, (), ids, lengths)

    def add_gumbel(self, o_t, eps=1e-10, gpu=0):
        """o_t + Gumbel(0,1) noise (generator.py:84-96); on the hot path this is fused into sample()."""
        u = torch.empty_like(o_t, dtype=torch.float32).uniform_(0, 1)
        return o_t + (-torch.log(-torch.log(u + eps) + eps))


# ------------------------------------------------------------------------------------------ visual-attention decoder
class _AttnSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, temperature, pretrain, max_len, noise_u, seed, states, fmap, features, *params):
        dparams = [p.detach() for p in params]
        out, ids, st = eng.sample_fwd(dparams, features.detach().float(), fmap.detach(), max_len, temperature, pretrain, noise_u, seed,
                                      states=states)
        ctx.eng, ctx.temperature, ctx.pretrain, ctx.st, ctx.dparams = eng, temperature, pretrain, st, dparams
        ctx.save_for_backward(out, ids)
        ctx.mark_non_differentiable(ids)
        return out, ids

    @staticmethod
    def backward(ctx, d_out, _d_ids):
        out, ids = ctx.saved_tensors
        grads = ctx.eng.sample_bwd(ctx.dparams, ctx.st, out, ids, d_out, ctx.temperature, ctx.pretrain)
        ctx.st = None
        return (None, None, None, None, None, None, None, None, grads[-1], *grads[:-1])


class _AttnForwardTfFn(torch.autograd.Function):
    """AttnDecoder.forward with autograd: gic_attn_forward_tf / gic_attn_forward_tf_bwd; the alphas are differentiable too."""

    @staticmethod
    def forward(ctx, eng, drop, temperature, pretrain, caps, lengths, noise_u, seed, tmax, fmap, features, *params):
        dparams = [p.detach() for p in params]
        pred, (h_n, c_n), alphas, saved = eng.forward_tf(dparams, features.detach().float(), fmap.detach(), caps, lengths, temperature,
                                                         pretrain, noise_u, seed, want_alphas=True, keep_state=True, tmax=tmax,
                                                         **_drop_kw(drop))
        ctx.eng, ctx.temperature, ctx.pretrain, ctx.saved, ctx.dparams = eng, temperature, pretrain, saved, dparams
        ctx.save_for_backward(pred)
        ctx.mark_non_differentiable(h_n, c_n)
        ctx.set_materialize_grads(False)
        return pred, h_n, c_n, alphas

    @staticmethod
    def backward(ctx, d_pred, _d_h, _d_c, d_alphas):
        (pred,) = ctx.saved_tensors
        grads = ctx.eng.forward_tf_bwd(ctx.dparams, ctx.saved, pred, d_pred, ctx.temperature, ctx.pretrain, d_alphas=d_alphas)
        ctx.saved = None
        return (None, None, None, None, None, None, None, None, None, None, grads[-1], *grads[:-1])


class _AttnForwardSsFn(torch.autograd.Function):
    """AttnDecoder.forward_scheduled with autograd: gic_attn_forward_ss, then gic_attn_forward_tf_bwd over the inputs it realised."""

    @staticmethod
    def forward(ctx, eng, drop, sample_prob, pick, caps, lengths, coin_u, noise_u, seed, tmax, fmap, features, *params):
        dparams = [p.detach() for p in params]
        pred, (h_n, c_n), alphas, saved, inputs, replaced = eng.forward_scheduled(dparams, features.detach().float(), fmap.detach(), caps,
                                                                                   lengths, sample_prob, pick, coin_u, noise_u, seed,
                                                                                   tmax=tmax, **_drop_kw(drop))
        ctx.eng, ctx.saved, ctx.dparams = eng, saved, dparams
        ctx.save_for_backward(pred)
        ctx.mark_non_differentiable(h_n, c_n, inputs, replaced)
        ctx.set_materialize_grads(False)
        return pred, h_n, c_n, alphas, inputs, replaced

    @staticmethod
    def backward(ctx, d_pred, _d_h, _d_c, d_alphas, _d_in, _d_rep):
        (pred,) = ctx.saved_tensors
        grads = ctx.eng.forward_tf_bwd(ctx.dparams, ctx.saved, pred, d_pred, 1.0, True, d_alphas=d_alphas)
        ctx.saved = None
        return (None, None, None, None, None, None, None, None, None, None, None, grads[-1], *grads[:-1])


class _AttnParams(nn.Module):
    """Additive (Show-Attend-Tell) attention parameters: e_i = w_a . tanh(W_f a_i + b_f + W_h h)."""

    def __init__(self, feat_c: int, hidden: int, attn: int):
        super().__init__()
        k = 1.0 / math.sqrt(attn)
        self.w_f = nn.Parameter(torch.empty(attn, feat_c).uniform_(-k, k))
        self.b_f = nn.Parameter(torch.zeros(attn))
        self.w_h = nn.Parameter(torch.empty(attn, hidden).uniform_(-k, k))
        self.w_a = nn.Parameter(torch.empty(attn).uniform_(-k, k))


class AttnDecoder(nn.Module):
    """Caption decoder with soft visual attention over the trunk's feature map (``--decoder attention``, BASELINE config 4).  NO
    reference counterpart: the reference's Decoder (generator.py:27-96) with a context vector z_t = sum_i alpha_ti a_i concatenated
    to the LSTM input (oracle/cpu_attention.py).  One LSTM layer; same ``embed`` / ``lstm`` / ``linear`` state-dict keys as the
    reference's Decoder plus ``attn.*``; ``sample`` takes the feature map next to the start features."""

    def __init__(self, args, feat_c: int, positions: int):
        super().__init__()
        if args.gen_num_layers != 1:
            raise ValueError("--decoder attention supports one LSTM layer")
        if args.vocab_size % 4 or args.gen_embed_dim % 8 or args.gen_hidden_dim % 8 or feat_c % 8 or int(getattr(args, "attn_dim", 512)) % 8:
            # gic_attn_* (attention.hip check_attn_dims) would refuse these at the first step: say so at construction
            raise ValueError("--decoder attention needs vocab_size % 4 == 0 and gen_embed_dim / gen_hidden_dim / attn_dim % 8 == 0 "
                             f"(got V={args.vocab_size}, E={args.gen_embed_dim}, H={args.gen_hidden_dim}); main.py pads the vocabulary")
        self.embed = Embedding(args.vocab_size, args.gen_embed_dim)
        self.lstm = _LSTMParams(args.gen_embed_dim + feat_c, args.gen_hidden_dim, 1)
        self.linear = _LinearParams(args.gen_hidden_dim, args.vocab_size)
        self.attn = _AttnParams(feat_c, args.gen_hidden_dim, int(getattr(args, "attn_dim", 512)))
        self.max_seq_length = args.max_seq_len
        self.temperature = args.temperature
        self.args, self.feat_c, self.positions = args, feat_c, positions
        self._engine = None

    def engine(self):
        if self._engine is None:
            a = self.args
            self._engine = engine.AttnDecoderEngine(a.vocab_size, a.gen_embed_dim, a.gen_hidden_dim, self.feat_c, self.positions,
                                                    self.attn.w_a.numel(), _compute_dtype(a))
        return self._engine

    def param_list(self) -> List[nn.Parameter]:
        return [self.embed.weight] + self.lstm.layer_params(0) + [self.linear.weight, self.linear.bias, self.attn.w_f, self.attn.b_f,
                                                                   self.attn.w_h, self.attn.w_a]

    def beam_search(self, features, fmap=None, beam_size=3, max_caption_len=None, eos_id=2, length_penalty=0.0, states=None,
                    return_beams=False, return_alphas=False, beam_groups=1, diversity=0.0, force_words=None, return_met=False,
                    no_repeat_ngram=0, min_length=0, suppress_tokens=()):
        """Beam-search caption decode with attention (gicap.h gic_attn_beam_search): Decoder.beam_search's search over the token
        log-probabilities of sample(features, fmap, pretrain=True).  ``fmap`` [B, P, C]: the trunk's last feature map
        (Encoder.forward_with_map).  Returns detached (ids int64 [B, L], scores f32 [B], lengths int32 [B]) of the best beam, or all beams
        ([B, k, L], [B, k], [B, k]) with ``return_beams``; ``return_alphas`` appends the attention weights with which each token was
        produced, f32 [B, L, P] (all beams: [B, k, L, P]), zero past a beam's length.  ``states`` = (h0, c0), each [1, B, H].
        ``beam_groups`` / ``diversity``: diverse beam search (gic_attn_diverse_beam_search) as in Decoder.beam_search, and so are the
        decode constraints ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``.  ``force_words`` / ``return_met``: lexically
        constrained beam search as in Decoder.beam_search (gic_attn_forced_beam_search); met comes after the alphas."""
        if fmap is None:                # (checked before anything touches self: the LSTM decoder's call form has no map)
            raise NotImplementedError("the attention decoder's beam search needs the trunk's feature map: beam_search(features, fmap), "
                                      "or Generator.caption(images)")
        return _beam_search(self, features, (fmap,), beam_size, max_caption_len, eos_id, length_penalty, states, return_beams, beam_groups,
                            diversity, force_words=force_words, return_met=return_met, want_alphas=bool(return_alphas),
                            no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=suppress_tokens)

    def sample_captions(self, features, fmap=None, num_samples=5, top_k=0, top_p=1.0, temperature=1.0, max_caption_len=None, eos_id=2,
                        seed=None, noise_u=None, states=None, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
        """Caption sampling with attention (gicap.h gic_attn_sample_captions): Decoder.sample_captions with the step of sample(features,
        fmap).  ``fmap`` [B, P, C]: the trunk's last feature map (Encoder.forward_with_map).  ``states`` = (h0, c0), each [1, B, H].
        ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``: the decode constraints of Decoder.sample_captions."""
        if fmap is None:                # (checked before anything touches self: the LSTM decoder's call form has no map)
            raise NotImplementedError("the attention decoder's sampling needs the trunk's feature map: sample_captions(features, fmap), "
                                      "or Generator.sample_captions(images)")
        return _sample_captions(self, features, (fmap,), num_samples, top_k, top_p, temperature, max_caption_len, eos_id, seed, noise_u, states,
                                no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=suppress_tokens)

    def forward(self, features, fmap, caps, lengths, pretrain=False, noise_u=None, return_alphas=False, max_length=None, dropout=0.0,
                dropout_seed=None, keep_u=None):
        """Teacher-forced decode (Decoder.forward with the attention step, gicap.h gic_attn_forward_tf): step 0 is fed ``features``,
        step t > 0 embed(caps[:, t-1]), packed with ``lengths`` (each 1..caps.shape[1] + 1).  Returns (pred [B, max(lengths), V],
        (h_n, c_n) [1, B, H]) with pred = logits (pretrain) or softmax((logits + gumbel) * temperature); ``return_alphas`` appends the
        attention weights f32 [B, max(lengths), P] (zero past a caption's length), differentiable like ``pred``.  Gradients flow to the
        decoder parameters and ``features`` (padded positions reach the projection's bias only); the returned hidden state is not
        differentiated.  ``fmap`` [B, P, C]: the trunk's last feature map (no gradient into it).  ``noise_u`` [B, max(lengths), V]
        replaces the device draw.  ``max_length`` and the output dropout (``dropout``, ``dropout_seed``, ``keep_u``) as Decoder.forward."""
        if fmap is None:
            raise ValueError("the attention decoder needs the trunk's feature map: forward(features, fmap, caps, lengths)")
        seed = 0 if noise_u is not None else SEEDS.next()
        drop = _drop_args(dropout, dropout_seed, keep_u)
        params = self.param_list()
        if not torch.is_grad_enabled() or not (features.requires_grad or any(p.requires_grad for p in params)):
            pred, hc, alphas = self._forward_no_grad(features, fmap, caps, lengths, pretrain, noise_u, seed, max_length, return_alphas, drop)
        else:
            pred, h_n, c_n, alphas = _AttnForwardTfFn.apply(self.engine(), drop, float(self.temperature), bool(pretrain), caps, lengths, noise_u,
                                                            seed, max_length, fmap, features, *params)
            hc = (h_n, c_n)
        if return_alphas:
            return pred, hc, alphas
        return pred, hc

    def _forward_no_grad(self, features, fmap, caps, lengths, pretrain, noise_u, seed, max_length, return_alphas=False,
                         drop=(0.0, 0, None)):
        """``forward`` without autograd, with the seed of its device draw given: (pred, (h_n, c_n), alphas or None).  Also
        log_likelihood's decode (which never drops)."""
        with torch.no_grad():
            return self.engine().forward_tf([p.detach() for p in self.param_list()], features.detach().float(), fmap.detach(), caps, lengths,
                                            float(self.temperature), bool(pretrain), noise_u, seed, want_alphas=bool(return_alphas),
                                            tmax=max_length, **_drop_kw(drop))

    def log_likelihood(self, features, fmap, ids, lengths):
        """Decoder.log_likelihood with the attention step: (logp f32 [B], tokens int32 [B]) of ``ids`` int64 [B, L] given ``features`` and
        ``fmap`` [B, P, C]."""
        if fmap is None:
            raise ValueError("the attention decoder needs the trunk's feature map: log_likelihood(features, fmap, ids, lengths)")
        return _log_likelihood(self, features, (fmap,), ids, lengths)

    def forward_scheduled(self, features, fmap, caps, lengths, sample_prob, pick="sample", coin_u=None, noise_u=None, seed=None,
                          max_length=None, return_alphas=False, return_inputs=False, dropout=0.0, dropout_seed=None, keep_u=None):
        """``forward(features, fmap, caps, lengths, pretrain=True)`` with scheduled sampling (Decoder.forward_scheduled; gicap.h
        gic_attn_forward_ss).  Returns (pred, (h_n, c_n)); ``return_alphas`` appends the attention weights (differentiable, as in
        ``forward``), ``return_inputs`` then (inputs, replaced).  ``sample_prob`` = 0 is ``forward`` itself.  Output dropout
        (``dropout``, ``dropout_seed``, ``keep_u``) as Decoder.forward_scheduled."""
        if fmap is None:
            raise ValueError("the attention decoder needs the trunk's feature map: forward_scheduled(features, fmap, caps, lengths, p)")
        p, seed = _ss_args(sample_prob, pick, coin_u, noise_u, seed)
        if p == 0.0:
            pred, hc, alphas = self.forward(features, fmap, caps, lengths, pretrain=True, return_alphas=True, max_length=max_length,
                                            dropout=dropout, dropout_seed=dropout_seed, keep_u=keep_u)
            inputs, replaced = _teacher_inputs(caps, self.args.vocab_size) if return_inputs else (None, None)
        else:
            drop = _drop_args(dropout, dropout_seed, keep_u)
            params = self.param_list()
            if not torch.is_grad_enabled() or not (features.requires_grad or any(q.requires_grad for q in params)):
                with torch.no_grad():
                    pred, hc, alphas, _, inputs, replaced = self.engine().forward_scheduled(
                        [q.detach() for q in params], features.detach().float(), fmap.detach(), caps, lengths, p, pick, coin_u, noise_u, seed,
                        tmax=max_length, **_drop_kw(drop))
            else:
                pred, h_n, c_n, alphas, inputs, replaced = _AttnForwardSsFn.apply(self.engine(), drop, p, pick, caps, lengths, coin_u, noise_u, seed,
                                                                                  max_length, fmap, features, *params)
                hc = (h_n, c_n)
        return (pred, hc) + ((alphas,) if return_alphas else ()) + (((inputs, replaced),) if return_inputs else ())

    def monte_carlo_rollouts(self, features, fmap, captions, num_rollouts, noise_u=None, seed=None):
        """Monte-Carlo roll-outs of ``captions`` int64 [B, L] (gicap.h gic_attn_rollout), for a reward of the caller's own: for every
        prefix length t = 1..L-1, ``num_rollouts`` completions of captions[:, :t] sampled from the decoder at temperature 1.  Returns
        detached int64 [L-1, N, B, L]; [t-1, n, b] = roll-out n of caption b, which starts with captions[b, :t].  ``features`` [B, E],
        ``fmap`` [B, P, C] as for ``sample``.  ``noise_u`` f32 [L, (L-1)*N*B, V] replaces the device draw (row (t-1)*N*B + n*B + b)."""
        if fmap is None:
            raise ValueError("the attention decoder needs the trunk's feature map: monte_carlo_rollouts(features, fmap, captions, n)")
        B, Lc = captions.shape
        eng = self.engine()
        with torch.no_grad():
            params = [p.detach() for p in self.param_list()]
            saved = eng.forward_tf(params, features.detach().float(), fmap.detach(), captions[:, :-1], [Lc] * B, 1.0, pretrain=True,
                                   keep_state=True)[3]
            ids = eng.rollout(params, saved, captions, int(num_rollouts), noise_u=noise_u,
                              seed=0 if noise_u is not None else (SEEDS.next() if seed is None else int(seed)))
        return ids.view(Lc - 1, int(num_rollouts), B, Lc)

    def sample(self, features, fmap=None, states=None, pretrain=False, max_caption_len=34, noise_u=None):
        """(outputs [B,L,V], ids [B,L]) as Decoder.sample; ``fmap`` [B, P, C]: the trunk's last feature map (no gradient into it)."""
        if fmap is None:
            raise ValueError("the attention decoder needs the trunk's feature map: sample(features, fmap)")
        if states is not None:          # (h0, c0), each [1, B, H] as nn.LSTM takes them (generator.py:55,61); constants of the backward pass
            states = tuple(t.detach() for t in states)
        seed = 0 if noise_u is not None else SEEDS.next()
        return _AttnSampleFn.apply(self.engine(), float(self.temperature), bool(pretrain), int(max_caption_len), noise_u, seed, states, fmap,
                                   features, *self.param_list())


# ------------------------------------------------------------------------------------------ encoder
class _EncoderHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dtype, training, momentum, eps, trunk_feat, weight, bias, gamma, beta, running_mean, running_var):
        out, saved = encoder_head_fwd(dtype, trunk_feat.detach(), weight.detach(), bias.detach(), gamma.detach(), beta.detach(),
                                      running_mean, running_var, training, momentum, eps)
        ctx.saved, ctx.dtype = saved, dtype
        ctx.w = weight.detach()
        ctx.gamma = gamma.detach()
        return out

    @staticmethod
    def backward(ctx, d_out):
        dw, db, dgamma, dbeta = encoder_head_bwd(ctx.dtype, ctx.saved, ctx.w, ctx.gamma, d_out.contiguous())
        return None, None, None, None, None, dw, db, dgamma, dbeta, None, None


class _BatchNorm1dParams(nn.Module):
    def __init__(self, num_features: int, momentum: float):
        super().__init__()
        self.num_features, self.momentum, self.eps = num_features, momentum, 1e-5
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class Encoder(nn.Module):
    """ResNet trunk (frozen, forward only) -> Linear -> BatchNorm1d(momentum=0.01) (generator.py:8-25)."""

    def __init__(self, args):
        super().__init__()
        self.resnet = ResNetTrunk(getattr(args, "encoder_arch", "resnet18"))
        self.linear = _LinearParams(self.resnet.out_features, args.gen_embed_dim)
        self.bn = _BatchNorm1dParams(args.gen_embed_dim, momentum=0.01)
        self.args = args

    def forward(self, images, next_images=None):
        """generator.py:19-25.  ``next_images`` (optional, the next batch's images): their trunk forward is enqueued on the look-ahead
        stream now and picked up by the next call that is handed the same tensor."""
        with torch.no_grad():                                        # generator.py:21-22
            main = torch.cuda.current_stream(images.device)
            start = main.record_event()
            feats = self.take_trunk(images, self.training, main)
            if next_images is not None:
                self.prefetch_trunk(next_images, self.training, start)
        feats = feats.reshape(feats.size(0), -1)
        self.last_trunk = feats                                      # the pooled trunk features of this call (a conditioned D reads them)
        return _EncoderHeadFn.apply(_compute_dtype(self.args), self.training, self.bn.momentum, self.bn.eps, feats,
                                    self.linear.weight, self.linear.bias, self.bn.weight, self.bn.bias,
                                    self.bn.running_mean, self.bn.running_var)

    def head(self, feats):
        """Linear -> BatchNorm1d on given pooled trunk features [B, F] (an Ensemble's members that share one trunk)."""
        return _EncoderHeadFn.apply(_compute_dtype(self.args), self.training, self.bn.momentum, self.bn.eps, feats,
                                    self.linear.weight, self.linear.bias, self.bn.weight, self.bn.bias,
                                    self.bn.running_mean, self.bn.running_var)

    def forward_with_map(self, images, next_images=None):
        """(features [B,E] as forward(), feature map [B, P, C] = the trunk's last activation, detached) for the attention decoder.
        ``next_images``: as in forward() -- the look-ahead pass also keeps a copy of its feature map."""
        with torch.no_grad():
            main = torch.cuda.current_stream(images.device)
            start = main.record_event()
            pre, self._pre = getattr(self, "_pre", None), None
            fmap = None
            if pre is not None:
                main.wait_event(pre[3])             # the look-ahead pass (used or not: it shares the plan's buffers)
                if pre[0] is images and pre[1] == bool(self.training) and pre[4] is not None:
                    feats, fmap = pre[2], pre[4]
                    feats.record_stream(main)
                    fmap.record_stream(main)
            if fmap is None:
                busy = getattr(self, "_busy", None)
                if busy is not None:
                    main.wait_event(busy)
                feats = self.trunk_features(images, self.training).clone()      # a pass here: the map is the plan's live buffer
                fmap = self.resnet._plan.last_map(images.shape[0], images.shape[2]).clone()
                self._busy = main.record_event()
            if next_images is not None:
                self.prefetch_trunk(next_images, self.training, start, want_map=True)
        feats = feats.reshape(feats.size(0), -1)
        self.last_trunk = feats
        out = _EncoderHeadFn.apply(_compute_dtype(self.args), self.training, self.bn.momentum, self.bn.eps, feats,
                                   self.linear.weight, self.linear.bias, self.bn.weight, self.bn.bias,
                                   self.bn.running_mean, self.bn.running_var)
        return out, fmap.view(fmap.shape[0], -1, fmap.shape[-1])

    # ---- trunk look-ahead: the trunk is frozen (generator.py:21), so the pass for the NEXT batch depends on nothing the current
    # step updates; it runs on its own stream under the step's launch-bound phases and hands over a private copy of its output.
    def prefetch_trunk(self, images, training: bool, after, mark=None, want_map: bool = False) -> None:
        if getattr(self, "_s_pre", None) is None:
            self._s_pre = torch.cuda.Stream(device=images.device)
        s = self._s_pre
        with engine.on_stream(s):
            s.wait_event(after)                 # `images` is ready
            busy, self._busy = getattr(self, "_busy", None), None
            if busy is not None:
                # a synchronous pass on another stream (cold step, mispredicted look-ahead) is still using the plan's
                # shared buffers (packed image, statistics arena, activations): this pass starts behind it
                s.wait_event(busy)
            if mark is not None:
                mark("trunk prefetch start [s_pre]", s)
            feats = self.trunk_features(images, training).clone()
            fmap = self.resnet._plan.last_map(images.shape[0], images.shape[2]).clone() if want_map else None
            done = s.record_event()
            if mark is not None:
                mark("trunk prefetch done [s_pre]", s)
        images.record_stream(s)
        self._pre = (images, bool(training), feats, done, fmap)

    def take_trunk(self, images, training: bool, stream):
        """Trunk features of ``images`` on ``stream``: the prefetched copy if this very tensor was announced, else a pass now."""
        pre, self._pre = getattr(self, "_pre", None), None
        if pre is not None:
            stream.wait_event(pre[3])           # also orders a synchronous pass behind an unused look-ahead (shared buffers)
            if pre[0] is images and pre[1] == bool(training):
                pre[2].record_stream(stream)
                return pre[2]
        # synchronous pass: hand out a private copy (the plan's own output buffer is overwritten by the next pass, which may
        # run on the look-ahead stream) and remember where this pass ends for prefetch_trunk
        busy = getattr(self, "_busy", None)
        if busy is not None:
            stream.wait_event(busy)             # an earlier synchronous pass on some other stream
        feats = self.trunk_features(images, training).clone()
        self._busy = stream.record_event()
        return feats

    def take_trunk_with_map(self, images, training: bool, stream):
        """(trunk features, the trunk's last feature map [N, h, w, C]) of ``images`` on ``stream`` for the attention decoder: the
        look-ahead pass's private copies if this very tensor was announced (prefetch_trunk(want_map=True)), else a pass now."""
        pre, self._pre = getattr(self, "_pre", None), None
        if pre is not None:
            stream.wait_event(pre[3])           # also orders a synchronous pass behind an unused look-ahead (shared buffers)
            if pre[0] is images and pre[1] == bool(training) and pre[4] is not None:
                pre[2].record_stream(stream)
                pre[4].record_stream(stream)
                return pre[2], pre[4]
        busy = getattr(self, "_busy", None)
        if busy is not None:
            stream.wait_event(busy)
        feats = self.trunk_features(images, training).clone()
        fmap = self.resnet._plan.last_map(images.shape[0], images.shape[2]).clone()
        self._busy = stream.record_event()
        return feats, fmap

    # ---- direct (no autograd) forms used by the fused step driver
    def trunk_features(self, images, training: bool):
        """The frozen trunk alone (generator.py:20-22): pooled features in the compute dtype, in the plan's own buffer."""
        return self.resnet(images, _compute_dtype(self.args), training)

    def forward_fused(self, images, training: bool, trunk_feats=None):
        dt = _compute_dtype(self.args)
        feats = trunk_feats if trunk_feats is not None else self.resnet(images, dt, training)
        out, self._saved = encoder_head_fwd(dt, feats, self.linear.weight.detach(), self.linear.bias.detach(),
                                            self.bn.weight.detach(), self.bn.bias.detach(), self.bn.running_mean,
                                            self.bn.running_var, training, self.bn.momentum, self.bn.eps)
        return out

    def backward_fused(self, d_feat):
        """Gradients of the head into the .grad views of its four parameters (the trunk is frozen)."""
        grads = (self.linear.weight.grad, self.linear.bias.grad, self.bn.weight.grad, self.bn.bias.grad)
        encoder_head_bwd(_compute_dtype(self.args), self._saved, self.linear.weight.detach(), self.bn.weight.detach(), d_feat,
                         grads=grads)
        self._saved = None


class Generator(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.encoder = Encoder(args)
        if getattr(args, "decoder", "lstm") == "attention":
            if int(args.conditional_gan) != 1:
                raise ValueError("--decoder attention attends over image features: it needs --conditional-gan 1")
            side = int(getattr(args, "image_size", 224)) // 32
            self.decoder = AttnDecoder(args, self.encoder.resnet.out_features, side * side)
        else:
            self.decoder = Decoder(args)
        self.args = args
        self.init_params()

    def caption(self, images, beam_size=3, max_caption_len=None, eos_id=2, length_penalty=0.0, return_beams=False, return_alphas=False,
                beam_groups=1, diversity=0.0, force_words=None, return_met=False, rerank_disc=None, rerank_weight=1.0, return_rerank=False,
                consensus=None, consensus_weight=1.0, return_consensus=False, no_repeat_ngram=0, min_length=0, suppress_tokens=()):
        """Captions for ``images`` by beam search: features as the trainer forms them (training.py:66-68) -- the encoder in the
        module's current mode, or embed(<S>) with --conditional-gan 0 -- under no-grad, then ``decoder.beam_search``.  With
        --decoder attention the encoder also gives the feature map, and ``return_alphas`` appends the attention weights
        (AttnDecoder.beam_search).  ``beam_groups`` / ``diversity``: diverse beam search (Decoder.beam_search).  ``no_repeat_ngram`` /
        ``min_length`` / ``suppress_tokens``: decode constraints (Decoder.beam_search).
        ``rerank_disc`` (a Discriminator; None = the search's own order, nothing else runs): the ``beam_size`` beams are re-ranked by
        score / max(len, 1) ** length_penalty + ``rerank_weight`` * rerank_disc.score (discriminator.rerank: a conditioned D scores them
        against this call's pooled trunk features, any other D the captions alone); the best caption, or all beams with
        ``return_beams``, come in the new order, the attention weights with them; ``scores`` stay G's log-probabilities.
        ``return_rerank`` appends (final [B, k], d [B, k]) in the new order.
        ``consensus`` (a CiderD; None = nothing else runs): consensus (minimum-Bayes-risk) selection instead -- the beams are re-ranked by
        score / max(len, 1) ** length_penalty + ``consensus_weight`` * each beam's mean CIDEr-D against the other beams
        (CiderD.pairwise, then the same gic_rerank: its order, tie rule and outputs); ``return_consensus`` appends (final [B, k],
        consensus [B, k]) in the new order.  One re-ranking at a time: ``consensus`` with ``rerank_disc`` is refused.
        ``force_words`` / ``return_met``: lexically constrained beam search (Decoder.beam_search): words the caption must contain; met
        comes last.  Its order is the search's own: ``rerank_disc`` and ``consensus`` are refused with it."""
        kw = dict(beam_size=beam_size, max_caption_len=max_caption_len, eos_id=eos_id, length_penalty=length_penalty, return_beams=return_beams,
                  beam_groups=beam_groups, diversity=diversity, no_repeat_ngram=no_repeat_ngram, min_length=min_length,
                  suppress_tokens=suppress_tokens)
        if force_words is not None:
            if rerank_disc is not None or consensus is not None:
                raise ValueError("force_words with rerank_disc or consensus: a forced search keeps its own order (constraints met first)")
            kw.update(force_words=force_words, return_met=return_met)
        elif return_met:
            raise ValueError("return_met needs force_words")
        if return_alphas and not isinstance(self.decoder, AttnDecoder):
            raise ValueError("attention weights exist for --decoder attention only")
        if rerank_disc is None and return_rerank:
            raise ValueError("return_rerank needs rerank_disc")
        self._check_consensus(consensus, rerank_disc, return_consensus)
        with torch.no_grad():
            features, fmap = self._features(images)
            if rerank_disc is not None or consensus is not None:
                kw["return_beams"] = True
            if fmap is None:
                out = self.decoder.beam_search(features, **kw)
            else:
                out = self.decoder.beam_search(features, fmap, return_alphas=return_alphas, **kw)
            if rerank_disc is None and consensus is None:
                return out
            if consensus is not None:
                r = self._rerank_consensus(consensus, out, consensus_weight, length_penalty)
            else:
                r = self._rerank(rerank_disc, out, rerank_weight, length_penalty)
        res = (r["ids"], r["scores"], r["lengths"]) + ((r["alphas"],) if return_alphas else ())
        if not return_beams:
            res = tuple(t[:, 0] for t in res)
        return res + (((r["final"], r["d"]),) if return_rerank or return_consensus else ())

    @staticmethod
    def _check_consensus(consensus, rerank_disc, return_consensus=False):
        if consensus is not None and rerank_disc is not None:
            raise ValueError("consensus with rerank_disc: one re-ranking at a time")
        if consensus is None and return_consensus:
            raise ValueError("return_consensus needs consensus")

    @staticmethod
    def _rerank_consensus(scorer, cands, weight, length_penalty=0.0):
        """engine.rerank of this call's candidates (ids, scores, lengths[, alphas]) with each candidate's consensus -- its mean CIDEr-D
        against the image's other candidates (``scorer``: a CiderD) -- in the place of D's score (R = 1): ``d`` of the result."""
        ids, scores, lengths = cands[0], cands[1], cands[2]
        cons = scorer.pairwise(ids, lengths, want_matrix=False, want_self_cider=False)["consensus"]
        return engine.rerank(scores, lengths, cons.view(-1), 1, float(weight), float(length_penalty), ids=ids,
                             alphas=cands[3] if len(cands) > 3 else None)

    def _rerank(self, disc, cands, weight, length_penalty=0.0):
        """discriminator.rerank of this call's candidates (ids, scores, lengths[, alphas]) against this call's pooled trunk features."""
        from .discriminator import rerank
        feats = None
        if getattr(disc, "cond", "none") == "projection":
            if not self.args.conditional_gan:
                raise ValueError("a discriminator built with --disc-cond projection scores (image, caption) pairs: it needs --conditional-gan 1")
            feats = self.encoder.last_trunk
        return rerank(disc, feats, cands[0], cands[1], cands[2], weight=weight, length_penalty=length_penalty,
                      alphas=cands[3] if len(cands) > 3 else None)

    def sample_captions(self, images, num_samples=5, top_k=0, top_p=1.0, temperature=1.0, max_caption_len=None, eos_id=2, seed=None,
                        noise_u=None, rerank_disc=None, rerank_weight=1.0, consensus=None, consensus_weight=1.0, no_repeat_ngram=0,
                        min_length=0, suppress_tokens=()):
        """``num_samples`` sampled captions per image (decoder.sample_captions), with the features formed as ``caption`` forms them:
        the encoder in the module's current mode, or embed(<S>) with --conditional-gan 0, under no-grad; with --decoder attention the
        encoder also gives the feature map.  ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``: decode constraints
        (Decoder.sample_captions).  Returns (ids [B, n, L], scores [B, n], lengths [B, n]) in draw order; with ``rerank_disc``
        (best-of-n) ordered by scores + ``rerank_weight`` * rerank_disc.score instead, with ``consensus`` (a CiderD) by scores +
        ``consensus_weight`` * each sample's mean CIDEr-D against the other samples (``caption``); not both."""
        kw = dict(num_samples=num_samples, top_k=top_k, top_p=top_p, temperature=temperature, max_caption_len=max_caption_len,
                  eos_id=eos_id, seed=seed, noise_u=noise_u, no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=suppress_tokens)
        self._check_consensus(consensus, rerank_disc)
        with torch.no_grad():
            features, fmap = self._features(images)
            out = self.decoder.sample_captions(features, *(() if fmap is None else (fmap,)), **kw)
            if rerank_disc is None and consensus is None:
                return out
            r = self._rerank_consensus(consensus, out, consensus_weight) if consensus is not None else self._rerank(rerank_disc, out, rerank_weight)
        return r["ids"], r["scores"], r["lengths"]

    def score_captions(self, images, ids, lengths):
        """How likely given captions are under the generator: (logp, tokens) in the shape of ``lengths``, logp = the teacher-forced
        log-probability of each caption given its image (decoder.log_likelihood: the units of the beam and sample scores), tokens = the
        positions summed.  ``ids`` int64 [B, L] with ``lengths`` [B], or K captions per image, [B, K, L] with [B, K]: the image goes
        through the encoder once and its features (and feature map) are repeated for its captions.  Features as ``caption`` forms them
        (the encoder in the module's current mode, or embed(<S>) with --conditional-gan 0), under no-grad."""
        lengths = torch.as_tensor(lengths).to(ids.device)
        if ids.dim() not in (2, 3) or tuple(lengths.shape) != tuple(ids.shape[:-1]) or ids.shape[0] != len(images):
            raise ValueError("score_captions: ids must be [B, L] with lengths [B], or [B, K, L] with lengths [B, K], B = len(images)")
        K = ids.shape[1] if ids.dim() == 3 else 1
        with torch.no_grad():
            features, fmap = self._features(images)
            if K > 1:
                features = features.repeat_interleave(K, 0)
                fmap = None if fmap is None else fmap.repeat_interleave(K, 0)
            logp, tokens = self.decoder.log_likelihood(features, *(() if fmap is None else (fmap,)), ids.reshape(-1, ids.shape[-1]),
                                                       lengths.reshape(-1))
        return logp.view(lengths.shape), tokens.view(lengths.shape)

    def forward(self, images, caps, lengths, pretrain=False):
        features, fmap = self._features(images)
        return self.decoder(features, *(() if fmap is None else (fmap,)), caps, lengths, pretrain)

    def _features(self, images):
        """(features, fmap or None) as the trainer forms them (training.py:66-68), in the caller's grad mode: the encoder in the module's
        current mode, with the feature map for --decoder attention, or embed(<S>) with --conditional-gan 0."""
        if isinstance(self.decoder, AttnDecoder):
            return self.encoder.forward_with_map(images)
        if self.args.conditional_gan:
            return self.encoder(images), None
        return self.decoder.embed(torch.ones(len(images), dtype=torch.long, device=images.device)), None

    def init_params(self):
        """generator.py:116-123: every parameter with >= 1 dim (biases, BN affine and trunk convs included)."""
        for param in self.parameters():
            if param.requires_grad and len(param.shape) > 0:
                if self.args.gen_init == "uniform":
                    torch.nn.init.uniform_(param, a=-0.05, b=0.05)
                elif self.args.gen_init == "normal":
                    torch.nn.init.normal_(param, std=1 / math.sqrt(param.shape[0]))


class Ensemble:
    """Decode-time ensemble of ``Generator`` modules of one decoder kind, dims and compute dtype (gicap.h gic_*_ensemble_*).  At every
    step each member, in its own recurrent state, gives its logits; with lp_m = log_softmax(l_m) the search runs on z = log sum_m w_m
    exp(lp_m) (``mode`` "prob": the arithmetic mean of the probabilities) or z = sum_m w_m lp_m ("logprob": the geometric mean), exactly
    as it runs on one model's logits; ``weights`` (None: uniform) are normalised to sum 1.  Members that share one trunk module object
    (``encoder.resnet``) run the trunk once and their own heads on it.  Not a module: it owns no parameters and nothing trains
    through it.  ``eval()`` / ``train()`` / ``training`` / ``encoder`` / ``decoder`` / ``args`` follow member 0, so the evaluations can
    be handed an Ensemble where they take a Generator."""

    def __init__(self, members, weights=None, mode="prob"):
        self.members = list(members)
        if not self.members:
            raise ValueError("an ensemble needs at least one member")
        g0 = self.members[0]
        for m, g in enumerate(self.members):
            if not isinstance(g, Generator) or type(g.decoder) is not type(g0.decoder):
                raise ValueError(f"ensemble member {m}: the members must be Generator modules of one decoder kind")
        self.opts = engine.ensemble_opts(len(self.members), weights, mode)       # (checks the count, the weights and the mode)
        self.weights = None if weights is None else [float(w) for w in weights]
        self.mode = mode

    # ---- the Generator surface the evaluations read
    encoder = property(lambda self: self.members[0].encoder)
    decoder = property(lambda self: self.members[0].decoder)
    args = property(lambda self: self.members[0].args)
    training = property(lambda self: self.members[0].training)

    def train(self, mode=True):
        for g in self.members:
            g.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def _features(self, images):
        """Every member's (features, fmap or None): Generator._features per member, except that a member whose trunk module is an
        earlier member's takes that member's pooled trunk features (and feature map) and runs its own head on them."""
        out, trunks = [], {}
        for g in self.members:
            key = (id(g.encoder.resnet), bool(g.encoder.training))
            if not g.args.conditional_gan or key not in trunks:
                f, fmap = g._features(images)
                if g.args.conditional_gan:
                    trunks[key] = (g.encoder.last_trunk, fmap)
            else:
                feats, fmap = trunks[key]
                f = g.encoder.head(feats)
            out.append((f, fmap))
        return out

    def _members(self):
        return [(g.decoder.engine(), [p.detach() for p in g.decoder.param_list()]) for g in self.members]

    def _inputs(self, images):
        fm = self._features(images)
        feats = [f.detach().float() for f, _ in fm]
        maps = None if fm[0][1] is None else [m.detach() for _, m in fm]
        return feats, maps

    def _len(self, max_caption_len):
        return int(self.decoder.max_seq_length if max_caption_len is None else max_caption_len)

    def caption(self, images, beam_size=3, max_caption_len=None, eos_id=2, length_penalty=0.0, return_beams=False, return_alphas=False,
                beam_groups=1, diversity=0.0, force_words=None, return_met=False, rerank_disc=None, rerank_weight=1.0, return_rerank=False,
                consensus=None, consensus_weight=1.0, return_consensus=False, no_repeat_ngram=0, min_length=0, suppress_tokens=(), states=None):
        """Generator.caption on the ensemble's logits: the same keywords, outputs and re-rankings (a conditioned ``rerank_disc`` reads
        member 0's pooled trunk features).  ``return_alphas`` and ``states`` are refused: an ensemble has no one attention map and no
        one initial state."""
        if force_words is not None or return_met:              # (Generator.caption's keywords, in its positions; refused here)
            raise ValueError("force_words with an ensemble: the forced search runs one model")
        if return_alphas:
            raise ValueError("an ensemble returns no attention weights (return_alphas): every member attends on its own")
        if states is not None:
            raise ValueError("an ensemble search takes no initial states (states=)")
        if rerank_disc is None and return_rerank:
            raise ValueError("return_rerank needs rerank_disc")
        g0 = self.members[0]
        g0._check_consensus(consensus, rerank_disc, return_consensus)
        with torch.no_grad():
            feats, maps = self._inputs(images)
            out = g0.decoder.engine().ensemble_beam_search(self._members(), feats, maps, self._len(max_caption_len), int(beam_size),
                                                           self.weights, self.mode, int(beam_groups), float(diversity), int(eos_id), 0,
                                                           float(length_penalty), no_repeat_ngram=no_repeat_ngram, min_length=min_length,
                                                           suppress_tokens=suppress_tokens)
            if rerank_disc is None and consensus is None:
                return out if return_beams else tuple(t[:, 0] for t in out)
            if consensus is not None:
                r = g0._rerank_consensus(consensus, out, consensus_weight, length_penalty)
            else:
                r = g0._rerank(rerank_disc, out, rerank_weight, length_penalty)
        res = (r["ids"], r["scores"], r["lengths"])
        if not return_beams:
            res = tuple(t[:, 0] for t in res)
        return res + (((r["final"], r["d"]),) if return_rerank or return_consensus else ())

    def sample_captions(self, images, num_samples=5, top_k=0, top_p=1.0, temperature=1.0, max_caption_len=None, eos_id=2, seed=None,
                        noise_u=None, rerank_disc=None, rerank_weight=1.0, consensus=None, consensus_weight=1.0, no_repeat_ngram=0,
                        min_length=0, suppress_tokens=(), states=None):
        """Generator.sample_captions on the ensemble's logits: the same keywords, outputs and re-rankings."""
        if states is not None:
            raise ValueError("an ensemble search takes no initial states (states=)")
        g0 = self.members[0]
        g0._check_consensus(consensus, rerank_disc)
        seed = (0 if noise_u is not None else SEEDS.next()) if seed is None else int(seed)
        with torch.no_grad():
            feats, maps = self._inputs(images)
            out = g0.decoder.engine().ensemble_sample_captions(self._members(), feats, maps, self._len(max_caption_len), int(num_samples),
                                                               self.weights, self.mode, int(top_k), float(top_p), float(temperature),
                                                               int(eos_id), 0, seed, noise_u, no_repeat_ngram=no_repeat_ngram,
                                                               min_length=min_length, suppress_tokens=suppress_tokens)
            if rerank_disc is None and consensus is None:
                return out
            r = g0._rerank_consensus(consensus, out, consensus_weight) if consensus is not None else g0._rerank(rerank_disc, out, rerank_weight)
        return r["ids"], r["scores"], r["lengths"]

    def score_captions(self, images, ids, lengths):
        """Generator.score_captions under the ensemble: every member's teacher-forced no-grad logits, engine.ensemble_mix over
        [M, B * L, V], then gic_xent_seq masked by ``lengths``: (logp, tokens) in the shape of ``lengths``, in the units of the
        ensemble's beam and sample scores."""
        lengths = torch.as_tensor(lengths).to(ids.device)
        if ids.dim() not in (2, 3) or tuple(lengths.shape) != tuple(ids.shape[:-1]) or ids.shape[0] != len(images):
            raise ValueError("score_captions: ids must be [B, L] with lengths [B], or [B, K, L] with lengths [B, K], B = len(images)")
        if ids.dtype != torch.int64 or ids.shape[-1] < 2:
            raise ValueError("score_captions: ids must be int64 with L >= 2")
        K = ids.shape[1] if ids.dim() == 3 else 1
        flat, L = ids.reshape(-1, ids.shape[-1]), ids.shape[-1]
        n = flat.shape[0]
        lens = lengths.reshape(-1).to(torch.int32)
        with torch.no_grad():
            preds = []
            for g, (f, fmap) in zip(self.members, self._features(images)):
                if K > 1:
                    f = f.repeat_interleave(K, 0)
                    fmap = None if fmap is None else fmap.repeat_interleave(K, 0)
                maps = () if fmap is None else (fmap,)
                pred = g.decoder._forward_no_grad(f, *maps, flat[:, :-1].contiguous(), lens.clamp(1, L), True, None, 0, L)[0]
                preds.append(pred.reshape(n * L, pred.shape[-1]).float())
            z = engine.ensemble_mix(torch.stack(preds), self.weights, self.mode)
            out = engine.xent_seq(z, flat.reshape(-1), L, lengths=lens, want_grad=False)
        return (-out["cap_nll"]).view(lengths.shape), out["cap_tokens"].view(lengths.shape)
